"""The shifted-Gram style term (--shift-weight) on the GPU: the kernels of shiftgram.hip through stx_op_shift_terms
and stx_shift_gram, the tile path, the farm and the command line -- against tests/shift_ref.py (float64 on the same
float32 inputs).

Bounds.  X_d within 1e-5 max |X_d| (tests/gpu_helpers.TIGHT, the project's loss bound), E / 2 and sum |S| to 1e-5
relative, S within 1e-5 max |S|.  The targets lie 0.5 .. 1.5 times off the blob's own X_d, so D = X - T is not a
cancelled difference.  The tile path is held as tests/gpu_helpers.check_tile holds the Gram path (TIGHT): every one
of its clauses.

Observed worst values on an MI355X: X 8.6e-7 of max |X|, E / 2 5.8e-8, sum |S| 9.4e-8, S 1.1e-6 of max |S|; the tiles'
loss 1.4e-7 (1.9e-7 against the oracle's own loss), their activations 1.0e-6, the term alone 6.2e-7, the gradient
8.9e-7 of its maximum against the oracle's backward pass on the GPU's activations, 2.3e-6 against the oracle's own on
every pixel (no decision flips in either case); beside the statistics term 7.3e-7 and 2.1e-6.  Every case prints its
figures before it asserts (pytest -s)."""

import ctypes
import functools
import re

import numpy as np
import pytest
from PIL import Image

from oracle.caffe_net import synthetic_weights
from style_transfer_amd import lib
from style_transfer_amd.netspec import builtin_net
from tests import shift_ref, stat_ref
from tests.gpu_helpers import TIGHT, decision_taint, gpu_engine, l2_rel, loss_from_activations, max_rel

pytestmark = pytest.mark.gpu
FLIP_L2 = 1e-2

OP_CASES = [
    (32, 5, 7, [(0, 1), (1, 0), (0, 6), (4, 0)]),           # smallest; one pair per row / one row
    (64, 9, 70, [(0, 1), (0, 4), (3, 0)]),                  # w - dx off every tile multiple
    (96, 33, 31, [(0, 2), (0, 30), (32, 0)]),               # three channel blocks, nearly empty P
    (128, 130, 3, [(0, 2), (64, 0)]),                       # narrow map, tall
    (512, 4, 4, [(0, 1), (0, 3), (1, 0)]),                  # many channel blocks, K = 3072 in the gradient
    (64, 257, 263, [(0, 8), (64, 0), (0, 2), (2, 0), (0, 4), (4, 0)]),      # several K slices, a ragged last one
]


def _blob(c, h, w, offsets):
    """Seeded rectified data with an all-zero channel and a channel of one non-zero pixel; targets 0.5 .. 1.5 times
    off the blob's own X."""
    rng = np.random.RandomState(c + h + w)
    feat = np.maximum(rng.standard_normal((c, h, w)) * 2 + 0.5, 0).astype(np.float32)
    feat[1] = 0
    feat[3] = 0
    feat[3, h // 2, w // 3] = 7.5
    own = shift_ref.shift_gram(feat, offsets)
    return feat, (own * rng.uniform(0.5, 1.5, own.shape)).astype(np.float32)


def _op(eng, d_feat, c, h, w, offsets, d_grams):
    s_out = eng.empty((c, h, w))
    out = (ctypes.c_double * 2)()
    flat = (ctypes.c_int * (2 * len(offsets)))(*[v for o in offsets for v in o])
    lib.call('stx_op_shift_terms', eng.handle, d_feat.ptr, c, h, w, flat, len(offsets), d_grams.ptr, s_out.ptr, out)
    s = s_out.get()
    s_out.free()
    return s, out[0], out[1]


@pytest.mark.parametrize('c,h,w,offsets', OP_CASES)
def test_shift_kernels_against_float64(c, h, w, offsets):
    eng = gpu_engine()
    feat, T = _blob(c, h, w, offsets)
    x_ref = shift_ref.shift_gram(feat, offsets)
    half_ref, s_ref, asum_ref = shift_ref.shift_terms(feat, offsets, T)
    d_feat, d_T = eng.to_device(feat), eng.to_device(T)
    # --- stx_shift_gram, from the device and from the host
    x = eng.shift_gram(d_feat, offsets)
    again = eng.shift_gram(feat, offsets)
    x_err = max(float(np.abs(x[i] - x_ref[i]).max() / np.abs(x_ref[i]).max()) for i in range(len(offsets)))
    # --- the term, twice
    s, half, asum = _op(eng, d_feat, c, h, w, offsets, d_T)
    s2, half2, asum2 = _op(eng, d_feat, c, h, w, offsets, d_T)
    s_err = float(np.abs(s - s_ref).max() / np.abs(s_ref).max())
    print('C %d %dx%d, %d offsets: X %.2e of max |X|, E/2 %.2e, sum|S| %.2e, S %.2e of max |S|'
          % (c, h, w, len(offsets), x_err, abs(half / half_ref - 1), abs(asum / asum_ref - 1), s_err))
    assert np.all(np.isfinite(s)) and np.isfinite(half) and np.isfinite(asum)
    assert x.shape == (len(offsets), c, c) and x.dtype == np.float32
    for i in range(len(offsets)):
        assert np.abs(x[i] - x_ref[i]).max() <= TIGHT * np.abs(x_ref[i]).max(), offsets[i]
    assert half == pytest.approx(half_ref, rel=TIGHT)
    assert asum == pytest.approx(asum_ref, rel=TIGHT)
    assert s_err <= TIGHT
    assert np.array_equal(x, again)
    assert half == half2 and asum == asum2 and np.array_equal(s, s2)
    # --- the blob's own X as targets: exactly nothing
    d_own = eng.to_device(x)
    s0, half0, asum0 = _op(eng, d_feat, c, h, w, offsets, d_own)
    assert half0 == 0 and asum0 == 0 and not s0.any()
    for arr in (d_feat, d_T, d_own):
        arr.free()


def test_refusals_of_the_kernels_entry_points():
    eng = gpu_engine()
    feat = np.ones((48, 6, 6), np.float32)
    with pytest.raises(lib.StxError, match='48 channels.*multiple of 32') as err:
        eng.shift_gram(feat, [(0, 1)])
    assert err.value.code == -4                 # STX_ERR_UNSUPPORTED
    feat = np.ones((32, 6, 6), np.float32)
    for bad in ([(1, 1)], [(0, 0)], [(0, -1)], [(0, 1)] * 17):
        with pytest.raises(lib.StxError) as err:
            eng.shift_gram(feat, bad)
        assert err.value.code == -1             # STX_ERR_ARG
    with pytest.raises(lib.StxError, match=r'offset \(0, 6\).*6 x 6') as err:
        eng.shift_gram(feat, [(0, 5), (0, 6)])
    assert err.value.code == -1
    d_feat, d_T = eng.to_device(np.ones((48, 6, 6), np.float32)), eng.to_device(np.zeros((1, 48, 48), np.float32))
    with pytest.raises(lib.StxError, match='multiple of 32'):
        _op(eng, d_feat, 48, 6, 6, [(0, 1)], d_T)
    d_feat.free()
    d_T.free()


# --------------------------------------------------------------------------------- the tile path
SL = ['conv1_1', 'conv2_1', 'conv3_1']
SW = {l: 1 / 3 for l in SL}
LW = {'conv2_1': 1.5}
FRAME = (128, 128)
OFFSETS = [(0, 1), (1, 0), (0, 2), (2, 0)]      # --shift-offsets 1 2
# the shift layers: conv2_1 carries a Gram term too (two style terms: stand-alone injection); the other one is tapped
# by nothing else -- conv2_2 feeds a pooling layer, conv3_2 a convolution (the fused epilogue's sgrad path)
CASES = {'pool': (['conv3_2'], ['conv2_1', 'conv2_2']), 'conv': (['conv3_3'], ['conv2_1', 'conv3_2'])}
SHIFT_W = {'conv2_1': 0.7, 'conv2_2': 1.3, 'conv3_2': 1.3}


@functools.lru_cache(maxsize=None)
def _scene(case):
    """Oracle with targets of a 128 x 128 frame, computed once."""
    cl, shift_layers = CASES[case]
    net = builtin_net('vgg19')
    om = shift_ref.ShiftOracleModel(net.as_dicts(), synthetic_weights(net.as_dicts(), 0))
    rng = np.random.RandomState(13)
    full = rng.uniform(-110, 120, (3,) + FRAME).astype(np.float32)
    style = rng.uniform(-110, 120, (3, 40, 44)).astype(np.float32)
    om.styles = [om.style_grams([style], SL, 512)]
    om.contents = [om.prepare_features(full, cl, 512)]
    feats = om.features_tile(style, shift_layers)
    targets = {layer: (OFFSETS, np.float32(shift_ref.shift_gram(feats[layer], OFFSETS))) for layer in shift_layers}
    stats = tuple(np.float32(v) for v in stat_ref.feature_stats(feats['conv2_1']))
    return om, full, cl, {l: 0.05 for l in cl}, targets, stats


def _arm(eng, om, targets):
    eng.set_contents_and_styles(om.contents, om.styles)
    eng.set_shift_targets(targets, SHIFT_W)
    om.shift_targets = {l: (offs, np.float64(T)) for l, (offs, T) in targets.items()}
    om.shift_weights = dict(SHIFT_W)


def _disarm(om):
    om.shift_targets, om.shift_weights, om.extra_layers, om.extra_term = {}, {}, (), None


def _tile(full, th, tw, start, roll):
    rolled = np.roll(full, (roll[0], roll[1]), axis=(-1, -2))
    return np.ascontiguousarray(rolled[:, start[0]:start[0] + th, start[1]:start[1] + tw])


def _against_the_oracle(eng, om, tile, start, roll, cl, cw, plain, extra64, what):
    """The clauses of tests/gpu_helpers.check_tile for an armed engine and oracle; ``extra64(acts)``: the float64
    value of the terms beside the shifted-Gram one that ``plain`` (the evaluation without any of them) lacks."""
    plain_loss, plain_grad = plain
    loss, grad = eng.sc_grad_tile(tile, start, roll, cl, SL, LW, cw, SW)
    alone, _ = eng.sc_grad_tile(tile, start, roll, [], [], LW, {}, {})         # the target layers only
    deepest = om.deep_to_shallow(cl + SL + list(om.shift_targets))[0]
    blobs = om.blob_names[:om.blob_names.index(deepest) + 1]
    acts = eng.features_tile(tile, blobs)
    om.roll_contents(roll)
    try:
        ref_loss, oracle_grad = om.sc_grad_tile(tile, start, cl, SL, LW, cw, SW)
        ref_acts = {b: om.net.blobs[b].data[0].copy() for b in blobs}
        same_loss, same_grad = om.sc_grad_tile(tile, start, cl, SL, LW, cw, SW, activations=acts)
        base64, _ = loss_from_activations(om, ref_acts, start, cl, SL, LW, cw, SW, np.float64)
        term64 = om.shift_loss64(ref_acts, LW) + extra64(ref_acts)
    finally:
        om.roll_contents(-np.asarray(roll))
    taint, n_relu, n_pool = decision_taint(om.net.layers, acts, ref_acts, deepest, {'data': tile.shape})
    clean = ~taint
    scale = np.abs(oracle_grad).max()
    stats = dict(loss=abs(loss / (base64 + term64) - 1), term=term64 / base64,
                 oracle_loss=abs(loss / ref_loss - 1), same_loss=abs(loss / same_loss - 1),
                 act=max(max_rel(acts[b], ref_acts[b]) for b in blobs),
                 term_alone=abs(alone / term64 - 1), same=max_rel(grad, same_grad), all=max_rel(grad, oracle_grad),
                 moved=max_rel(grad, plain_grad), l2=l2_rel(grad, oracle_grad),
                 clean=float(np.abs(np.float64(grad) - oracle_grad)[:, clean].max() / scale) if clean.any() else 0.0,
                 flips=(n_relu, n_pool))
    print(what, tile.shape, start, roll, stats)
    assert np.all(np.isfinite(grad))
    assert stats['moved'] > 1e-3                              # the term is not lost in the others
    assert stats['act'] < TIGHT, stats
    assert loss == pytest.approx(base64 + term64, rel=TIGHT), (loss, base64, term64, ref_loss, same_loss)
    assert loss == pytest.approx(ref_loss, rel=TIGHT), (loss, ref_loss)
    assert loss == pytest.approx(same_loss, rel=TIGHT), (loss, same_loss)
    # (each of the two losses is within TIGHT of its own float64 value)
    assert loss - plain_loss == pytest.approx(term64, abs=2 * TIGHT * (base64 + term64))
    assert alone == pytest.approx(term64, rel=TIGHT), (alone, term64)
    assert stats['same'] < TIGHT, stats
    assert stats['clean'] < TIGHT, stats
    if n_relu == 0 and n_pool == 0:
        assert stats['all'] < TIGHT, stats
    assert stats['l2'] < FLIP_L2, stats


@pytest.mark.parametrize('case,th,tw,start,roll', [('pool', 64, 48, (0, 0), (0, 0)),
                                                   ('conv', 37, 53, (64, 32), (-24, 40))])
def test_shift_tile_against_the_oracle(case, th, tw, start, roll):
    """The evaluation with shifted-Gram targets on two layers is the evaluation without them plus the term (float64,
    from the oracle's blobs, through the oracle's backward pass): tests/gpu_helpers.check_tile's bounds on the loss
    and on the image gradient."""
    om, full, cl, cw, targets, _ = _scene(case)
    eng = gpu_engine()
    tile = _tile(full, th, tw, start, roll)
    eng.set_contents_and_styles(om.contents, om.styles)
    plain = eng.sc_grad_tile(tile, start, roll, cl, SL, LW, cw, SW)
    _arm(eng, om, targets)
    try:
        _against_the_oracle(eng, om, tile, start, roll, cl, cw, plain, lambda acts: 0.0, 'shift tile ' + case)
    finally:
        _disarm(om)
        eng.set_shift_targets({})


def test_shift_beside_the_statistics_term_on_one_blob():
    """conv2_1 with a Gram tap, a statistics target and a shifted-Gram target: three gradient slots and two scratch
    regions of one tap.  The evaluation is the sum of the separately checked terms: ShiftOracleModel with the
    statistics term (tests/stat_ref.py) added in front, at TIGHT."""
    om, full, cl, cw, targets, stats = _scene('conv')
    eng = gpu_engine()
    start, roll = (64, 32), (-24, 40)
    tile = _tile(full, 37, 53, start, roll)
    stat_w = 0.9
    mu64, sd64 = np.float64(stats[0]), np.float64(stats[1])

    def stat_term(b, feat, lw):
        half, S, _, _ = stat_ref.stat_terms(feat, mu64, sd64)
        return lw * stat_w * half, lw * stat_w * stat_ref.normalized(S)

    eng.set_contents_and_styles(om.contents, om.styles)
    plain = eng.sc_grad_tile(tile, start, roll, cl, SL, LW, cw, SW)
    _arm(eng, om, targets)
    eng.set_stat_targets({'conv2_1': stats}, {'conv2_1': stat_w})
    om.extra_layers, om.extra_term = ('conv2_1',), stat_term
    try:
        extra64 = lambda acts: LW['conv2_1'] * stat_w * stat_ref.stat_terms(acts['conv2_1'], mu64, sd64)[0]
        _against_the_oracle(eng, om, tile, start, roll, cl, cw, plain, extra64, 'shift + stat')
    finally:
        _disarm(om)
        eng.set_stat_targets({})
        eng.set_shift_targets({})


def _untapped(eng, evaluate):
    """evaluate() with a tap list that names no layer for its shifted-Gram target alone (TileEngine adds a tap
    without flags for each): such a layer reaches the library through its target only, which adds it to the path
    with lw = 1."""
    kept, eng.primary.extra_taps['shift'] = eng.primary.extra_taps['shift'], []
    try:
        return evaluate()
    finally:
        eng.primary.extra_taps['shift'] = kept


def test_targets_of_the_tile_itself_change_no_bit_and_targets_are_cleared():
    from style_transfer_amd.engine import TileEngine
    from tests.gpu_helpers import require_gpu
    require_gpu()
    om, full, cl, cw, targets, _ = _scene('conv')
    net = builtin_net('vgg19')
    eng = TileEngine(net, 0, synthetic_weights(net.as_dicts(), 0))       # no such target was ever set on this one
    tile = _tile(full, 64, 48, (0, 0), (0, 0))
    run = lambda lw=LW: eng.sc_grad_tile(tile, (0, 0), (0, 0), cl, SL, lw, cw, SW)
    eng.set_contents_and_styles(om.contents, om.styles)
    before = run()
    acts = eng.features_tile(tile, om.blob_names[:om.blob_names.index('conv3_3') + 1])
    own = {layer: (OFFSETS, eng.shift_gram(acts[layer], OFFSETS)) for layer in targets}
    eng.set_shift_targets(own, SHIFT_W)
    on_target = run()
    assert on_target[0] == before[0] and np.array_equal(on_target[1], before[1])      # the term is exactly 0
    eng.set_shift_targets(targets, SHIFT_W)
    moved = run()
    assert moved[0] != before[0] and not np.array_equal(moved[1], before[1])
    # an untapped shift layer joins the path at layer_weight 1: bit for bit the evaluation that names it, and not
    # the one that names it at another weight
    bare = _untapped(eng, run)
    assert bare[0] == moved[0] and np.array_equal(bare[1], moved[1])
    doubled = run(dict(LW, conv3_2=2.0))
    assert doubled[0] != moved[0] and not np.array_equal(doubled[1], moved[1])
    eng.set_shift_targets({})
    cleared = run()
    assert cleared[0] == before[0] and np.array_equal(cleared[1], before[1])
    eng.set_shift_targets(targets, SHIFT_W)
    eng.set_contents_and_styles(om.contents, om.styles)                  # clears the shifted-Gram targets
    fresh = run()
    assert fresh[0] == before[0] and np.array_equal(fresh[1], before[1])
    # a tap list with no content, style or Deep-Dream layer -- an empty one too -- is taken when such targets exist
    with pytest.raises(lib.StxError):
        eng.sc_grad_tile(tile, (0, 0), (0, 0), [], [], LW, {}, {})
    eng.set_shift_targets(targets, SHIFT_W)
    only = eng.sc_grad_tile(tile, (0, 0), (0, 0), [], [], LW, {}, {})
    none = _untapped(eng, lambda: eng.sc_grad_tile(tile, (0, 0), (0, 0), [], [], {}, {}, {}))
    assert np.isfinite(only[0]) and only[0] > 0 and only[1].any()
    assert np.isfinite(none[0]) and none[0] > 0 and none[1].any()
    # a wrong channel count and an unknown layer are errors at the call
    with pytest.raises(lib.StxError, match='channels') as err:
        eng.set_shift_targets({'conv2_1': (OFFSETS, np.zeros((4, 64, 64), np.float32))})
    assert err.value.code == -1
    with pytest.raises(lib.StxError, match='conv9_9'):
        eng.set_shift_targets({'conv9_9': (OFFSETS, np.zeros((4, 64, 64), np.float32))})
    # an offset that leaves the tile's blob without a pair is an error at the evaluation, which names both
    eng.set_shift_targets({'conv3_2': ([(0, 1), (16, 0)], np.zeros((2, 256, 256), np.float32))})
    with pytest.raises(lib.StxError, match=r'conv3_2.*offset \(16, 0\)') as err:
        run()                                   # a 64 x 48 tile: 16 x 12 at conv3_2
    assert err.value.code == -1
    eng.close()


def test_shift_tile_is_bit_identical_across_sum_schedules_and_runs(monkeypatch):
    om, full, cl, cw, targets, _ = _scene('pool')
    eng = gpu_engine()
    eng.set_contents_and_styles(om.contents, om.styles)
    eng.set_shift_targets(targets, SHIFT_W)
    tile = _tile(full, 64, 48, (0, 0), (0, 0))
    run = lambda: eng.sc_grad_tile(tile, (0, 0), (0, 0), cl, SL, LW, cw, SW)
    first, again = run(), run()
    assert first[0] == again[0] and np.array_equal(first[1], again[1])
    monkeypatch.setenv('STX_SUMS_LATE', '0')            # in-place sums (the fixture re-reads the switches)
    in_place = run()
    monkeypatch.delenv('STX_SUMS_LATE')
    assert in_place[0] == first[0] and np.array_equal(in_place[1], first[1])
    eng.set_shift_targets({})


def test_farm_step_with_shift_targets_repeats_bit_identically():
    """A 96 x 80 image in 2 x 2 tiles of 48 x 40 with a roll: one TileFarm step, twice."""
    from style_transfer_amd.farm import TileFarm
    from tests.gpu_helpers import require_gpu
    require_gpu()
    om, _, cl, cw, targets, _ = _scene('pool')
    net = builtin_net('vgg19')
    rng = np.random.RandomState(23)
    img = rng.uniform(-110, 120, (3, 96, 80)).astype(np.float32)
    farm = TileFarm(net, [0], synthetic_weights(net.as_dicts(), 0), verbose=False)
    contents = [farm.prepare_features_device(img, cl, 64, passes=1)]
    farm.set_contents_and_styles(contents, om.styles)
    d_img, d_grad = farm.master.to_device(img), farm.master.empty(img.shape)
    plain = farm.eval_sc_grad(d_img, d_grad, (8, -16), cl, SL, LW, cw, SW, 64)
    farm.set_shift_targets(targets, SHIFT_W)
    first = farm.eval_sc_grad(d_img, d_grad, (8, -16), cl, SL, LW, cw, SW, 64)
    grad = d_grad.get()
    second = farm.eval_sc_grad(d_img, d_grad, (8, -16), cl, SL, LW, cw, SW, 64)
    assert farm.tile_evals == 12
    assert np.isfinite(first) and first > plain and np.all(np.isfinite(grad))
    assert first == second and np.array_equal(grad, d_grad.get())
    farm.close()


# ------------------------------------------------------------------------------ the command line
def _cli_run(tmp_path, monkeypatch, capsys, name, extra):
    import csv
    import glob
    from style_transfer_amd import cli
    where = tmp_path / name
    where.mkdir()
    monkeypatch.chdir(where)
    argv = ['-ci', '../c.png', '-si', '../s.png', '--size', '64', '--min-size', '64', '-i', '3', '--tile-size', '64',
            '--model', 'vgg19', '--weights', 'synthetic:0', '--devices', '0', '-oi', 'out.png'] + extra
    assert cli.main(argv) == 0
    capsys.readouterr()
    final = Image.open(where / 'out.png')
    logs = glob.glob(str(where / '*_log.csv'))
    assert len(logs) == 1
    with open(logs[0], newline='') as f:
        losses = [float(row['loss']) for row in csv.DictReader(f)]
    return np.asarray(final.convert('RGB')), final.text['Comment'], losses


def test_cli_shift_weight_without_gram_layers(tmp_path, monkeypatch, capsys):
    rng = np.random.RandomState(5)
    picture = lambda hw: Image.fromarray(np.uint8(rng.uniform(0, 255, hw + (3,))))
    picture((64, 56)).save(tmp_path / 'c.png')
    picture((48, 52)).save(tmp_path / 's.png')
    shift = _cli_run(tmp_path, monkeypatch, capsys, 'shift', ['--shift-weight', '1', '--style-layers'])
    bare = _cli_run(tmp_path, monkeypatch, capsys, 'bare', [])
    assert shift[0].shape == (64, 56, 3) and len(shift[2]) == 3 and np.all(np.isfinite(shift[2]))
    assert re.search(r'shift_weight=1\.0', shift[1]) and 'style_layers=[]' in shift[1]
    assert 'shift_layers' not in shift[1] and 'shift_offsets' not in shift[1]
    # without the option the comment names nothing of it: the reference's option names and no others
    assert 'shift_' not in bare[1]
    assert not np.array_equal(shift[0], bare[0]) and shift[2] != bare[2]
