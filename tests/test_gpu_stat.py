"""The mean / std style term (--stat-weight) on the GPU: the three kernels of stat.hip through
stx_op_stat_terms and stx_feature_stats, the tile path, the farm and the command line -- against
tests/stat_ref.py (float64 on the same float32 inputs).

Bounds.  mu, sd, E / 2 and sum |S| to 1e-5 relative (tests/gpu_helpers.TIGHT, the project's loss bound); sd of
a channel without spread to 1e-5 absolute.  S within 1e-5 max |S| + |b_c| max |F_c| 2^-23 in channel c: the
second part is what the rounding of mu_c to float32 moves b_c (F_c - mu_c) by, stated, not measured.  The
targets lie 0.5 .. 1.5 times off the blob's own statistics, so a = mu - MU is not a cancelled difference.  The
tile path is held as tests/gpu_helpers.check_tile holds the Gram path (TIGHT): every one of its clauses.

Observed worst values on an MI355X: mu 9.7e-8, sd 1.3e-7, E / 2 3.1e-7, sum |S| 1.9e-7, S at 2.0e-2 of its
bound; the tiles' loss 6.6e-8 (1.3e-7 against the oracle's own loss), their activations 1.0e-6, the term alone
5.7e-7, the gradient 1.3e-6 of its maximum against the oracle's backward pass on the GPU's activations, 1.7e-6
against the oracle's own on every pixel (no decision flips in either case).  Every case prints its figures
before it asserts (pytest -s)."""

import ctypes
import functools
import re

import numpy as np
import pytest
from PIL import Image

from oracle.caffe_net import synthetic_weights
from style_transfer_amd import lib
from style_transfer_amd.netspec import builtin_net
from tests import stat_ref
from tests.gpu_helpers import TIGHT, decision_taint, gpu_engine, l2_rel, loss_from_activations, max_rel

pytestmark = pytest.mark.gpu
FLIP_L2 = 1e-2

# 35 pixels: every channel start is misaligned; var = 0; several slices with a ragged last one; two more
OP_SHAPES = [(64, 5, 7), (3, 1, 1), (8, 257, 263), (128, 33, 31), (512, 4, 4)]


def _blob(c, h, w):
    """Seeded rectified data; in a blob of eight channels or more, four special channels: all zero, constant,
    one non-zero pixel, and mean 1e3 with standard deviation 0.1 (the cancellation case)."""
    rng = np.random.RandomState(c + h + w)
    feat = np.maximum(rng.standard_normal((c, h, w)) * 2 + 0.5, 0).astype(np.float32)
    if c >= 8:
        feat[1] = 0
        feat[2] = 0.3
        feat[3] = 0
        feat[3, h // 2, w // 3] = 7.5
        feat[5] = (1e3 + 0.1 * rng.standard_normal((h, w))).astype(np.float32)
    mu, sd = stat_ref.feature_stats(feat)
    MU = (mu * rng.uniform(0.5, 1.5, c) + 0.05 * rng.standard_normal(c)).astype(np.float32)
    SD = (sd * rng.uniform(0.5, 1.5, c)).astype(np.float32)
    return feat, MU, SD


def _op(eng, d_feat, c, h, w, d_mu, d_sd):
    s_out = eng.empty((c, h, w))
    out = (ctypes.c_double * 2)()
    lib.call('stx_op_stat_terms', eng.handle, d_feat.ptr, c, h, w, d_mu.ptr, d_sd.ptr, s_out.ptr, out)
    s = s_out.get()
    s_out.free()
    return s, out[0], out[1]


@pytest.mark.parametrize('c,h,w', OP_SHAPES)
def test_stat_kernels_against_float64(c, h, w):
    eng = gpu_engine()
    feat, MU, SD = _blob(c, h, w)
    mu_ref, sd_ref = stat_ref.feature_stats(feat)
    half_ref, s_ref, asum_ref, b_ref = stat_ref.stat_terms(feat, MU, SD)
    d_feat, d_mu, d_sd = eng.to_device(feat), eng.to_device(MU), eng.to_device(SD)
    # --- stx_feature_stats, from the device and from the host, twice
    mu, sd = eng.feature_stats(d_feat)
    again = eng.feature_stats(feat)
    flat = feat.reshape(c, -1)
    spread = flat.max(axis=1) > flat.min(axis=1)
    mu_err = float(np.max(np.abs(mu - mu_ref) / np.maximum(np.abs(mu_ref), 1e-300)))
    sd_err = float(np.max(np.abs(sd - sd_ref)[spread] / sd_ref[spread])) if spread.any() else 0.0
    sd_abs = float(np.max(np.abs(sd - sd_ref)[~spread])) if (~spread).any() else 0.0
    # --- the term, twice
    s, half, asum = _op(eng, d_feat, c, h, w, d_mu, d_sd)
    s2, half2, asum2 = _op(eng, d_feat, c, h, w, d_mu, d_sd)
    bound = TIGHT * np.abs(s_ref).max() + np.abs(b_ref) * np.abs(flat).max(axis=1) * 2.0 ** -23
    s_err = np.abs(s.reshape(c, -1) - s_ref.reshape(c, -1)).max(axis=1)
    print('C %d %dx%d: mu %.2e, sd %.2e (no spread: %.2e abs), E/2 %.2e, sum|S| %.2e, S %.2e of its bound'
          % (c, h, w, mu_err, sd_err, sd_abs, abs(half / half_ref - 1), abs(asum / asum_ref - 1),
             float((s_err / bound).max())))
    assert np.all(np.isfinite(s)) and np.isfinite(half) and np.isfinite(asum)
    assert np.all(np.abs(mu - mu_ref) <= TIGHT * np.abs(mu_ref))
    assert sd_err <= TIGHT and sd_abs <= 1e-5
    assert half == pytest.approx(half_ref, rel=TIGHT)
    assert asum == pytest.approx(asum_ref, rel=TIGHT)
    assert np.all(s_err <= bound), float((s_err / bound).max())
    assert np.array_equal(mu, again[0]) and np.array_equal(sd, again[1])
    assert half == half2 and asum == asum2 and np.array_equal(s, s2)
    # --- the blob's own statistics as targets: exactly nothing
    d_own_mu, d_own_sd = eng.to_device(mu), eng.to_device(sd)
    s0, half0, asum0 = _op(eng, d_feat, c, h, w, d_own_mu, d_own_sd)
    assert half0 == 0 and asum0 == 0 and not s0.any()
    for arr in (d_feat, d_mu, d_sd, d_own_mu, d_own_sd):
        arr.free()


def test_stat_kernels_on_a_misaligned_gradient_array():
    """S at an address that is not F's modulo 16 bytes: the scalar form of the gradient pass."""
    eng = gpu_engine()
    c, h, w = 8, 19, 23
    feat, MU, SD = _blob(c, h, w)
    _, s_ref, asum_ref, _ = stat_ref.stat_terms(feat, MU, SD)
    d_feat, d_mu, d_sd = eng.to_device(feat), eng.to_device(MU), eng.to_device(SD)
    room = eng.empty((c * h * w + 4,))
    from style_transfer_amd.engine import DeviceArray
    shifted = DeviceArray.from_pointer(eng, room.ptr + 4, (c, h, w), owner=room)
    out = (ctypes.c_double * 2)()
    lib.call('stx_op_stat_terms', eng.handle, d_feat.ptr, c, h, w, d_mu.ptr, d_sd.ptr, shifted.ptr, out)
    s = shifted.get()
    assert max_rel(s, s_ref) <= TIGHT and out[1] == pytest.approx(asum_ref, rel=TIGHT)
    for arr in (d_feat, d_mu, d_sd, room):
        arr.free()


# --------------------------------------------------------------------------------- the tile path
SL = ['conv1_1', 'conv2_1', 'conv3_1']
SW = {l: 1 / 3 for l in SL}
LW = {'conv2_1': 1.5}
FRAME = (128, 128)
# the statistics layers: conv2_1 carries a Gram term too (two style terms: stand-alone injection); the other
# one is tapped by nothing else -- conv2_2 feeds a pooling layer, conv3_2 a convolution (the fused epilogue)
CASES = {'pool': (['conv3_2'], ['conv2_1', 'conv2_2']), 'conv': (['conv3_3'], ['conv2_1', 'conv3_2'])}
STAT_W = {'conv2_1': 0.7, 'conv2_2': 1.3, 'conv3_2': 1.3}


@functools.lru_cache(maxsize=None)
def _scene(case):
    """Oracle with targets of a 128 x 128 frame, computed once."""
    cl, stat_layers = CASES[case]
    net = builtin_net('vgg19')
    om = stat_ref.StatOracleModel(net.as_dicts(), synthetic_weights(net.as_dicts(), 0))
    rng = np.random.RandomState(13)
    full = rng.uniform(-110, 120, (3,) + FRAME).astype(np.float32)
    style = rng.uniform(-110, 120, (3, 40, 44)).astype(np.float32)
    om.styles = [om.style_grams([style], SL, 512)]
    om.contents = [om.prepare_features(full, cl, 512)]
    feats = om.features_tile(style, stat_layers)
    targets = {}
    for layer in stat_layers:
        mu, sd = stat_ref.feature_stats(feats[layer])
        targets[layer] = (mu.astype(np.float32), sd.astype(np.float32))
    return om, full, cl, {l: 0.05 for l in cl}, targets


def _arm(eng, om, targets):
    eng.set_contents_and_styles(om.contents, om.styles)
    eng.set_stat_targets(targets, STAT_W)
    om.stat_targets = {l: (np.float64(m), np.float64(s)) for l, (m, s) in targets.items()}
    om.stat_weights = dict(STAT_W)


def _tile(full, th, tw, start, roll):
    rolled = np.roll(full, (roll[0], roll[1]), axis=(-1, -2))
    return np.ascontiguousarray(rolled[:, start[0]:start[0] + th, start[1]:start[1] + tw])


@pytest.mark.parametrize('case,th,tw,start,roll', [('pool', 64, 48, (0, 0), (0, 0)),
                                                   ('conv', 37, 53, (64, 32), (-24, 40))])
def test_stat_tile_against_the_oracle(case, th, tw, start, roll):
    """The evaluation with statistics targets on two layers is the evaluation without them plus the term
    (float64, from the oracle's blobs, through the oracle's backward pass): tests/gpu_helpers.check_tile's
    bounds on the loss and on the image gradient."""
    om, full, cl, cw, targets = _scene(case)
    eng = gpu_engine()
    tile = _tile(full, th, tw, start, roll)
    eng.set_contents_and_styles(om.contents, om.styles)
    plain_loss, plain_grad = eng.sc_grad_tile(tile, start, roll, cl, SL, LW, cw, SW)
    _arm(eng, om, targets)
    try:
        loss, grad = eng.sc_grad_tile(tile, start, roll, cl, SL, LW, cw, SW)
        alone, _ = eng.sc_grad_tile(tile, start, roll, [], [], LW, {}, {})     # the statistics layers only
        deepest = om.deep_to_shallow(cl + SL + list(targets))[0]
        blobs = om.blob_names[:om.blob_names.index(deepest) + 1]
        acts = eng.features_tile(tile, blobs)
        om.roll_contents(roll)
        try:
            ref_loss, oracle_grad = om.sc_grad_tile(tile, start, cl, SL, LW, cw, SW)
            ref_acts = {b: om.net.blobs[b].data[0].copy() for b in blobs}
            same_loss, same_grad = om.sc_grad_tile(tile, start, cl, SL, LW, cw, SW, activations=acts)
            base64, _ = loss_from_activations(om, ref_acts, start, cl, SL, LW, cw, SW, np.float64)
            term64 = om.stat_loss64(ref_acts, LW)
        finally:
            om.roll_contents(-np.asarray(roll))
    finally:
        om.stat_targets, om.stat_weights = {}, {}
        eng.set_stat_targets({})
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
    print('stat tile', case, tile.shape, start, roll, stats)
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


def _untapped(eng, evaluate):
    """evaluate() with a tap list that names no layer for its statistics target alone (TileEngine adds a tap
    without flags for each): such a layer reaches the library through its target only, which adds it to the
    path with lw = 1."""
    kept, eng.primary.extra_taps['stat'] = eng.primary.extra_taps['stat'], []
    try:
        return evaluate()
    finally:
        eng.primary.extra_taps['stat'] = kept


@pytest.mark.parametrize('case', ['pool', 'conv'])
def test_a_statistics_layer_outside_the_tap_list_joins_the_path_with_layer_weight_one(case):
    """The library's own taps for the layers that only a target names: bit for bit the evaluation whose tap
    list names them without flags at layer_weight 1 -- beside content and Gram taps (conv2_1 stays tapped, as a
    Gram layer, at its own weight), and with no tap at all (n_taps = 0)."""
    om, full, cl, cw, targets = _scene(case)
    eng = gpu_engine()
    start, roll = (64, 32), (-24, 40)
    tile = _tile(full, 37, 53, start, roll)
    only = [l for l in targets if l not in SL][0]
    assert LW.get(only, 1.0) == 1.0
    eng.set_contents_and_styles(om.contents, om.styles)
    plain = eng.sc_grad_tile(tile, start, roll, cl, SL, LW, cw, SW)
    eng.set_stat_targets(targets, STAT_W)
    try:
        full_taps = lambda lw: eng.sc_grad_tile(tile, start, roll, cl, SL, lw, cw, SW)
        no_taps = lambda lw: eng.sc_grad_tile(tile, start, roll, [], [], lw, {}, {})
        assert eng._taps(cl, SL, LW, cw, SW)[1] == len(cl) + len(SL) + 1
        assert _untapped(eng, lambda: eng._taps(cl, SL, LW, cw, SW))[1] == len(cl) + len(SL)
        assert _untapped(eng, lambda: eng._taps([], [], {}, {}, {}))[1] == 0
        for evaluate, weights in ((full_taps, LW), (no_taps, {})):
            named = evaluate(weights)
            bare = _untapped(eng, lambda: evaluate(weights))
            again = _untapped(eng, lambda: evaluate(weights))
            assert np.isfinite(named[0]) and np.all(np.isfinite(named[1])) and named[1].any()
            assert bare[0] == named[0] and np.array_equal(bare[1], named[1])
            assert again[0] == bare[0] and np.array_equal(again[1], bare[1])
            # the weight is 1, not another one: the same layer named at layer_weight 2 gives another result
            doubled = evaluate(dict(weights, **{only: 2.0}))
            assert doubled[0] != named[0] and not np.array_equal(doubled[1], named[1])
        assert full_taps(LW)[0] != plain[0]
    finally:
        eng.set_stat_targets({})
    with pytest.raises(lib.StxError):       # no targets: the empty tap list is refused again
        _untapped(eng, lambda: no_taps({}))


def test_a_statistics_layer_off_the_path_is_refused_at_the_evaluation():
    """vgg19_big: conv2_1 reads conv1_2, pool1 is a dead end.  A target there does not lie on the path to a
    tapped conv2_1 -- named by a tap or not -- and is the whole path when nothing else is tapped."""
    eng = gpu_engine('vgg19_big')
    rng = np.random.RandomState(31)
    tile = rng.uniform(-110, 120, (3, 24, 20)).astype(np.float32)
    gram = rng.standard_normal((128, 128)).astype(np.float32)
    feats = eng.features_tile(tile, ['conv1_2', 'pool1'])
    on_path = {'conv1_2': (np.zeros(64, np.float32), np.ones(64, np.float32))}
    off_path = {'pool1': (np.zeros(64, np.float32), np.ones(64, np.float32))}
    assert feats['pool1'].shape == (64, 12, 10)
    style = lambda: eng.sc_grad_tile(tile, (0, 0), (0, 0), [], ['conv2_1'], {}, {}, {'conv2_1': 1.0})
    eng.set_contents_and_styles([], [{'conv2_1': gram}])
    try:
        before = style()
        eng.set_stat_targets(off_path)
        with pytest.raises(lib.StxError, match="one path.*'pool1' does not feed 'conv2_1'"):
            _untapped(eng, style)
        with pytest.raises(lib.StxError, match="one path.*'pool1' does not feed 'conv2_1'"):
            style()
        alone = _untapped(eng, lambda: eng.sc_grad_tile(tile, (0, 0), (0, 0), [], [], {}, {}, {}))
        half = stat_ref.stat_terms(feats['pool1'], *off_path['pool1'])[0]
        assert alone[0] == pytest.approx(half, rel=TIGHT) and alone[1].any()
        eng.set_stat_targets(on_path)
        moved = _untapped(eng, style)
        half = stat_ref.stat_terms(feats['conv1_2'], *on_path['conv1_2'])[0]
        assert moved[0] - before[0] == pytest.approx(half, abs=2 * TIGHT * moved[0])
        eng.set_stat_targets({})
        after = style()
        assert after[0] == before[0] and np.array_equal(after[1], before[1])
    finally:
        eng.set_stat_targets({})


def test_targets_of_the_tile_itself_change_no_bit_and_targets_are_cleared():
    from style_transfer_amd.engine import TileEngine
    from tests.gpu_helpers import require_gpu
    require_gpu()
    om, full, cl, cw, targets = _scene('conv')
    net = builtin_net('vgg19')
    eng = TileEngine(net, 0, synthetic_weights(net.as_dicts(), 0))       # no statistics were ever set on this one
    tile = _tile(full, 64, 48, (0, 0), (0, 0))
    run = lambda: eng.sc_grad_tile(tile, (0, 0), (0, 0), cl, SL, LW, cw, SW)
    eng.set_contents_and_styles(om.contents, om.styles)
    before = run()
    acts = eng.features_tile(tile, om.blob_names[:om.blob_names.index('conv3_3') + 1])
    own = {layer: eng.feature_stats(acts[layer]) for layer in targets}
    eng.set_stat_targets(own, STAT_W)
    on_target = run()
    assert on_target[0] == before[0] and np.array_equal(on_target[1], before[1])      # the term is exactly 0
    eng.set_stat_targets(targets, STAT_W)
    moved = run()
    assert moved[0] != before[0] and not np.array_equal(moved[1], before[1])
    eng.set_stat_targets({})
    cleared = run()
    assert cleared[0] == before[0] and np.array_equal(cleared[1], before[1])
    eng.set_stat_targets(targets, STAT_W)
    eng.set_contents_and_styles(om.contents, om.styles)                  # clears the statistics targets
    fresh = run()
    assert fresh[0] == before[0] and np.array_equal(fresh[1], before[1])
    # a tap list with no content, style or Deep-Dream layer is taken when statistics targets exist
    with pytest.raises(lib.StxError):
        eng.sc_grad_tile(tile, (0, 0), (0, 0), [], [], LW, {}, {})
    eng.set_stat_targets(targets, STAT_W)
    only = eng.sc_grad_tile(tile, (0, 0), (0, 0), [], [], LW, {}, {})
    assert np.isfinite(only[0]) and only[0] > 0 and only[1].any()
    # a wrong channel count is an error at the call, and so is a layer off the path at the evaluation
    with pytest.raises(lib.StxError, match='channels'):
        eng.set_stat_targets({'conv2_1': (np.zeros(64, np.float32), np.ones(64, np.float32))})
    with pytest.raises(lib.StxError):
        eng.set_stat_targets({'conv9_9': (np.zeros(64, np.float32), np.ones(64, np.float32))})
    eng.close()


def test_stat_tile_is_bit_identical_across_sum_schedules_and_runs(monkeypatch):
    om, full, cl, cw, targets = _scene('pool')
    eng = gpu_engine()
    eng.set_contents_and_styles(om.contents, om.styles)
    eng.set_stat_targets(targets, STAT_W)
    tile = _tile(full, 64, 48, (0, 0), (0, 0))
    run = lambda: eng.sc_grad_tile(tile, (0, 0), (0, 0), cl, SL, LW, cw, SW)
    first, again = run(), run()
    assert first[0] == again[0] and np.array_equal(first[1], again[1])
    monkeypatch.setenv('STX_SUMS_LATE', '0')            # in-place sums (the fixture re-reads the switches)
    in_place = run()
    monkeypatch.delenv('STX_SUMS_LATE')
    assert in_place[0] == first[0] and np.array_equal(in_place[1], first[1])
    eng.set_stat_targets({})


def test_farm_step_with_statistics_repeats_bit_identically():
    """A 96 x 80 image in 2 x 2 tiles of 48 x 40 with a roll: one TileFarm step, twice."""
    from style_transfer_amd.farm import TileFarm
    from tests.gpu_helpers import require_gpu
    require_gpu()
    om, _, cl, cw, targets = _scene('pool')
    net = builtin_net('vgg19')
    rng = np.random.RandomState(23)
    img = rng.uniform(-110, 120, (3, 96, 80)).astype(np.float32)
    farm = TileFarm(net, [0], synthetic_weights(net.as_dicts(), 0), verbose=False)
    contents = [farm.prepare_features_device(img, cl, 64, passes=1)]
    farm.set_contents_and_styles(contents, om.styles)
    d_img, d_grad = farm.master.to_device(img), farm.master.empty(img.shape)
    plain = farm.eval_sc_grad(d_img, d_grad, (8, -16), cl, SL, LW, cw, SW, 64)
    farm.set_stat_targets(targets, STAT_W)
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


def test_cli_stat_weight_without_gram_layers(tmp_path, monkeypatch, capsys):
    rng = np.random.RandomState(5)
    picture = lambda hw: Image.fromarray(np.uint8(rng.uniform(0, 255, hw + (3,))))
    picture((64, 56)).save(tmp_path / 'c.png')
    picture((48, 52)).save(tmp_path / 's.png')
    stat = _cli_run(tmp_path, monkeypatch, capsys, 'stat', ['--stat-weight', '1', '--style-layers'])
    bare = _cli_run(tmp_path, monkeypatch, capsys, 'bare', [])
    assert stat[0].shape == (64, 56, 3) and len(stat[2]) == 3 and np.all(np.isfinite(stat[2]))
    assert re.search(r'stat_weight=1\.0', stat[1]) and 'style_layers=[]' in stat[1] and 'stat_layers' not in stat[1]
    # without the option the comment names nothing of it: the reference's option names and no others
    assert 'stat_weight' not in bare[1] and 'stat_layers' not in bare[1]
    assert not np.array_equal(stat[0], bare[0]) and stat[2] != bare[2]
