"""The self-similarity content term (--selfsim-weight) on the GPU: the kernels of selfsim.hip through
stx_op_selfsim_terms, the tile path, the farm and the command line -- against tests/selfsim_ref.py (float64 on the
same float32 inputs).

Bounds.  T_ij is the sign of a difference of two nearly equal numbers wherever result and content agree, so the
signs are held to account first: outside the undecided pairs (|d64| <= tau, tau = 4 x the largest |d32 - d64| of the
float32 restatement on the case's inputs) signs_out IS the float64 sign, and the pairs where it differs are within the
cap max(2, N^2 / 1e5) that tests/test_selfsim_host.py holds the inputs to.  E, sum |S| and S are then compared with
the reference UNDER THE DEVICE'S SIGNS (one flipped sign moves S by 9e-3 of its maximum at N = 576) to 4 x the error
of the float32 restatement against float64 on the same inputs, computed here: the factor is for the other order a
device adds in.  The tile path is held as tests/test_gpu_swd.py holds the sliced Wasserstein term: the loss to 1e-5
relative (tests/gpu_helpers.TIGHT, the project's loss bound), the gradient to l2_rel < 1e-2 (FLIP_L2: the signs are
discrete decisions; max_rel is printed and not asserted).  Every case prints its figures before it asserts
(pytest -s); DESIGN.md 3.21 lists what an MI355X gave."""

import ctypes
import functools
import re

import numpy as np
import pytest
from PIL import Image

from oracle.caffe_net import synthetic_weights
from style_transfer_amd import lib
from style_transfer_amd.netspec import builtin_net
from tests import selfsim_ref
from tests.gpu_helpers import TIGHT, gpu_engine, l2_rel, loss_from_activations, max_rel

pytestmark = pytest.mark.gpu
FLIP_L2 = 1e-2


@functools.lru_cache(maxsize=None)
def _case(c, h, w, points):
    """Inputs and CPU figures of one op case, computed once: float64 terms, tau and the undecided pairs."""
    feat, content = selfsim_ref.case_inputs(c, h, w, points)
    tau, und, _, N = selfsim_ref.undecided(feat, content, points)
    return feat, content, selfsim_ref.terms(feat, content, points), tau, und, N


def _op(eng, d_feat, d_content, c, h, w, points, signs=True):
    N = selfsim_ref.grid(h, w, points)[1]
    s_out = eng.empty((c, h, w))
    t_out = eng.empty((N, N), np.int8) if signs else None
    out = (ctypes.c_double * 2)()
    lib.call('stx_op_selfsim_terms', eng.handle, d_feat.ptr, d_content.ptr, c, h, w, points, s_out.ptr, out,
             t_out.ptr if signs else None)
    s, t = s_out.get(), t_out.get() if signs else None
    s_out.free()
    if signs:
        t_out.free()
    return s, t, out[0], out[1]


@pytest.mark.parametrize('c,h,w,points', selfsim_ref.OP_SHAPES)
def test_selfsim_kernels_against_float64(c, h, w, points):
    eng = gpu_engine()
    feat, content, (e64, s64, a64, t64, d64), tau, und, N = _case(c, h, w, points)
    g, _, pos = selfsim_ref.grid(h, w, points)
    d_feat, d_content = eng.to_device(feat), eng.to_device(content)
    s, t, e, a = _op(eng, d_feat, d_content, c, h, w, points)
    s2, t2, e2, a2 = _op(eng, d_feat, d_content, c, h, w, points)
    s3, _, e3, a3 = _op(eng, d_feat, d_content, c, h, w, points, signs=False)
    for arr in (d_feat, d_content):
        arr.free()
    # --- the signs
    differ = t != t64
    # --- the sums and S under the device's signs, against 4 x the float32 restatement's error
    e_ref, s_ref, a_ref, _, _ = selfsim_ref.terms(feat, content, points, signs=t)
    e32, s32, a32, _, _ = selfsim_ref.terms32(feat, content, points, signs=t)
    tol_e, tol_a, tol_s = 4 * abs(e32 - e_ref), 4 * abs(a32 - a_ref), 4 * float(np.abs(s32 - s_ref).max())
    err_e, err_a, err_s = abs(e - e_ref), abs(a - a_ref), float(np.abs(s - s_ref).max())
    on_grid = np.zeros((h, w), bool)
    on_grid[pos[:, 0], pos[:, 1]] = True
    print('C %d %dx%d points %d: g %d N %d, tau %.2e, undecided %d, signs differ at %d (decided: %d); E %.4g err %.2e of '
          'tol %.2e; sum|S| %.4g err %.2e of tol %.2e; S max %.2e err %.2e of tol %.2e'
          % (c, h, w, points, g, N, tau, int(und.sum()), int(differ.sum()), int((differ & ~und).sum()), e_ref, err_e,
             tol_e, a_ref, err_a, tol_a, float(np.abs(s_ref).max()), err_s, tol_s))
    assert t.shape == (N, N) and np.all(np.isin(t, (-1, 0, 1))) and not np.diag(t).any()
    assert not (differ & ~und).any()
    assert differ.sum() <= selfsim_ref.undecided_cap(N)
    assert np.all(np.isfinite(s)) and np.isfinite(e) and np.isfinite(a)
    assert 0 <= e <= 2
    assert err_e <= tol_e, (e, e_ref, e32)
    assert err_a <= tol_a, (a, a_ref, a32)
    assert err_s <= tol_s, (err_s, tol_s)
    assert not s[:, ~on_grid].view(np.uint32).any()                 # exactly 0 off the grid
    assert e == e2 and a == a2 and np.array_equal(s, s2) and np.array_equal(t, t2)
    assert e == e3 and a == a3 and np.array_equal(s, s3)
    if N == 1:
        assert e == 0 and a == 0 and not s.any()


@pytest.mark.parametrize('c,h,w,points', [(64, 9, 11, 30), (256, 24, 24, 576)])
def test_identical_inputs_give_exact_zeros(c, h, w, points):
    eng = gpu_engine()
    feat, _ = selfsim_ref.case_inputs(c, h, w, points)
    d_feat, d_same = eng.to_device(feat), eng.to_device(feat.copy())
    s, t, e, a = _op(eng, d_feat, d_same, c, h, w, points)
    for arr in (d_feat, d_same):
        arr.free()
    assert e == 0.0 and a == 0.0 and not t.any()
    assert not s.view(np.uint32).any()          # +0 everywhere: adding it changes no bit


def test_selfsim_refusals():
    eng = gpu_engine()
    feat = selfsim_ref.blob(192, 3, 3, 1)
    d_feat, s_out = eng.to_device(feat), eng.empty((192, 3, 3))
    out = (ctypes.c_double * 2)()
    call = lambda c, points: lib.call('stx_op_selfsim_terms', eng.handle, d_feat.ptr, d_feat.ptr, c, 3, 3, points,
                                      s_out.ptr, out, None)
    call(64, 4)
    call(128, 4096)
    for c, points, code in ((96, 4, -4), (64, 1, -1), (64, 4097, -1), (0, 4, -1)):
        with pytest.raises(lib.StxError) as err:
            call(c, points)
        assert err.value.code == code, (c, points, err.value.code)
    for arr in (d_feat, s_out):
        arr.free()
    # a target at a layer without a content map (of content_index 0), an unknown layer, a layer given twice is not
    # possible through a dict; points out of range
    cmap = np.zeros((256, 4, 4), np.float32)
    eng.set_contents_and_styles([{'conv3_2': cmap}], [])
    try:
        eng.set_selfsim_targets({'conv3_2': 64})
        with pytest.raises(lib.StxError, match='content map') as err:
            eng.set_selfsim_targets({'conv3_1': 64})
        assert err.value.code == -1
        with pytest.raises(lib.StxError):
            eng.set_selfsim_targets({'conv9_9': 64})
        for points in (1, 4097):
            with pytest.raises(lib.StxError) as err:
                eng.set_selfsim_targets({'conv3_2': points})
            assert err.value.code == -1
        eng.set_contents_and_styles([{}, {'conv3_2': cmap}], [])       # a map of content_index 1 only
        with pytest.raises(lib.StxError, match='content map'):
            eng.set_selfsim_targets({'conv3_2': 64})
    finally:
        eng.set_contents_and_styles([], [])


# --------------------------------------------------------------------------------- the tile path
SL = ['conv1_1', 'conv2_1', 'conv3_1']
SW = {l: 1 / 3 for l in SL}
LW = {'conv2_1': 1.5, 'conv3_2': 0.8}
FRAME = (128, 128)
# the term's layers: the content layer itself (beside the content term, named by the tap list) and one that nothing
# else taps -- conv2_2 feeds a pooling layer, conv3_2 a convolution (the fused epilogue)
CASES = {'pool': (['conv3_2'], ['conv3_2', 'conv2_2']), 'conv': (['conv3_3'], ['conv3_3', 'conv3_2'])}
SELFSIM_W = {'conv2_2': 1.3, 'conv3_2': 0.7, 'conv3_3': 0.9}
POINTS = 100        # below every blob's pixel count here: g = 2 or 3


@functools.lru_cache(maxsize=None)
def _scene(case):
    """Oracle with targets of a 128 x 128 frame, computed once; content maps at the content and the term's layers."""
    cl, layers = CASES[case]
    net = builtin_net('vgg19')
    om = selfsim_ref.SelfsimOracleModel(net.as_dicts(), synthetic_weights(net.as_dicts(), 0))
    rng = np.random.RandomState(17)
    full = rng.uniform(-110, 120, (3,) + FRAME).astype(np.float32)
    style = rng.uniform(-110, 120, (3, 40, 44)).astype(np.float32)
    om.styles = [om.style_grams([style], SL, 512)]
    om.contents = [om.prepare_features(full, list(dict.fromkeys(cl + layers)), 512)]
    return om, full, cl, {l: 0.05 for l in cl}, {l: POINTS for l in layers}


def _arm(eng, om, points):
    eng.set_contents_and_styles(om.contents, om.styles)
    eng.set_selfsim_targets(points, SELFSIM_W)
    om.selfsim_points = dict(points)
    om.selfsim_weights = dict(SELFSIM_W)


def _tile(full, th, tw, start, roll):
    rolled = np.roll(full, (roll[0], roll[1]), axis=(-1, -2))
    return np.ascontiguousarray(rolled[:, start[0]:start[0] + th, start[1]:start[1] + tw])


@pytest.mark.parametrize('case,th,tw,start,roll', [('pool', 64, 48, (0, 0), (0, 0)),
                                                   ('conv', 37, 53, (64, 72), (-40, -48))])
def test_selfsim_tile_against_the_oracle(case, th, tw, start, roll):
    """The evaluation with self-similarity targets on two layers -- one beside the content term -- is the evaluation
    without them plus the term (float64, from the oracle's blobs, through the oracle's backward pass).  The second
    tile's content window wraps in both axes: its origin in the map as it lies is (64 + 48, 72 + 40), and 112 + 37
    rows and 112 + 53 columns pass the 128 of the frame."""
    om, full, cl, cw, points = _scene(case)
    eng = gpu_engine()
    tile = _tile(full, th, tw, start, roll)
    eng.set_contents_and_styles(om.contents, om.styles)
    plain_loss, plain_grad = eng.sc_grad_tile(tile, start, roll, cl, SL, LW, cw, SW)
    _arm(eng, om, points)
    try:
        loss, grad = eng.sc_grad_tile(tile, start, roll, cl, SL, LW, cw, SW)
        alone, alone_grad = eng.sc_grad_tile(tile, start, roll, [], [], LW, {}, {})    # the term's layers only
        deepest = om.deep_to_shallow(cl + SL + list(points))[0]
        blobs = om.blob_names[:om.blob_names.index(deepest) + 1]
        acts = eng.features_tile(tile, blobs)
        om.roll_contents(roll)
        try:
            ref_loss, oracle_grad = om.sc_grad_tile(tile, start, cl, SL, LW, cw, SW)
            ref_acts = {b: om.net.blobs[b].data[0].copy() for b in blobs}
            same_loss, same_grad = om.sc_grad_tile(tile, start, cl, SL, LW, cw, SW, activations=acts)
            base64, _ = loss_from_activations(om, ref_acts, start, cl, SL, LW, cw, SW, np.float64)
            term64 = om.selfsim_loss64(ref_acts, LW, start)
            _, alone_ref = om.sc_grad_tile(tile, start, [], [], LW, {}, {}, activations=acts)
        finally:
            om.roll_contents(-np.asarray(roll))
    finally:
        om.selfsim_points, om.selfsim_weights = {}, {}
        eng.set_selfsim_targets({})
    stats = dict(loss=abs(loss / (base64 + term64) - 1), term=term64 / base64, oracle_loss=abs(loss / ref_loss - 1),
                 same_loss=abs(loss / same_loss - 1), term_alone=abs(alone / term64 - 1),
                 max_rel_same=max_rel(grad, same_grad), max_rel_all=max_rel(grad, oracle_grad),
                 moved=max_rel(grad, plain_grad), l2_same=l2_rel(grad, same_grad), l2=l2_rel(grad, oracle_grad),
                 l2_alone=l2_rel(alone_grad, alone_ref))
    print('selfsim tile', case, tile.shape, start, roll, stats)
    assert np.all(np.isfinite(grad))
    assert stats['moved'] > 1e-3                              # the term is not lost in the others
    assert loss == pytest.approx(base64 + term64, rel=TIGHT), (loss, base64, term64, ref_loss, same_loss)
    assert loss - plain_loss == pytest.approx(term64, abs=2 * TIGHT * (base64 + term64))
    assert alone == pytest.approx(term64, rel=TIGHT), (alone, term64)
    assert stats['l2_same'] < FLIP_L2, stats
    assert stats['l2'] < FLIP_L2, stats
    assert stats['l2_alone'] < FLIP_L2, stats


def _untapped(eng, evaluate):
    """evaluate() with a tap list that names no layer for its self-similarity target alone (TileEngine adds a tap
    without flags for each): such a layer reaches the library through its target only, which adds it to the path
    with lw = 1."""
    kept, eng.primary.extra_taps['selfsim'] = eng.primary.extra_taps['selfsim'], []
    try:
        return evaluate()
    finally:
        eng.primary.extra_taps['selfsim'] = kept


@pytest.mark.parametrize('case', ['pool', 'conv'])
def test_a_selfsim_layer_outside_the_tap_list_joins_the_path_with_layer_weight_one(case):
    om, full, cl, cw, points = _scene(case)
    eng = gpu_engine()
    start, roll = (64, 72), (-40, -48)
    tile = _tile(full, 37, 53, start, roll)
    only = [l for l in points if l not in cl][0]
    eng.set_contents_and_styles(om.contents, om.styles)
    plain = eng.sc_grad_tile(tile, start, roll, cl, SL, LW, cw, SW)
    eng.set_selfsim_targets({only: POINTS}, SELFSIM_W)
    try:
        full_taps = lambda lw: eng.sc_grad_tile(tile, start, roll, cl, SL, lw, cw, SW)
        no_taps = lambda lw: eng.sc_grad_tile(tile, start, roll, [], [], lw, {}, {})
        assert eng._taps(cl, SL, LW, cw, SW)[1] == len(cl) + len(SL) + 1
        assert _untapped(eng, lambda: eng._taps(cl, SL, LW, cw, SW))[1] == len(cl) + len(SL)
        for evaluate in (full_taps, no_taps):
            one = {k: v for k, v in LW.items() if k != only}        # the layer's weight left at 1
            named = evaluate(one)
            bare = _untapped(eng, lambda: evaluate(one))
            assert np.isfinite(named[0]) and np.all(np.isfinite(named[1])) and named[1].any()
            assert bare[0] == named[0] and np.array_equal(bare[1], named[1])
            # the weight is 1, not another one: the same layer named at layer_weight 2 gives another result
            doubled = evaluate(dict(one, **{only: 2.0}))
            assert doubled[0] != named[0] and not np.array_equal(doubled[1], named[1])
        assert full_taps(LW)[0] != plain[0]
    finally:
        eng.set_selfsim_targets({})
    with pytest.raises(lib.StxError):       # no targets: the empty tap list is refused again
        _untapped(eng, lambda: no_taps({}))


def test_a_selfsim_layer_off_the_path_is_refused_at_the_evaluation():
    """vgg19_big: conv2_1 reads conv1_2, pool1 is a dead end.  A target there does not lie on the path to a tapped
    conv2_1 -- named by a tap or not."""
    eng = gpu_engine('vgg19_big')
    rng = np.random.RandomState(31)
    tile = rng.uniform(-110, 120, (3, 24, 20)).astype(np.float32)
    gram = rng.standard_normal((128, 128)).astype(np.float32)
    feats = eng.features_tile(tile, ['conv1_2', 'pool1'])
    other = eng.features_tile(rng.uniform(-110, 120, (3, 24, 20)).astype(np.float32), ['conv1_2', 'pool1'])
    style = lambda: eng.sc_grad_tile(tile, (0, 0), (0, 0), [], ['conv2_1'], {}, {}, {'conv2_1': 1.0})
    eng.set_contents_and_styles([other], [{'conv2_1': gram}])
    try:
        before = style()
        eng.set_selfsim_targets({'pool1': 64})
        with pytest.raises(lib.StxError, match="one path.*'pool1' does not feed 'conv2_1'"):
            _untapped(eng, style)
        with pytest.raises(lib.StxError, match="one path.*'pool1' does not feed 'conv2_1'"):
            style()
        alone = _untapped(eng, lambda: eng.sc_grad_tile(tile, (0, 0), (0, 0), [], [], {}, {}, {}))
        half = 0.5 * selfsim_ref.energy(feats['pool1'], other['pool1'], 64)
        assert alone[0] == pytest.approx(half, rel=TIGHT) and alone[1].any()
        eng.set_selfsim_targets({'conv1_2': 64})
        moved = _untapped(eng, style)
        half = 0.5 * selfsim_ref.energy(feats['conv1_2'], other['conv1_2'], 64)
        assert moved[0] - before[0] == pytest.approx(half, abs=2 * TIGHT * moved[0])
        eng.set_selfsim_targets({})
        after = style()
        assert after[0] == before[0] and np.array_equal(after[1], before[1])
    finally:
        eng.set_contents_and_styles([], [])


def test_the_content_pictures_own_tile_changes_no_bit_and_targets_are_cleared():
    """A tile whose blobs ARE the content maps' windows -- the maps are the tile's own feature maps -- adds exactly 0
    to the loss and to the gradient; a content map that no content tap and no target names changes nothing either;
    stx_set_contents_and_styles clears the targets."""
    from style_transfer_amd.engine import TileEngine
    from tests.gpu_helpers import require_gpu
    require_gpu()
    om, full, cl, cw, points = _scene('conv')
    net = builtin_net('vgg19')
    eng = TileEngine(net, 0, synthetic_weights(net.as_dicts(), 0))     # no such target was ever set on this one
    tile = _tile(full, 64, 48, (0, 0), (0, 0))
    run = lambda: eng.sc_grad_tile(tile, (0, 0), (0, 0), cl, SL, LW, cw, SW)
    layers = list(dict.fromkeys(cl + list(points)))
    own = eng.features_tile(tile, layers)
    eng.set_contents_and_styles([{l: own[l] for l in cl}], om.styles)
    before = run()
    eng.set_contents_and_styles([own], om.styles)       # more maps than content taps: nothing names the others
    unnamed = run()
    assert unnamed[0] == before[0] and np.array_equal(unnamed[1], before[1])
    eng.set_selfsim_targets(points, SELFSIM_W)
    on_target = run()
    assert on_target[0] == before[0] and np.array_equal(on_target[1], before[1])      # the term is exactly 0
    eng.set_contents_and_styles(om.contents, om.styles)                  # other maps; clears the targets
    cleared = run()
    eng.set_selfsim_targets(points, SELFSIM_W)
    moved = run()
    assert moved[0] != cleared[0] and not np.array_equal(moved[1], cleared[1])
    again = run()
    assert again[0] == moved[0] and np.array_equal(again[1], moved[1])
    eng.set_selfsim_targets({})
    off = run()
    assert off[0] == cleared[0] and np.array_equal(off[1], cleared[1])
    eng.set_selfsim_targets(points, SELFSIM_W)
    eng.set_contents_and_styles(om.contents, om.styles)                  # clears the targets
    fresh = run()
    assert fresh[0] == cleared[0] and np.array_equal(fresh[1], cleared[1])
    # a tap list with no content, style or Deep-Dream layer is taken when targets exist
    with pytest.raises(lib.StxError):
        eng.sc_grad_tile(tile, (0, 0), (0, 0), [], [], LW, {}, {})
    eng.set_selfsim_targets(points, SELFSIM_W)
    only = eng.sc_grad_tile(tile, (0, 0), (0, 0), [], [], LW, {}, {})
    assert np.isfinite(only[0]) and only[0] > 0 and only[1].any()
    eng.close()


def test_selfsim_tile_is_bit_identical_across_sum_schedules(monkeypatch):
    om, full, cl, cw, points = _scene('pool')
    eng = gpu_engine()
    eng.set_contents_and_styles(om.contents, om.styles)
    eng.set_selfsim_targets(points, SELFSIM_W)
    tile = _tile(full, 64, 48, (0, 0), (0, 0))
    run = lambda: eng.sc_grad_tile(tile, (0, 0), (0, 0), cl, SL, LW, cw, SW)
    first = run()
    monkeypatch.setenv('STX_SUMS_LATE', '0')            # in-place sums (the fixture re-reads the switches)
    in_place = run()
    monkeypatch.delenv('STX_SUMS_LATE')
    assert in_place[0] == first[0] and np.array_equal(in_place[1], first[1])
    eng.set_selfsim_targets({})


def test_farm_step_with_selfsim_targets_repeats_bit_identically():
    """A 96 x 80 image in 2 x 2 tiles of 48 x 40 with a roll: one TileFarm step, twice."""
    from style_transfer_amd.farm import TileFarm
    from tests.gpu_helpers import require_gpu
    require_gpu()
    om, _, cl, cw, points = _scene('pool')
    net = builtin_net('vgg19')
    rng = np.random.RandomState(23)
    img = rng.uniform(-110, 120, (3, 96, 80)).astype(np.float32)
    farm = TileFarm(net, [0], synthetic_weights(net.as_dicts(), 0), verbose=False)
    contents = [farm.prepare_features_device(img, list(points), 64, passes=1)]
    farm.set_contents_and_styles(contents, om.styles)
    d_img, d_grad = farm.master.to_device(img), farm.master.empty(img.shape)
    plain = farm.eval_sc_grad(d_img, d_grad, (8, -16), cl, SL, LW, cw, SW, 64)
    farm.set_selfsim_targets(points, SELFSIM_W)
    first = farm.eval_sc_grad(d_img, d_grad, (8, -16), cl, SL, LW, cw, SW, 64)
    grad = d_grad.get()
    second = farm.eval_sc_grad(d_img, d_grad, (8, -16), cl, SL, LW, cw, SW, 64)
    assert np.isfinite(first) and first > plain and np.all(np.isfinite(grad))
    assert first == second and np.array_equal(grad, d_grad.get())
    farm.close()


# ------------------------------------------------------------------------------ the command line
def _cli_run(tmp_path, monkeypatch, capsys, name, extra):
    from style_transfer_amd import cli
    where = tmp_path / name
    where.mkdir()
    monkeypatch.chdir(where)
    argv = ['-ci', '../c.png', '-si', '../s.png', '--size', '96', '--min-size', '64', '-i', '4', '--tile-size', '64',
            '--model', 'vgg19', '--weights', 'synthetic:0', '--devices', '0', '-oi', 'out.png'] + extra
    assert cli.main(argv) == 0
    capsys.readouterr()
    data = (where / 'out.png').read_bytes()
    return data, Image.open(where / 'out.png').text['Comment']


def _pictures(tmp_path):
    rng = np.random.RandomState(5)
    picture = lambda hw: Image.fromarray(np.uint8(rng.uniform(0, 255, hw + (3,))))
    picture((96, 84)).save(tmp_path / 'c.png')
    picture((72, 78)).save(tmp_path / 's.png')


def test_cli_selfsim_weight_twice_and_runs_without_it(tmp_path, monkeypatch, capsys):
    """--selfsim-weight 1 at --size 96 in two scales: twice, the same bytes; a run without the option names nothing
    of it and has the pixels of a run with the weight 0 (the comment differs: it names the option)."""
    _pictures(tmp_path)
    first = _cli_run(tmp_path, monkeypatch, capsys, 'ss1', ['--selfsim-weight', '1'])
    second = _cli_run(tmp_path, monkeypatch, capsys, 'ss2', ['--selfsim-weight', '1'])
    bare = _cli_run(tmp_path, monkeypatch, capsys, 'bare', [])
    off = _cli_run(tmp_path, monkeypatch, capsys, 'off', ['--selfsim-weight', '0'])
    assert first[0] == second[0]
    assert re.search(r'selfsim_weight=1\.0', first[1]) and 'selfsim_layers' not in first[1]
    assert 'selfsim' not in bare[1]
    assert first[0] != bare[0]
    assert Image.open(tmp_path / 'off' / 'out.png').tobytes() == Image.open(tmp_path / 'bare' / 'out.png').tobytes()


def test_cli_selfsim_without_content_layers_and_with_jitter(tmp_path, monkeypatch, capsys):
    """An empty --content-layers beside --selfsim-weight 1 (the term replaces the content term: its default layer
    is conv4_2) and --jitter (the maps are retaken every iteration, the term re-armed behind them) run."""
    _pictures(tmp_path)
    alone = _cli_run(tmp_path, monkeypatch, capsys, 'alone', ['--selfsim-weight', '1', '--content-layers'])
    jitter = _cli_run(tmp_path, monkeypatch, capsys, 'jitter', ['--selfsim-weight', '1', '--jitter'])
    assert 'content_layers=[]' in alone[1] and re.search(r'selfsim_weight=1\.0', alone[1])
    assert re.search(r'jitter=True', jitter[1]) and alone[0] != jitter[0]
