"""The sliced Wasserstein style term (--swd-weight) on the GPU: the kernels of swd.hip through stx_op_swd_terms
and stx_swd_target, the tile path, the farm and the command line -- against tests/swd_ref.py (float64 on the same
float32 inputs).

Bounds.  tau[d][i] = C 2^-24 sum_c |V[d][c]| |F[c][i]| is the worst error of any float32 summation order of a
projection; order statistics are 1-Lipschitz in the sup norm, so a target may be off by max_i tau[d][i] and no more.
The sort is held to account through rank_out: every row a permutation, the float64 projections non-decreasing
along it up to the two elements' tau, exactly equal projections in index order.  E / 2 and sum |S| are compared with
the reference UNDER THE GPU'S RANKS to 1e-5 relative (tests/gpu_helpers.TIGHT, the project's loss bound), S within
1e-5 max |S| + max tau (what the projection's rounding can move g by: stated, not measured).  That the GPU's ranks
are as good as the true ones is a clause of its own: E under them is no smaller than E under the true ranks (the
rearrangement inequality, tests/test_swd_host.py) and exceeds it by 1e-5 of it at most.  The tile path is held as
tests/test_gpu_stat.py holds the statistics term; its gradient to l2_rel < 1e-2 (FLIP_L2: ranks are discrete
decisions, and a near-tie moves single entries of S by one target step, so max_rel is printed and not asserted).

Observed worst values on an MI355X: targets at 0.18 of tau; up to 131 200 exact ties in a case, all in index order;
the least slack along the ranks 0 (the ties); E / 2 6.5e-8, sum |S| 5.1e-8, S at 1.4e-2 of its bound; E under the
GPU's ranks 1.1e-13 above E under the true ranks.  The tiles' loss 6.5e-8 (1.3e-7 against the oracle's own loss), the
term alone 8.9e-7, the gradient l2_rel 2.4e-4 against the oracle's own backward pass and 1.6e-4 on the GPU's
activations, max_rel 9.9e-4 and 5.6e-4.  Every case prints its figures before it asserts (pytest -s)."""

import ctypes
import functools
import re

import numpy as np
import pytest
from PIL import Image

from oracle.caffe_net import synthetic_weights
from style_transfer_amd import lib
from style_transfer_amd.config_system import swd_directions
from style_transfer_amd.netspec import builtin_net
from tests import swd_ref
from tests.gpu_helpers import TIGHT, gpu_engine, l2_rel, loss_from_activations, max_rel

pytestmark = pytest.mark.gpu
FLIP_L2 = 1e-2


@functools.lru_cache(maxsize=None)
def _case(c, h, w, d, q):
    """Inputs and float64 figures of one op case, computed once."""
    feat, V, other = swd_ref.case_inputs(c, h, w, d, q)
    return feat, V, other, swd_ref.project(feat, V), swd_ref.tau(feat, V), swd_ref.target(other, V, q), \
        swd_ref.tau(other, V)


def _op(eng, d_feat, c, h, w, d_v, d, d_tq, q, ranks=True):
    s_out = eng.empty((c, h, w))
    r_out = eng.empty((d, h * w), np.int32) if ranks else None
    out = (ctypes.c_double * 2)()
    lib.call('stx_op_swd_terms', eng.handle, d_feat.ptr, c, h, w, d_v.ptr, d, d_tq.ptr, q, s_out.ptr,
             r_out.ptr if ranks else None, out)
    s, r = s_out.get(), r_out.get() if ranks else None
    s_out.free()
    if ranks:
        r_out.free()
    return s, r, out[0], out[1]


@pytest.mark.parametrize('c,h,w,d,q', swd_ref.OP_SHAPES)
def test_swd_kernels_against_float64(c, h, w, d, q):
    eng = gpu_engine()
    feat, V, other, p64, tau, tq_ref, tau_other = _case(c, h, w, d, q)
    n = h * w
    # --- target making: from the host and from the device, the same bits; within the worst projection error
    tq = eng.swd_target(other, V, q)
    d_other = eng.to_device(other)
    tq_again = eng.swd_target(d_other, V, q)
    tq_err = np.abs(tq - tq_ref).max(axis=1) / tau_other.max(axis=1)
    # --- the term, twice
    d_feat, d_v, d_tq = eng.to_device(feat), eng.to_device(V), eng.to_device(tq)
    s, ranks, half, asum = _op(eng, d_feat, c, h, w, d_v, d, d_tq, q)
    s2, ranks2, half2, asum2 = _op(eng, d_feat, c, h, w, d_v, d, d_tq, q)
    s3, _, half3, asum3 = _op(eng, d_feat, c, h, w, d_v, d, d_tq, q, ranks=False)
    # --- the sort: permutations; non-decreasing up to tau; exact ties by index
    order = np.argsort(ranks, axis=1, kind='stable')
    is_perm = np.array_equal(np.sort(ranks, axis=1), np.broadcast_to(np.arange(n), (d, n)))
    along, tau_along = np.take_along_axis(p64, order, 1), np.take_along_axis(tau, order, 1)
    slack = (along[:, 1:] - along[:, :-1]) + (tau_along[:, 1:] + tau_along[:, :-1])
    by_value = np.lexsort((np.broadcast_to(np.arange(n), (d, n)), p64), axis=1)        # (value, index)
    v_sorted, r_sorted = np.take_along_axis(p64, by_value, 1), np.take_along_axis(ranks, by_value, 1)
    tied = v_sorted[:, 1:] == v_sorted[:, :-1]
    ties_in_order = bool(np.all(r_sorted[:, 1:][tied] > r_sorted[:, :-1][tied]))
    # --- the sums and S under the GPU's ranks; the ranks' quality
    half_ref, s_ref, asum_ref, _ = swd_ref.terms(feat, V, tq, ranks)
    e_true, e_gpu = swd_ref.rank_quality(feat, V, tq, ranks)
    bound = TIGHT * np.abs(s_ref).max() + tau.max()
    s_err = float(np.abs(s - s_ref).max())
    print('C %d %dx%d D %d Q %d: Tq %.2e of tau, ties %d, least slack %.2e, E/2 %.2e, sum|S| %.2e, S %.2e of its bound, '
          'E excess %.2e' % (c, h, w, d, q, float(tq_err.max()), int(tied.sum()), float(slack.min()) if n > 1 else 0.0,
                             abs(half / half_ref - 1), abs(asum / asum_ref - 1), s_err / bound, e_gpu / e_true - 1))
    assert np.all(np.isfinite(tq)) and np.all(np.diff(tq, axis=1) >= 0)
    assert np.all(tq_err <= 1.0), float(tq_err.max())
    assert np.array_equal(tq, tq_again)
    assert is_perm
    assert n == 1 or slack.min() >= 0
    assert ties_in_order and (n < 8 or tied.sum() >= d * (n // 4 - 1))
    assert np.all(np.isfinite(s)) and np.isfinite(half) and np.isfinite(asum)
    assert half == pytest.approx(half_ref, rel=TIGHT)
    assert asum == pytest.approx(asum_ref, rel=TIGHT)
    assert s_err <= bound, s_err / bound
    assert e_gpu >= e_true * (1 - 1e-12) and e_gpu - e_true <= TIGHT * e_true, (e_gpu, e_true)
    assert half == half2 and asum == asum2 and np.array_equal(s, s2) and np.array_equal(ranks, ranks2)
    assert half == half3 and asum == asum3 and np.array_equal(s, s3)
    # --- the blob's own sorted projections as targets (Q = n, where the library takes that many quantiles: 2 to
    # 65536): exactly nothing
    if 2 <= n <= 65536:
        own = eng.swd_target(d_feat, V, n)
        d_own = eng.to_device(own)
        s0, _, half0, asum0 = _op(eng, d_feat, c, h, w, d_v, d, d_own, n)
        d_own.free()
        assert np.allclose(own, np.sort(p64, axis=1), rtol=0, atol=float(tau.max()))
        assert half0 == 0 and asum0 == 0 and not s0.view(np.uint32).any()
    for arr in (d_feat, d_v, d_tq, d_other):
        arr.free()


def test_swd_refusals():
    eng = gpu_engine()
    feat, V, _ = swd_ref.case_inputs(8, 3, 3, 4, 8)
    d_feat, d_v, d_tq, s_out = eng.to_device(feat), eng.to_device(V), eng.to_device(np.zeros((4, 8), np.float32)), \
        eng.empty((8, 3, 3))
    out = (ctypes.c_double * 2)()
    call = lambda c, d, q: lib.call('stx_op_swd_terms', eng.handle, d_feat.ptr, c, 3, 3, d_v.ptr, d, d_tq.ptr, q,
                                    s_out.ptr, None, out)
    call(8, 4, 8)
    for c, d, q, code in ((8, 0, 8, -1), (8, 4, 1, -1), (6, 4, 8, -4), (8, 4097, 8, -4), (8, 4, 65537, -4)):
        with pytest.raises(lib.StxError) as err:
            call(c, d, q)
        assert err.value.code == code, (c, d, q, err.value.code)
    with pytest.raises(lib.StxError):
        eng.swd_target(feat, V, 1)
    with pytest.raises(lib.StxError, match='channels'):
        eng.set_swd_targets({'conv2_1': (np.zeros((4, 64), np.float32), np.zeros((4, 8), np.float32))})
    with pytest.raises(lib.StxError):
        eng.set_swd_targets({'conv9_9': (np.zeros((4, 64), np.float32), np.zeros((4, 8), np.float32))})
    with pytest.raises(lib.StxError):
        eng.set_swd_targets({'conv1_1': (np.zeros((4, 64), np.float32), np.zeros((4, 1), np.float32))})
    for arr in (d_feat, d_v, d_tq, s_out):
        arr.free()


# --------------------------------------------------------------------------------- the tile path
SL = ['conv1_1', 'conv2_1', 'conv3_1']
SW = {l: 1 / 3 for l in SL}
LW = {'conv2_1': 1.5}
FRAME = (128, 128)
# the SWD layers: conv2_1 carries a Gram term too (two style terms: stand-alone injection); the other one is tapped
# by nothing else -- conv2_2 feeds a pooling layer, conv3_2 a convolution (the fused epilogue)
CASES = {'pool': (['conv3_2'], ['conv2_1', 'conv2_2']), 'conv': (['conv3_3'], ['conv2_1', 'conv3_2'])}
SWD_W = {'conv2_1': 0.7, 'conv2_2': 1.3, 'conv3_2': 1.3}
DIRS, QUANTILES = 24, 50


@functools.lru_cache(maxsize=None)
def _scene(case):
    """Oracle with targets of a 128 x 128 frame, computed once."""
    cl, swd_layers = CASES[case]
    net = builtin_net('vgg19')
    om = swd_ref.SwdOracleModel(net.as_dicts(), synthetic_weights(net.as_dicts(), 0))
    rng = np.random.RandomState(13)
    full = rng.uniform(-110, 120, (3,) + FRAME).astype(np.float32)
    style = rng.uniform(-110, 120, (3, 40, 44)).astype(np.float32)
    om.styles = [om.style_grams([style], SL, 512)]
    om.contents = [om.prepare_features(full, cl, 512)]
    feats = om.features_tile(style, swd_layers)
    targets = {}
    for layer in swd_layers:
        V = swd_directions(3, layer, feats[layer].shape[0], DIRS)
        targets[layer] = (V, swd_ref.target(feats[layer], V, QUANTILES).astype(np.float32))
    return om, full, cl, {l: 0.05 for l in cl}, targets


def _arm(eng, om, targets):
    eng.set_contents_and_styles(om.contents, om.styles)
    eng.set_swd_targets(targets, SWD_W)
    om.swd_targets = dict(targets)
    om.swd_weights = dict(SWD_W)


def _tile(full, th, tw, start, roll):
    rolled = np.roll(full, (roll[0], roll[1]), axis=(-1, -2))
    return np.ascontiguousarray(rolled[:, start[0]:start[0] + th, start[1]:start[1] + tw])


@pytest.mark.parametrize('case,th,tw,start,roll', [('pool', 64, 48, (0, 0), (0, 0)),
                                                   ('conv', 37, 53, (64, 32), (-24, 40))])
def test_swd_tile_against_the_oracle(case, th, tw, start, roll):
    """The evaluation with sliced Wasserstein targets on two layers is the evaluation without them plus the term
    (float64, from the oracle's blobs, through the oracle's backward pass)."""
    om, full, cl, cw, targets = _scene(case)
    eng = gpu_engine()
    tile = _tile(full, th, tw, start, roll)
    eng.set_contents_and_styles(om.contents, om.styles)
    plain_loss, plain_grad = eng.sc_grad_tile(tile, start, roll, cl, SL, LW, cw, SW)
    _arm(eng, om, targets)
    try:
        loss, grad = eng.sc_grad_tile(tile, start, roll, cl, SL, LW, cw, SW)
        alone, _ = eng.sc_grad_tile(tile, start, roll, [], [], LW, {}, {})     # the SWD layers only
        deepest = om.deep_to_shallow(cl + SL + list(targets))[0]
        blobs = om.blob_names[:om.blob_names.index(deepest) + 1]
        acts = eng.features_tile(tile, blobs)
        om.roll_contents(roll)
        try:
            ref_loss, oracle_grad = om.sc_grad_tile(tile, start, cl, SL, LW, cw, SW)
            ref_acts = {b: om.net.blobs[b].data[0].copy() for b in blobs}
            same_loss, same_grad = om.sc_grad_tile(tile, start, cl, SL, LW, cw, SW, activations=acts)
            base64, _ = loss_from_activations(om, ref_acts, start, cl, SL, LW, cw, SW, np.float64)
            term64 = om.swd_loss64(ref_acts, LW)
        finally:
            om.roll_contents(-np.asarray(roll))
    finally:
        om.swd_targets, om.swd_weights = {}, {}
        eng.set_swd_targets({})
    stats = dict(loss=abs(loss / (base64 + term64) - 1), term=term64 / base64, oracle_loss=abs(loss / ref_loss - 1),
                 same_loss=abs(loss / same_loss - 1), term_alone=abs(alone / term64 - 1),
                 max_rel_same=max_rel(grad, same_grad), max_rel_all=max_rel(grad, oracle_grad),
                 moved=max_rel(grad, plain_grad), l2_same=l2_rel(grad, same_grad), l2=l2_rel(grad, oracle_grad))
    print('swd tile', case, tile.shape, start, roll, stats)
    assert np.all(np.isfinite(grad))
    assert stats['moved'] > 1e-3                              # the term is not lost in the others
    assert loss == pytest.approx(base64 + term64, rel=TIGHT), (loss, base64, term64, ref_loss, same_loss)
    assert loss - plain_loss == pytest.approx(term64, abs=2 * TIGHT * (base64 + term64))
    assert alone == pytest.approx(term64, rel=TIGHT), (alone, term64)
    assert stats['l2_same'] < FLIP_L2, stats
    assert stats['l2'] < FLIP_L2, stats


def _untapped(eng, evaluate):
    """evaluate() with a tap list that names no layer for its SWD target alone (TileEngine adds a tap without flags
    for each): such a layer reaches the library through its target only, which adds it to the path with lw = 1."""
    kept, eng.primary.extra_taps['swd'] = eng.primary.extra_taps['swd'], []
    try:
        return evaluate()
    finally:
        eng.primary.extra_taps['swd'] = kept


@pytest.mark.parametrize('case', ['pool', 'conv'])
def test_an_swd_layer_outside_the_tap_list_joins_the_path_with_layer_weight_one(case):
    om, full, cl, cw, targets = _scene(case)
    eng = gpu_engine()
    start, roll = (64, 32), (-24, 40)
    tile = _tile(full, 37, 53, start, roll)
    only = [l for l in targets if l not in SL][0]
    assert LW.get(only, 1.0) == 1.0
    eng.set_contents_and_styles(om.contents, om.styles)
    plain = eng.sc_grad_tile(tile, start, roll, cl, SL, LW, cw, SW)
    eng.set_swd_targets(targets, SWD_W)
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
        eng.set_swd_targets({})
    with pytest.raises(lib.StxError):       # no targets: the empty tap list is refused again
        _untapped(eng, lambda: no_taps({}))


def test_an_swd_layer_off_the_path_is_refused_at_the_evaluation():
    """vgg19_big: conv2_1 reads conv1_2, pool1 is a dead end.  A target there does not lie on the path to a
    tapped conv2_1 -- named by a tap or not -- and is the whole path when nothing else is tapped."""
    eng = gpu_engine('vgg19_big')
    rng = np.random.RandomState(31)
    tile = rng.uniform(-110, 120, (3, 24, 20)).astype(np.float32)
    gram = rng.standard_normal((128, 128)).astype(np.float32)
    feats = eng.features_tile(tile, ['conv1_2', 'pool1'])
    V = swd_directions(1, 'pool1', 64, 16)
    tq = np.sort(rng.standard_normal((16, 32)).astype(np.float32), axis=1)
    on_path, off_path = {'conv1_2': (V, tq)}, {'pool1': (V, tq)}
    style = lambda: eng.sc_grad_tile(tile, (0, 0), (0, 0), [], ['conv2_1'], {}, {}, {'conv2_1': 1.0})
    eng.set_contents_and_styles([], [{'conv2_1': gram}])
    try:
        before = style()
        eng.set_swd_targets(off_path)
        with pytest.raises(lib.StxError, match="one path.*'pool1' does not feed 'conv2_1'"):
            _untapped(eng, style)
        with pytest.raises(lib.StxError, match="one path.*'pool1' does not feed 'conv2_1'"):
            style()
        alone = _untapped(eng, lambda: eng.sc_grad_tile(tile, (0, 0), (0, 0), [], [], {}, {}, {}))
        assert alone[0] == pytest.approx(swd_ref.half_e(feats['pool1'], V, tq), rel=TIGHT) and alone[1].any()
        eng.set_swd_targets(on_path)
        moved = _untapped(eng, style)
        half = swd_ref.half_e(feats['conv1_2'], V, tq)
        assert moved[0] - before[0] == pytest.approx(half, abs=2 * TIGHT * moved[0])
        eng.set_swd_targets({})
        after = style()
        assert after[0] == before[0] and np.array_equal(after[1], before[1])
    finally:
        eng.set_swd_targets({})


def test_targets_of_the_tile_itself_change_no_bit_and_targets_are_cleared():
    from style_transfer_amd.engine import TileEngine
    from tests.gpu_helpers import require_gpu
    require_gpu()
    om, full, cl, cw, targets = _scene('conv')
    net = builtin_net('vgg19')
    eng = TileEngine(net, 0, synthetic_weights(net.as_dicts(), 0))       # no SWD target was ever set on this one
    tile = _tile(full, 64, 48, (0, 0), (0, 0))
    run = lambda: eng.sc_grad_tile(tile, (0, 0), (0, 0), cl, SL, LW, cw, SW)
    eng.set_contents_and_styles(om.contents, om.styles)
    before = run()
    acts = eng.features_tile(tile, om.blob_names[:om.blob_names.index('conv3_3') + 1])
    own = {layer: (V, eng.swd_target(acts[layer], V, acts[layer][0].size)) for layer, (V, _) in targets.items()}
    eng.set_swd_targets(own, SWD_W)
    on_target = run()
    assert on_target[0] == before[0] and np.array_equal(on_target[1], before[1])      # the term is exactly 0
    eng.set_swd_targets(targets, SWD_W)
    moved = run()
    assert moved[0] != before[0] and not np.array_equal(moved[1], before[1])
    again = run()
    assert again[0] == moved[0] and np.array_equal(again[1], moved[1])
    eng.set_swd_targets({})
    cleared = run()
    assert cleared[0] == before[0] and np.array_equal(cleared[1], before[1])
    eng.set_swd_targets(targets, SWD_W)
    eng.set_contents_and_styles(om.contents, om.styles)                  # clears the SWD targets
    fresh = run()
    assert fresh[0] == before[0] and np.array_equal(fresh[1], before[1])
    # a tap list with no content, style or Deep-Dream layer is taken when SWD targets exist
    with pytest.raises(lib.StxError):
        eng.sc_grad_tile(tile, (0, 0), (0, 0), [], [], LW, {}, {})
    eng.set_swd_targets(targets, SWD_W)
    only = eng.sc_grad_tile(tile, (0, 0), (0, 0), [], [], LW, {}, {})
    assert np.isfinite(only[0]) and only[0] > 0 and only[1].any()
    eng.close()


def test_swd_tile_is_bit_identical_across_sum_schedules(monkeypatch):
    om, full, cl, cw, targets = _scene('pool')
    eng = gpu_engine()
    eng.set_contents_and_styles(om.contents, om.styles)
    eng.set_swd_targets(targets, SWD_W)
    tile = _tile(full, 64, 48, (0, 0), (0, 0))
    run = lambda: eng.sc_grad_tile(tile, (0, 0), (0, 0), cl, SL, LW, cw, SW)
    first = run()
    monkeypatch.setenv('STX_SUMS_LATE', '0')            # in-place sums (the fixture re-reads the switches)
    in_place = run()
    monkeypatch.delenv('STX_SUMS_LATE')
    assert in_place[0] == first[0] and np.array_equal(in_place[1], first[1])
    eng.set_swd_targets({})


def test_farm_step_with_swd_targets_repeats_bit_identically():
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
    farm.set_swd_targets(targets, SWD_W)
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


def test_cli_swd_weight_alone_twice_and_a_run_without_it(tmp_path, monkeypatch, capsys):
    """--swd-weight 1 --style-layers (the term alone) at --size 96 in two scales: twice, the same bytes; without
    the option the comment names nothing of it."""
    rng = np.random.RandomState(5)
    picture = lambda hw: Image.fromarray(np.uint8(rng.uniform(0, 255, hw + (3,))))
    picture((96, 84)).save(tmp_path / 'c.png')
    picture((72, 78)).save(tmp_path / 's.png')
    first = _cli_run(tmp_path, monkeypatch, capsys, 'swd1', ['--swd-weight', '1', '--style-layers'])
    second = _cli_run(tmp_path, monkeypatch, capsys, 'swd2', ['--swd-weight', '1', '--style-layers'])
    bare = _cli_run(tmp_path, monkeypatch, capsys, 'bare', [])
    assert first[0] == second[0]
    assert re.search(r'swd_weight=1\.0', first[1]) and 'style_layers=[]' in first[1] and 'swd_layers' not in first[1]
    assert 'swd' not in bare[1]
    assert first[0] != bare[0]
