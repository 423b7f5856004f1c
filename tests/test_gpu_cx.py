"""The contextual style term (--cx-weight) on the GPU: the kernels of cx.hip through stx_op_cx_terms, stx_cx_bank,
the tile path, the farm and the command line -- against tests/cx_ref.py (float64 on the same float32 inputs).

Bounds.  k*_i and i*_k are argmaxes, so the decisions are held to account first: outside the undecided set (a row
whose two best scores, a column whose two best p lie closer than 4 x the float32 restatement's largest error on the
case's inputs) kbest_out and winner_out ARE the float64 decisions, and the decisions that differ are within the cap
max(2, (N + M) / 256) that tests/test_cx_host.py holds the inputs to.  E, sum |S| and S are then compared with the
reference UNDER THE DEVICE'S DECISIONS to 4 x the error of the float32 restatement against float64 on the same
inputs, computed here: the factor is for the other order a device adds in.  The device's exp is the accurate expf;
no factor is widened.  The tile path is held as tests/test_gpu_selfsim.py holds the self-similarity term: the loss
to 1e-5 relative (tests/gpu_helpers.TIGHT), the gradient to l2_rel < 1e-2 (FLIP_L2: the decisions are discrete;
max_rel is printed and not asserted).  Every case prints its figures before it asserts (pytest -s); DESIGN.md 3.23
lists what an MI355X gave."""

import ctypes
import functools
import re

import numpy as np
import pytest
from PIL import Image

from oracle.caffe_net import synthetic_weights
from style_transfer_amd import lib
from style_transfer_amd.netspec import builtin_net
from tests import cx_ref, stat_ref
from tests.gpu_helpers import TIGHT, gpu_engine, l2_rel, loss_from_activations, max_rel

pytestmark = pytest.mark.gpu
FLIP_L2 = 1e-2


@functools.lru_cache(maxsize=None)
def _case(shape, eta):
    """Inputs and CPU figures of one op case, computed once: the float64 terms and the undecided decisions."""
    feat, B, mu = cx_ref.case_inputs(*shape)
    return feat, B, mu, cx_ref.terms(feat, B, mu, shape[3], eta), cx_ref.undecided(feat, B, mu, shape[3], eta)


def _op(eng, feat, B, mu, points, eta, decisions=True):
    """(S, k*, i*, E, sum |S|) of stx_op_cx_terms on host arrays."""
    c, h, w = feat.shape
    M, N = len(B), cx_ref.grid(h, w, points)[1]
    d_feat, d_bank, d_mu = eng.to_device(feat), eng.to_device(B), eng.to_device(mu)
    s_out = eng.empty((c, h, w))
    k_out, w_out = (eng.empty((N,), np.int32), eng.empty((M,), np.int32)) if decisions else (None, None)
    out = (ctypes.c_double * 2)()
    try:
        lib.call('stx_op_cx_terms', eng.handle, d_feat.ptr, c, h, w, points, d_bank.ptr, d_mu.ptr, M, float(eta),
                 s_out.ptr, out, k_out.ptr if decisions else None, w_out.ptr if decisions else None)
        return s_out.get(), k_out.get() if decisions else None, w_out.get() if decisions else None, out[0], out[1]
    finally:
        for arr in (d_feat, d_bank, d_mu, s_out, k_out, w_out):
            if arr is not None:
                arr.free()


def _held_under_the_devices_decisions(what, feat, B, mu, points, eta, s, kstar, winner, e, a):
    """E, sum |S| and S against the float64 terms under (kstar, winner), within 4 x the float32 restatement's error."""
    ref = cx_ref.terms(feat, B, mu, points, eta, decisions=(kstar, winner))
    r32 = cx_ref.terms32(feat, B, mu, points, eta, decisions=(kstar, winner))
    tol_e, tol_a = 4 * abs(r32.E - ref.E), 4 * abs(r32.abs_sum - ref.abs_sum)
    tol_s = 4 * float(np.abs(r32.S - ref.S).max())
    err_e, err_a, err_s = abs(e - ref.E), abs(a - ref.abs_sum), float(np.abs(s - ref.S).max())
    print('%s: E %.6g err %.2e of tol %.2e; sum|S| %.4g err %.2e of tol %.2e; S max %.2e err %.2e of tol %.2e'
          % (what, ref.E, err_e, tol_e, ref.abs_sum, err_a, tol_a, float(np.abs(ref.S).max()), err_s, tol_s))
    assert np.all(np.isfinite(s)) and np.isfinite(e) and np.isfinite(a)
    assert e >= 0
    assert err_e <= tol_e, (e, ref.E, r32.E)
    assert err_a <= tol_a, (a, ref.abs_sum, r32.abs_sum)
    assert err_s <= tol_s, (err_s, tol_s)


@pytest.mark.parametrize('shape,eta', cx_ref.OP_CASES)
def test_cx_kernels_against_float64(shape, eta):
    eng = gpu_engine()
    c, h, w, points, M = shape
    feat, B, mu, t64, (und_rows, und_cols) = _case(shape, eta)
    g, N, pos = cx_ref.grid(h, w, points)
    s, kstar, winner, e, a = _op(eng, feat, B, mu, points, eta)
    s2, kstar2, winner2, e2, a2 = _op(eng, feat, B, mu, points, eta)
    s3, _, _, e3, a3 = _op(eng, feat, B, mu, points, eta, decisions=False)
    # --- the decisions
    k_differ, w_differ = kstar != t64.kstar, winner != t64.winner
    print('C %d %dx%d points %d M %d eta %g: g %d N %d, undecided rows %d columns %d, k* differs at %d (decided: %d), '
          'i* at %d (decided: %d)' % (c, h, w, points, M, eta, g, N, int(und_rows.sum()), int(und_cols.sum()),
                                      int(k_differ.sum()), int((k_differ & ~und_rows).sum()), int(w_differ.sum()),
                                      int((w_differ & ~und_cols).sum())))
    assert kstar.shape == (N,) and winner.shape == (M,)
    assert np.all((0 <= kstar) & (kstar < M)) and np.all((0 <= winner) & (winner < N))
    assert not (k_differ & ~und_rows).any() and not (w_differ & ~und_cols).any()
    assert k_differ.sum() + w_differ.sum() <= cx_ref.undecided_cap(N, M)
    # --- the sums and S under the device's decisions
    _held_under_the_devices_decisions('  ', feat, B, mu, points, eta, s, kstar, winner, e, a)
    on_grid = np.zeros((h, w), bool)
    on_grid[pos[:, 0], pos[:, 1]] = True
    assert not s[:, ~on_grid].view(np.uint32).any()                 # exactly 0 off the grid
    assert e == e2 and a == a2 and np.array_equal(s, s2) and np.array_equal(kstar, kstar2)
    assert np.array_equal(winner, winner2)
    assert e == e3 and a == a3 and s.tobytes() == s3.tobytes()
    if N == 1 and M == 1:
        assert e == 0 and a == 0 and not s.any()


def test_identical_bank_rows_give_the_lower_k():
    """Bank rows 5 and 70 (two 64-column blocks of the score tiles) and 100 and 300 (two K slices of 128 rows of
    the gradient product) are equal, and a query is planted on each pair: its two best scores tie exactly."""
    eng = gpu_engine()
    shape, eta = (64, 9, 11, 30, 2115), 0.5
    feat, B, mu = (arr.copy() for arr in cx_ref.case_inputs(*shape))
    g, N, pos = cx_ref.grid(9, 11, 30)
    B[70], B[300] = B[5], B[100]
    for i, k in ((7, 5), (3, 100)):
        feat[:, pos[i, 0], pos[i, 1]] = mu + np.float32(3) * B[k] + np.float32(0.01) * feat[:, pos[i, 0], pos[i, 1]]
    s, kstar, winner, e, a = _op(eng, feat, B, mu, 30, eta)
    t64 = cx_ref.terms(feat, B, mu, 30, eta)
    print('tied bank rows: k* of the planted queries', kstar[7], kstar[3], 'float64', t64.kstar[7], t64.kstar[3])
    assert kstar[7] == 5 and kstar[3] == 100
    und_rows, _ = cx_ref.undecided(feat, B, mu, 30, eta)
    assert und_rows[7] and und_rows[3] and not ((kstar != t64.kstar) & ~und_rows).any()
    _held_under_the_devices_decisions('tied bank rows', feat, B, mu, 30, eta, s, kstar, winner, e, a)


def test_identical_query_columns_give_the_lower_i():
    """Grid positions 10 and 100 (two 64-row blocks) and 20 and 21 (one block) hold equal columns, each pair planted
    on a bank row: the two rows of p are equal bit for bit, and every column they own goes to the lower one."""
    eng = gpu_engine()
    shape, eta = (128, 13, 10, 4096, 1000), 0.5
    feat, B, mu = (arr.copy() for arr in cx_ref.case_inputs(*shape))
    g, N, pos = cx_ref.grid(13, 10, 4096)
    for (lo, hi), k in (((10, 100), 40), ((20, 21), 777)):
        col = mu + np.float32(3) * B[k] + np.float32(0.01) * feat[:, pos[lo, 0], pos[lo, 1]]
        feat[:, pos[lo, 0], pos[lo, 1]] = feat[:, pos[hi, 0], pos[hi, 1]] = col
    s, kstar, winner, e, a = _op(eng, feat, B, mu, 4096, eta)
    print('tied query columns: i* of the planted rows', winner[40], winner[777], 'columns owned by 10 / 20:',
          int((winner == 10).sum()), int((winner == 20).sum()))
    assert winner[40] == 10 and winner[777] == 20
    assert not (winner == 100).any() and not (winner == 21).any()
    assert kstar[10] == kstar[100] == 40 and kstar[20] == kstar[21] == 777
    _held_under_the_devices_decisions('tied query columns', feat, B, mu, 4096, eta, s, kstar, winner, e, a)


def test_skipping_the_row_blocks_that_own_no_column_changes_no_bit(monkeypatch):
    """N = 130: the columns of grid positions 64 .. 127 are copies of those of 0 .. 63, so every tie in i* goes to the
    lower row, the whole second block of 64 rows owns no column (P_i = 0) and its gradient product is skipped.  With
    STX_CX_SKIP=0 the product runs for it too: the same bytes."""
    eng = gpu_engine()
    shape, eta = (128, 13, 10, 4096, 1000), 0.5
    feat, B, mu = (arr.copy() for arr in cx_ref.case_inputs(*shape))
    g, N, pos = cx_ref.grid(13, 10, 4096)
    feat[:, pos[64:128, 0], pos[64:128, 1]] = feat[:, pos[:64, 0], pos[:64, 1]]
    s, kstar, winner, e, a = _op(eng, feat, B, mu, 4096, eta)
    monkeypatch.setenv('STX_CX_SKIP', '0')              # (the fixture re-reads the switches)
    s_all, kstar_all, winner_all, e_all, a_all = _op(eng, feat, B, mu, 4096, eta)
    monkeypatch.delenv('STX_CX_SKIP')
    owned = np.bincount(winner, minlength=N)
    print('skipped block: columns owned by rows 0..63 / 64..127 / 128..129: %d / %d / %d'
          % (owned[:64].sum(), owned[64:128].sum(), owned[128:].sum()))
    assert not owned[64:128].any() and owned[:64].any()
    assert np.array_equal(kstar[64:128], kstar[:64])
    assert s.tobytes() == s_all.tobytes() and e == e_all and a == a_all
    assert np.array_equal(kstar, kstar_all) and np.array_equal(winner, winner_all)
    assert s.any() and not s[:, pos[64:128, 0], pos[64:128, 1]].view(np.uint32).any()      # +0 there, not -0


def test_a_query_planted_on_a_bank_row():
    """One query equals a bank row after centring: a_i ~ 0 and tau_i ~ eta eps, the sharpest softmax there is."""
    eng = gpu_engine()
    shape, eta = (64, 9, 11, 30, 129), 0.5
    feat, B, mu = (arr.copy() for arr in cx_ref.case_inputs(*shape))
    g, N, pos = cx_ref.grid(9, 11, 30)
    feat[:, pos[11, 0], pos[11, 1]] = mu + np.float32(5) * B[66]
    s, kstar, winner, e, a = _op(eng, feat, B, mu, 30, eta)
    t64 = cx_ref.terms(feat, B, mu, 30, eta)
    und_rows, und_cols = cx_ref.undecided(feat, B, mu, 30, eta)
    print('planted query: 1 - s = %.3e, k* %d, i* of the row %d' % (1 - t64.s[11, 66], kstar[11], winner[66]))
    assert 1 - t64.s[11, 66] < 1e-6 and kstar[11] == 66 and winner[66] == 11
    assert not ((kstar != t64.kstar) & ~und_rows).any() and not ((winner != t64.winner) & ~und_cols).any()
    _held_under_the_devices_decisions('planted query', feat, B, mu, 30, eta, s, kstar, winner, e, a)


@pytest.mark.parametrize('M,c', [(1, 64), (70, 64), (513, 128)])
def test_cx_bank_against_float64(M, c):
    eng = gpu_engine()
    raw = cx_ref.noise((M, c), 100 + M)
    mu64, B64 = cx_ref.bank(raw)
    mu, B = np.empty(c, np.float32), np.empty((M, c), np.float32)
    lib.call('stx_cx_bank', eng.handle, raw.ctypes.data, lib.HOST, c, M, mu.ctypes.data, B.ctypes.data, lib.HOST)
    d_raw, d_mu, d_bank = eng.to_device(raw), eng.empty((c,)), eng.empty((M, c))
    lib.call('stx_cx_bank', eng.handle, d_raw.ptr, lib.DEVICE, c, M, d_mu.ptr, d_bank.ptr, lib.DEVICE)
    again_mu, again = d_mu.get(), d_bank.get()
    for arr in (d_raw, d_mu, d_bank):
        arr.free()
    err, err_mu = float(np.abs(B - B64).max()), float(np.abs(mu - mu64).max())
    print('cx bank %d x %d: rows %.2e, mu %.2e' % (M, c, err, err_mu))
    assert err <= 1e-6 and err_mu <= 1e-6 * max(1.0, float(np.abs(mu64).max()))
    if M > 1:
        assert np.all(np.abs(np.linalg.norm(np.float64(B), axis=1) - 1) <= 1e-6)
    else:
        assert not B.any()                              # one row is its own mean: a zero row
    assert B.tobytes() == again.tobytes() and mu.tobytes() == again_mu.tobytes()


def test_cx_rows_gathers_the_grid_bit_for_bit():
    eng = gpu_engine()
    feat = cx_ref.noise((64, 9, 11), 5)
    for budget in (4096, 30, 1):
        g, N, pos = cx_ref.grid(9, 11, budget)
        d_rows = eng.cx_rows(eng.to_device(feat), budget)
        rows = d_rows.get()
        d_rows.free()
        assert rows.shape == (N, 64)
        assert rows.tobytes() == np.ascontiguousarray(feat[:, pos[:, 0], pos[:, 1]].T).tobytes()


def test_cx_refusals():
    eng = gpu_engine()
    feat, B, mu = cx_ref.noise((192, 3, 3), 1), cx_ref.noise((40, 192), 2), np.zeros(192, np.float32)
    d_feat, d_bank, d_mu, s_out = eng.to_device(feat), eng.to_device(B), eng.to_device(mu), eng.empty((192, 3, 3))
    out = (ctypes.c_double * 2)()
    call = lambda c, points, M, eta: lib.call('stx_op_cx_terms', eng.handle, d_feat.ptr, c, 3, 3, points, d_bank.ptr,
                                               d_mu.ptr, M, eta, s_out.ptr, out, None, None)
    call(64, 4, 40, 0.5)
    call(128, 4096, 60, 0.1)
    # stx_cx_rows gathers in whole blocks of 64 channels: any other count is refused before a launch
    d_rows = eng.empty((9, 192))
    for c, code in ((96, -4), (3, -4), (0, -1)):
        with pytest.raises(lib.StxError) as err:
            lib.call('stx_cx_rows', eng.handle, d_feat.ptr, lib.DEVICE, c, 3, 3, 16, d_rows.ptr, lib.DEVICE)
        assert err.value.code == code, (c, err.value.code)
    with pytest.raises(lib.StxError) as err:
        lib.call('stx_cx_rows', eng.handle, d_feat.ptr, lib.DEVICE, 64, 3, 3, 0, d_rows.ptr, lib.DEVICE)
    assert err.value.code == -1
    lib.call('stx_cx_rows', eng.handle, d_feat.ptr, lib.DEVICE, 192, 3, 3, 16, d_rows.ptr, lib.DEVICE)
    d_rows.free()
    for c, points, M, eta, code in ((96, 4, 40, 0.5, -4), (64, 1, 40, 0.5, -1), (64, 4097, 40, 0.5, -1),
                                    (64, 4, 0, 0.5, -1), (64, 4, 16385, 0.5, -1), (64, 4, 40, 0.0, -1),
                                    (64, 4, 40, -1.0, -1), (64, 4, 40, float('inf'), -1), (64, 4, 40, float('nan'), -1),
                                    (64, 4096, 4097, 0.5, -4)):
        with pytest.raises(lib.StxError) as err:
            call(c, points, M, eta)
        assert err.value.code == code, (c, points, M, eta, err.value.code)
    for arr in (d_feat, d_bank, d_mu, s_out):
        arr.free()
    eng.set_contents_and_styles([], [])
    rows = cx_ref.noise((40, 256), 3)
    try:
        eng.set_cx_targets({'conv3_2': rows}, points=64)
        with pytest.raises(lib.StxError, match='channels') as err:
            eng.set_cx_targets({'conv2_1': rows}, points=64)
        assert err.value.code == -1
        with pytest.raises(lib.StxError, match='conv9_9'):
            eng.set_cx_targets({'conv9_9': rows}, points=64)
        for points, h, code in ((1, 0.5, -1), (4097, 0.5, -1), (64, 0.0, -1)):
            with pytest.raises(lib.StxError) as err:
                eng.set_cx_targets({'conv3_2': rows}, points=points, h=h)
            assert err.value.code == code
        with pytest.raises(lib.StxError, match='2\\^24') as err:      # refused at set time
            eng.set_cx_targets({'conv3_2': np.zeros((4097, 256), np.float32)}, points=4096)
        assert err.value.code == -4
    finally:
        eng.set_cx_targets({})


# --------------------------------------------------------------------------------- the tile path
SL = ['conv1_1', 'conv2_1', 'conv3_1']
SW = {l: 1 / 3 for l in SL}
LW = {'conv2_1': 1.5, 'conv3_2': 0.8}
FRAME = (128, 128)
CL = ['conv3_2']
CX_LAYERS = ['conv2_1', 'conv3_2']      # one beside a Gram tap, one beside the content term
CX_W = {'conv2_1': 1.3, 'conv3_2': 0.7}
POINTS = 100        # below every blob's pixel count here: g = 2 to 4


@functools.lru_cache(maxsize=None)
def _scene():
    """Oracle with targets of a 128 x 128 frame, computed once; the contextual banks are raw rows of a style
    picture's feature maps on a grid of at most 150 positions."""
    net = builtin_net('vgg19')
    om = cx_ref.CxOracleModel(net.as_dicts(), synthetic_weights(net.as_dicts(), 0))
    rng = np.random.RandomState(17)
    full = rng.uniform(-110, 120, (3,) + FRAME).astype(np.float32)
    style = rng.uniform(-110, 120, (3, 40, 44)).astype(np.float32)
    om.styles = [om.style_grams([style], SL, 512)]
    om.contents = [om.prepare_features(full, CL, 512)]
    feats = om.prepare_features(style, CX_LAYERS, 512)
    banks = {}
    for layer in CX_LAYERS:
        g, _, pos = cx_ref.grid(*feats[layer].shape[1:], 150)
        banks[layer] = np.ascontiguousarray(feats[layer][:, pos[:, 0], pos[:, 1]].T, np.float32)
    stats = stat_ref.feature_stats(feats['conv2_1'])
    return om, full, {l: 0.05 for l in CL}, banks, stats


def _arm(eng, om, banks):
    eng.set_contents_and_styles(om.contents, om.styles)
    eng.set_cx_targets(banks, CX_W, POINTS, 0.5)
    om.cx_banks, om.cx_weights, om.cx_points, om.cx_eta = dict(banks), dict(CX_W), POINTS, 0.5


def _tile(full, th, tw, start, roll):
    rolled = np.roll(full, (roll[0], roll[1]), axis=(-1, -2))
    return np.ascontiguousarray(rolled[:, start[0]:start[0] + th, start[1]:start[1] + tw])


def _against_the_oracle(eng, om, tile, start, roll, plain, extra_term, extra64, what):
    cl, cw = CL, {l: 0.05 for l in CL}
    plain_loss, plain_grad = plain
    loss, grad = eng.sc_grad_tile(tile, start, roll, cl, SL, LW, cw, SW)
    alone, alone_grad = eng.sc_grad_tile(tile, start, roll, [], [], LW, {}, {})        # the target layers only
    deepest = om.deep_to_shallow(cl + SL + list(om.cx_banks))[0]
    blobs = om.blob_names[:om.blob_names.index(deepest) + 1]
    acts = eng.features_tile(tile, blobs)
    om.roll_contents(roll)
    try:
        ref_loss, oracle_grad = om.sc_grad_tile(tile, start, cl, SL, LW, cw, SW, extra_term=extra_term)
        ref_acts = {b: om.net.blobs[b].data[0].copy() for b in blobs}
        same_loss, same_grad = om.sc_grad_tile(tile, start, cl, SL, LW, cw, SW, activations=acts,
                                               extra_term=extra_term)
        base64, _ = loss_from_activations(om, ref_acts, start, cl, SL, LW, cw, SW, np.float64)
        term64 = om.cx_loss64(ref_acts, LW) + extra64(ref_acts)
        _, alone_ref = om.sc_grad_tile(tile, start, [], [], LW, {}, {}, activations=acts, extra_term=extra_term)
    finally:
        om.roll_contents(-np.asarray(roll))
    stats = dict(loss=abs(loss / (base64 + term64) - 1), term=term64 / base64, oracle_loss=abs(loss / ref_loss - 1),
                 same_loss=abs(loss / same_loss - 1), term_alone=abs(alone / term64 - 1),
                 max_rel_same=max_rel(grad, same_grad), max_rel_all=max_rel(grad, oracle_grad),
                 moved=max_rel(grad, plain_grad), l2_same=l2_rel(grad, same_grad), l2=l2_rel(grad, oracle_grad),
                 l2_alone=l2_rel(alone_grad, alone_ref))
    print(what, tile.shape, start, roll, stats)
    assert np.all(np.isfinite(grad))
    assert stats['moved'] > 1e-3                              # the term is not lost in the others
    assert loss == pytest.approx(base64 + term64, rel=TIGHT), (loss, base64, term64, ref_loss, same_loss)
    assert loss - plain_loss == pytest.approx(term64, abs=2 * TIGHT * (base64 + term64))
    assert alone == pytest.approx(term64, rel=TIGHT), (alone, term64)
    assert stats['l2_same'] < FLIP_L2, stats
    assert stats['l2'] < FLIP_L2, stats
    assert stats['l2_alone'] < FLIP_L2, stats


@pytest.mark.parametrize('th,tw,start,roll', [(64, 48, (0, 0), (0, 0)), (37, 53, (64, 72), (-40, -48))])
def test_cx_tile_against_the_oracle(th, tw, start, roll):
    """The evaluation with contextual targets on two layers -- one beside a Gram tap, one beside the content term --
    is the evaluation without them plus the term (float64, from the oracle's blobs, through the oracle's backward
    pass)."""
    om, full, cw, banks, _ = _scene()
    eng = gpu_engine()
    tile = _tile(full, th, tw, start, roll)
    eng.set_contents_and_styles(om.contents, om.styles)
    plain = eng.sc_grad_tile(tile, start, roll, CL, SL, LW, cw, SW)
    _arm(eng, om, banks)
    try:
        _against_the_oracle(eng, om, tile, start, roll, plain, None, lambda acts: 0.0, 'cx tile')
    finally:
        om.cx_banks, om.cx_weights = {}, {}
        eng.set_cx_targets({})


def test_cx_beside_a_gram_tap_and_the_statistics_term_on_one_blob():
    """conv2_1 with a Gram tap, a statistics target and a contextual target: three gradient slots and two scratch
    regions of one tap."""
    om, full, cw, banks, stats = _scene()
    eng = gpu_engine()
    start, roll = (64, 72), (-40, -48)
    tile = _tile(full, 37, 53, start, roll)
    stat_w = 0.9
    mu64, sd64 = np.float64(stats[0]), np.float64(stats[1])

    def stat_term(b, feat):
        if b != 'conv2_1':
            return None
        half, S, _, _ = stat_ref.stat_terms(feat, mu64, sd64)
        return stat_w * half, stat_w * stat_ref.normalized(S)

    eng.set_contents_and_styles(om.contents, om.styles)
    plain = eng.sc_grad_tile(tile, start, roll, CL, SL, LW, cw, SW)
    _arm(eng, om, banks)
    eng.set_stat_targets({'conv2_1': stats}, {'conv2_1': stat_w})
    try:
        extra64 = lambda acts: LW['conv2_1'] * stat_w * stat_ref.stat_terms(acts['conv2_1'], mu64, sd64)[0]
        _against_the_oracle(eng, om, tile, start, roll, plain, stat_term, extra64, 'cx + stat')
    finally:
        om.cx_banks, om.cx_weights = {}, {}
        eng.set_stat_targets({})
        eng.set_cx_targets({})


def test_cx_tile_is_bit_identical_across_sum_schedules_and_cleared_targets_leave_no_trace(monkeypatch):
    om, full, cw, banks, _ = _scene()
    eng = gpu_engine()
    eng.set_contents_and_styles(om.contents, om.styles)
    tile = _tile(full, 64, 48, (0, 0), (0, 0))
    run = lambda: eng.sc_grad_tile(tile, (0, 0), (0, 0), CL, SL, LW, cw, SW)
    before = run()
    eng.set_cx_targets(banks, CX_W, POINTS, 0.5)
    first, again = run(), run()
    assert first[0] != before[0] and not np.array_equal(first[1], before[1])
    assert first[0] == again[0] and np.array_equal(first[1], again[1])
    monkeypatch.setenv('STX_SUMS_LATE', '0')            # in-place sums (the fixture re-reads the switches)
    in_place = run()
    monkeypatch.delenv('STX_SUMS_LATE')
    assert in_place[0] == first[0] and np.array_equal(in_place[1], first[1])
    eng.set_cx_targets({})
    cleared = run()
    assert cleared[0] == before[0] and np.array_equal(cleared[1], before[1])
    eng.set_cx_targets(banks, CX_W, POINTS, 0.5)
    eng.set_contents_and_styles(om.contents, om.styles)                  # clears the contextual targets
    fresh = run()
    assert fresh[0] == before[0] and np.array_equal(fresh[1], before[1])


def test_farm_step_with_cx_targets_repeats_bit_identically():
    """A 96 x 80 image in 2 x 2 tiles of 48 x 40 with a roll: one TileFarm step, twice."""
    from style_transfer_amd.farm import TileFarm
    from tests.gpu_helpers import require_gpu
    require_gpu()
    om, _, cw, banks, _ = _scene()
    net = builtin_net('vgg19')
    rng = np.random.RandomState(23)
    img = rng.uniform(-110, 120, (3, 96, 80)).astype(np.float32)
    farm = TileFarm(net, [0], synthetic_weights(net.as_dicts(), 0), verbose=False)
    contents = [farm.prepare_features_device(img, CL, 64, passes=1)]
    farm.set_contents_and_styles(contents, om.styles)
    d_img, d_grad = farm.master.to_device(img), farm.master.empty(img.shape)
    plain = farm.eval_sc_grad(d_img, d_grad, (8, -16), CL, SL, LW, cw, SW, 64)
    farm.set_cx_targets(banks, CX_W, POINTS, 0.5)
    first = farm.eval_sc_grad(d_img, d_grad, (8, -16), CL, SL, LW, cw, SW, 64)
    grad = d_grad.get()
    second = farm.eval_sc_grad(d_img, d_grad, (8, -16), CL, SL, LW, cw, SW, 64)
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
    argv = ['-ci', '../c.png', '--size', '128', '--min-size', '128', '--tile-size', '128', '--model', 'vgg19',
            '--weights', 'synthetic:0', '--devices', '0', '-oi', 'out.png'] + extra
    assert cli.main(argv) == 0
    printed = capsys.readouterr().out
    final = Image.open(where / 'out.png')
    logs = glob.glob(str(where / '*_log.csv'))
    assert len(logs) == 1
    with open(logs[0], newline='') as f:
        losses = [float(row['loss']) for row in csv.DictReader(f)]
    return np.asarray(final.convert('RGB')), final.text['Comment'], losses, printed


def _bank_rows(sizes_hw, budget):
    """Rows of the concatenated conv3_1 bank (two poolings: ceil(size / 4) a side) of style pictures of these sizes
    under a budget of ``budget`` rows each."""
    return sum(cx_ref.grid(-(-hh // 4), -(-ww // 4), budget)[1] for hh, ww in sizes_hw)


def test_cli_cx_runs_lower_the_term_and_concatenate_the_rows(tmp_path, monkeypatch, capsys):
    rng = np.random.RandomState(5)
    picture = lambda hw: Image.fromarray(np.uint8(rng.uniform(0, 255, hw + (3,))))
    picture((96, 128)).save(tmp_path / 'c.png')
    picture((96, 128)).save(tmp_path / 's.png')
    picture((64, 80)).save(tmp_path / 't.png')
    # the term alone: no Gram, the content term at weight 0, no regulariser -- the logged loss is weight E
    alone = ['--cx-weight', '1', '--cx-layers', 'conv3_1', '--style-layers', '--content-layers', 'conv3_2', '-cw', '0',
             '-tw', '0', '-pw', '0']
    one = _cli_run(tmp_path, monkeypatch, capsys, 'one', ['-si', '../s.png', '-i', '20'] + alone)
    print('20 Adam steps, E: %.6f -> %.6f' % (one[2][0], one[2][-1]))
    assert one[0].shape == (96, 128, 3) and len(one[2]) == 20 and np.all(np.isfinite(one[2]))
    assert one[2][-1] < one[2][0]
    assert re.search(r'cx_weight=1\.0', one[1]) and 'cx_points' not in one[1] and 'cx_rows' not in one[1]
    assert 'CX bank rows: conv3_1 %d\n' % _bank_rows([(96, 128)], 4096) in one[3], one[3]
    two = _cli_run(tmp_path, monkeypatch, capsys, 'two',
                   ['-si', '../s.png', '../t.png', '-i', '2', '--cx-rows', '200', '--cx-points', '300',
                    '--cx-h', '0.25'] + alone)
    both = [(96, 128), (64, 80)]
    assert _bank_rows(both, 200) == 12 * 16 + 8 * 10
    assert 'CX bank rows: conv3_1 %d\n' % _bank_rows(both, 200) in two[3], two[3]
    assert re.search(r'cx_h=0\.25', two[1]) and re.search(r'cx_rows=200', two[1])
    bare = _cli_run(tmp_path, monkeypatch, capsys, 'bare', ['-si', '../s.png', '-i', '2'])
    assert 'cx_' not in bare[1] and 'CX' not in bare[3]
