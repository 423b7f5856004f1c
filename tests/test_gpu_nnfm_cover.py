"""The coverage part of the nearest-neighbour term (--nnfm-cover) on the GPU: the reverse search
(nnfm_search_kernel<false, 1> with the operands exchanged), the inverted index and the segmented gradient through
stx_op_nnfm_cover_terms, the tile path and the command line -- against tests/nnfm_cover_ref.py (float64 on the same
float32 inputs).  The bounds are those of tests/test_gpu_nnfm_knn.py, applied in the same way; no number here is new.

Bounds.
  * Winners.  tau = 4 x the worst |emulated score - float64 score| of the case with the operands in the reverse roles
    (``_reverse_search_error``: nnfm_ref.emulated_scores with the columns' pieces on the bank side of every product).
    A bank row whose float64 best and second-best columns lie more than 1e-3 apart is CLEAR: the GPU's winner is the
    float64 one.  Every other row's winner scores within tau of the float64 maximum.
  * Planted inputs (column i = alpha_i (b_{p_i} + 1e-3 of unit noise), distinct p_i, alpha_i in [1e-2, 1e3], as many
    as fit; the other columns random): the planted rows are clear -- asserted before the GPU is asked, the case drawn
    again otherwise -- and win their columns.
  * Exact ties (a column three times across the 128-column blocks, which are the slices of the 200-row bank and the
    steps of one workgroup's walk for the 32 769-row bank): the lowest i.
  * E, E_cov, sum |S| (relative) and S (of max |S_ref|) to 1e-5 (TIGHT) against the reference AT THE GPU'S OWN INDEX
    SETS AND WINNERS, wherever 1 - c is not a cancelled difference: random inputs and rows turned away from their
    columns by half a unit of noise.  Planted inputs print their figures and hold the winners only, as the k-nearest
    tests do (c = 1 - 5e-7 there: float32's 1 - c has no digit in common with float64's).
  * The tile path: loss and gradient to TIGHT of the oracle's backward pass on the GPU's activations fed the
    reference's S at the GPU's index sets and winners (the op call on the tile's blob gives them).

Observed worst values on an MI355X.  Winners, over the 208 calls that check them (159 037 rows, 156 179 of them
clear): tau at most 1.04e-6, no row off the float64 winner, worst shortfall 0.  Values, over the 110 held calls (48
random shapes x 2 factors x 2 K, the two paths of the reverse search, the list of 1000, the lists of one, the zeros):
E 1.9e-7, E_cov 1.6e-7, sum |S| 1.7e-7, S 2.1e-6 of its maximum (the list of 1000 at factor 2).  Planted inputs (96
calls, printed only): E 1.1e-2, E_cov 0.76 (E_cov itself is 1e-6 there), sum |S| 6.8e-6, S 4.7e-4.  The 45 x 47 map
against 64 rows runs 17 slices, 15 columns against 32 769 rows run one (257 query blocks; longest list 2589); the tied
rows take the columns 5, 127 and 100 on both paths (6 slices and 1).  Tiles (110 bank rows, longest list 5, 177 of
the 256 columns without a row): loss 1.1e-7 .. 4.4e-7, gradient 6.2e-7 .. 9.9e-7 of its maximum.  The command-line
run lowers E / 2 from 0.087712 to 0.057401 in 20 Adam steps.  The whole file: 65 cases in 4.2 s, the slowest 1.1 s
(the ties against 32 769 rows, most of it the float64 reference).  Every case prints its figures before it asserts
(pytest -s)."""

import ctypes
import functools
import hashlib
import json
import os
import pickle
import re
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

from oracle.caffe_net import synthetic_weights
from style_transfer_amd import lib
from style_transfer_amd.netspec import builtin_net
from tests import nnfm_cover_ref as ref
from tests import nnfm_knn_ref, nnfm_ref
from tests.gpu_helpers import TIGHT, gpu_engine, max_rel

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHANNELS = [64, 256]
MAPS = [(1, 1), (3, 5), (3, 43)]        # n = 1; 15; 129: two 128-row blocks of the reverse search's bank side
ROWS = [3, 31, 129, 1000]               # one ragged query block of the reverse search; a block boundary; many blocks
COVERS = [0.5, 2.0]
KS = [1, 3]
ERR_ARG = -1


def _unit_rows(rng, m, width):
    b = rng.standard_normal((m, width))
    return (b / np.linalg.norm(b, axis=1, keepdims=True)).astype(np.float32)


def _op(eng, feat, bank, k, cover, profile=False):
    """(S, J [k, n], winner [M], E, sum |S|, E_cov[, the reverse search's slice count]) of stx_op_nnfm_cover_terms."""
    c, h, w = feat.shape
    m = bank.shape[0]
    d_feat, d_bank = eng.to_device(feat), eng.to_device(bank)
    s_out = eng.empty((c, h, w))
    idx = eng.empty((k, h * w), np.int32)
    win = eng.to_device(np.full((m,), -7, np.int32), np.int32)
    out = (ctypes.c_double * 3)(-1.0, -1.0, -1.0)
    if profile:
        eng.profile(True)
    try:
        lib.call('stx_op_nnfm_cover_terms', eng.handle, d_feat.ptr, c, h, w, 1, k, float(cover), d_bank.ptr, m,
                 s_out.ptr, idx.ptr, win.ptr, out)
        result = (s_out.get(), idx.get().astype(np.int64), win.get().astype(np.int64), out[0], out[1], out[2])
        if profile:
            labels = [row[0] for row in eng.profile_read()]
            slices = [int(f.group(1)) for f in (re.fullmatch(r'nnfm cover search op x(\d+)', l) for l in labels) if f]
            assert len(slices) == 1, labels
            assert 'nnfm cover index op' in labels and 'nnfm cover grad op' in labels, labels
            result += (slices[0],)
    finally:
        if profile:
            eng.profile(False)
        for arr in (d_feat, d_bank, s_out, idx, win):
            arr.free()
    return result


def _reverse_search_error(feat, bank):
    """nnfm_ref.search_error with the operands in the reverse roles: the same pieces -- of f (1/r 2^13) and of b
    2^13 --, the same three products per 16-channel step, smallest first, with the columns' pieces where the
    forward search has the bank's (lo of the bank side times hi of the query side first)."""
    f = np.asarray(feat, np.float32).reshape(feat.shape[0], -1).T
    r = np.sqrt((f.astype(np.float64) ** 2).sum(axis=1))
    inv = np.divide(1.0, r, out=np.zeros_like(r), where=r > 0).astype(np.float32)
    xh, xl = nnfm_ref._split((f * (inv * np.float32(nnfm_ref.SCALE))[:, None]).astype(np.float32))
    bh, bl = nnfm_ref._split(np.asarray(bank, np.float32) * np.float32(nnfm_ref.SCALE))
    acc = np.zeros((f.shape[0], bh.shape[0]), np.float32)
    for k in range(0, f.shape[1], 16):
        s = slice(k, k + 16)
        for side, query in ((xl, bh), (xh, bl), (xh, bh)):
            acc = (acc.astype(np.float64) + side[:, s] @ query[:, s].T).astype(np.float32)
    return float(np.abs(acc.astype(np.float64) / nnfm_ref.SCALE ** 2 - nnfm_ref.scores64(feat, bank)).max())


def _clear_rows(scores):
    """Per bank row: the float64 best and second-best columns lie more than 1e-3 apart (one column: clear)."""
    if scores.shape[0] == 1:
        return np.ones(scores.shape[1], bool)
    top = -np.partition(-scores, 1, axis=0)[:2]
    return top[0] - top[1] > 1e-3


def _check_winners(tag, feat, bank, winner, tau=None):
    scores = nnfm_ref.scores64(feat, bank)              # [n, M]
    n, m = scores.shape
    assert winner.shape == (m,) and winner.min() >= 0 and winner.max() < n, tag
    tau = 4 * _reverse_search_error(feat, bank) if tau is None else tau
    clear = _clear_rows(scores)
    best = ref.winners(feat, bank)
    short = scores.max(axis=0) - scores[winner, np.arange(m)]
    print('%s winners: tau %.2e, %d of %d rows clear, %d rows off the float64 winner, worst shortfall %.2e'
          % (tag, tau, np.count_nonzero(clear), m, np.count_nonzero(winner != best), short.max()))
    assert np.array_equal(winner[clear], best[clear]), (tag, np.flatnonzero(winner != best)[:8])
    assert np.all(short <= tau), tag
    return clear


def _held_at_own(tag, feat, bank, got, cover, hold=True):
    s, J, winner, e, asum, e_cov = got[:6]
    e_ref, s_ref, asum_ref, e_cov_ref = ref.terms_at(feat, bank, J, winner, cover)
    errs = (abs(e / e_ref - 1), abs(e_cov / e_cov_ref - 1), abs(asum / asum_ref - 1), max_rel(s, s_ref))
    lens = np.bincount(winner, minlength=feat.shape[1] * feat.shape[2])
    print('%s: E %.6g (%.2e), E_cov %.6g (%.2e), sum|S| %.6g (%.2e), S %.2e of max; longest list %d, %d empty'
          % (tag, e, errs[0], e_cov, errs[1], asum, errs[2], errs[3], lens.max(), np.count_nonzero(lens == 0)))
    assert np.all(np.isfinite(s)) and np.isfinite(e) and np.isfinite(asum) and np.isfinite(e_cov)
    if hold:
        assert max(errs) <= TIGHT, (tag, errs)
    return errs


def _case(eng, tag, feat, bank, hold=True, settings=None):
    """Every (cover, k): the winners, the values at the GPU's own sets, the same bytes twice."""
    tau = 4 * _reverse_search_error(feat, bank)
    first = None
    for cover, k in settings or [(cover, k) for cover in COVERS for k in KS]:
        got = _op(eng, feat, bank, k, cover)
        name = '%s cover %g K %d' % (tag, cover, k)
        _check_winners(name, feat, bank, got[2], tau)
        _held_at_own(name, feat, bank, got, cover, hold)
        again = _op(eng, feat, bank, k, cover)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got[:3], again[:3])) and got[3:] == again[3:], name
        first = first or got
        assert np.array_equal(got[2], first[2])         # the winners depend on neither the factor nor k
    return first


def _planted(rng, bank, h, w):
    """Columns alpha_i (b_{p_i} + 1e-3 of unit noise) on distinct rows p_i, as many as fit; random columns behind
    them.  (feat, p)"""
    m, c = bank.shape
    n = h * w
    cols = rng.standard_normal((n, c))
    p = rng.permutation(m)[:min(n, m)]
    noise = rng.standard_normal((len(p), c))
    noise /= np.linalg.norm(noise, axis=1, keepdims=True)
    cols[:len(p)] = 10.0 ** rng.uniform(-2, 3, (len(p), 1)) * (bank[p].astype(np.float64) + 1e-3 * noise)
    return np.ascontiguousarray(cols.T.reshape(c, h, w), np.float32), p


@pytest.mark.parametrize('m', ROWS)
@pytest.mark.parametrize('h,w', MAPS)
@pytest.mark.parametrize('c', CHANNELS)
def test_cover_kernels_against_float64(c, h, w, m):
    eng = gpu_engine()
    rng = np.random.RandomState(c + 7 * h + 13 * w + m)
    bank = _unit_rows(rng, m, c)
    feat = (rng.standard_normal((c, h, w)) * 10.0 ** rng.uniform(-2, 3, (h, w))).astype(np.float32)
    _case(eng, 'random C %d %dx%d M %d' % (c, h, w, m), feat, bank)


@pytest.mark.parametrize('m', ROWS)
@pytest.mark.parametrize('h,w', MAPS)
@pytest.mark.parametrize('c', CHANNELS)
def test_planted_rows_win_their_columns(c, h, w, m):
    eng = gpu_engine()
    rng = np.random.RandomState(1 + c + 7 * h + 13 * w + m)
    bank = _unit_rows(rng, m, c)
    for draw in range(20):
        feat, p = _planted(rng, bank, h, w)
        if np.all(_clear_rows(nnfm_ref.scores64(feat, bank))[p]):
            break
    assert np.all(_clear_rows(nnfm_ref.scores64(feat, bank))[p]), 'the planted rows are not clear'
    assert np.array_equal(ref.winners(feat, bank)[p], np.arange(len(p)))
    got = _case(eng, 'planted C %d %dx%d M %d' % (c, h, w, m), feat, bank, hold=False)
    assert np.array_equal(got[2][p], np.arange(len(p)))


@pytest.mark.parametrize('h,w,m,sliced', [(45, 47, 64, True), (3, 5, 32769, False)])
def test_both_paths_of_the_reverse_search(h, w, m, sliced):
    """2115 columns against 64 rows: one reverse query block, the columns cut into slices.  15 columns against
    32 769 rows: 257 reverse query blocks, no slicing, 8 MB of bank."""
    eng = gpu_engine()
    rng = np.random.RandomState(m)
    c = 64
    bank = _unit_rows(rng, m, c)
    feat = rng.standard_normal((c, h, w)).astype(np.float32)
    got = _op(eng, feat, bank, 3, 2.0, profile=True)
    print('reverse search %dx%d M %d: %d slices' % (h, w, m, got[6]))
    assert (got[6] > 1) == sliced
    _case(eng, 'C 64 %dx%d M %d' % (h, w, m), feat, bank, settings=[(0.5, 1), (2.0, 3)])


@pytest.mark.parametrize('m', [200, 32769])
def test_exact_ties_take_the_lowest_column(m):
    """Columns copied three times (exact multiples, so the same pieces) across the 128-column blocks of a 20 x 35
    map -- the slices for 200 rows (two reverse query blocks), the steps of one workgroup's walk for 32 769 rows (257:
    no slicing).  A bank row that is such a column's direction scores the same on all three."""
    eng = gpu_engine()
    rng = np.random.RandomState(m)
    c, h, w = 64, 20, 35
    groups = [(5, 130, 131), (127, 128, 384), (100, 300, 650)]
    cols = rng.standard_normal((h * w, c)).astype(np.float32)
    for g in groups:
        for i, shift in zip(g[1:], (3, -2)):
            cols[i] = cols[g[0]] * np.float32(2.0 ** shift)
    feat = np.ascontiguousarray(cols.T.reshape(c, h, w))
    bank = _unit_rows(rng, m, c)
    rows = [7, 150, m - 1]
    for j, g in zip(rows, groups):
        d = cols[g[0]].astype(np.float64)
        bank[j] = (d / np.linalg.norm(d)).astype(np.float32)
    scores = nnfm_ref.scores64(feat, bank)
    for j, g in zip(rows, groups):          # exactly equal on the copies, and far above every other column
        assert scores[g[0], j] == scores[g[1], j] == scores[g[2], j]
        assert np.sort(scores[:, j])[-4] < scores[g[0], j] - 1e-3
    assert list(ref.winners(feat, bank)[rows]) == [g[0] for g in groups]
    got = _op(eng, feat, bank, 1, 1.0, profile=True)
    print('ties M %d: %d slices; winners of the tied rows %s' % (m, got[6], got[2][rows]))
    assert (got[6] > 1) == (m == 200)
    assert list(got[2][rows]) == [g[0] for g in groups]
    _check_winners('ties M %d' % m, feat, bank, got[2])


def test_one_column_owns_every_row():
    """1000 rows turned away from ONE direction by half a unit of noise, and a column that holds that direction: one
    list of 1000, every other list empty."""
    eng = gpu_engine()
    rng = np.random.RandomState(77)
    c, h, w, m, at = 64, 3, 43, 1000, 70
    d = rng.standard_normal(c)
    d /= np.linalg.norm(d)
    noise = rng.standard_normal((m, c))
    rows = d + 0.5 * noise / np.linalg.norm(noise, axis=1, keepdims=True)
    bank = (rows / np.linalg.norm(rows, axis=1, keepdims=True)).astype(np.float32)
    cols = rng.standard_normal((h * w, c))
    cols[at] = 37.5 * d
    feat = np.ascontiguousarray(cols.T.reshape(c, h, w), np.float32)
    assert np.all(ref.winners(feat, bank) == at) and np.all(_clear_rows(nnfm_ref.scores64(feat, bank)))
    got = _case(eng, 'one list of 1000', feat, bank)
    assert np.all(got[2] == at)


def test_every_column_owns_one_row():
    """The bank is a permutation of the unit columns, each turned by half a unit of noise (so that 1 - c' is a
    number and not a cancelled difference): every list has one entry."""
    eng = gpu_engine()
    rng = np.random.RandomState(78)
    c, h, w = 64, 3, 43
    n = h * w
    feat = (rng.standard_normal((c, h, w)) * 10.0 ** rng.uniform(-2, 3, (h, w))).astype(np.float32)
    perm = rng.permutation(n)
    noise = rng.standard_normal((n, c))
    rows = nnfm_ref.unit_columns(feat)[0][perm] + 0.5 * noise / np.linalg.norm(noise, axis=1, keepdims=True)
    bank = (rows / np.linalg.norm(rows, axis=1, keepdims=True)).astype(np.float32)
    assert np.array_equal(ref.winners(feat, bank), perm) and np.all(_clear_rows(nnfm_ref.scores64(feat, bank)))
    got = _case(eng, 'lists of one', feat, bank)
    assert np.array_equal(got[2], perm) and np.all(np.bincount(got[2], minlength=n) == 1)


def test_zero_columns_and_zero_rows():
    """Zero bank rows go to column 0 (every score is 0), add 2 / M each and nothing to S; a zero column that wins a
    row that every live column is turned away from costs 1 - 0 and keeps S = 0."""
    eng = gpu_engine()
    rng = np.random.RandomState(79)
    c, h, w, m = 64, 3, 5, 31
    feat = np.abs(rng.standard_normal((c, h, w))).astype(np.float32)
    feat[:, 1, 2] = 0
    bank = _unit_rows(rng, m, c)
    bank[5] = -np.abs(bank[5])
    bank[9] = 0
    bank[30] = 0
    got = _case(eng, 'zeros', feat, bank, settings=[(0.5, 1), (2.0, 3)])
    assert got[2][5] == 1 * w + 2 and got[2][9] == 0 and got[2][30] == 0
    assert not got[0][:, 1, 2].any()


@pytest.mark.parametrize('k', KS)
def test_cover_0_gives_the_bytes_of_the_knn_entry_point(k):
    eng = gpu_engine()
    rng = np.random.RandomState(11 + k)
    c, h, w, m = 64, 9, 13, 150
    feat = rng.standard_normal((c, h, w)).astype(np.float32)
    bank = _unit_rows(rng, m, c)
    d_feat, d_bank = eng.to_device(feat), eng.to_device(bank)
    s_out, idx, out = eng.empty((c, h, w)), eng.empty((k, h * w), np.int32), (ctypes.c_double * 2)()
    lib.call('stx_op_nnfm_knn_terms', eng.handle, d_feat.ptr, c, h, w, 1, k, d_bank.ptr, m, s_out.ptr, idx.ptr, out)
    old = (s_out.get(), idx.get(), out[0], out[1])
    for arr in (d_feat, d_bank, s_out, idx):
        arr.free()
    new = _op(eng, feat, bank, k, 0.0)
    assert old[0].tobytes() == new[0].tobytes() and np.array_equal(old[1], new[1]) and old[2:] == new[3:5]
    assert np.all(new[2] == -7) and new[5] == -1.0          # the winners and E_cov's place are untouched
    on = _op(eng, feat, bank, k, 0.5)
    assert np.array_equal(on[1], new[1]) and on[0].tobytes() != new[0].tobytes() and on[3] > new[3]


def test_bad_arguments_leave_every_output_alone():
    eng = gpu_engine()
    feat = eng.to_device(np.ones((64, 4, 4), np.float32))
    bank = eng.to_device(np.ones((3, 64), np.float32) / 8)
    wide = eng.to_device(np.ones((3, 9 * 64), np.float32) / 24)
    s_out = eng.to_device(np.full((64, 4, 4), 7.0, np.float32))
    idx = eng.to_device(np.full((16,), 9, np.int32), np.int32)
    win = eng.to_device(np.full((3,), 9, np.int32), np.int32)
    out = (ctypes.c_double * 3)(5.0, 5.0, 5.0)
    call = lambda patch, cover, b: lib.call('stx_op_nnfm_cover_terms', eng.handle, feat.ptr, 64, 4, 4, patch, 1,
                                            float(cover), b.ptr, 3, s_out.ptr, idx.ptr, win.ptr, out)
    for patch, cover, b in ((1, -1.0, bank), (1, float('nan'), bank), (1, float('inf'), bank), (3, 1.0, wide),
                            (2, 1.0, bank)):
        with pytest.raises(lib.StxError) as err:
            call(patch, cover, b)
        assert err.value.code == ERR_ARG, (patch, cover)
    assert np.all(s_out.get() == 7.0) and np.all(idx.get() == 9) and np.all(win.get() == 9) and list(out) == [5.0] * 3
    table = (lib.NnfmCoverTarget * 1)()
    t = table[0]
    for patch, cover, b in ((1, -1.0, bank), (1, float('nan'), bank), (3, 1.0, wide)):
        t.layer, t.channels, t.patch, t.k, t.rows, t.bank, t.mem, t.weight = b'conv1_1', 64, patch, 1, 3, b.ptr, lib.DEVICE, 1.0
        t.cover = cover
        with pytest.raises(lib.StxError) as err:
            lib.call('stx_set_nnfm_cover_targets', eng.handle, table, 1)
        assert err.value.code == ERR_ARG, (patch, cover)
    call(1, 1.0, bank)          # and the same arrays in order are taken
    assert np.all(np.isfinite(s_out.get())) and np.all(win.get() < 16) and out[2] >= 0
    for arr in (feat, bank, wide, s_out, idx, win):
        arr.free()


# --------------------------------------------------------------------------------- the tile path
SL = ['conv1_1', 'conv2_1', 'conv3_1']
SW = {l: 1 / 3 for l in SL}
LW = {'conv3_1': 1.5}
NNFM_W = {'conv3_1': 0.7}
COVER = 1.0
TILE_CASES = {'alone k1': ([], 1), 'alone k3': ([], 3), 'gram k1': (SL, 1), 'gram k3': (SL, 3)}    # style layers, K


@functools.lru_cache(maxsize=None)
def _scene():
    """Oracle with targets of a 64 x 64 frame and the conv3_1 bank of a 40 x 44 style picture."""
    net = builtin_net('vgg19')
    om = ref.CoverOracleModel(net.as_dicts(), synthetic_weights(net.as_dicts(), 0))
    rng = np.random.RandomState(29)
    full = rng.uniform(-110, 120, (3, 64, 64)).astype(np.float32)
    style = rng.uniform(-110, 120, (3, 40, 44)).astype(np.float32)
    om.styles = [om.style_grams([style], SL, 512)]
    om.contents = [om.prepare_features(full, ['conv3_2'], 512)]
    feat = om.features_tile(style, ['conv3_1'])['conv3_1']
    return om, full, nnfm_ref.bank_of(feat).astype(np.float32)


def _evaluate(eng, full, bank, case):
    sl, k = TILE_CASES[case]
    eng.set_nnfm_targets({'conv3_1': bank}, NNFM_W, 1, k, COVER)
    try:
        return eng.sc_grad_tile(full, (0, 0), (0, 0), [], sl, LW, {}, SW)
    finally:
        eng.set_nnfm_targets({})


def _sums_in_place_child(scene_path, out_path):
    """In a process of its own with STX_SUMS_LATE=0: every setting's loss and gradient, as hex and a digest."""
    os.environ['STX_SUMS_LATE'] = '0'
    with open(scene_path, 'rb') as f:
        contents, styles, full, bank = pickle.load(f)
    eng = gpu_engine()
    eng.set_contents_and_styles(contents, styles)
    result = {}
    for case in TILE_CASES:
        loss, grad = _evaluate(eng, full, bank, case)
        result[case] = [float(loss).hex(), hashlib.sha256(np.ascontiguousarray(grad).tobytes()).hexdigest()]
    eng.close()
    with open(out_path, 'w') as f:
        json.dump(result, f)


@pytest.mark.parametrize('case', list(TILE_CASES))
def test_cover_tile_against_the_oracle(case):
    om, full, bank = _scene()
    sl, k = TILE_CASES[case]
    eng = gpu_engine()
    start, roll = (0, 0), (0, 0)
    eng.set_contents_and_styles(om.contents, om.styles)
    plain = eng.sc_grad_tile(full, start, roll, [], sl, LW, {}, SW) if sl else None
    loss, grad = _evaluate(eng, full, bank, case)
    again = _evaluate(eng, full, bank, case)
    blobs = om.blob_names[:om.blob_names.index('conv3_1') + 1]
    acts = eng.features_tile(full, blobs)
    blob = np.ascontiguousarray(acts['conv3_1'], np.float32)
    got = _op(eng, blob, bank, k, COVER)                # the GPU's index sets and winners
    lens = np.bincount(got[2], minlength=blob.shape[1] * blob.shape[2])
    om.nnfm_banks, om.nnfm_weights = {'conv3_1': np.float64(bank)}, dict(NNFM_W)
    om.nnfm_k, om.nnfm_index = k, {'conv3_1': got[1]}
    om.nnfm_cover, om.nnfm_winner = COVER, {'conv3_1': got[2]}
    try:
        same_loss, same_grad = om.sc_grad_tile(full, start, [], sl, LW, {}, SW, activations=acts)
        term64 = om.nnfm_loss64(acts, LW)
    finally:
        om.nnfm_banks, om.nnfm_weights, om.nnfm_index, om.nnfm_winner = {}, {}, {}, {}
        om.nnfm_k, om.nnfm_cover = 1, 0.0
    stats = dict(loss=abs(loss / same_loss - 1), term=term64, e_cov=got[5], grad=max_rel(grad, same_grad),
                 moved=max_rel(grad, plain[1]) if plain else None, longest_list=int(lens.max()),
                 empty_lists=int(np.count_nonzero(lens == 0)), rows=len(bank))
    print('nnfm cover tile', case, stats)
    assert np.all(np.isfinite(grad)) and grad.any()
    assert again[0] == loss and np.array_equal(again[1], grad)
    assert loss == pytest.approx(same_loss, rel=TIGHT), (loss, same_loss)
    if plain:
        assert loss - plain[0] == pytest.approx(term64, abs=2 * TIGHT * loss)
        assert stats['moved'] > 1e-3        # the term is not lost in the others
    else:
        assert loss == pytest.approx(term64, rel=TIGHT)
    assert stats['grad'] < TIGHT, stats


def test_cleared_targets_change_no_bit_and_the_cover_changes_the_term():
    om, full, bank = _scene()
    eng = gpu_engine()
    run = lambda: eng.sc_grad_tile(full, (0, 0), (0, 0), [], SL, LW, {}, SW)
    eng.set_contents_and_styles(om.contents, om.styles)
    before = run()
    eng.set_nnfm_targets({'conv3_1': bank}, NNFM_W, 1, 3)
    without = run()
    eng.set_nnfm_targets({'conv3_1': bank}, NNFM_W, 1, 3, COVER)
    moved = run()
    eng.set_nnfm_targets({'conv3_1': bank}, NNFM_W, 1, 3, 0.0)      # any setter replaces the whole set: no cover
    off = run()
    eng.set_nnfm_targets({'conv3_1': bank}, NNFM_W, k=3, cover=COVER)
    back = run()
    eng.set_nnfm_targets({})
    cleared = run()
    assert moved[0] > without[0] and not np.array_equal(moved[1], without[1])       # E_cov >= 0 is added
    assert off[0] == without[0] and np.array_equal(off[1], without[1])
    assert back[0] == moved[0] and np.array_equal(back[1], moved[1])
    assert cleared[0] == before[0] and np.array_equal(cleared[1], before[1])


def test_sums_in_place_give_the_same_bits(tmp_path):
    """STX_SUMS_LATE=0 in a fresh process against the default here, every setting."""
    om, full, bank = _scene()
    eng = gpu_engine()
    eng.set_contents_and_styles(om.contents, om.styles)
    here = {}
    for case in TILE_CASES:
        loss, grad = _evaluate(eng, full, bank, case)
        here[case] = [float(loss).hex(), hashlib.sha256(np.ascontiguousarray(grad).tobytes()).hexdigest()]
    scene, out = str(tmp_path / 'scene.pkl'), str(tmp_path / 'child.json')
    with open(scene, 'wb') as f:
        pickle.dump((om.contents, om.styles, full, bank), f)
    code = 'import sys; sys.path.insert(0, %r); from tests.test_gpu_nnfm_cover import _sums_in_place_child; ' \
           '_sums_in_place_child(%r, %r)' % (REPO, scene, out)
    env = {name: value for name, value in os.environ.items() if name != 'STX_SUMS_LATE'}
    proc = subprocess.run([sys.executable, '-c', code], cwd=REPO, env=env, stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT, text=True, timeout=300)
    assert proc.returncode == 0, proc.stdout[-3000:]
    with open(out) as f:
        assert json.load(f) == here


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


def test_cli_run_with_a_cover_lowers_the_term(tmp_path, monkeypatch, capsys):
    rng = np.random.RandomState(5)
    picture = lambda hw: Image.fromarray(np.uint8(rng.uniform(0, 255, hw + (3,))))
    picture((96, 128)).save(tmp_path / 'c.png')
    picture((96, 128)).save(tmp_path / 's.png')
    # the term alone: no Gram, the content term at weight 0, no regulariser -- the logged loss is weight E / 2
    alone = ['-si', '../s.png', '-i', '20', '--nnfm-weight', '1', '--nnfm-layers', 'conv3_1', '--style-layers',
             '--content-layers', 'conv3_2', '-cw', '0', '-tw', '0', '-pw', '0']
    rows = nnfm_ref.bank_rows(24, 32)
    cover = _cli_run(tmp_path, monkeypatch, capsys, 'cover', alone + ['--nnfm-cover', '1'])
    with capsys.disabled():
        print('20 Adam steps, cover 1, E / 2: %.6f -> %.6f' % (cover[2][0], cover[2][-1]))
    assert cover[0].shape == (96, 128, 3) and len(cover[2]) == 20 and np.all(np.isfinite(cover[2]))
    assert cover[2][-1] < cover[2][0]
    assert re.search(r'nnfm_cover=1\b', cover[1])
    assert 'NNFM bank rows: conv3_1 %d; cover 1\n' % rows in cover[3], cover[3]
    bare = _cli_run(tmp_path, monkeypatch, capsys, 'bare', alone)
    assert 'nnfm_cover' not in bare[1] and 'NNFM bank rows: conv3_1 %d\n' % rows in bare[3], bare[3]
    assert '; cover' not in bare[3]
    assert bare[2][0] < cover[2][0]         # E_cov >= 0 is added
