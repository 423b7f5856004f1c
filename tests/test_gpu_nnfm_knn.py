"""The k-nearest form of the nearest-neighbour term (--nnfm-k) on the GPU: nnfm_search_kernel<*, K>, the K-fold
merge and the gradient kernels over K gathered rows through stx_op_nnfm_knn_terms, the tile path and the command
line -- against tests/nnfm_knn_ref.py (float64 on the same float32 inputs).  The bounds are those of
tests/test_gpu_nnfm.py and tests/test_gpu_nnfm_patch.py, applied in the same way; no number here is new.

Bounds.
  * Planted inputs (column i = alpha_i sum_r w_r b_{p_ir} + 1e-3 alpha_i of unit noise, w = 1, .85, .7, .55, .4 on
    five distinct rows -- as many as the bank has --, alpha_i in [1e-2, 1e3]; a column is drawn again until the
    float64 scores of its ranks 1 .. 5 lie more than 1e-3 apart, and this is asserted before the GPU is asked):
    every index list equals the reference's, rank for rank, and the ranks from min(K, M) on hold -1.  The patch
    form takes the blob as the weighted sum of five random maps of its size, against the patches of all five.
  * Exact ties (a bank row three times, across block and slice boundaries): the copies in ascending order.
  * Random inputs, tau = 4 x the worst |emulated score - float64 score| of the case (nnfm_ref.search_error): the
    min(K, M) indices of a query are distinct and inside the bank; every chosen row has cos64 >= the K'-th best
    cos64 - tau; every other row has cos64 <= the worst chosen cos64 + tau; consecutive ranks are ordered up to tau.
  * E, sum |S| (relative) and S (of max |S_ref|) to 1e-5 (TIGHT) against the reference AT THE GPU'S OWN INDEX SETS.
  * The tile path: loss and gradient to TIGHT of the oracle's backward pass on the GPU's activations fed the
    reference's S at the GPU's index sets (the op call on the tile's blob gives them).

Observed worst values on an MI355X over the 87 random settings (24 op-level shapes, the 45 x 47 map, three patch
shapes and the sliced case, K = 2, 3, 4 each): emulated search error 1.01e-7 (tau 4.05e-7), the GPU's worst excess
over any of the three order bounds 0 (each of the 13 218 index sets is the float64 set, in the float64 order), E
1.3e-7, sum |S| 4.6e-7, S 2.8e-7 of its maximum; planted inputs: every list exact (2 201 of the 3 480 are the planted
rows themselves in their order; the patch maps' smallest gap between ranks is 1.7e-3); the sliced case runs 47
slices and 63 of its 64 queries have their two best rows in different slices; the tiles' loss 1.1e-7 .. 7.1e-7,
their gradient 8.7e-7 .. 1.2e-6 of its maximum; the command-line run lowers E / 2 from 0.046051 to 0.028302 in 20
Adam steps.  Every case prints its figures before it asserts (pytest -s)."""

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
from tests import nnfm_knn_ref as ref
from tests import nnfm_patch_ref, nnfm_ref
from tests.gpu_helpers import TIGHT, gpu_engine, max_rel

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHANNELS = [64, 256]
MAPS = [(1, 1), (3, 5), (3, 43)]                # n = 1 (one lane), 15 (a ragged block), 129 (two query blocks)
ROWS = [3, 31, 129, 1000]                       # M < K; one ragged bank block; a block boundary; many blocks
KS = [2, 3, 4]
WEIGHTS = np.array([1.0, 0.85, 0.7, 0.55, 0.4])
ERR_ARG = -1


def _unit_rows(rng, m, width):
    b = rng.standard_normal((m, width))
    return (b / np.linalg.norm(b, axis=1, keepdims=True)).astype(np.float32)


def _op(eng, feat, bank, k, patch=1, profile=False):
    """(S, J [k, n], E, sum |S|[, the search's slice count]) of stx_op_nnfm_knn_terms."""
    c, h, w = feat.shape
    d_feat, d_bank = eng.to_device(feat), eng.to_device(bank)
    s_out = eng.empty((c, h, w))
    idx = eng.empty((k, h * w), np.int32)
    out = (ctypes.c_double * 2)()
    if profile:
        eng.profile(True)
    try:
        lib.call('stx_op_nnfm_knn_terms', eng.handle, d_feat.ptr, c, h, w, patch, k, d_bank.ptr, bank.shape[0],
                 s_out.ptr, idx.ptr, out)
        result = (s_out.get(), idx.get().astype(np.int64), out[0], out[1])
        if profile:
            labels = [row[0] for row in eng.profile_read()]
            form = r'nnfm %s%ssearch op x(\d+)' % ('patch ' if patch == 3 else '', 'k%d ' % k if k > 1 else '')
            slices = [int(m.group(1)) for m in (re.fullmatch(form, l) for l in labels) if m]
            assert len(slices) == 1, labels
            result += (slices[0],)
    finally:
        if profile:
            eng.profile(False)
        for arr in (d_feat, d_bank, s_out, idx):
            arr.free()
    return result


def _held_at_own_sets(tag, feat, bank, s, J, e, asum, patch=1, hold=True):
    e_ref, s_ref, asum_ref, _ = ref.terms_at(feat, bank, J, patch)
    s_err = max_rel(s, s_ref) if np.abs(s_ref).max() > 0 else float(np.abs(s).max())
    e_err = abs(e / e_ref - 1) if e_ref else abs(e)
    a_err = abs(asum / asum_ref - 1) if asum_ref else abs(asum)
    print('%s: E %.6g (%.2e), sum|S| %.6g (%.2e), S %.2e of max' % (tag, e, e_err, asum, a_err, s_err))
    assert np.all(np.isfinite(s)) and np.isfinite(e) and np.isfinite(asum)
    if hold:
        assert s_err <= TIGHT and a_err <= TIGHT and e_err <= TIGHT
    return e_err, a_err, s_err


def _separated(scores, ranks):
    """Per query: the float64 scores of the best ``ranks`` rows lie more than 1e-3 apart."""
    top = -np.sort(-scores, axis=1)[:, :ranks]
    return np.all(top[:, :-1] - top[:, 1:] > 1e-3, axis=1) if top.shape[1] > 1 else np.ones(len(top), bool)


def _planted(rng, bank, h, w):
    """A blob whose columns are weighted sums of five distinct bank rows, each drawn until its ranks 1 .. 5 are
    separated; (feat, the planted rows [n, min(5, M)])."""
    m, c = bank.shape
    n, ranks = h * w, min(5, m)
    cols, picks = np.empty((n, c)), np.empty((n, ranks), np.int64)
    b64 = bank.astype(np.float64)
    for i in range(n):
        for _ in range(200):
            pick = rng.choice(m, ranks, replace=False)
            noise = rng.standard_normal(c)
            col = 10.0 ** rng.uniform(-2, 3) * (WEIGHTS[:ranks] @ b64[pick] + 1e-3 * noise / np.linalg.norm(noise))
            col = np.float64(np.float32(col))
            if _separated((col / np.linalg.norm(col) @ b64.T)[None], ranks)[0]:
                break
        else:
            raise AssertionError('no separated column in 200 draws')
        cols[i], picks[i] = col, pick
    return np.ascontiguousarray(cols.T.reshape(c, h, w), np.float32), picks


def _lanes_of(J):
    """Where the rows of index sets lie in the search's walk: (lane half, wave, 128-row block) per entry."""
    return (J >> 2) & 1, (J % 128) // 64, J // 128


@pytest.mark.parametrize('m', ROWS)
@pytest.mark.parametrize('h,w', MAPS)
@pytest.mark.parametrize('c', CHANNELS)
def test_planted_index_lists_are_exact(c, h, w, m):
    eng = gpu_engine()
    rng = np.random.RandomState(c + 7 * h + 13 * w + m)
    bank = _unit_rows(rng, m, c)
    feat, picks = _planted(rng, bank, h, w)
    scores = nnfm_ref.scores64(feat, bank)
    assert np.all(_separated(scores, min(5, m))), 'the planted ranks are not separated'
    for k in KS:
        J_ref = ref.topk(feat, bank, k)
        kk = min(k, m)
        s, J, e, asum = _op(eng, feat, bank, k)
        planted = np.count_nonzero(np.all(J_ref[:kk].T == picks[:, :kk], axis=1))
        print('planted C %d %dx%d M %d K %d: %d of %d lists are the planted rows in their order' % (c, h, w, m, k, planted, h * w))
        assert np.array_equal(J, J_ref), (k, np.argwhere(J != J_ref)[:8])
        assert np.all(J[kk:] == -1)
        _held_at_own_sets('planted K %d' % k, feat, bank, s, J, e, asum, hold=False)
    if m >= 129 and h * w >= 15:        # over the queries, the best rows lie in both lane halves, both waves, two blocks
        half, wave, block = _lanes_of(ref.topk(feat, bank, 2))
        assert np.any(half[0] != half[1]) and np.any(wave[0] != wave[1])
        assert m == 129 or np.any(block[0] != block[1])         # (129 rows: the second block is one row)


def _planted_patches(h, w, c=64):
    """Five random style maps of the blob's own size; the blob is their weighted sum (WEIGHTS) plus 1e-3 of noise,
    and the bank holds the patches of all five, map after map: the patch at p lies nearest the patches at p of the
    five maps, mostly in the order of the weights.  (feat, bank [5 h w, 9 c])"""
    rng = np.random.RandomState(c + 7 * h + 13 * w)
    maps = rng.standard_normal((5, c, h, w))
    bank = np.concatenate([nnfm_patch_ref.patch_bank_of(one) for one in maps]).astype(np.float32)
    noise = rng.standard_normal((c, h, w))
    noise /= np.linalg.norm(noise, axis=0, keepdims=True)
    feat = 10.0 ** rng.uniform(-2, 3) * (np.tensordot(WEIGHTS, maps, 1) + 1e-3 * noise)
    return np.ascontiguousarray(feat, np.float32), bank


@pytest.mark.parametrize('h,w', [(5, 7), (1, 9)])
def test_planted_patch_index_lists_are_exact(h, w):
    eng = gpu_engine()
    feat, bank = _planted_patches(h, w)
    n = h * w
    scores = nnfm_patch_ref.scores64(feat, bank)
    top = -np.sort(-scores, axis=1)[:, :5]
    print('planted patches %dx%d: smallest gap between the ranks 1 .. 5: %.2e' % (h, w, (top[:, :-1] - top[:, 1:]).min()))
    assert np.all(_separated(scores, 5)), 'the ranks are not separated'
    for k in KS:
        J_ref = ref.topk(feat, bank, k, 3)
        planted = np.count_nonzero(np.all(J_ref == np.arange(k)[:, None] * n + np.arange(n)[None, :], axis=0))
        print('planted patches %dx%d K %d: %d of %d lists are the planted patches in their order' % (h, w, k, planted, n))
        s, J, e, asum = _op(eng, feat, bank, k, 3)
        assert np.array_equal(J, J_ref), (k, np.argwhere(J != J_ref)[:8])
        _held_at_own_sets('planted patches K %d' % k, feat, bank, s, J, e, asum, 3, hold=False)


def test_the_sliced_bank_path():
    """n = 64 columns against M = 6000 rows: one query block, the bank cut across workgroups, K candidates a slice
    merged.  The planted rows of a query lie in different slices."""
    eng = gpu_engine()
    rng = np.random.RandomState(6000)
    c, h, w, m = 64, 8, 8, 6000
    bank = _unit_rows(rng, m, c)
    feat, picks = _planted(rng, bank, h, w)
    assert np.all(_separated(nnfm_ref.scores64(feat, bank), 5))
    for k in KS:
        J_ref = ref.topk(feat, bank, k)
        s, J, e, asum, slices = _op(eng, feat, bank, k, profile=True)
        per_slice = -(-(-(-m // 128)) // slices) * 128      # rows of a slice: whole 128-row blocks
        spread = np.count_nonzero(J_ref[0] // per_slice != J_ref[1] // per_slice)
        print('sliced K %d: %d slices, %d of 64 queries with their two best rows in different slices' % (k, slices, spread))
        assert slices > 1 and spread > 0
        assert np.array_equal(J, J_ref), (k, np.argwhere(J != J_ref)[:8])
    _random_case(eng, 'sliced', rng.standard_normal((c, h, w)).astype(np.float32), bank)


@pytest.mark.parametrize('h,w', [(8, 8), (181, 181)])
def test_exact_ties_come_in_ascending_order(h, w):
    """Bank rows repeated three times across the 128-row blocks -- which are the slices of the 8 x 8 map (one query
    block) and the steps of one workgroup's walk for the 181 x 181 map (256 query blocks: no slicing): a column
    that is an exact multiple of such a row scores the same on every copy.  K = 2: the two lowest copies, ascending.
    K = 4: all three, then the next row -- held to the reference where that row leads the one behind it by more
    than 1e-3 in float64, which is asserted for the columns on the copies before the GPU is asked."""
    eng = gpu_engine()
    rng = np.random.RandomState(h)
    c, m = 64, 700
    bank = _unit_rows(rng, m, c)
    groups = [(100, 300, 650), (255, 256, 699), (127, 128, 384), (5, 130, 131)]
    for g in groups:
        for j in g[1:]:
            bank[j] = bank[g[0]]
    copies = [j for g in groups for j in g]
    group_of = {j: g for g in groups for j in g}
    n = h * w
    for attempt in range(50):       # the columns on the copies: rank 4 and rank 5 are separated
        pick = rng.randint(0, m, n)
        pick[:len(copies) * 3] = np.tile(copies, 3)
        alpha = (2.0 ** rng.randint(-6, 10, n)).astype(np.float32)        # exact multiples: no rounding
        feat = np.ascontiguousarray((alpha[:, None] * bank[pick]).T.reshape(c, h, w))
        scores = nnfm_ref.scores64(feat, bank)
        top = -np.sort(np.partition(-scores, 5, axis=1)[:, :5], axis=1)
        if np.all(top[:len(copies) * 3, 3] - top[:len(copies) * 3, 4] > 1e-3):
            break
    on_copies = np.arange(len(copies) * 3)
    assert np.all(top[on_copies, 3] - top[on_copies, 4] > 1e-3) and np.all(top[on_copies, 2] - top[on_copies, 3] > 1e-3)
    for k in (2, 4):
        J_ref = ref.topk(feat, bank, k)
        for i in on_copies:
            assert tuple(J_ref[:min(k, 3), i]) == group_of[pick[i]][:min(k, 3)]
        s, J, e, asum, slices = _op(eng, feat, bank, k, profile=True)
        print('ties %dx%d K %d: %d slices' % (h, w, k, slices))
        assert (slices > 1) == (h == 8)
        assert np.array_equal(J[:, on_copies], J_ref[:, on_copies]), np.argwhere(J[:, on_copies] != J_ref[:, on_copies])[:8]
        # every other column: exact wherever the float64 ranks are separated (a pair of copies is a tie, in order)
        gaps = top[:, :k] - top[:, 1:k + 1]
        tied = np.array([[scores[i, J_ref[r, i]] == scores[i, J_ref[r + 1, i]] for r in range(k - 1)] + [False]
                         for i in range(n)])
        clear = np.all((gaps > 1e-3) | tied, axis=1)
        print('ties %dx%d K %d: %d of %d columns with separated ranks' % (h, w, k, np.count_nonzero(clear), n))
        assert np.array_equal(J[:, clear], J_ref[:, clear])


def _random_case(eng, tag, feat, bank, patch=1, ks=KS):
    n, m = feat.shape[1] * feat.shape[2], bank.shape[0]
    scores = nnfm_patch_ref.scores64(feat, bank, patch)
    tau = 4 * nnfm_patch_ref.search_error(feat, bank, patch)
    ranked = -np.sort(-scores, axis=1)
    rows = np.arange(n)
    worst = (0.0, 0.0, 0.0)
    for k in ks:
        kk = min(k, m)
        s, J, e, asum = _op(eng, feat, bank, k, patch)
        assert np.all(J[kk:] == -1) and J[:kk].min() >= 0 and J[:kk].max() < m
        assert all(len(set(J[:kk, i])) == kk for i in range(n)), 'an index twice'
        chosen = scores[rows[None, :], J[:kk]]                      # [kk, n]
        low = ranked[:, kk - 1] - chosen.min(axis=0)                # the K'-th best against the worst chosen
        others = scores.copy()
        others[rows[None, :], J[:kk]] = -np.inf
        high = others.max(axis=1) - chosen.min(axis=0) if kk < m else np.full(n, -np.inf)
        order = (chosen[1:] - chosen[:-1]).max() if kk > 1 else -np.inf
        differ = np.count_nonzero(np.any(np.sort(J[:kk], axis=0) != np.sort(ref.topk(feat, bank, k, patch)[:kk], axis=0), axis=0))
        print('%s K %d random: emulated worst %.2e, tau %.2e, worst excess %.2e (chosen) %.2e (left out) %.2e (order), '
              '%d of %d sets off the float64 set' % (tag, k, tau / 4, tau, low.max(), high.max(), order, differ, n))
        assert np.all(low <= tau) and np.all(high <= tau) and order <= tau, (tag, k)
        errs = _held_at_own_sets('%s K %d random' % (tag, k), feat, bank, s, J, e, asum, patch)
        worst = tuple(max(a, b) for a, b in zip(worst, errs))
        s2, J2, e2, asum2 = _op(eng, feat, bank, k, patch)
        assert s.tobytes() == s2.tobytes() and np.array_equal(J, J2) and e == e2 and asum == asum2
    return worst


@pytest.mark.parametrize('m', ROWS)
@pytest.mark.parametrize('h,w', MAPS)
@pytest.mark.parametrize('c', CHANNELS)
def test_knn_kernels_against_float64(c, h, w, m):
    eng = gpu_engine()
    rng = np.random.RandomState(c + 7 * h + 13 * w + m)
    bank = _unit_rows(rng, m, c)
    _random_case(eng, 'C %d %dx%d M %d' % (c, h, w, m), rng.standard_normal((c, h, w)).astype(np.float32), bank)


def test_knn_kernels_on_many_query_blocks():
    eng = gpu_engine()
    rng = np.random.RandomState(2115)
    bank = _unit_rows(rng, 1000, 256)
    _random_case(eng, 'C 256 45x47 M 1000', rng.standard_normal((256, 45, 47)).astype(np.float32), bank)


@pytest.mark.parametrize('h,w,m', [(5, 7, 31), (1, 9, 3), (31, 33, 129)])
def test_knn_patch_kernels_against_float64(h, w, m):
    eng = gpu_engine()
    rng = np.random.RandomState(7 * h + 13 * w + m)
    bank = _unit_rows(rng, m, 9 * 64)
    feat = (rng.standard_normal((64, h, w)) * 10.0 ** rng.uniform(-2, 3)).astype(np.float32)
    _random_case(eng, 'patch C 64 %dx%d M %d' % (h, w, m), feat, bank, 3)


def test_zero_columns_take_the_first_rows():
    eng = gpu_engine()
    rng = np.random.RandomState(3)
    c, h, w, m = 64, 9, 11, 140
    bank = _unit_rows(rng, m, c)
    feat = rng.standard_normal((c, h, w)).astype(np.float32)
    zero = [0, 4 * w + 5, 8 * w + 10]
    feat.reshape(c, -1)[:, zero] = 0
    s, J, e, asum = _op(eng, feat, bank, 3)
    assert np.array_equal(J[:, zero], np.tile(np.arange(3)[:, None], (1, 3))) and not s.reshape(c, -1)[:, zero].any()
    _held_at_own_sets('zeros', feat, bank, s, J, e, asum)


@pytest.mark.parametrize('patch', [1, 3])
def test_k_1_gives_the_bytes_of_the_patch_entry_point(patch):
    eng = gpu_engine()
    rng = np.random.RandomState(11 + patch)
    c, h, w, m = 64, 9, 13, 150
    feat = rng.standard_normal((c, h, w)).astype(np.float32)
    bank = _unit_rows(rng, m, patch * patch * c)
    d_feat, d_bank = eng.to_device(feat), eng.to_device(bank)
    s_out, idx, out = eng.empty((c, h, w)), eng.empty((h * w,), np.int32), (ctypes.c_double * 2)()
    lib.call('stx_op_nnfm_patch_terms', eng.handle, d_feat.ptr, c, h, w, patch, d_bank.ptr, m, s_out.ptr, idx.ptr, out)
    old = (s_out.get(), idx.get(), out[0], out[1])
    for arr in (d_feat, d_bank, s_out, idx):
        arr.free()
    new = _op(eng, feat, bank, 1, patch)
    assert old[0].tobytes() == new[0].tobytes() and np.array_equal(old[1], new[1][0]) and old[2:] == new[2:]


def test_k_outside_1_to_4_leaves_the_output_alone():
    eng = gpu_engine()
    feat = eng.to_device(np.ones((64, 4, 4), np.float32))
    bank = eng.to_device(np.ones((3, 64), np.float32) / 8)
    s_out = eng.to_device(np.full((64, 4, 4), 7.0, np.float32))
    idx = eng.to_device(np.full((5, 16), 9, np.int32), np.int32)
    out = (ctypes.c_double * 2)(5.0, 5.0)
    call = lambda k: lib.call('stx_op_nnfm_knn_terms', eng.handle, feat.ptr, 64, 4, 4, 1, k, bank.ptr, 3, s_out.ptr,
                              idx.ptr, out)
    for k in (0, 5, -1):
        with pytest.raises(lib.StxError) as err:
            call(k)
        assert err.value.code == ERR_ARG, k
    assert np.all(s_out.get() == 7.0) and np.all(idx.get() == 9) and list(out) == [5.0, 5.0]
    table = (lib.NnfmKnnTarget * 1)()
    t = table[0]
    t.layer, t.channels, t.patch, t.k, t.rows, t.bank, t.mem, t.weight = b'conv1_1', 64, 1, 5, 3, bank.ptr, lib.DEVICE, 1.0
    with pytest.raises(lib.StxError) as err:
        lib.call('stx_set_nnfm_knn_targets', eng.handle, table, 1)
    assert err.value.code == ERR_ARG
    call(4)         # and the same arrays in order are taken: three rows, the fourth rank empty
    got = idx.get()
    assert np.all(np.isfinite(s_out.get())) and np.all(got[3] == -1) and np.all(got[4] == 9) and got[:3].max() < 3
    for arr in (feat, bank, s_out, idx):
        arr.free()


# --------------------------------------------------------------------------------- the tile path
SL = ['conv1_1', 'conv2_1', 'conv3_1']
SW = {l: 1 / 3 for l in SL}
LW = {'conv3_1': 1.5}
NNFM_W = {'conv3_1': 0.7}
TILE_CASES = {'alone': ([], 1, 3), 'gram': (SL, 1, 3), 'patch': ([], 3, 2)}        # style layers, patch, K


@functools.lru_cache(maxsize=None)
def _scene():
    """Oracle with targets of a 64 x 64 frame and the conv3_1 banks (plain and patch) of a 40 x 44 style picture."""
    net = builtin_net('vgg19')
    om = ref.KnnOracleModel(net.as_dicts(), synthetic_weights(net.as_dicts(), 0))
    rng = np.random.RandomState(29)
    full = rng.uniform(-110, 120, (3, 64, 64)).astype(np.float32)
    style = rng.uniform(-110, 120, (3, 40, 44)).astype(np.float32)
    om.styles = [om.style_grams([style], SL, 512)]
    om.contents = [om.prepare_features(full, ['conv3_2'], 512)]
    feat = om.features_tile(style, ['conv3_1'])['conv3_1']
    banks = {1: nnfm_ref.bank_of(feat).astype(np.float32), 3: nnfm_patch_ref.patch_bank_of(feat).astype(np.float32)}
    return om, full, banks


def _evaluate(eng, full, banks, case):
    sl, patch, k = TILE_CASES[case]
    eng.set_nnfm_targets({'conv3_1': banks[patch]}, NNFM_W, patch, k)
    try:
        return eng.sc_grad_tile(full, (0, 0), (0, 0), [], sl, LW, {}, SW)
    finally:
        eng.set_nnfm_targets({})


def _sums_in_place_child(scene_path, out_path):
    """In a process of its own with STX_SUMS_LATE=0: the three settings' loss and gradient, as hex and a digest."""
    os.environ['STX_SUMS_LATE'] = '0'
    with open(scene_path, 'rb') as f:
        contents, styles, full, banks = pickle.load(f)
    eng = gpu_engine()
    eng.set_contents_and_styles(contents, styles)
    result = {}
    for case in TILE_CASES:
        loss, grad = _evaluate(eng, full, banks, case)
        result[case] = [float(loss).hex(), hashlib.sha256(np.ascontiguousarray(grad).tobytes()).hexdigest()]
    eng.close()
    with open(out_path, 'w') as f:
        json.dump(result, f)


@pytest.mark.parametrize('case', list(TILE_CASES))
def test_knn_tile_against_the_oracle(case):
    """K = 3 alone (no tap at all), K = 3 beside a Gram term on the same blob, the patch form with K = 2."""
    om, full, banks = _scene()
    sl, patch, k = TILE_CASES[case]
    bank = banks[patch]
    eng = gpu_engine()
    start, roll = (0, 0), (0, 0)
    eng.set_contents_and_styles(om.contents, om.styles)
    plain = eng.sc_grad_tile(full, start, roll, [], sl, LW, {}, SW) if sl else None
    loss, grad = _evaluate(eng, full, banks, case)
    again = _evaluate(eng, full, banks, case)
    blobs = om.blob_names[:om.blob_names.index('conv3_1') + 1]
    acts = eng.features_tile(full, blobs)
    J = _op(eng, np.ascontiguousarray(acts['conv3_1'], np.float32), bank, k, patch)[1]      # the GPU's index sets
    differ = np.count_nonzero(np.any(J != ref.topk(acts['conv3_1'], bank, k, patch), axis=0))
    om.nnfm_banks, om.nnfm_weights = {'conv3_1': np.float64(bank)}, dict(NNFM_W)
    om.nnfm_k, om.nnfm_patch, om.nnfm_index = k, patch, {'conv3_1': J}
    try:
        same_loss, same_grad = om.sc_grad_tile(full, start, [], sl, LW, {}, SW, activations=acts)
        term64 = om.nnfm_loss64(acts, LW)
    finally:
        om.nnfm_banks, om.nnfm_weights, om.nnfm_index = {}, {}, {}
        om.nnfm_k, om.nnfm_patch = 1, 1
    stats = dict(loss=abs(loss / same_loss - 1), term=term64, grad=max_rel(grad, same_grad),
                 moved=max_rel(grad, plain[1]) if plain else None, lists_off_float64=differ)
    print('nnfm knn tile', case, stats)
    assert np.all(np.isfinite(grad)) and grad.any()
    assert again[0] == loss and np.array_equal(again[1], grad)
    assert loss == pytest.approx(same_loss, rel=TIGHT), (loss, same_loss)
    if plain:
        assert loss - plain[0] == pytest.approx(term64, abs=2 * TIGHT * loss)
        assert stats['moved'] > 1e-3        # the term is not lost in the others
    else:
        assert loss == pytest.approx(term64, rel=TIGHT)
    assert stats['grad'] < TIGHT, stats


def test_cleared_targets_change_no_bit_and_k_changes_the_term():
    om, full, banks = _scene()
    eng = gpu_engine()
    run = lambda: eng.sc_grad_tile(full, (0, 0), (0, 0), [], SL, LW, {}, SW)
    eng.set_contents_and_styles(om.contents, om.styles)
    before = run()
    eng.set_nnfm_targets({'conv3_1': banks[1]}, NNFM_W, 1, 3)
    moved = run()
    eng.set_nnfm_targets({'conv3_1': banks[1]}, NNFM_W)             # any setter replaces the whole set: k = 1
    one = run()
    eng.set_nnfm_targets({'conv3_1': banks[1]}, NNFM_W, k=3)
    back = run()
    eng.set_nnfm_targets({})
    cleared = run()
    assert moved[0] != before[0] and not np.array_equal(moved[1], before[1])
    assert one[0] != moved[0] and one[0] != before[0]
    assert back[0] == moved[0] and np.array_equal(back[1], moved[1])
    assert cleared[0] == before[0] and np.array_equal(cleared[1], before[1])


def test_sums_in_place_give_the_same_bits(tmp_path):
    """STX_SUMS_LATE=0 in a fresh process against the default here, all three settings."""
    om, full, banks = _scene()
    eng = gpu_engine()
    eng.set_contents_and_styles(om.contents, om.styles)
    here = {}
    for case in TILE_CASES:
        loss, grad = _evaluate(eng, full, banks, case)
        here[case] = [float(loss).hex(), hashlib.sha256(np.ascontiguousarray(grad).tobytes()).hexdigest()]
    scene, out = str(tmp_path / 'scene.pkl'), str(tmp_path / 'child.json')
    with open(scene, 'wb') as f:
        pickle.dump((om.contents, om.styles, full, banks), f)
    code = 'import sys; sys.path.insert(0, %r); from tests.test_gpu_nnfm_knn import _sums_in_place_child; ' \
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


def test_cli_run_with_k_3_lowers_the_term(tmp_path, monkeypatch, capsys):
    rng = np.random.RandomState(5)
    picture = lambda hw: Image.fromarray(np.uint8(rng.uniform(0, 255, hw + (3,))))
    picture((96, 128)).save(tmp_path / 'c.png')
    picture((96, 128)).save(tmp_path / 's.png')
    # the term alone: no Gram, the content term at weight 0, no regulariser -- the logged loss is weight E / 2
    alone = ['-si', '../s.png', '-i', '20', '--nnfm-weight', '1', '--nnfm-layers', 'conv3_1', '--style-layers',
             '--content-layers', 'conv3_2', '-cw', '0', '-tw', '0', '-pw', '0']
    rows = nnfm_ref.bank_rows(24, 32)
    three = _cli_run(tmp_path, monkeypatch, capsys, 'three', alone + ['--nnfm-k', '3'])
    with capsys.disabled():
        print('20 Adam steps, k 3, E / 2: %.6f -> %.6f' % (three[2][0], three[2][-1]))
    assert three[0].shape == (96, 128, 3) and len(three[2]) == 20 and np.all(np.isfinite(three[2]))
    assert three[2][-1] < three[2][0]
    assert re.search(r'nnfm_k=3', three[1])
    assert 'NNFM bank rows: conv3_1 %d; k 3\n' % rows in three[3], three[3]
    bare = _cli_run(tmp_path, monkeypatch, capsys, 'bare', alone)
    assert 'nnfm_k' not in bare[1] and 'NNFM bank rows: conv3_1 %d\n' % rows in bare[3], bare[3]
    assert bare[2][0] < three[2][0]         # the best row alone lies nearer than the mean of the three best
