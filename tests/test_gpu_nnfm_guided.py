"""The region-guided nearest-neighbour term (--nnfm-masks) on the GPU: the mask window pass, the segmented search
and merge and the guided gradient kernels through stx_op_nnfm_guided_terms, the tile path and the command line --
against tests/nnfm_guided_ref.py (float64 on the same float32 inputs).  TIGHT = 1e-5 of tests/gpu_helpers.py is the
only tolerance; everything else is exact.

  * Identity 1: wherever a pair (segment, 128-column block) is searched, the lists are those of stx_op_nnfm_knn_terms
    on the same blob against that segment's rows alone, index for index; elsewhere all k ranks hold -1.
  * Identity 2: one segment with m = 1 gives the bytes of the unguided op and a == 1.0; m = 0.5 gives half of S
    byte for byte, a == 0.5 and E to TIGHT of half.
  * E, sum |S|, a (relative) and S (of max |S_ref|) to TIGHT against the reference AT THE GPU'S OWN LISTS.
  * The tile path: loss and gradient to TIGHT of the oracle's backward pass on the GPU's activations at the GPU's
    lists (the op call on the tile's blob gives them).

Observed worst values on an MI355X over the 199 op-level settings: E 1.6e-7, sum |S| 5.4e-7, a 1.3e-7, S 2.1e-7 of its
maximum; every list of a searched pair is the segment's own, every other pair holds -1; the sliced case runs 47
slices; the tiles' loss 9.7e-8 .. 1.9e-7, their gradient 7.9e-7 .. 1.4e-6 of its maximum, a = 0.617 and 0.503, three of
four and two of two pairs searched; the command-line run lowers E / 2 from 0.045109 to 0.025255 in 20 Adam steps.
Every case prints its figures before it asserts (pytest -s)."""

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
from tests import nnfm_guided_ref as ref
from tests import nnfm_ref
from tests.gpu_helpers import TIGHT, gpu_engine, max_rel
from tests.masked_style_ref import mask_map

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHANNELS = [64, 256]
MAPS = [(1, 1), (3, 5), (3, 43), (9, 43)]       # n = 1, 15, 129 (two query blocks), 387 (four)
SEGMENTS = [(3, 31), (129, 1000), (40, 129, 7)]
KS = [1, 3]
PATTERNS = ['random', 'stripes', 'one segment zero', 'one column']
ERR_ARG = -1


def _unit_rows(rng, m, width):
    b = rng.standard_normal((m, width))
    return (b / np.linalg.norm(b, axis=1, keepdims=True)).astype(np.float32)


def _op(eng, feat, bank, seg_rows, maps, k, oy=0, ox=0, roll=(0, 0), profile=False):
    """(S, J [segments, k, n], E, sum |S|, a[, the search's slice count]) of stx_op_nnfm_guided_terms."""
    c, h, w = feat.shape
    maps = np.ascontiguousarray(maps, np.float32)
    segments, mh, mw = maps.shape
    d_feat, d_bank, d_maps = eng.to_device(feat), eng.to_device(bank), eng.to_device(maps)
    s_out = eng.empty((c, h, w))
    idx = eng.empty((segments, k, h * w), np.int32)
    out = (ctypes.c_double * 3)()
    if profile:
        eng.profile(True)
    try:
        lib.call('stx_op_nnfm_guided_terms', eng.handle, d_feat.ptr, c, h, w, k, d_bank.ptr,
                 (ctypes.c_int * segments)(*seg_rows), segments, d_maps.ptr, mh, mw, oy, ox, (ctypes.c_int * 2)(*roll),
                 s_out.ptr, idx.ptr, out)
        result = (s_out.get(), idx.get().astype(np.int64), out[0], out[1], out[2])
        if profile:
            labels = [row[0] for row in eng.profile_read()]
            form = r'nnfm guided %ssearch op x(\d+) s%d' % ('k%d ' % k if k > 1 else '', segments)
            slices = [int(m.group(1)) for m in (re.fullmatch(form, l) for l in labels) if m]
            assert len(slices) == 1, labels
            result += (slices[0],)
    finally:
        if profile:
            eng.profile(False)
        for arr in (d_feat, d_bank, d_maps, s_out, idx):
            arr.free()
    return result


def _plain(eng, feat, bank, k):
    """(S, J [k, n], E, sum |S|) of stx_op_nnfm_knn_terms: the unguided term."""
    c, h, w = feat.shape
    d_feat, d_bank = eng.to_device(feat), eng.to_device(bank)
    s_out, idx, out = eng.empty((c, h, w)), eng.empty((k, h * w), np.int32), (ctypes.c_double * 2)()
    try:
        lib.call('stx_op_nnfm_knn_terms', eng.handle, d_feat.ptr, c, h, w, 1, k, d_bank.ptr, bank.shape[0], s_out.ptr,
                 idx.ptr, out)
        return s_out.get(), idx.get().astype(np.int64), out[0], out[1]
    finally:
        for arr in (d_feat, d_bank, s_out, idx):
            arr.free()


def _pattern(kind, rng, segments, n):
    m = rng.uniform(0, 1, (segments, n)).astype(np.float32)
    blocks = -(-n // ref.BLOCK)
    if kind == 'stripes':           # hard edges on the query blocks: block b belongs to segment b mod S
        owner = np.repeat(np.arange(blocks) % segments, ref.BLOCK)[:n]
        m = (np.arange(segments)[:, None] == owner[None, :]).astype(np.float32)
    elif kind == 'one segment zero':
        m[-1] = 0
    elif kind == 'one column':      # the last block of segment 0: zero but for its last column
        m[0, (blocks - 1) * ref.BLOCK:] = 0
        m[0, n - 1] = 0.75
    return m


def _lists_are_the_segments_own(tag, J, m, alone, seg_rows):
    """Identity 1 and the -1 rule, block by block; returns (searched pairs, pairs)."""
    on = ref.searched(m)
    n = m.shape[1]
    for s in range(len(seg_rows)):
        for b in range(on.shape[1]):
            cols = slice(ref.BLOCK * b, min(ref.BLOCK * (b + 1), n))
            if on[s, b]:
                assert np.array_equal(J[s][:, cols], alone[s][:, cols]), (tag, s, b)
                assert J[s][:, cols].min() >= 0 and J[s][:, cols].max() < seg_rows[s], (tag, s, b)
            else:
                assert np.all(J[s][:, cols] == -1), (tag, s, b)
    return int(on.sum()), on.size


def _held_at_own_lists(tag, feat, bank, seg_rows, m, s, J, e, asum, a):
    e_ref, s_ref, asum_ref, a_ref = ref.terms_at(feat, bank, seg_rows, m, J)
    s_err = max_rel(s, s_ref) if np.abs(s_ref).max() > 0 else float(np.abs(s).max())
    e_err = abs(e / e_ref - 1) if e_ref else abs(e)
    asum_err = abs(asum / asum_ref - 1) if asum_ref else abs(asum)
    a_err = abs(a / a_ref - 1) if a_ref else abs(a)
    print('%s: E %.6g (%.2e), sum|S| %.6g (%.2e), a %.6g (%.2e), S %.2e of max'
          % (tag, e, e_err, asum, asum_err, a, a_err, s_err))
    assert np.all(np.isfinite(s)) and np.isfinite(e) and np.isfinite(asum) and np.isfinite(a)
    assert s_err <= TIGHT and asum_err <= TIGHT and e_err <= TIGHT and a_err <= TIGHT
    return e_err, asum_err, a_err, s_err


@pytest.mark.parametrize('seg_rows', SEGMENTS)
@pytest.mark.parametrize('h,w', MAPS)
@pytest.mark.parametrize('c', CHANNELS)
def test_guided_kernels_against_float64(c, h, w, seg_rows):
    eng = gpu_engine()
    rng = np.random.RandomState(c + 7 * h + 13 * w + sum(seg_rows))
    n, segments = h * w, len(seg_rows)
    bank = _unit_rows(rng, sum(seg_rows), c)
    feat = (rng.standard_normal((c, h, w)) * 10.0 ** rng.uniform(-2, 3, (h, w))).astype(np.float32)
    off = ref.offsets(seg_rows)
    for k in KS:
        alone = [_plain(eng, feat, bank[off[s]:off[s] + seg_rows[s]], k)[1] for s in range(segments)]
        for kind in PATTERNS:
            tag = 'C %d %dx%d segments %s K %d %s' % (c, h, w, seg_rows, k, kind)
            m = _pattern(kind, rng, segments, n)
            s, J, e, asum, a = _op(eng, feat, bank, seg_rows, m.reshape(segments, h, w), k)
            searched, pairs = _lists_are_the_segments_own(tag, J, m, alone, seg_rows)
            print('%s: %d of %d pairs searched' % (tag, searched, pairs))
            _held_at_own_lists(tag, feat, bank, seg_rows, m, s, J, e, asum, a)
            again = _op(eng, feat, bank, seg_rows, m.reshape(segments, h, w), k)
            assert s.tobytes() == again[0].tobytes() and np.array_equal(J, again[1]) and (e, asum, a) == again[2:]
            if kind == 'stripes' and n > ref.BLOCK:
                assert searched == -(-n // ref.BLOCK) and a == 1.0          # one segment per block: 1 / S of the pairs


def test_the_window_is_taken_like_a_content_maps():
    """The window at (2, 5) of maps larger than the blob, behind a roll that wraps on both axes."""
    eng = gpu_engine()
    rng = np.random.RandomState(17)
    c, h, w, seg_rows, k = 64, 9, 43, (40, 129, 7), 3
    mh, mw, oy, ox, roll = h + 6, w + 9, 2, 5, (7, -(h + 2))
    bank = _unit_rows(rng, sum(seg_rows), c)
    feat = rng.standard_normal((c, h, w)).astype(np.float32)
    maps = rng.uniform(0, 1, (3, mh, mw)).astype(np.float32)
    maps[2, :, :] = 0
    maps[2, 1, 3] = 1.0         # lands in the window or not: the reference says which block, if any, is searched
    m = ref.windows(maps, oy, ox, h, w, roll)
    s, J, e, asum, a = _op(eng, feat, bank, seg_rows, maps, k, oy, ox, roll)
    off = ref.offsets(seg_rows)
    alone = [_plain(eng, feat, bank[off[i]:off[i] + seg_rows[i]], k)[1] for i in range(3)]
    print('window: %d of %d pairs searched' % _lists_are_the_segments_own('window', J, m, alone, seg_rows))
    _held_at_own_lists('window', feat, bank, seg_rows, m, s, J, e, asum, a)
    # a window outside the maps is the range error of the other windows, and leaves the outputs alone
    with pytest.raises(lib.StxError) as err:
        _op(eng, feat, bank, seg_rows, maps, k, 7, 5, roll)
    assert err.value.code == ERR_ARG


@pytest.mark.parametrize('k', KS)
def test_the_sliced_path_against_a_long_and_a_short_segment(k):
    """64 columns against a 6000-row segment beside a 200-row one: one query block, slices sized from the long
    segment, most of them past the short segment's end."""
    eng = gpu_engine()
    rng = np.random.RandomState(6200 + k)
    c, h, w, seg_rows = 64, 8, 8, (6000, 200)
    bank = _unit_rows(rng, sum(seg_rows), c)
    feat = rng.standard_normal((c, h, w)).astype(np.float32)
    m = rng.uniform(0.1, 1, (2, 64)).astype(np.float32)
    s, J, e, asum, a, slices = _op(eng, feat, bank, seg_rows, m.reshape(2, h, w), k, profile=True)
    print('sliced K %d: %d slices' % (k, slices))
    assert slices > 2
    alone = [_plain(eng, feat, bank[:6000], k)[1], _plain(eng, feat, bank[6000:], k)[1]]
    _lists_are_the_segments_own('sliced', J, m, alone, seg_rows)
    _held_at_own_lists('sliced K %d' % k, feat, bank, seg_rows, m, s, J, e, asum, a)
    m[1] = 0                # the short segment is not searched at all
    s, J, e, asum, a = _op(eng, feat, bank, seg_rows, m.reshape(2, h, w), k)
    assert np.all(J[1] == -1) and np.array_equal(J[0], alone[0])
    _held_at_own_lists('sliced K %d, one segment' % k, feat, bank, seg_rows, m, s, J, e, asum, a)


@pytest.mark.parametrize('c,h,w,rows', [(64, 9, 43, 1000), (256, 3, 5, 31), (64, 8, 8, 6000)])
@pytest.mark.parametrize('k', KS)
def test_one_segment_of_ones_gives_the_bytes_of_the_unguided_term(k, c, h, w, rows):
    eng = gpu_engine()
    rng = np.random.RandomState(rows + k)
    bank = _unit_rows(rng, rows, c)
    feat = (rng.standard_normal((c, h, w)) * 10.0 ** rng.uniform(-2, 3, (h, w))).astype(np.float32)
    s0, J0, e0, asum0 = _plain(eng, feat, bank, k)
    s, J, e, asum, a = _op(eng, feat, bank, [rows], np.ones((1, h, w)), k)
    print('one segment, m = 1, C %d %dx%d M %d K %d: E %.9g against %.9g, sum|S| %.9g against %.9g, a %r'
          % (c, h, w, rows, k, e, e0, asum, asum0, a))
    assert np.array_equal(J[0], J0)
    assert s.tobytes() == s0.tobytes() and e == e0 and asum == asum0 and a == 1.0
    s, J, e, asum, a = _op(eng, feat, bank, [rows], np.full((1, h, w), 0.5), k)
    print('m = 0.5: E %.9g against %.9g, a %r' % (e, 0.5 * e0, a))
    assert np.array_equal(J[0], J0)
    assert s.tobytes() == (np.float32(0.5) * s0).tobytes() and a == 0.5
    assert e == pytest.approx(0.5 * e0, rel=TIGHT)


def test_masks_keep_a_column_from_the_rows_it_lies_nearest():
    """Columns that are exact multiples of rows of segment 1, under masks that give them to segment 0."""
    eng = gpu_engine()
    rng = np.random.RandomState(41)
    c, h, w, seg_rows = 64, 3, 43, (129, 200)
    n = h * w
    bank = _unit_rows(rng, sum(seg_rows), c)
    pick = 129 + rng.randint(0, 200, n)
    feat = np.ascontiguousarray(((2.0 ** rng.randint(-3, 6, n))[:, None] * bank[pick]).T.reshape(c, h, w), np.float32)
    maps = np.stack([np.ones((h, w), np.float32), np.zeros((h, w), np.float32)])
    s, J, e, asum, a = _op(eng, feat, bank, seg_rows, maps, 1)
    s_all, J_all, e_all, asum_all = _plain(eng, feat, bank, 1)
    print('guidance: E %.6g guided, %.6g over the whole bank' % (e, e_all))
    assert np.array_equal(J_all[0], pick)                        # unguided: every column finds its own row, in segment 1
    assert np.all(J[1] == -1) and J[0].min() >= 0 and J[0].max() < 129
    assert np.array_equal(J[0], _plain(eng, feat, bank[:129], 1)[1])
    assert e > e_all + 0.1 and not np.array_equal(s, s_all) and a == 1.0
    _held_at_own_lists('guidance', feat, bank, seg_rows, maps.reshape(2, n), s, J, e, asum, a)


def test_zero_columns_and_zero_masks_add_nothing():
    eng = gpu_engine()
    rng = np.random.RandomState(43)
    c, h, w, seg_rows, k = 64, 9, 11, (60, 80), 3
    bank = _unit_rows(rng, sum(seg_rows), c)
    feat = rng.standard_normal((c, h, w)).astype(np.float32)
    zero = [0, 4 * w + 5, 8 * w + 10]
    feat.reshape(c, -1)[:, zero] = 0
    m = rng.uniform(0.2, 1, (2, h * w)).astype(np.float32)
    s, J, e, asum, a = _op(eng, feat, bank, seg_rows, m.reshape(2, h, w), k)
    assert not s.reshape(c, -1)[:, zero].any()
    assert np.array_equal(J[:, :, zero], np.tile(np.arange(3)[None, :, None], (2, 1, 3)))       # the first rows, as unguided
    _held_at_own_lists('zero columns', feat, bank, seg_rows, m, s, J, e, asum, a)
    s, J, e, asum, a = _op(eng, feat, bank, seg_rows, np.zeros((2, h, w)), k)
    assert e == 0 and asum == 0 and a == 0 and not s.any() and np.all(J == -1)


def test_bad_arguments_leave_the_outputs_alone():
    eng = gpu_engine()
    feat = eng.to_device(np.ones((64, 4, 4), np.float32))
    bank = eng.to_device(np.ones((9, 64), np.float32) / 8)
    maps = eng.to_device(np.ones((9, 4, 4), np.float32))
    s_out = eng.to_device(np.full((64, 4, 4), 7.0, np.float32))
    idx = eng.to_device(np.full((9, 5, 16), 9, np.int32), np.int32)
    out = (ctypes.c_double * 3)(5.0, 5.0, 5.0)

    def call(k, seg_rows, segments):
        lib.call('stx_op_nnfm_guided_terms', eng.handle, feat.ptr, 64, 4, 4, k, bank.ptr,
                 (ctypes.c_int * 9)(*(list(seg_rows) + [1] * (9 - len(seg_rows)))), segments, maps.ptr, 4, 4, 0, 0,
                 (ctypes.c_int * 2)(0, 0), s_out.ptr, idx.ptr, out)

    for k, seg_rows, segments in ((2, [4, 5], 0), (1, [1] * 9, 9), (3, [7, 2], 2), (5, [4, 5], 2), (0, [4, 5], 2)):
        with pytest.raises(lib.StxError) as err:
            call(k, seg_rows, segments)
        assert err.value.code == ERR_ARG, (k, seg_rows, segments)
    assert np.all(s_out.get() == 7.0) and np.all(idx.get() == 9) and list(out) == [5.0, 5.0, 5.0]
    table = (lib.NnfmGuidedTarget * 1)()
    t = table[0]
    t.layer, t.channels, t.k, t.segments, t.bank, t.mem, t.weight = b'conv1_1', 64, 3, 2, bank.ptr, lib.DEVICE, 1.0
    t.seg_rows = (ctypes.c_int * 2)(7, 2)
    mask = np.ones((8, 8), np.float32)
    ptrs = (ctypes.c_void_p * 9)(*[mask.ctypes.data] * 9)
    for segments in (2, 0, 9):          # a segment below k; no segments; too many
        with pytest.raises(lib.StxError) as err:
            lib.call('stx_set_nnfm_guided_targets', eng.handle, table, 1, ptrs, segments, 8, 8, lib.HOST)
        assert err.value.code == ERR_ARG
    call(2, [4, 5], 2)          # and the same arrays in order are taken
    assert np.all(np.isfinite(s_out.get())) and list(out)[2] == 2.0 and idx.get().ravel()[:2 * 2 * 16].max() < 5
    for arr in (feat, bank, maps, s_out, idx):
        arr.free()


# --------------------------------------------------------------------------------- the tile path
SL = ['conv1_1', 'conv2_1', 'conv3_1']
SW = {l: 1 / 3 for l in SL}
LW = {'conv3_1': 1.5}
NNFM_W = {'conv3_1': 0.7}
FRAME = (96, 64)
K = 2
TILES = [(64, 48, (0, 0), (0, 0)), (40, 32, (32, 16), (-24, 40))]      # th, tw, start, roll: the second one's window wraps
TILE_CASES = {'alone': [], 'gram': SL}


def _masks(swap=False):
    """Two masks of the frame: a smooth one, and one that is its complement at 0.8 below row 44 and zero above -- so a
    is not 1, and whole query blocks of segment 1 are not searched."""
    y, x = np.mgrid[:FRAME[0], :FRAME[1]]
    m0 = np.float32(0.5 + 0.5 * np.sin(0.09 * x + 0.05 * y) * np.cos(0.04 * y - 0.02 * x))
    m1 = np.float32(0.8) * (1 - m0)
    m1[:44] = 0
    return [m1, m0] if swap else [m0, m1]


@functools.lru_cache(maxsize=None)
def _scene():
    """Oracle with targets of a 96 x 64 frame and the conv3_1 bank of two small style pictures, one segment each."""
    net = builtin_net('vgg19')
    om = ref.GuidedOracleModel(net.as_dicts(), synthetic_weights(net.as_dicts(), 0))
    rng = np.random.RandomState(31)
    full = rng.uniform(-110, 120, (3,) + FRAME).astype(np.float32)
    styles = [rng.uniform(-110, 120, (3, 40, 44)).astype(np.float32), rng.uniform(-110, 120, (3, 28, 36)).astype(np.float32)]
    om.styles = [om.style_grams(styles, SL, 512)]
    om.contents = [om.prepare_features(full, ['conv3_2'], 512)]
    parts = [nnfm_ref.bank_of(om.features_tile(s, ['conv3_1'])['conv3_1']) for s in styles]
    bank = nnfm_ref.concat_banks(parts).astype(np.float32)
    return om, full, bank, [len(p) for p in parts]


def _tile(full, th, tw, start, roll):
    rolled = np.roll(full, (roll[0], roll[1]), axis=(-1, -2))
    return np.ascontiguousarray(rolled[:, start[0]:start[0] + th, start[1]:start[1] + tw])


def _evaluate(eng, tile, start, roll, bank, seg_rows, masks, sl):
    eng.set_nnfm_targets({'conv3_1': bank}, NNFM_W, 1, K, segments={'conv3_1': seg_rows}, masks=masks)
    try:
        return eng.sc_grad_tile(tile, start, roll, [], sl, LW, {}, SW)
    finally:
        eng.set_nnfm_targets({})


@pytest.mark.parametrize('th,tw,start,roll', TILES)
@pytest.mark.parametrize('case', list(TILE_CASES))
def test_guided_tile_against_the_oracle(case, th, tw, start, roll):
    om, full, bank, seg_rows = _scene()
    sl, masks = TILE_CASES[case], _masks()
    eng = gpu_engine()
    tile = _tile(full, th, tw, start, roll)
    eng.set_contents_and_styles(om.contents, om.styles)
    plain = eng.sc_grad_tile(tile, start, roll, [], sl, LW, {}, SW) if sl else None
    loss, grad = _evaluate(eng, tile, start, roll, bank, seg_rows, masks, sl)
    again = _evaluate(eng, tile, start, roll, bank, seg_rows, masks, sl)
    blobs = om.blob_names[:om.blob_names.index('conv3_1') + 1]
    acts = eng.features_tile(tile, blobs)
    feat = np.ascontiguousarray(acts['conv3_1'], np.float32)
    maps = np.stack([mask_map(m, 4) for m in masks])
    oy, ox, froll = start[0] // 4, start[1] // 4, (roll[0] // 4, roll[1] // 4)
    _, J, e_op, _, a_op = _op(eng, feat, bank, seg_rows, maps, K, oy, ox, froll)        # the GPU's lists
    om.nnfm_banks, om.nnfm_weights = {'conv3_1': np.float64(bank)}, dict(NNFM_W)
    om.nnfm_segments, om.nnfm_masks, om.nnfm_roll = {'conv3_1': seg_rows}, masks, roll
    om.nnfm_k, om.nnfm_index = K, {'conv3_1': J}
    try:
        m = om.weights_of('conv3_1', feat.shape[-2:], start)
        assert np.array_equal(m, ref.windows(maps, oy, ox, feat.shape[1], feat.shape[2], froll))
        same_loss, same_grad = om.sc_grad_tile(tile, start, [], sl, LW, {}, SW, activations=acts)
        term64 = om.nnfm_loss64(acts, LW, start)
    finally:
        om.nnfm_banks, om.nnfm_weights, om.nnfm_index, om.nnfm_segments, om.nnfm_masks = {}, {}, {}, {}, []
    on = ref.searched(m)
    stats = dict(loss=abs(loss / same_loss - 1), term=term64, grad=max_rel(grad, same_grad), a=a_op,
                 searched='%d of %d' % (on.sum(), on.size), moved=max_rel(grad, plain[1]) if plain else None)
    print('nnfm guided tile', case, (th, tw), start, roll, stats)
    assert np.all(np.isfinite(grad)) and grad.any()
    assert again[0] == loss and np.array_equal(again[1], grad)
    assert 0 < a_op < 1                     # the masks' level counts ...
    assert on.sum() < on.size or roll != (0, 0)         # ... and the first tile leaves a pair out
    assert loss == pytest.approx(same_loss, rel=TIGHT), (loss, same_loss)
    if plain:
        assert loss - plain[0] == pytest.approx(term64, abs=2 * TIGHT * loss)
        assert stats['moved'] > 1e-3
    else:
        assert loss == pytest.approx(term64, rel=TIGHT)
    assert stats['grad'] < TIGHT, stats


def test_cleared_targets_restore_the_bits_and_swapped_masks_change_the_term():
    om, full, bank, seg_rows = _scene()
    eng = gpu_engine()
    th, tw, start, roll = TILES[1]
    tile = _tile(full, th, tw, start, roll)
    run = lambda: eng.sc_grad_tile(tile, start, roll, [], SL, LW, {}, SW)
    guided = lambda masks: eng.set_nnfm_targets({'conv3_1': bank}, NNFM_W, 1, K, segments={'conv3_1': seg_rows}, masks=masks)
    eng.set_contents_and_styles(om.contents, om.styles)
    before = run()
    guided(_masks())
    moved = run()
    guided(_masks(swap=True))
    swapped = run()
    guided([np.zeros(FRAME, np.float32)] * 2)
    nothing = run()             # all masks zero: the tile's diff gets nothing (0 / EPS), the loss nothing
    nothing_alone = eng.sc_grad_tile(tile, start, roll, [], [], LW, {}, SW)
    eng.set_nnfm_targets({'conv3_1': bank}, NNFM_W, 1, K)       # any setter replaces the whole set: unguided
    unguided = run()
    guided(_masks())
    back = run()
    eng.set_nnfm_targets({})
    cleared = run()
    guided(_masks())
    eng.set_contents_and_styles(om.contents, om.styles)         # clears the banks with their masks
    fresh = run()
    assert moved[0] != before[0] and not np.array_equal(moved[1], before[1])
    assert swapped[0] != moved[0] and not np.array_equal(swapped[1], moved[1])
    assert unguided[0] != moved[0] and unguided[0] != before[0]
    # (a second gradient term at conv3_1 takes the Gram term off the fused epilogue: the same sum by another kernel)
    assert nothing[0] == before[0] and max_rel(nothing[1], before[1]) < TIGHT
    assert nothing_alone[0] == 0 and not nothing_alone[1].any()
    assert back[0] == moved[0] and np.array_equal(back[1], moved[1])
    assert cleared[0] == before[0] and np.array_equal(cleared[1], before[1])
    assert fresh[0] == before[0] and np.array_equal(fresh[1], before[1])
    # masks of another frame surface as the window range error
    guided([m[:40, :40] for m in _masks()])
    with pytest.raises(lib.StxError, match='mask'):
        run()
    eng.set_nnfm_targets({})


def _digests(eng, full, bank, seg_rows):
    result = {}
    for case, sl in TILE_CASES.items():
        for i, (th, tw, start, roll) in enumerate(TILES):
            loss, grad = _evaluate(eng, _tile(full, th, tw, start, roll), start, roll, bank, seg_rows, _masks(), sl)
            result['%s %d' % (case, i)] = [float(loss).hex(), hashlib.sha256(np.ascontiguousarray(grad).tobytes()).hexdigest()]
    return result


def _sums_in_place_child(scene_path, out_path):
    """In a process of its own with STX_SUMS_LATE=0: every setting's loss and gradient, as hex and a digest."""
    os.environ['STX_SUMS_LATE'] = '0'
    with open(scene_path, 'rb') as f:
        contents, styles, full, bank, seg_rows = pickle.load(f)
    eng = gpu_engine()
    eng.set_contents_and_styles(contents, styles)
    result = _digests(eng, full, bank, seg_rows)
    eng.close()
    with open(out_path, 'w') as f:
        json.dump(result, f)


def test_sums_in_place_give_the_same_bits(tmp_path):
    """STX_SUMS_LATE=0 in a fresh process against the default here."""
    om, full, bank, seg_rows = _scene()
    eng = gpu_engine()
    eng.set_contents_and_styles(om.contents, om.styles)
    here = _digests(eng, full, bank, seg_rows)
    scene, out = str(tmp_path / 'scene.pkl'), str(tmp_path / 'child.json')
    with open(scene, 'wb') as f:
        pickle.dump((om.contents, om.styles, full, bank, seg_rows), f)
    code = 'import sys; sys.path.insert(0, %r); from tests.test_gpu_nnfm_guided import _sums_in_place_child; ' \
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


def test_cli_run_with_half_masks_lowers_the_term(tmp_path, monkeypatch, capsys):
    rng = np.random.RandomState(6)
    picture = lambda hw: Image.fromarray(np.uint8(rng.uniform(0, 255, hw + (3,))))
    picture((96, 128)).save(tmp_path / 'c.png')
    picture((96, 128)).save(tmp_path / 's1.png')
    picture((64, 80)).save(tmp_path / 's2.png')
    left = np.zeros((96, 128), np.uint8)
    left[:, :64] = 255
    Image.fromarray(left).save(tmp_path / 'left.png')
    Image.fromarray(255 - left).save(tmp_path / 'right.png')
    # the term alone: no Gram, the content term at weight 0, no regulariser -- the logged loss is weight E / 2
    alone = ['-si', '../s1.png', '../s2.png', '-i', '20', '--nnfm-weight', '1', '--nnfm-layers', 'conv3_1',
             '--style-layers', '--content-layers', 'conv3_2', '-cw', '0', '-tw', '0', '-pw', '0']
    first = nnfm_ref.bank_rows(24, 32)          # the first picture's rows, as tests/test_gpu_nnfm_knn.py counts them
    lr = _cli_run(tmp_path, monkeypatch, capsys, 'lr', alone + ['--nnfm-masks', '../left.png', '../right.png'])
    with capsys.disabled():
        print('20 Adam steps, left / right masks, E / 2: %.6f -> %.6f' % (lr[2][0], lr[2][-1]))
    assert lr[0].shape == (96, 128, 3) and len(lr[2]) == 20 and np.all(np.isfinite(lr[2]))
    assert lr[2][-1] < lr[2][0]
    assert re.search(r"nnfm_masks=\['\.\./left\.png', '\.\./right\.png'\]", lr[1])
    line = re.search(r'NNFM bank rows: conv3_1 (\d+) \((\d+) \+ (\d+)\)\n', lr[3])
    assert line, lr[3]
    total, seg0, seg1 = map(int, line.groups())
    assert seg0 == first and seg1 > 0 and total == seg0 + seg1
    rl = _cli_run(tmp_path, monkeypatch, capsys, 'rl', alone + ['--nnfm-masks', '../right.png', '../left.png'])
    assert not np.array_equal(lr[0], rl[0]) and lr[2] != rl[2]          # which picture goes where matters
    bare = _cli_run(tmp_path, monkeypatch, capsys, 'bare', alone)
    assert 'nnfm_masks' not in bare[1] and 'NNFM bank rows: conv3_1 %d\n' % total in bare[3], bare[3]
