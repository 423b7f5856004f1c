"""The 3 x 3 patch form of the nearest-neighbour term (--nnfm-patch 3) on the GPU: the patch kernels of nnfm.hip
through stx_op_nnfm_patch_terms and stx_nnfm_patch_bank, the tile path and the command line -- against
tests/nnfm_patch_ref.py (float64 on the same float32 inputs).  The bounds are those of tests/test_gpu_nnfm.py,
applied in the same way.

Bounds.
  * Planted inputs (a window of a random style map times one alpha in [1e-2, 1e3] and a per-pixel factor in
    [0.5, 2], plus 1e-3 alpha of unit noise per column, against the map's stride-1 patch bank; the float64 winner
    leads the runner-up by more than 1e-2, asserted before the GPU is asked): every index equals the float64
    argmax.  E, sum |S| and S are printed only there (cancelled differences, as in the plain term's test).
  * Exact ties (duplicated bank rows across block and slice boundaries; all-zero scores): the lowest index.
  * Random inputs: cos64(X_p, b_jgpu) >= max_j cos64 - tau for every patch, tau = 4 x the worst
    |emulated score - float64 score| of the case in cosine units (nnfm_patch_ref.search_error).
  * E, sum |S| (relative) and S (of max |S_ref|) to 1e-5 (TIGHT) against the reference AT THE GPU'S OWN INDICES.
  * stx_nnfm_patch_bank: the row count, rows to 1e-6 of the reference's unit patches.
  * The tile path: the loss to TIGHT of the float64 term on the GPU's activations, the gradient to TIGHT of the
    oracle's backward pass on the GPU's activations fed the reference's S.

Observed worst values on an MI355X over the 48 op-level shapes, the case at C = 512 and the sliced case: emulated
search error 1.14e-7 (tau 4.6e-7), the GPU's worst excess over the float64 maximum 0 (each of the 25 447 patches
took the float64 argmax), E 8.7e-8, sum |S| 4.1e-7, S 2.3e-7 of its maximum; the planted windows' smallest lead
0.142, every winner the patch at the same position; bank rows 2.1e-8; the tiles' loss 3.7e-7, their gradient
1.7e-6 of its maximum; the command-line run's figures are in DESIGN 3.16.  Every case prints its figures before it
asserts (pytest -s)."""

import ctypes
import functools
import re

import numpy as np
import pytest
from PIL import Image

from oracle.caffe_net import synthetic_weights
from style_transfer_amd import lib
from style_transfer_amd.netspec import builtin_net
from tests import nnfm_patch_ref as ref
from tests.gpu_helpers import TIGHT, gpu_engine, max_rel

pytestmark = pytest.mark.gpu

CHANNELS = [64, 256]                                            # 18 and 72 stages
MAPS = [(1, 1), (1, 7), (2, 2), (3, 5), (31, 33), (45, 47)]     # centre only; no row above or below; ...; a query
ROWS = [1, 31, 129, 1000]                                       # block spans rows; ragged last bank blocks
ERR_ARG, ERR_UNSUPPORTED = -1, -4


def _unit_rows(rng, m, width):
    b = rng.standard_normal((m, width))
    return (b / np.linalg.norm(b, axis=1, keepdims=True)).astype(np.float32)


def _op(eng, feat, bank, patch=3, profile=False, name='stx_op_nnfm_patch_terms'):
    """(S, j, E, sum |S|[, the search's slice count]) of stx_op_nnfm_patch_terms (or of the plain entry point)."""
    c, h, w = feat.shape
    d_feat, d_bank = eng.to_device(feat), eng.to_device(bank)
    s_out = eng.empty((c, h, w))
    idx = eng.empty((h * w,), np.int32)
    out = (ctypes.c_double * 2)()
    if profile:
        eng.profile(True)
    try:
        if name == 'stx_op_nnfm_patch_terms':
            lib.call(name, eng.handle, d_feat.ptr, c, h, w, patch, d_bank.ptr, bank.shape[0], s_out.ptr, idx.ptr, out)
        else:
            lib.call(name, eng.handle, d_feat.ptr, c, h, w, d_bank.ptr, bank.shape[0], s_out.ptr, idx.ptr, out)
        result = (s_out.get(), idx.get().astype(np.int64), out[0], out[1])
        if profile:
            labels = [row[0] for row in eng.profile_read()]
            slices = [int(m.group(1)) for m in (re.fullmatch(r'nnfm patch search op x(\d+)', l) for l in labels) if m]
            assert len(slices) == 1, labels
            assert 'nnfm patch prepare op' in labels and 'nnfm patch grad op' in labels
            result += (slices[0],)
    finally:
        if profile:
            eng.profile(False)
        for arr in (d_feat, d_bank, s_out, idx):
            arr.free()
    return result


def _held_at_own_indices(tag, feat, bank, s, j, e, asum, hold=True):
    e_ref, s_ref, asum_ref, _ = ref.terms_at(feat, bank, j)
    s_err = max_rel(s, s_ref) if np.abs(s_ref).max() > 0 else float(np.abs(s).max())
    e_err = abs(e / e_ref - 1) if e_ref else abs(e)
    a_err = abs(asum / asum_ref - 1) if asum_ref else abs(asum)
    print('%s: E %.6g (%.2e), sum|S| %.6g (%.2e), S %.2e of max' % (tag, e, e_err, asum, a_err, s_err))
    assert np.all(np.isfinite(s)) and np.isfinite(e) and np.isfinite(asum)
    if hold:
        assert s_err <= TIGHT and a_err <= TIGHT and e_err <= TIGHT


def _random_case(eng, tag, feat, bank, twice=True):
    n = feat.shape[1] * feat.shape[2]
    scores = ref.scores64(feat, bank)
    tau = 4 * ref.search_error(feat, bank)
    s, j, e, asum = _op(eng, feat, bank)
    assert j.min() >= 0 and j.max() < bank.shape[0]
    excess = scores.max(axis=1) - scores[np.arange(n), j]
    print('%s random: emulated worst %.2e, tau %.2e, worst excess %.2e, %d of %d patches off the float64 argmax'
          % (tag, tau / 4, tau, excess.max(), np.count_nonzero(j != np.argmax(scores, axis=1)), n))
    assert np.all(excess <= tau), (tag, float(excess.max()), tau)
    _held_at_own_indices(tag + ' random', feat, bank, s, j, e, asum)
    if twice:
        s2, j2, e2, asum2 = _op(eng, feat, bank)
        assert s.tobytes() == s2.tobytes() and np.array_equal(j, j2) and e == e2 and asum == asum2


@pytest.mark.parametrize('m', ROWS)
@pytest.mark.parametrize('h,w', MAPS)
@pytest.mark.parametrize('c', CHANNELS)
def test_patch_kernels_against_float64(c, h, w, m):
    eng = gpu_engine()
    rng = np.random.RandomState(c + 7 * h + 13 * w + m)
    bank = _unit_rows(rng, m, 9 * c)
    feat = (rng.standard_normal((c, h, w)) * 10.0 ** rng.uniform(-2, 3)).astype(np.float32)
    _random_case(eng, 'C %d %dx%d M %d' % (c, h, w, m), feat, bank)


def test_patch_kernels_at_512_channels():
    eng = gpu_engine()
    rng = np.random.RandomState(512)
    bank = _unit_rows(rng, 129, 9 * 512)
    _random_case(eng, 'C 512 7x9 M 129', rng.standard_normal((512, 7, 9)).astype(np.float32), bank)


# windows (y0, x0, h, w) of the 33 x 31 style map: interior ones and ones flush with its border; the whole map
WINDOWS = [(16, 15, 1, 1), (0, 0, 1, 1), (10, 9, 3, 5), (0, 26, 3, 5), (28, 0, 5, 7), (11, 12, 5, 7), (1, 0, 31, 31),
           (0, 0, 33, 31)]


@functools.lru_cache(maxsize=None)
def _style_map(c):
    rng = np.random.RandomState(c)
    style = rng.standard_normal((c, 33, 31)).astype(np.float32)
    return style, ref.patch_bank_of(style).astype(np.float32)


@pytest.mark.parametrize('window', WINDOWS, ids=lambda v: '%d_%d_%dx%d' % v)
@pytest.mark.parametrize('c', CHANNELS)
def test_planted_windows_take_the_float64_argmax(c, window):
    eng = gpu_engine()
    style, bank = _style_map(c)
    y0, x0, h, w = window
    rng = np.random.RandomState(c + y0 + 3 * x0 + 5 * h)
    alpha = 10.0 ** rng.uniform(-2, 3)
    noise = rng.standard_normal((c, h, w))
    noise /= np.linalg.norm(noise, axis=0, keepdims=True)
    feat = alpha * (style[:, y0:y0 + h, x0:x0 + w] * rng.uniform(0.5, 2, (h, w)) + 1e-3 * noise)
    feat = np.ascontiguousarray(feat, np.float32)
    scores = ref.scores64(feat, bank)
    j_ref = np.argmax(scores, axis=1)
    top2 = np.partition(scores, -2, axis=1)[:, -2:]
    lead = float((top2[:, 1] - top2[:, 0]).min())
    same = np.count_nonzero(j_ref == ((y0 + np.arange(h))[:, None] * 31 + x0 + np.arange(w)).ravel())
    print('planted C %d window %s alpha %.3g: smallest lead %.3f, %d of %d winners at the same position'
          % (c, window, alpha, lead, same, h * w))
    assert lead > 1e-2, 'the planted winner is not separated'
    s, j, e, asum = _op(eng, feat, bank)
    assert np.array_equal(j, j_ref), np.flatnonzero(j != j_ref)[:8]
    _held_at_own_indices('planted', feat, bank, s, j, e, asum, hold=False)


def test_the_sliced_bank_path():
    """n = 64 patches against M = 6000 rows: one query block, the bank cut across workgroups and merged."""
    eng = gpu_engine()
    rng = np.random.RandomState(6000)
    c, h, w, m = 64, 8, 8, 6000
    bank = _unit_rows(rng, m, 9 * c)
    feat = rng.standard_normal((c, h, w)).astype(np.float32)
    slices = _op(eng, feat, bank, profile=True)[4]
    print('sliced: %d slices' % slices)
    assert slices > 1
    _random_case(eng, 'sliced', feat, bank, twice=False)


@pytest.mark.parametrize('h,w', [(8, 8), (181, 181)])
def test_exact_ties_take_the_lowest_index(h, w):
    """Bank rows duplicated across the 128-row blocks -- the slices of the 8 x 8 map (one query block) and the
    steps of one workgroup's walk for the 181 x 181 map (256 query blocks: no slicing).  Every bank row has its
    centre tap alone; the map's pixels at odd y and odd x are multiples of such a row's centre and all
    others are zero, so a patch there is a multiple of the row and scores the same on every copy -- and every
    other patch sees one pixel at a tap that no row has: all its scores are exactly 0 and row 0 is taken."""
    eng = gpu_engine()
    rng = np.random.RandomState(h)
    c, m = 64, 700
    centre = _unit_rows(rng, m, c)
    groups = [(5, 130), (127, 128), (100, 300, 650), (255, 256, 699)]
    for g in groups:
        for k in g[1:]:
            centre[k] = centre[g[0]]
    bank = np.zeros((m, 9, c), np.float32)
    bank[:, 4] = centre
    bank = bank.reshape(m, 9 * c)
    ys, xs = np.arange(1, h, 2), np.arange(1, w, 2)
    pick = rng.randint(0, m, (len(ys), len(xs)))
    copies = [k for g in groups for k in g]
    pick.ravel()[:len(copies)] = copies
    alpha = (2.0 ** rng.randint(-6, 10, pick.shape)).astype(np.float32)
    feat = np.zeros((c, h, w), np.float32)
    feat[:, 1::2, 1::2] = (alpha[..., None] * centre[pick]).transpose(2, 0, 1)
    lowest = {k: g[0] for g in groups for k in g}
    j_ref = np.zeros((h, w), np.int64)
    j_ref[1::2, 1::2] = np.vectorize(lambda k: lowest.get(k, k))(pick)
    j_ref = j_ref.ravel()
    if h == 8:
        assert np.array_equal(j_ref, ref.nearest(feat, bank))
    s, j, e, asum, slices = _op(eng, feat, bank, profile=True)
    print('ties %dx%d: %d slices' % (h, w, slices))
    assert (slices > 1) == (h == 8)
    assert np.array_equal(j, j_ref), np.flatnonzero(j != j_ref)[:8]


def test_zero_patches_and_zero_rows():
    eng = gpu_engine()
    rng = np.random.RandomState(3)
    c, h, w, m = 64, 9, 11, 140
    bank = _unit_rows(rng, m, 9 * c)
    bank[[0, 7, 128, 139]] = 0
    feat = rng.standard_normal((c, h, w)).astype(np.float32)
    feat[:, 2:7, 3:8] = 0           # a 5 x 5 hole: the patches centred at (3..5, 4..6) are all zero
    s, j, e, asum = _op(eng, feat, bank)
    zero = [y * w + x for y in (3, 4, 5) for x in (4, 5, 6)]
    scores = ref.scores64(feat, bank)
    assert np.all(np.isfinite(s)) and np.isfinite(e) and np.isfinite(asum)
    assert np.all(j[zero] == 0)
    assert not s[:, 4, 5].any()     # the hole's centre: every patch that reads it is zero -- no contribution
    live = np.setdiff1d(np.arange(h * w), zero)
    assert np.array_equal(j[live], np.argmax(scores, axis=1)[live])     # ... and its neighbours are correct
    assert np.all(scores[live, j[live]] > 0) and not np.isin(j[live], [0, 7, 128, 139]).any()
    assert np.array_equal(j, ref.nearest(feat, bank))
    _held_at_own_indices('zeros', feat, bank, s, j, e, asum)


def test_a_bank_of_the_blob_itself_matches_every_patch_to_itself():
    eng = gpu_engine()
    rng = np.random.RandomState(17)
    c, h, w = 64, 31, 33
    feat = rng.standard_normal((c, h, w)).astype(np.float32)
    d_bank = eng.nnfm_bank(feat, 1, 3)
    bank = d_bank.get()
    d_bank.free()
    assert bank.shape == (h * w, 9 * c)
    tau = 4 * ref.search_error(feat, bank)
    s, j, e, asum = _op(eng, feat, bank)
    print('patch self-match: tau %.2e, E %.3e' % (tau, e))
    assert np.array_equal(j, np.arange(h * w))
    assert 0 <= e + 1e-7 and e <= 2 * tau


def test_patch_1_gives_the_bytes_of_the_plain_entry_points():
    eng = gpu_engine()
    rng = np.random.RandomState(11)
    c, h, w, m = 64, 9, 13, 150
    feat = rng.standard_normal((c, h, w)).astype(np.float32)
    bank = _unit_rows(rng, m, c)
    old, new = _op(eng, feat, bank, name='stx_op_nnfm_terms'), _op(eng, feat, bank, patch=1)
    assert old[0].tobytes() == new[0].tobytes() and np.array_equal(old[1], new[1]) and old[2:] == new[2:]
    d_feat = eng.to_device(feat)
    for stride in (1, 2):
        b = eng.nnfm_bank(d_feat, stride, 1)
        a, out = eng.empty(b.shape), eng.empty(b.shape)
        lib.call('stx_nnfm_bank', eng.handle, d_feat.ptr, lib.DEVICE, c, h, w, stride, a.ptr, lib.DEVICE)
        lib.call('stx_nnfm_patch_bank', eng.handle, d_feat.ptr, lib.DEVICE, c, h, w, 1, stride, out.ptr, lib.DEVICE)
        assert a.get().tobytes() == b.get().tobytes() == out.get().tobytes()
        for arr in (a, b, out):
            arr.free()
    d_feat.free()
    om, full, _ = _scene()
    style_bank = np.ascontiguousarray(_scene()[2].reshape(-1, 9, 256)[:, 4])      # any [rows, 256] array
    eng.set_contents_and_styles(om.contents, om.styles)
    run = lambda: eng.sc_grad_tile(full, (0, 0), (0, 0), [], SL, LW, {}, SW)
    d_bank = eng.to_device(style_bank)
    table = (lib.NnfmTarget * 1)()          # the plain setter itself (TileEngine sets both forms as patch targets)
    t = table[0]
    t.layer, t.channels, t.rows, t.bank, t.mem = b'conv3_1', 256, style_bank.shape[0], d_bank.ptr, lib.DEVICE
    t.weight = NNFM_W['conv3_1']
    lib.call('stx_set_nnfm_targets', eng.handle, table, 1)
    eng.primary.extra_taps['nnfm'] = ['conv3_1']
    plain = run()
    table = (lib.NnfmPatchTarget * 1)()
    t = table[0]
    t.layer, t.channels, t.patch, t.rows, t.bank, t.mem = b'conv3_1', 256, 1, style_bank.shape[0], d_bank.ptr, lib.DEVICE
    t.weight = NNFM_W['conv3_1']
    lib.call('stx_set_nnfm_patch_targets', eng.handle, table, 1)
    eng.primary.extra_taps['nnfm'] = ['conv3_1']
    try:
        through_patch = run()
    finally:
        eng.set_nnfm_targets({})
    assert plain[0] == through_patch[0] and np.array_equal(plain[1], through_patch[1])


def test_argument_errors_leave_the_output_alone():
    eng = gpu_engine()
    feat = eng.to_device(np.ones((64, 4, 4), np.float32))
    wide = eng.to_device(np.ones((96, 4, 4), np.float32))
    bank = eng.to_device(np.ones((3, 9 * 64), np.float32) / 24)
    s_out = eng.to_device(np.full((96, 4, 4), 7.0, np.float32))
    idx = eng.to_device(np.full((16,), 9, np.int32), np.int32)
    out = (ctypes.c_double * 2)(5.0, 5.0)
    call = lambda f, c, patch, bank_ptr, rows: lib.call('stx_op_nnfm_patch_terms', eng.handle, f.ptr, c, 4, 4, patch,
                                                        bank_ptr, rows, s_out.ptr, idx.ptr, out)
    cases = (((feat, 64, 2, bank.ptr, 3), ERR_ARG), ((feat, 64, 0, bank.ptr, 3), ERR_ARG),
             ((wide, 96, 3, bank.ptr, 3), ERR_UNSUPPORTED), ((feat, 64, 3, None, 3), ERR_ARG),
             ((feat, 64, 3, bank.ptr, 0), ERR_ARG), ((feat, 64, 3, bank.ptr, -2), ERR_ARG))
    for args, code in cases:
        with pytest.raises(lib.StxError) as err:
            call(*args)
        assert err.value.code == code, (args[1:], err.value.code)
    bank_out = eng.to_device(np.full((16, 9 * 96), 7.0, np.float32))
    for c, patch, code in ((64, 2, ERR_ARG), (96, 3, ERR_UNSUPPORTED)):
        with pytest.raises(lib.StxError) as err:
            lib.call('stx_nnfm_patch_bank', eng.handle, wide.ptr, lib.DEVICE, c, 4, 4, patch, 1, bank_out.ptr, lib.DEVICE)
        assert err.value.code == code
    assert np.all(s_out.get() == 7.0) and np.all(idx.get() == 9) and list(out) == [5.0, 5.0]
    assert np.all(bank_out.get() == 7.0)
    table = (lib.NnfmPatchTarget * 1)()
    t = table[0]
    t.layer, t.channels, t.patch, t.rows, t.bank, t.mem, t.weight = b'conv1_1', 64, 2, 3, bank.ptr, lib.DEVICE, 1.0
    with pytest.raises(lib.StxError) as err:
        lib.call('stx_set_nnfm_patch_targets', eng.handle, table, 1)
    assert err.value.code == ERR_ARG
    with pytest.raises(lib.StxError) as err:        # 9 x 64 values a row are not conv3_1's 9 x 256
        eng.set_nnfm_targets({'conv3_1': np.ones((3, 9 * 64), np.float32)}, patch=3)
    assert err.value.code == ERR_ARG
    call(feat, 64, 3, bank.ptr, 3)      # and the same arrays in order are taken
    assert np.all(np.isfinite(s_out.get())) and np.all(idx.get() < 3)
    for arr in (feat, wide, bank, s_out, idx, bank_out):
        arr.free()


@pytest.mark.parametrize('h,w', [(5, 7), (31, 33)])
@pytest.mark.parametrize('stride', [1, 2, 3])
def test_patch_bank_against_float64(stride, h, w):
    eng = gpu_engine()
    rng = np.random.RandomState(h + stride)
    feat = np.maximum(rng.standard_normal((64, h, w)), 0).astype(np.float32)
    feat[:, :2, :2] = 0             # the patch centred at (0, 0) is all zero
    expect = ref.patch_bank_of(feat, stride)
    d_bank = eng.nnfm_bank(eng.to_device(feat), stride, 3)
    bank = d_bank.get()
    again = np.empty_like(bank)     # from the host, to the host
    lib.call('stx_nnfm_patch_bank', eng.handle, feat.ctypes.data, lib.HOST, 64, h, w, 3, stride, again.ctypes.data,
             lib.HOST)
    assert bank.shape == expect.shape == (ref.bank_rows(h, w, stride), 9 * 64)
    err = float(np.abs(bank - expect).max())
    print('patch bank %dx%d stride %d: %d rows, %.2e' % (h, w, stride, bank.shape[0], err))
    assert err <= 1e-6 and not bank[0].any()
    assert np.all(np.abs(np.linalg.norm(np.float64(bank[1:]), axis=1) - 1) <= 1e-6)
    assert bank.tobytes() == again.tobytes()


# --------------------------------------------------------------------------------- the tile path
SL = ['conv1_1', 'conv2_1', 'conv3_1']
SW = {l: 1 / 3 for l in SL}
LW = {'conv3_1': 1.5}
NNFM_W = {'conv3_1': 0.7}
TILE_CASES = {'alone': ([], []), 'gram': ([], SL), 'content': (['conv3_2'], [])}


@functools.lru_cache(maxsize=None)
def _scene():
    """Oracle with targets of a 64 x 64 frame and the conv3_1 patch bank of a 40 x 44 style picture, computed once."""
    net = builtin_net('vgg19')
    om = ref.NnfmPatchOracleModel(net.as_dicts(), synthetic_weights(net.as_dicts(), 0))
    rng = np.random.RandomState(29)
    full = rng.uniform(-110, 120, (3, 64, 64)).astype(np.float32)
    style = rng.uniform(-110, 120, (3, 40, 44)).astype(np.float32)
    om.styles = [om.style_grams([style], SL, 512)]
    om.contents = [om.prepare_features(full, ['conv3_2'], 512)]
    bank = ref.patch_bank_of(om.features_tile(style, ['conv3_1'])['conv3_1']).astype(np.float32)
    return om, full, bank


@pytest.mark.parametrize('case', list(TILE_CASES))
def test_patch_tile_against_the_oracle(case, monkeypatch):
    """The term alone (no tap at all), beside a Gram term on the same blob and beside a content term on the blob
    above; then the same call with the sums in place (STX_SUMS_LATE=0): the same bits."""
    om, full, bank = _scene()
    cl, sl = TILE_CASES[case]
    cw = {l: 0.05 for l in cl}
    eng = gpu_engine()
    start, roll = (0, 0), (0, 0)
    eng.set_contents_and_styles(om.contents, om.styles)
    plain = eng.sc_grad_tile(full, start, roll, cl, sl, LW, cw, SW) if cl or sl else None
    eng.set_nnfm_targets({'conv3_1': bank}, NNFM_W, patch=3)
    om.nnfm_banks, om.nnfm_weights = {'conv3_1': np.float64(bank)}, dict(NNFM_W)
    try:
        loss, grad = eng.sc_grad_tile(full, start, roll, cl, sl, LW, cw, SW)
        again = eng.sc_grad_tile(full, start, roll, cl, sl, LW, cw, SW)
        monkeypatch.setenv('STX_SUMS_LATE', '0')
        in_place = eng.sc_grad_tile(full, start, roll, cl, sl, LW, cw, SW)
        monkeypatch.delenv('STX_SUMS_LATE')
        deepest = om.deep_to_shallow(cl + sl + ['conv3_1'])[0]
        blobs = om.blob_names[:om.blob_names.index(deepest) + 1]
        acts = eng.features_tile(full, blobs)
        same_loss, same_grad = om.sc_grad_tile(full, start, cl, sl, LW, cw, SW, activations=acts)
        term64 = om.nnfm_loss64(acts, LW)
    finally:
        om.nnfm_banks, om.nnfm_weights = {}, {}
        eng.set_nnfm_targets({})
    stats = dict(loss=abs(loss / same_loss - 1), term=term64, grad=max_rel(grad, same_grad),
                 moved=max_rel(grad, plain[1]) if plain else None)
    print('nnfm patch tile', case, stats)
    assert np.all(np.isfinite(grad)) and grad.any()
    assert again[0] == loss and np.array_equal(again[1], grad)
    assert in_place[0] == loss and np.array_equal(in_place[1], grad)
    assert loss == pytest.approx(same_loss, rel=TIGHT), (loss, same_loss)
    if plain:
        assert loss - plain[0] == pytest.approx(term64, abs=2 * TIGHT * loss)
        assert stats['moved'] > 1e-3        # the term is not lost in the others
    else:
        assert loss == pytest.approx(term64, rel=TIGHT)
    assert stats['grad'] < TIGHT, stats


def test_cleared_targets_change_no_bit():
    om, full, bank = _scene()
    eng = gpu_engine()
    cl, cw = ['conv3_2'], {'conv3_2': 0.05}
    run = lambda: eng.sc_grad_tile(full, (0, 0), (0, 0), cl, SL, LW, cw, SW)
    eng.set_contents_and_styles(om.contents, om.styles)
    before = run()
    eng.set_nnfm_targets({'conv3_1': bank}, NNFM_W, patch=3)
    moved = run()
    assert moved[0] != before[0] and not np.array_equal(moved[1], before[1])
    # either setter replaces the whole set: a plain bank takes the patch bank's place
    eng.set_nnfm_targets({'conv3_1': np.ascontiguousarray(bank.reshape(-1, 9, 256)[:, 4])}, NNFM_W)
    replaced = run()
    assert replaced[0] != moved[0] and replaced[0] != before[0]
    eng.set_nnfm_targets({'conv3_1': bank}, NNFM_W, patch=3)
    back = run()
    assert back[0] == moved[0] and np.array_equal(back[1], moved[1])
    eng.set_contents_and_styles(om.contents, om.styles)                  # clears the banks
    cleared = run()
    assert cleared[0] == before[0] and np.array_equal(cleared[1], before[1])


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


def _bank_rows(sizes_hw, stride):
    """Rows of the concatenated conv3_1 bank (two poolings: ceil(size / 4) a side) of style pictures of these sizes."""
    return sum(ref.bank_rows(-(-hh // 4), -(-ww // 4), stride) for hh, ww in sizes_hw)


def test_cli_patch_runs_lower_the_term_and_concatenate_the_banks(tmp_path, monkeypatch, capsys):
    rng = np.random.RandomState(5)
    picture = lambda hw: Image.fromarray(np.uint8(rng.uniform(0, 255, hw + (3,))))
    picture((96, 128)).save(tmp_path / 'c.png')
    picture((96, 128)).save(tmp_path / 's.png')
    picture((64, 80)).save(tmp_path / 't.png')
    # the term alone: no Gram, the content term at weight 0, no regulariser -- the logged loss is weight E / 2
    alone = ['--nnfm-weight', '1', '--nnfm-layers', 'conv3_1', '--style-layers', '--content-layers', 'conv3_2', '-cw', '0',
             '-tw', '0', '-pw', '0']
    one = _cli_run(tmp_path, monkeypatch, capsys, 'one', ['-si', '../s.png', '-i', '20', '--nnfm-patch', '3'] + alone)
    with capsys.disabled():     # (the figure for DESIGN 3.16; capsys holds what a passing test prints)
        print('20 Adam steps, patch 3, E / 2: %.6f -> %.6f' % (one[2][0], one[2][-1]))
    assert one[0].shape == (96, 128, 3) and len(one[2]) == 20 and np.all(np.isfinite(one[2]))
    assert one[2][-1] < one[2][0]
    assert re.search(r'nnfm_patch=3', one[1])
    assert 'NNFM bank rows: conv3_1 %d; patch 3\n' % _bank_rows([(96, 128)], 1) in one[3], one[3]
    two = _cli_run(tmp_path, monkeypatch, capsys, 'two',
                   ['-si', '../s.png', '../t.png', '-i', '2', '--nnfm-stride', '2', '--nnfm-patch', '3'] + alone)
    both = [(96, 128), (64, 80)]
    assert _bank_rows(both, 2) == 12 * 16 + 8 * 10
    assert 'NNFM bank rows: conv3_1 %d; patch 3\n' % _bank_rows(both, 2) in two[3], two[3]
    bare = _cli_run(tmp_path, monkeypatch, capsys, 'bare', ['-si', '../s.png', '-i', '2'] + alone)
    flagged = _cli_run(tmp_path, monkeypatch, capsys, 'flagged', ['-si', '../s.png', '-i', '2', '--nnfm-patch', '1'] + alone)
    assert np.array_equal(bare[0], flagged[0]) and bare[2] == flagged[2]
    assert 'nnfm_patch' not in bare[1] and 'NNFM bank rows: conv3_1 %d\n' % _bank_rows([(96, 128)], 1) in bare[3]
    assert not np.array_equal(bare[0], two[0])
