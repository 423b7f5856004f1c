"""Every stx_op_* hook under guard bands (tests/guarded.py): what the kernels do AROUND their arrays.

One table, CASES.  Per case every device operand -- x, w, b, dy, the mask blob, features, targets, banks, maps and
every float, int or byte output -- lies between NaN guards, the outputs pre-filled with poison, and the case asserts
  1. the values, against the float64 reference of the hook's own test file at that file's bound (2e-5 of max for the
     convolutions and the style terms, exact MAX / 1e-6 AVE pooling, 1e-5 content terms, the term files' own bounds;
     no bound here is new);
  2. an empty verdict: no guard word changed, no output element left unwritten, no input changed, nothing non-finite;
  3. that engine-held scratch (the packed bank in the upload buffer, the split-K workspace, the amax slots, the term
     scratch) does not leak between calls: case A, a case of another shape and family, A again -- the same bits.
The hook names of the table are the stx_op_* names of lib.SIGNATURES, all of them (test_the_table_covers_every_hook).
`pytest -s` prints, per case, the branch it reaches and the worst value error beside its bound.

The branch beside a convolution row -- family, tiling, and 'unsplit', 'split f' or 'tail' -- is stated in the table
and held to the launchers' own arithmetic, restated in tests/conv_plan.py (conv_dispatch.cpp: conv_choose;
conv_h2.hip: h2_plan; conv_wino2.hip: wino2_uniform_plan, wino2_tail_plan; conv_mfma.hip: conv_pick_config,
direct_splitk_factor), by test_the_conv_rows_state_the_launchers_plan here and on the CPU by
tests/test_guarded_host.py.  It matters which: an unsplit launch stores y from its own epilogue (where a ragged
channel tile's surplus channels would go astray), a split one stores into the engine's workspace and only the
reduce pass touches y.  Both models slice K on every small plane as soon as a slice keeps enough chunks (fp16-split:
from 4 chunk pairs, K >= 128; fp32 Winograd and direct: from 8 chunks of 8, K >= 57), so the unsplit rows with a
ragged channel tile have K = 64 / 96 (fp16-split) and K = 56 (the others).  The other branches are from reading
conv_small_launch, splitk_reduce_launch, conv_first_launch and pool.hip's grid_for.
Rows that differ from the list they were drawn up from:
  * 64 -> 66 at 17 x 35 under wino2a / b / c runs SPLIT in two both ways (8 and 9 chunks), and so do 72 -> 40 at
    19 x 67 forward (9 chunks) and 128 -> 130 at 9 x 33 under h2a / b / c (4 chunk pairs); the backward passes of
    64 -> 66, 96 -> 130 and 128 -> 130 under a forced fp16-split tiling fall to the Winograd kernel by geometry,
    split too.  They stay, labelled as what they are, and 56 -> 66 / 66 -> 56 at 17 x 35 (Winograd, direct) and
    96 -> 130 at 9 x 33 (fp16-split, a 128-channel tile 2 over) join them as the unsplit ragged rows.
  * 72 -> 40 at 19 x 67 under wino2a has NO ragged K chunk in that kernel (its chunk is 8 channels, 72 = 9 x 8).
    20 -> 36 at 19 x 31 joins it: 2.5 chunks of 8.
  * direct 3 x 3: the three listed rows are all unsplit (at most 5 chunks; 130 -> 20 forward runs variant 3, which
    has no partial epilogue).  64 -> 66 at 17 x 35 is added as the split direct row.
  * Pooling with C = 70 at 129 x 131 has 70 x 65 x 66 = 300 300 outputs, under grid_for's 4096 x 256 threads (the
    kernels run one thread per OUTPUT), so no thread takes a second element.  70 planes of 257 x 259 have 1 173 900.
  * 64 -> 512 at 9 x 11 is added beside 512 -> 64: the backward pass of the latter has K = 64 and cannot split, so
    without it no split launch would run the reduce pass's mask.
  * stx_op_pool_backward reads its mask argument as a flag only (the mask IS the pool input), so no mask blob is
    built for it; pool_bwd_codes_kernel's float2 store is not reachable through a hook.
Documented partly written outputs: winner_out of stx_op_nnfm_cover_terms at cover 0 (include/stx.h: "out[2] and
winner_out untouched") -- the case states the whole array as untouched.

Pointer alignment (test_pointer_alignment_branches): only launchers that test the pointer themselves get a pointer
that is float- but not 16-byte aligned -- y of conv_first_launch, dy of conv_small_launch, y and the mask of
splitk_reduce_launch.  Bit-identity: the reduce pass says so itself ("bit-identical either way"); conv_first_kernel
computes the tile into LDS and STORE 0 / 1 differ in the store instruction only (16-byte or four dword buffer
stores of the same registers); conv3x3_m4_kernel<VEC> differs in how the patch is LOADED into LDS (16-byte loads
plus halo dwords, or dwords), the LDS contents and the MFMA order are the same.  Every other operand stays 16-byte
aligned: no other launcher states a contract for less."""

import collections
import ctypes
import functools

import numpy as np
import pytest

from oracle import layers as L
from oracle import num_ops
from style_transfer_amd import lib
from tests import (conv_plan, cx_ref, nnfm_cover_ref, nnfm_guided_ref, nnfm_knn_ref, nnfm_patch_ref, nnfm_ref, selfsim_ref,
                   shift_ref, stat_ref, swd_ref)
from tests.content_mask_ref import masked_content_terms
from tests.gpu_helpers import TIGHT, gpu_engine, max_rel
from tests.guarded import guarded_call
from tests.masked_style_ref import masked_style_terms

pytestmark = pytest.mark.gpu

SWITCHES = ('STX_CONV_ALGO', 'STX_CONV_SYMM', 'STX_CONV_H2', 'STX_CONV_H2_BWD', 'STX_GRAM', 'STX_SYMM', 'STX_WINO2_TAIL',
            'STX_REDUCE_VEC', 'STX_SMALL_NOVEC', 'STX_CONV_FIRST_FUSED', 'STX_FIRST_WGS', 'STX_FIRST_STRIDED')
Case = collections.namedtuple('Case', 'hook name branch env run')
CASES = []


def _case(hook, name, branch, run, env=None):
    CASES.append(Case(hook, name, branch, dict(env or {}), run))


def _f64(a):
    return np.asarray(a, np.float64)


def _rel(got, ref):
    return abs(got / ref - 1) if ref else abs(got)


class Worst:
    """The worst value error of a case beside its bound; hold() asserts and keeps it for the printed line."""

    def __init__(self):
        self.ratio, self.text = -1.0, 'nothing held'

    def hold(self, what, err, bound):
        err, bound = float(err), float(bound)
        ratio = err / bound if bound > 0 else (0.0 if err == 0 else np.inf)
        if ratio > self.ratio:
            self.ratio, self.text = ratio, '%s %.2e of bound %.2e' % (what, err, bound)
        assert err <= bound, (what, err, bound)


# ------------------------------------------------------------------------------------------ convolutions
@functools.lru_cache(maxsize=None)
def _conv_data(cin, cout, h, w, ks):
    """Operands as tests/test_gpu_kernels.py draws them, and the four float64 references (oracle.layers on float64
    operands), computed once and never written to."""
    rng = np.random.RandomState(cin * 7 + cout + h)
    x = rng.standard_normal((cin, h, w)).astype(np.float32)
    wt = (rng.standard_normal((cout, cin, ks, ks)) * np.sqrt(2 / (ks * ks * cin))).astype(np.float32)
    b = (0.1 * rng.standard_normal(cout)).astype(np.float32)
    dy = rng.standard_normal((cout, h, w)).astype(np.float32)
    below = np.maximum(x, 0)
    for a in (x, wt, b, dy, below):
        a.setflags(write=False)
    return x, wt, b, dy, below


@functools.lru_cache(maxsize=None)
def _conv_ref(cin, cout, h, w, ks, direction):
    x, wt, b, dy, below = _conv_data(cin, cout, h, w, ks)
    pad = ks // 2
    if direction == 'f':
        fwd = L.conv_forward(_f64(x), _f64(wt), _f64(b), pad=pad)
        return np.maximum(fwd, 0), fwd
    bwd = L.conv_backward_data(_f64(dy), _f64(wt), pad=pad)
    return bwd, bwd * (below > 0)


def _conv_forward(eng, shape, relu, off=None):
    cin, cout, h, w, ks = shape
    x, wt, b, _, _ = _conv_data(*shape)
    off = off or {}
    with guarded_call(eng, 'conv forward %r relu %d' % (shape, relu)) as g:
        dx_, dw, db = g.input('x', x), g.input('w', wt), g.input('b', b)
        y = g.output('y', (cout, h, w), offset=off.get('y', 0))
        lib.call('stx_op_conv_forward', eng.handle, dx_.ptr, cin, h, w, dw.ptr, db.ptr, cout, ks, relu, y.ptr)
    return g.out['y']


def _conv_backward(eng, shape, masked, off=None):
    cin, cout, h, w, ks = shape
    _, wt, _, dy, below = _conv_data(*shape)
    off = off or {}
    with guarded_call(eng, 'conv backward %r mask %d' % (shape, masked)) as g:
        ddy, dw = g.input('dy', dy, offset=off.get('dy', 0)), g.input('w', wt)
        mask = g.input('mask', below, offset=off.get('mask', 0)) if masked else None
        gx = g.output('dx', (cin, h, w), offset=off.get('dx', 0))
        lib.call('stx_op_conv_backward_data', eng.handle, ddy.ptr, cout, h, w, dw.ptr, cin, ks,
                 mask.ptr if masked else None, gx.ptr)
    return g.out['dx']


def _run_conv(direction, cin, cout, h, w, ks=3):
    shape = (cin, cout, h, w, ks)

    def run(eng, worst):
        out = {}
        if direction == 'f':
            for relu, ref in zip((1, 0), _conv_ref(*shape, 'f')):
                out['y relu %d' % relu] = got = _conv_forward(eng, shape, relu)
                worst.hold('forward relu %d' % relu, max_rel(got, ref), 2e-5)
            assert np.count_nonzero(out['y relu 1']) < out['y relu 1'].size or cout * h * w < 8
        else:
            for masked, ref in zip((0, 1), _conv_ref(*shape, 'b')):
                out['dx mask %d' % masked] = got = _conv_backward(eng, shape, masked)
                worst.hold('backward mask %d' % masked, max_rel(got, ref), 2e-5)
        return out
    return run


CONV_PLANS = []         # (direction, Cin, Cout, H, W, ksize, STX_CONV_ALGO, the branch the row states)


def _conv_rows(rows, ks=3):
    """rows: (Cin, Cout, H, W, STX_CONV_ALGO or None, the forward branch, the backward branch, comment).  A branch is
    stated in the words of tests/conv_plan.py (family, tiling, 'unsplit' / 'split f' / 'tail items x slices'; None:
    that direction is not run) and test_the_conv_rows_state_the_launchers_plan holds it to the launchers' arithmetic."""
    for cin, cout, h, w, algo, fwd, bwd, comment in rows:
        env = {'STX_CONV_ALGO': algo} if algo else {}
        tag = '%d->%d %dx%d k%d %s' % (cin, cout, h, w, ks, algo or 'default')
        for direction, stated, hook in (('f', fwd, 'stx_op_conv_forward'), ('b', bwd, 'stx_op_conv_backward_data')):
            if stated:
                CONV_PLANS.append((direction, cin, cout, h, w, ks, algo, stated))
                _case(hook, tag, '%s; %s' % (stated, comment), _run_conv(direction, cin, cout, h, w, ks), env)


# fp16-split (conv_h2.hip: 16-channel chunks in pairs, 32-column patches of 8 or 16 rows, 64- or 128-channel tiles).
# h2_plan slices K as soon as a slice keeps two chunk pairs and the plane fits one round of 256 workgroups, so an
# UNSPLIT launch on a small plane has K = 64 or 96.  A backward pass whose gradient has no multiple of 32 channels
# (K = 66, 130) is not h2_usable and falls to the fp32 2-D Winograd kernel by geometry, as in the tile path; with 9
# and 17 chunks of 8 that launch is split.
for _algo, _t in (('h2a', '64x8x32'), ('h2b', '128x8x32'), ('h2c', '64x16x32')):
    _u, _s2, _s8 = 'h2 %s unsplit' % _t, 'h2 %s split 2' % _t, 'h2 %s split 8' % _t
    _conv_rows([
        (64, 64, 9, 33, _algo, _u, _u, 'two chunk pairs, ragged patch rows and columns'),
        (64, 66, 17, 35, _algo, _u, 'wino2 16x16 split 2', 'forward: the epilogue itself stores a ragged channel tile '
         '(66 = 64 + 2), ragged patch rows and columns'),
        (96, 130, 9, 33, _algo, _u, 'wino2 16x16 split 4', 'forward: three chunk pairs, the epilogue itself stores a '
         '128-channel tile 2 channels over'),
        (128, 130, 9, 33, _algo, _s2, 'wino2 16x16 split 4', 'forward: four chunk pairs in two slices; 130 channels '
         'through the reduce pass'),
        (512, 64, 9, 11, _algo, _s8, _u, 'forward: 16 chunk pairs in eight slices + the reduce pass'),
        (64, 512, 9, 11, _algo, _u, _s8, 'backward: eight slices + the reduce pass with the mask')])
# fp32 2-D Winograd (conv_wino2.hip: 8-channel chunks, 64-channel tiles; a: 4 x 64, b: 16 x 16, c: 8 x 32 patches).
# wino2_uniform_plan slices K in two from 8 chunks on wherever the plane fits one round, so an UNSPLIT launch on a
# small plane has K < 64: 56 -> 66 (forward) and 66 -> 56 (backward) store a ragged channel tile from the epilogue.
for _algo, _g in (('wino2a', '4x64'), ('wino2b', '16x16'), ('wino2c', '8x32')):
    _u, _s2, _s8 = 'wino2 %s unsplit' % _g, 'wino2 %s split 2' % _g, 'wino2 %s split 8' % _g
    _conv_rows([
        (72, 40, 19, 67, _algo, _s2, _u, '9 chunks forward (an odd count, sliced 5 + 4), 5 backward; partial channel tiles'),
        (20, 36, 19, 31, _algo, _u, _u, 'ragged K chunk (20 = 2.5 x 8) forward, 36 = 4.5 x 8 backward; one partial tile'),
        (56, 66, 17, 35, _algo, _u, _s2, 'forward: 7 chunks, the epilogue itself stores a ragged channel tile, patch rows '
         'and columns'),
        (66, 56, 17, 35, _algo, _s2, _u, 'backward: 7 chunks, the epilogue itself stores a ragged channel tile under the mask'),
        (64, 66, 17, 35, _algo, _s2, _s2, 'ragged channel tile, patch rows and columns through the reduce pass'),
        (512, 64, 9, 11, _algo, _s8, _s2, 'forward: uniform split 8 ways + the reduce pass'),
        (64, 512, 9, 11, _algo, _s2, _s8, 'backward: uniform split 8 ways + the reduce pass with the mask')])
_conv_rows([
    # direct 3 x 3 (conv_mfma.hip: conv_pick_config, direct_splitk_factor -- slices from 8 chunks of 8 on)
    (20, 36, 19, 31, 'direct', 'direct v5 unsplit', 'direct v3 unsplit', 'ragged chunk (20 = 2.5 x 8), partial channel tile'),
    (8, 33, 1, 1, 'direct', 'direct v5 unsplit', 'direct v3 unsplit', 'a plane of one pixel, 33 channels'),
    (130, 20, 13, 70, 'direct', 'direct v3 unsplit', 'direct v5 unsplit', 'M <= 32 forward (no partial epilogue: never '
     'sliced); 130 channels = three tiles backward, 3 chunks'),
    (56, 66, 17, 35, 'direct', 'direct v5 unsplit', 'direct v5 split 2', 'forward: 7 chunks, the epilogue stores a ragged '
     'channel tile'),
    (64, 66, 17, 35, 'direct', 'direct v5 split 2', 'direct v5 split 2', 'ragged channel tile through the reduce pass')])
_conv_rows([
    # direct 1 x 1: the three size classes of tests/test_gpu_kernels.CONV1X1_CASES (1 x 1 launches are never sliced)
    (64, 64, 17, 23, None, 'direct v12 unsplit', 'direct v12 unsplit', '<= 128 x 128'),
    (64, 128, 130, 131, None, 'direct v6 unsplit', 'direct v7 unsplit', 'above 128 x 128, M >= 128 forward'),
    (72, 40, 129, 130, None, 'direct v7 unsplit', 'direct v7 unsplit', 'M < 128 both ways, partial tile and chunk')], ks=1)
_conv_rows([
    # the first layer (conv_first.hip, forward only: min(H ceil(W / 128), 768) persistent workgroups)
    (3, 64, 33, 47, None, 'first', None, '33 tiles, one per workgroup; W % 4 != 0: dword stores'),
    (3, 64, 12, 64, None, 'first', None, 'W % 4 == 0: 16-byte stores'),
    (3, 64, 1000, 5, None, 'first', None, '1000 tiles on 768 workgroups: some take two, some one'),
    (1, 64, 9, 70, None, 'first', None, 'K = 1'),
    (2, 64, 9, 70, None, 'first', None, 'K = 2')])
_conv_rows([
    # backward into the image (conv_mfma.hip: conv3x3_m4_kernel through conv_small_launch; dy has 64 channels)
    (3, 64, 37, 50, None, None, 'm4', '8-row patches, !VEC (W % 4 != 0)'),
    (3, 64, 24, 128, None, None, 'm4', '8-row patches, VEC; two patch columns'),
    (3, 64, 16369, 6, None, None, 'm4', '16-row patches (1024 patches), !VEC'),
    (3, 64, 16369, 8, None, None, 'm4', '16-row patches (1024 patches), VEC'),
    (1, 64, 9, 66, None, None, 'm4', 'M = 1, !VEC, a second patch column of two pixels')])


def _run_tail_split(eng, worst, switches):
    """128 -> 64 at 259 x 261 under wino2b: 17 x 17 = 289 = 256 + 33 work items; wino2_tail_plan gives 4 slices for
    the last 33 at 67.6 model-us against 77.6 for the best uniform plan (unsplit, two rounds), so the reduce pass
    touches 33 patches of y only.  That the path ran: the bits differ from STX_WINO2_TAIL=0."""
    shape = (128, 64, 259, 261, 3)
    out = {}
    for relu, ref in zip((1, 0), _conv_ref(*shape, 'f')):
        out['y relu %d' % relu] = got = _conv_forward(eng, shape, relu)
        worst.hold('forward relu %d' % relu, max_rel(got, ref), 2e-5)
    switches({'STX_CONV_ALGO': 'wino2b', 'STX_WINO2_TAIL': '0'})
    plain = _conv_forward(eng, shape, 0)
    switches({'STX_CONV_ALGO': 'wino2b'})
    worst.hold('forward, tail split off', max_rel(plain, _conv_ref(*shape, 'f')[1]), 2e-5)
    differ = plain != out['y relu 0']
    assert differ.any(), 'the tail split did not run: the same bits as STX_WINO2_TAIL=0'
    # ... and in the 33 sliced items only, whichever patches of 16 x 16 pixels the work order gives them
    ys, xs = np.nonzero(differ.any(axis=0))
    assert len(set(zip(ys // 16, xs // 16))) <= 33
    return out


_run_tail_split.switches = True
CONV_PLANS.append(('f', 128, 64, 259, 261, 3, 'wino2b', 'wino2 16x16 tail 33x4'))
_case('stx_op_conv_forward', '128->64 259x261 k3 wino2b tail', 'wino2 16x16 tail 33x4; the last 33 of 289 items in 4 '
      'slices + a reduce pass over those patches only', _run_tail_split, {'STX_CONV_ALGO': 'wino2b'})


# ------------------------------------------------------------------------------------------------ pooling
@functools.lru_cache(maxsize=None)
def _pool_data(c, h, w, mode):
    rng = np.random.RandomState(h * 3 + w)
    x = np.maximum(rng.standard_normal((c, h, w)), 0).astype(np.float32)
    x[:, ::3] = 0          # whole windows of zeros: MAX must route to the FIRST element
    ref, aux = L.pool_forward(x, mode)
    dy = rng.standard_normal(ref.shape).astype(np.float32)
    gref = L.pool_backward(dy, x.shape, aux, mode)
    for a in (x, ref, dy, gref):
        a.setflags(write=False)
    return x, ref, dy, gref


def _run_pool(direction, c, h, w, mode):
    code = lib.POOL_MAX if mode == 'MAX' else lib.POOL_AVE

    def run(eng, worst):
        x, ref, dy, gref = _pool_data(c, h, w, mode)
        out = {}
        if direction == 'f':
            with guarded_call(eng, 'pool forward') as g:
                dx_, y = g.input('x', x), g.output('y', ref.shape)
                lib.call('stx_op_pool_forward', eng.handle, dx_.ptr, c, h, w, code, y.ptr)
            out['y'] = g.out['y']
            if mode == 'MAX':
                assert np.array_equal(out['y'], ref)
                worst.hold('forward MAX', 0.0, 0.0)
            else:
                worst.hold('forward AVE', max_rel(out['y'], ref), 1e-6)
            return out
        for masked in (0, 1):
            with guarded_call(eng, 'pool backward mask %d' % masked) as g:
                ddy, dx_, gx = g.input('dy', dy), g.input('x', x), g.output('dx', x.shape)
                lib.call('stx_op_pool_backward', eng.handle, ddy.ptr, dx_.ptr, c, h, w, code,
                         dx_.ptr if masked else None, gx.ptr)
            out['dx mask %d' % masked] = g.out['dx']
            worst.hold('backward mask %d' % masked, max_rel(g.out['dx'], gref * (x > 0) if masked else gref), 1e-6)
        return out
    return run


for _mode in ('MAX', 'AVE'):
    for _c, _h, _w, _branch in ((6, 1, 5, 'one row: windows of one row, a last window of one column'),
                                (6, 33, 2, 'one window per row, a last window of one row'),
                                (6, 7, 9, 'odd both ways'), (6, 64, 96, 'even both ways, several blocks'),
                                (70, 257, 259, '1 173 900 outputs on 4096 x 256 threads: a second grid-stride pass')):
        _case('stx_op_pool_forward', '%s C %d %dx%d' % (_mode, _c, _h, _w), 'pool_fwd_kernel<%s>: %s' % (_mode, _branch),
              _run_pool('f', _c, _h, _w, _mode))
        _case('stx_op_pool_backward', '%s C %d %dx%d' % (_mode, _c, _h, _w),
              'pool_bwd_kernel<%s, mask off / on>: %s' % (_mode, _branch), _run_pool('b', _c, _h, _w, _mode))


# ------------------------------------------------------------------------------------------- the style terms
@functools.lru_cache(maxsize=None)
def _style_data(c, h, w):
    """tests/test_gpu_kernels.test_style_terms_over_channel_counts_and_ranges at big = 1."""
    rng = np.random.RandomState(c + h)
    feat = np.maximum(rng.standard_normal((c, h, w)), 0).astype(np.float32)
    feat[rng.randint(c), rng.randint(h), rng.randint(w)] *= 37.0
    f64 = feat.reshape(c, -1).astype(np.float64)
    g = np.tril(f64 @ f64.T / f64.size)
    target = (g * np.tril(rng.uniform(0.5, 1.5, (c, c)))).astype(np.float32)
    d = np.tril(g - target)
    s_ref = ((d + np.tril(d, -1).T) @ f64).reshape(c, h, w)
    n_ref = s_ref / (np.abs(s_ref).sum() / s_ref.size + float(num_ops.EPS))
    return feat, target, 0.5 * float((d * d).sum()), s_ref, float(np.abs(s_ref).sum()), n_ref


def _run_style(c, h, w, with_norm):
    def run(eng, worst):
        feat, target, half_ref, s_ref, asum_ref, n_ref = _style_data(c, h, w)
        half, asum = ctypes.c_double(), ctypes.c_double()
        with guarded_call(eng, 'style terms') as g:
            d_feat, d_tgt = g.input('feat', feat), g.input('gram_target', target)
            s_out = g.output('s_out', (c, h, w))
            n_out = g.output('normalized_out', (c, h, w)) if with_norm else None
            lib.call('stx_op_style_terms', eng.handle, d_feat.ptr, c, h, w, d_tgt.ptr, s_out.ptr,
                     n_out.ptr if with_norm else None, ctypes.byref(half), ctypes.byref(asum))
        worst.hold('S', max_rel(g.out['s_out'], s_ref), 2e-5)
        worst.hold('1/2 sum D^2', _rel(half.value, half_ref), 2e-5)
        worst.hold('sum |S|', _rel(asum.value, asum_ref), 2e-5)
        if with_norm:
            worst.hold('normalized', max_rel(g.out['normalized_out'], n_ref), 2e-5)
        return dict(g.out, scalars=np.array([half.value, asum.value]))
    return run


for _variant, _env in (('fp16 split', {}), ('fp32', {'STX_GRAM': 'fp32', 'STX_SYMM': 'fp32'}),
                       ('bf3', {'STX_GRAM': 'bf3', 'STX_SYMM': 'bf3'})):
    for _c, _h, _w, _norm, _branch in (
            (68, 9, 11, True, 'ragged channel tile (68 = 64 + 4), 99 pixels; normalized_out given'),
            (128, 40, 33, False, 'two channel tiles, an odd plane'),
            (64, 81, 80, False, 'HW = 6480: 13 Gram slices, the four-way unrolled loop of gram_finish_kernel')):
        _case('stx_op_style_terms', 'C %d %dx%d %s' % (_c, _h, _w, _variant),
              'Gram / SYMM %s: %s' % (_variant, _branch), _run_style(_c, _h, _w, _norm), _env)


# --------------------------------------------------------------------------- the masked terms and the content term
OY, OX = 2, 5


def _behind_a_roll(window, mh, mw, roll, rng):
    """tests/test_gpu_content_mask._behind_a_roll: noise whose roll by `roll` = (x, y) holds `window` at (OY, OX)."""
    h, w = window.shape[-2:]
    rolled = rng.uniform(0, 1, window.shape[:-2] + (mh, mw)).astype(np.float32)
    rolled[..., OY:OY + h, OX:OX + w] = window
    return np.ascontiguousarray(np.roll(rolled, (-roll[0], -roll[1]), axis=(-1, -2)))


def _ramp(h, w):
    return np.outer(np.linspace(0.1, 1, h), np.linspace(0, 1, w)).astype(np.float32)


def _run_masked_style(eng, worst):
    c, h, w = 64, 37, 29                    # tests/test_gpu_style_masks.OP_SHAPES[0], the ramp, big = 1
    rng = np.random.RandomState(c + h + len('ramp'))
    feat = np.maximum(rng.standard_normal((c, h, w)) * 2 + 0.5, 0).astype(np.float32)
    f64 = feat.reshape(c, -1).astype(np.float64)
    gram = np.tril(f64 @ f64.T / f64.size)
    target = (gram * np.tril(rng.uniform(0.5, 1.5, (c, c)))).astype(np.float32)
    mh, mw, roll = h + 6, w + 9, (7, -(h + 2))
    m = _ramp(h, w)
    full = _behind_a_roll(m, mh, mw, roll, rng)
    half_ref, s_ref, asum_ref, a_ref = masked_style_terms(feat, m, target)
    out = (ctypes.c_double * 3)()
    with guarded_call(eng, 'masked style terms') as g:
        d_feat, d_map, d_tgt = g.input('feat', feat), g.input('mask_map', full), g.input('gram_target', target)
        s_out = g.output('sgrad_out', (c, h, w))
        lib.call('stx_op_masked_style_terms', eng.handle, d_feat.ptr, c, h, w, d_map.ptr, mh, mw, OY, OX,
                 (ctypes.c_int * 2)(*roll), d_tgt.ptr, s_out.ptr, out)
    worst.hold('S', np.abs(g.out['sgrad_out'] - s_ref).max() / np.abs(s_ref).max(), 2e-5)
    worst.hold('1/2 sum D^2', _rel(out[0], half_ref), 2e-5)
    worst.hold('sum |m S|', _rel(out[1], asum_ref), 2e-5)
    worst.hold('a', _rel(out[2], a_ref), 1e-6)
    return dict(g.out, scalars=np.array(list(out)))


def _run_masked_content(eng, worst):
    c, h, w = 5, 7, 70                      # tests/test_gpu_content_mask.OP_SHAPES[0], the ramp, big = 1
    rng = np.random.RandomState(c + h + len('ramp'))
    feat = np.maximum(rng.standard_normal((c, h, w)) * 2 + 0.5, 0).astype(np.float32)
    cwin = np.maximum(rng.standard_normal((c, h, w)) * 2 + 0.5, 0).astype(np.float32)
    m = _ramp(h, w)
    mh, mw, roll = h + 6, w + 9, (7, -(h + 2))
    content, full = _behind_a_roll(cwin, mh, mw, roll, rng), _behind_a_roll(m, mh, mw, roll, rng)
    half_ref, s_ref, asum_ref, a_ref = masked_content_terms(feat, cwin, m)
    out = (ctypes.c_double * 3)()
    with guarded_call(eng, 'masked content terms') as g:
        d_feat, d_content, d_map = g.input('feat', feat), g.input('content', content), g.input('mask_map', full)
        s_out = g.output('sgrad_out', (c, h, w))
        lib.call('stx_op_masked_content_terms', eng.handle, d_feat.ptr, c, h, w, d_content.ptr, mh, mw, d_map.ptr,
                 OY, OX, (ctypes.c_int * 2)(*roll), s_out.ptr, out)
    worst.hold('S', np.abs(g.out['sgrad_out'] - s_ref).max() / np.abs(s_ref).max(), 4e-6)
    worst.hold('E', _rel(out[0], half_ref), 2e-5)
    worst.hold('sum |m d|', _rel(out[1], asum_ref), 2e-5)
    worst.hold('a', _rel(out[2], a_ref), 1e-6)
    return dict(g.out, scalars=np.array(list(out)))


def _run_content(eng, worst):
    """tests/test_gpu_kernels.test_content_terms_match_reference_normalize: the rolled window of a content map."""
    from tests.golden import vectors
    feat = vectors.load()['num.feat']                       # [64, 17, 23]
    c, h, w = feat.shape
    content = np.random.RandomState(4).standard_normal((c, 31, 40)).astype(np.float32)
    roll_xy = (-7, 12)
    resid = _f64(feat) - _f64(num_ops.roll_xy(content.copy(), roll_xy)[:, 9:9 + h, 6:6 + w])
    n_ref = resid / (np.abs(resid).sum() / resid.size + float(num_ops.EPS))
    sums = (ctypes.c_double * 2)()
    with guarded_call(eng, 'content terms') as g:
        d_feat, d_content = g.input('feat', feat), g.input('content', content)
        n_out = g.output('normalized_out', (c, h, w))
        lib.call('stx_op_content_terms', eng.handle, d_feat.ptr, c, h, w, d_content.ptr, 31, 40, 9, 6,
                 (ctypes.c_int * 2)(*roll_xy), n_out.ptr, sums)
    worst.hold('normalized', max_rel(g.out['normalized_out'], n_ref), 1e-5)
    worst.hold('sum c^2', _rel(sums[0], float((resid ** 2).sum())), 1e-5)
    worst.hold('sum |c|', _rel(sums[1], float(np.abs(resid).sum())), 1e-5)
    return dict(g.out, scalars=np.array(list(sums)))


_case('stx_op_masked_style_terms', 'C 64 37x29 ramp', 'masked Gram / SYMM: a window behind a roll that wraps on both '
      'axes, 1073 pixels', _run_masked_style)
_case('stx_op_masked_content_terms', 'C 5 7x70 ramp', 'odd C, more than one 64-lane segment per row, a ragged tail',
      _run_masked_content)
_case('stx_op_content_terms', 'C 64 17x23 rolled window', 'the window at (9, 6) of a 31 x 40 map rolled by (-7, 12)',
      _run_content)


# ------------------------------------------------------------------------------------ statistics, SWD, shifted Gram
def _run_stat(eng, worst):
    c, h, w = 64, 5, 7                      # tests/test_gpu_stat.OP_SHAPES[0]: 35 pixels, every channel start misaligned
    rng = np.random.RandomState(c + h + w)
    feat = np.maximum(rng.standard_normal((c, h, w)) * 2 + 0.5, 0).astype(np.float32)
    feat[1] = 0
    feat[2] = 0.3
    feat[3] = 0
    feat[3, h // 2, w // 3] = 7.5
    feat[5] = (1e3 + 0.1 * rng.standard_normal((h, w))).astype(np.float32)
    mu, sd = stat_ref.feature_stats(feat)
    MU = (mu * rng.uniform(0.5, 1.5, c) + 0.05 * rng.standard_normal(c)).astype(np.float32)
    SD = (sd * rng.uniform(0.5, 1.5, c)).astype(np.float32)
    half_ref, s_ref, asum_ref, b_ref = stat_ref.stat_terms(feat, MU, SD)
    out = (ctypes.c_double * 2)()
    with guarded_call(eng, 'stat terms') as g:
        d_feat, d_mu, d_sd = g.input('feat', feat), g.input('MU', MU), g.input('SD', SD)
        s_out = g.output('s_out', (c, h, w))
        lib.call('stx_op_stat_terms', eng.handle, d_feat.ptr, c, h, w, d_mu.ptr, d_sd.ptr, s_out.ptr, out)
    flat = feat.reshape(c, -1)
    bound = TIGHT * np.abs(s_ref).max() + np.abs(b_ref) * np.abs(flat).max(axis=1) * 2.0 ** -23
    s_err = np.abs(g.out['s_out'].reshape(c, -1) - s_ref.reshape(c, -1)).max(axis=1)
    worst.hold('S, of its bound', (s_err / bound).max(), 1.0)
    worst.hold('E / 2', _rel(out[0], half_ref), TIGHT)
    worst.hold('sum |S|', _rel(out[1], asum_ref), TIGHT)
    return dict(g.out, scalars=np.array(list(out)))


def _run_swd(eng, worst):
    c, h, w, d, q = swd_ref.OP_SHAPES[1]                    # (64, 5, 7, 64, 35)
    feat, V, other = swd_ref.case_inputs(c, h, w, d, q)
    tau = swd_ref.tau(feat, V)
    tq = eng.swd_target(other, V, q)
    out = (ctypes.c_double * 2)()
    with guarded_call(eng, 'swd terms') as g:
        d_feat, d_v, d_tq = g.input('feat', feat), g.input('V', V), g.input('Tq', tq)
        s_out, r_out = g.output('s_out', (c, h, w)), g.output('rank_out', (d, h * w), np.int32)
        lib.call('stx_op_swd_terms', eng.handle, d_feat.ptr, c, h, w, d_v.ptr, d, d_tq.ptr, q, s_out.ptr, r_out.ptr, out)
    ranks = g.out['rank_out']
    assert np.array_equal(np.sort(ranks, axis=1), np.broadcast_to(np.arange(h * w), (d, h * w)))
    half_ref, s_ref, asum_ref, _ = swd_ref.terms(feat, V, tq, ranks)
    worst.hold('S', np.abs(g.out['s_out'] - s_ref).max(), TIGHT * np.abs(s_ref).max() + tau.max())
    worst.hold('E / 2', _rel(out[0], half_ref), TIGHT)
    worst.hold('sum |S|', _rel(out[1], asum_ref), TIGHT)
    return dict(g.out, scalars=np.array(list(out)))


def _run_shift(eng, worst):
    c, h, w, offsets = 32, 5, 7, [(0, 1), (1, 0), (0, 6), (4, 0)]           # tests/test_gpu_shift.OP_CASES[0]
    rng = np.random.RandomState(c + h + w)
    feat = np.maximum(rng.standard_normal((c, h, w)) * 2 + 0.5, 0).astype(np.float32)
    feat[1] = 0
    feat[3] = 0
    feat[3, h // 2, w // 3] = 7.5
    own = shift_ref.shift_gram(feat, offsets)
    T = (own * rng.uniform(0.5, 1.5, own.shape)).astype(np.float32)
    half_ref, s_ref, asum_ref = shift_ref.shift_terms(feat, offsets, T)
    out = (ctypes.c_double * 2)()
    flat = (ctypes.c_int * (2 * len(offsets)))(*[v for o in offsets for v in o])
    with guarded_call(eng, 'shift terms') as g:
        d_feat, d_t = g.input('feat', feat), g.input('grams', T)
        s_out = g.output('s_out', (c, h, w))
        lib.call('stx_op_shift_terms', eng.handle, d_feat.ptr, c, h, w, flat, len(offsets), d_t.ptr, s_out.ptr, out)
    worst.hold('S', np.abs(g.out['s_out'] - s_ref).max() / np.abs(s_ref).max(), TIGHT)
    worst.hold('E / 2', _rel(out[0], half_ref), TIGHT)
    worst.hold('sum |S|', _rel(out[1], asum_ref), TIGHT)
    return dict(g.out, scalars=np.array(list(out)))


_case('stx_op_stat_terms', 'C 64 5x7', 'stat.hip: 35 pixels, every channel start misaligned, a constant channel', _run_stat)
_case('stx_op_swd_terms', 'C 64 5x7 D 64 Q 35', 'swd.hip: projections, a device sort of 35 with exact ties, rank_out', _run_swd)
_case('stx_op_shift_terms', 'C 32 5x7, 4 offsets', 'shiftgram.hip: one channel block, one pair per row / one row', _run_shift)


# ------------------------------------------------------------------------------- self-similarity and contextual
def _run_selfsim(eng, worst):
    c, h, w, points = selfsim_ref.OP_SHAPES[1]              # (64, 9, 11, 30)
    feat, content = selfsim_ref.case_inputs(c, h, w, points)
    tau, und, _, N = selfsim_ref.undecided(feat, content, points)
    t64 = selfsim_ref.terms(feat, content, points)[3]
    out = (ctypes.c_double * 2)()
    with guarded_call(eng, 'selfsim terms') as g:
        d_feat, d_content = g.input('feat', feat), g.input('content', content)
        s_out, t_out = g.output('sgrad', (c, h, w)), g.output('signs_out', (N, N), np.int8)
        lib.call('stx_op_selfsim_terms', eng.handle, d_feat.ptr, d_content.ptr, c, h, w, points, s_out.ptr, out, t_out.ptr)
    s, t = g.out['sgrad'], g.out['signs_out']
    differ = t != t64
    assert np.all(np.isin(t, (-1, 0, 1))) and not np.diag(t).any()
    assert not (differ & ~und).any() and differ.sum() <= selfsim_ref.undecided_cap(N)
    e_ref, s_ref, a_ref, _, _ = selfsim_ref.terms(feat, content, points, signs=t)
    e32, s32, a32, _, _ = selfsim_ref.terms32(feat, content, points, signs=t)
    worst.hold('E', abs(out[0] - e_ref), 4 * abs(e32 - e_ref))
    worst.hold('sum |S|', abs(out[1] - a_ref), 4 * abs(a32 - a_ref))
    worst.hold('S', np.abs(s - s_ref).max(), 4 * float(np.abs(s32 - s_ref).max()))
    pos = selfsim_ref.grid(h, w, points)[2]
    on_grid = np.zeros((h, w), bool)
    on_grid[pos[:, 0], pos[:, 1]] = True
    assert not s[:, ~on_grid].view(np.uint32).any()         # exactly 0 off the grid, and written
    return dict(g.out, scalars=np.array(list(out)))


def _run_cx(eng, worst):
    (c, h, w, points, M), eta = cx_ref.OP_CASES[0]          # (64, 5, 7, 1024, 31), eta 0.5
    feat, B, mu = cx_ref.case_inputs(c, h, w, points, M)
    t64 = cx_ref.terms(feat, B, mu, points, eta)
    und_rows, und_cols = cx_ref.undecided(feat, B, mu, points, eta)
    N = cx_ref.grid(h, w, points)[1]
    out = (ctypes.c_double * 2)()
    with guarded_call(eng, 'cx terms') as g:
        d_feat, d_bank, d_mu = g.input('feat', feat), g.input('bank', B), g.input('mu', mu)
        s_out = g.output('sgrad', (c, h, w))
        k_out, w_out = g.output('kbest_out', (N,), np.int32), g.output('winner_out', (M,), np.int32)
        lib.call('stx_op_cx_terms', eng.handle, d_feat.ptr, c, h, w, points, d_bank.ptr, d_mu.ptr, M, float(eta),
                 s_out.ptr, out, k_out.ptr, w_out.ptr)
    s, kstar, winner = g.out['sgrad'], g.out['kbest_out'], g.out['winner_out']
    assert np.all((0 <= kstar) & (kstar < M)) and np.all((0 <= winner) & (winner < N))
    k_differ, w_differ = kstar != t64.kstar, winner != t64.winner
    assert not (k_differ & ~und_rows).any() and not (w_differ & ~und_cols).any()
    assert k_differ.sum() + w_differ.sum() <= cx_ref.undecided_cap(N, M)
    ref = cx_ref.terms(feat, B, mu, points, eta, decisions=(kstar, winner))
    r32 = cx_ref.terms32(feat, B, mu, points, eta, decisions=(kstar, winner))
    worst.hold('E', abs(out[0] - ref.E), 4 * abs(r32.E - ref.E))
    worst.hold('sum |S|', abs(out[1] - ref.abs_sum), 4 * abs(r32.abs_sum - ref.abs_sum))
    worst.hold('S', np.abs(s - ref.S).max(), 4 * float(np.abs(r32.S - ref.S).max()))
    return dict(g.out, scalars=np.array(list(out)))


_case('stx_op_selfsim_terms', 'C 64 9x11 points 30', 'selfsim.hip: a sample grid, int8 signs [N][N], zeros off the grid',
      _run_selfsim)
_case('stx_op_cx_terms', 'C 64 5x7 points 1024 M 31', 'cx.hip: every pixel a query, 31 bank rows (one ragged block), '
      'kbest_out and winner_out', _run_cx)


# ----------------------------------------------------------------------------------- nearest-neighbour matching
def _unit_rows(rng, m, width):
    b = rng.standard_normal((m, width))
    return (b / np.linalg.norm(b, axis=1, keepdims=True)).astype(np.float32)


def _hold_nnfm(worst, got, ref, e, asum):
    """E, sum |S| (relative) and S (of max |S_ref|) to TIGHT, against the reference at the device's own indices."""
    e_ref, s_ref, asum_ref = ref[:3]
    worst.hold('S', max_rel(got, s_ref), TIGHT)
    worst.hold('E', _rel(e, e_ref), TIGHT)
    worst.hold('sum |S|', _rel(asum, asum_ref), TIGHT)


def _run_nnfm(patch):
    """c = 64, a 3 x 5 map (less than an MFMA tile), 31 rows (one ragged bank block): the random inputs of
    tests/test_gpu_nnfm.py / test_gpu_nnfm_patch.py."""
    c, h, w, m = 64, 3, 5, 31
    hook = 'stx_op_nnfm_patch_terms' if patch else 'stx_op_nnfm_terms'

    def run(eng, worst):
        rng = np.random.RandomState(c + 7 * h + 13 * w + m)
        bank = _unit_rows(rng, m, (patch * patch if patch else 1) * c)
        feat = rng.standard_normal((c, h, w)).astype(np.float32)
        ref = nnfm_patch_ref if patch else nnfm_ref
        out = (ctypes.c_double * 2)()
        with guarded_call(eng, hook) as g:
            d_feat, d_bank = g.input('feat', feat), g.input('bank', bank)
            s_out, idx = g.output('s_out', (c, h, w)), g.output('index_out', (h * w,), np.int32)
            form = (patch,) if patch else ()
            lib.call(hook, eng.handle, d_feat.ptr, c, h, w, *form, d_bank.ptr, m, s_out.ptr, idx.ptr, out)
        j = g.out['index_out'].astype(np.int64)
        assert j.min() >= 0 and j.max() < m
        scores = ref.scores64(feat, bank)
        excess = scores.max(axis=1) - scores[np.arange(h * w), j]
        worst.hold('search excess', excess.max(), 4 * ref.search_error(feat, bank))
        _hold_nnfm(worst, g.out['s_out'], ref.terms_at(feat, bank, j), out[0], out[1])
        return dict(g.out, scalars=np.array(list(out)))
    return run


def _run_knn(eng, worst):
    """M = 3 < K = 4 (tests/test_gpu_nnfm_knn.ROWS[0]): the last rank of every query holds -1, written."""
    c, h, w, m, k = 64, 3, 5, 3, 4
    rng = np.random.RandomState(c + 7 * h + 13 * w + m)
    bank = _unit_rows(rng, m, c)
    feat = rng.standard_normal((c, h, w)).astype(np.float32)
    out = (ctypes.c_double * 2)()
    with guarded_call(eng, 'nnfm knn terms') as g:
        d_feat, d_bank = g.input('feat', feat), g.input('bank', bank)
        s_out, idx = g.output('s_out', (c, h, w)), g.output('index_out', (k, h * w), np.int32)
        lib.call('stx_op_nnfm_knn_terms', eng.handle, d_feat.ptr, c, h, w, 1, k, d_bank.ptr, m, s_out.ptr, idx.ptr, out)
    J = g.out['index_out'].astype(np.int64)
    assert np.all(J[m:] == -1) and J[:m].min() >= 0 and J[:m].max() < m
    assert np.array_equal(np.sort(J[:m], axis=0), np.broadcast_to(np.arange(m)[:, None], (m, h * w)))
    _hold_nnfm(worst, g.out['s_out'], nnfm_knn_ref.terms_at(feat, bank, J, 1), out[0], out[1])
    return dict(g.out, scalars=np.array(list(out)))


def _run_cover(cover):
    c, h, w, m, k = 64, 3, 5, 31, 3

    def run(eng, worst):
        rng = np.random.RandomState(c + 7 * h + 13 * w + m)
        bank = _unit_rows(rng, m, c)
        feat = rng.standard_normal((c, h, w)).astype(np.float32)
        out = (ctypes.c_double * 3)(-1.0, -1.0, -1.0)
        with guarded_call(eng, 'nnfm cover terms, cover %g' % cover) as g:
            d_feat, d_bank = g.input('feat', feat), g.input('bank', bank)
            s_out, idx = g.output('s_out', (c, h, w)), g.output('index_out', (k, h * w), np.int32)
            # cover 0 is stx_op_nnfm_knn_terms: "out[2] and winner_out untouched" (include/stx.h)
            win = g.output('winner_out', (m,), np.int32, untouched=np.ones(m, bool) if cover == 0 else None)
            lib.call('stx_op_nnfm_cover_terms', eng.handle, d_feat.ptr, c, h, w, 1, k, float(cover), d_bank.ptr, m,
                     s_out.ptr, idx.ptr, win.ptr, out)
        J = g.out['index_out'].astype(np.int64)
        assert J.min() >= 0 and J.max() < m
        if cover == 0:
            assert out[2] == -1.0
            winner = None
        else:
            winner = g.out['winner_out'].astype(np.int64)
            assert winner.min() >= 0 and winner.max() < h * w
        e_ref, s_ref, asum_ref, e_cov_ref = nnfm_cover_ref.terms_at(feat, bank, J, winner, cover)
        _hold_nnfm(worst, g.out['s_out'], (e_ref, s_ref, asum_ref), out[0], out[1])
        if cover:
            worst.hold('E_cov', _rel(out[2], e_cov_ref), TIGHT)
        return dict(g.out, scalars=np.array(list(out)))
    return run


def _run_guided(eng, worst):
    c, h, w, seg_rows, k = 64, 3, 5, (3, 31), 3             # tests/test_gpu_nnfm_guided: MAPS[1], SEGMENTS[0], random maps
    rng = np.random.RandomState(c + 7 * h + 13 * w + sum(seg_rows))
    n, segments = h * w, len(seg_rows)
    bank = _unit_rows(rng, sum(seg_rows), c)
    feat = (rng.standard_normal((c, h, w)) * 10.0 ** rng.uniform(-2, 3, (h, w))).astype(np.float32)
    m = rng.uniform(0, 1, (segments, n)).astype(np.float32)
    out = (ctypes.c_double * 3)()
    with guarded_call(eng, 'nnfm guided terms') as g:
        d_feat, d_bank = g.input('feat', feat), g.input('bank', bank)
        d_maps = g.input('mask_maps', m.reshape(segments, h, w))
        s_out, idx = g.output('s_out', (c, h, w)), g.output('index_out', (segments, k, n), np.int32)
        lib.call('stx_op_nnfm_guided_terms', eng.handle, d_feat.ptr, c, h, w, k, d_bank.ptr,
                 (ctypes.c_int * segments)(*seg_rows), segments, d_maps.ptr, h, w, 0, 0, (ctypes.c_int * 2)(0, 0),
                 s_out.ptr, idx.ptr, out)
    J = g.out['index_out'].astype(np.int64)
    for s in range(segments):
        assert J[s].min() >= 0 and J[s].max() < seg_rows[s]
    e_ref, s_ref, asum_ref, a_ref = nnfm_guided_ref.terms_at(feat, bank, seg_rows, m, J)
    _hold_nnfm(worst, g.out['s_out'], (e_ref, s_ref, asum_ref), out[0], out[1])
    worst.hold('a', _rel(out[2], a_ref), TIGHT)
    return dict(g.out, scalars=np.array(list(out)))


_case('stx_op_nnfm_terms', 'C 64 3x5 M 31', 'nnfm.hip: 15 queries (less than an MFMA tile), one ragged bank block', _run_nnfm(0))
_case('stx_op_nnfm_patch_terms', 'C 64 3x5 M 31 patch 3', 'nnfm.hip patch kernels: 18 stages, borders on every side', _run_nnfm(3))
_case('stx_op_nnfm_knn_terms', 'C 64 3x5 M 3 K 4', 'nnfm_search_kernel<*, 4> and the K-fold merge: M < K, -1 ranks', _run_knn)
_case('stx_op_nnfm_cover_terms', 'C 64 3x5 M 31 K 3 cover 0.5', 'the reverse search, winner lists, the coverage gradient',
      _run_cover(0.5))
_case('stx_op_nnfm_cover_terms', 'C 64 3x5 M 31 K 3 cover 0', 'cover 0: the k-nearest term; winner_out documented as untouched',
      _run_cover(0.0))
_case('stx_op_nnfm_guided_terms', 'C 64 3x5 segments (3, 31) K 3', 'guided search: two segments, one of exactly K rows; random maps, '
      'every (segment, block) pair searched', _run_guided)


# ------------------------------------------------------------------------------------------------ the tests
def test_the_table_covers_every_hook():
    assert {c.hook for c in CASES} == {k for k in lib.SIGNATURES if k.startswith('stx_op_')}
    assert len({c.hook for c in CASES}) == 18
    assert len({(c.hook, c.name) for c in CASES}) == len(CASES)
    assert all(c.branch for c in CASES)


def test_the_conv_rows_state_the_launchers_plan():
    """Family, tiling and split of every convolution row as the launchers' arithmetic gives them (tests/conv_plan.py
    restates conv_choose, h2_plan, wino2_uniform_plan, wino2_tail_plan and direct_splitk_factor): a row labelled
    'unsplit' stores y from its own epilogue, a 'split' one through the workspace and the reduce pass.  Both kinds
    stand in the table for every family and tiling, with a ragged channel tile above 64 channels in each."""
    for direction, cin, cout, h, w, ks, algo, stated in CONV_PLANS:
        assert conv_plan.branch(direction, cin, cout, h, w, ks, algo) == stated, (direction, cin, cout, h, w, ks, algo)
    stated = {(plan[6], plan[7]) for plan in CONV_PLANS}
    for algo, tiling in (('h2a', 'h2 64x8x32'), ('h2b', 'h2 128x8x32'), ('h2c', 'h2 64x16x32'), ('wino2a', 'wino2 4x64'),
                         ('wino2b', 'wino2 16x16'), ('wino2c', 'wino2 8x32'), ('direct', 'direct v5')):
        assert (algo, tiling + ' unsplit') in stated and (algo, tiling + ' split 2') in stated, (algo, tiling)
    for what, direction, shape, env, operand, stated in ALIGNMENT:
        assert conv_plan.branch(direction, *shape, env.get('STX_CONV_ALGO')) == stated, what


def _set_env(monkeypatch, env):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        assert name in SWITCHES
        monkeypatch.setenv(name, value)


def _by_name(hook, name):
    return next(c for c in CASES if c.hook == hook and c.name == name)


def _other(case):
    """The cases run between A and A: other families and shapes, which fill the scratch A may lean on -- a split
    fp16-split convolution (packed bank in the upload buffer, amax slots, split-K workspace), the style terms (Gram
    partials and scalars; the upload buffer as SYMM scratch) and a k-nearest search (the term scratch buffers)."""
    between = [_by_name('stx_op_conv_forward', '512->64 9x11 k3 h2a'), _by_name('stx_op_style_terms', 'C 128 40x33 fp16 split'),
               _by_name('stx_op_nnfm_knn_terms', 'C 64 3x5 M 3 K 4')]
    if case is between[0]:              # (itself a split forward launch: the split backward one of the other family)
        between[0] = _by_name('stx_op_conv_backward_data', '64->512 9x11 k3 wino2b')
    return [c for c in between if c is not case]


def _run(case, eng, worst, monkeypatch):
    if getattr(case.run, 'switches', False):        # a case that changes a switch half way takes the way to do it
        return case.run(eng, worst, lambda env: _set_env(monkeypatch, env))
    return case.run(eng, worst)


def _same_bits(a, b):
    assert a.keys() == b.keys()
    for key in a:
        assert a[key].dtype == b[key].dtype and a[key].tobytes() == b[key].tobytes(), key


@pytest.mark.parametrize('case', CASES, ids=['%s %s' % (c.hook[7:], c.name) for c in CASES])
def test_hook_under_guard_bands(case, monkeypatch):
    eng = gpu_engine()
    _set_env(monkeypatch, case.env)
    worst = Worst()
    first = _run(case, eng, worst, monkeypatch)
    print('\n%s %s | %s | worst: %s' % (case.hook, case.name, case.branch, worst.text))
    for other in _other(case):
        _set_env(monkeypatch, other.env)
        _run(other, eng, Worst(), monkeypatch)
    _set_env(monkeypatch, case.env)
    again = _run(case, eng, Worst(), monkeypatch)
    _same_bits(first, again)            # A, B, A: engine-held scratch leaks nothing from B into A


# The launchers that test a pointer themselves, at a shape whose rows (for the reduce pass: planes) are a multiple of
# four floats: once with the tested operand 16-byte aligned, once 4 bytes on.  Both runs are guarded and held to the
# float64 reference, and they give the same bits (the module docstring says where the source promises it).
ALIGNMENT = [
    ('conv_first.hip: vec_store, y', 'f', (3, 64, 12, 64, 3), {}, 'y', 'first'),
    ('conv_mfma.hip: conv_small_launch VEC, dy (8-row patches)', 'b', (3, 64, 24, 128, 3), {}, 'dy', 'm4'),
    ('conv_mfma.hip: conv_small_launch VEC, dy (16-row patches)', 'b', (3, 64, 16369, 8, 3), {}, 'dy', 'm4'),
    ('conv_mfma.hip: splitk_reduce_launch vec4, y (forward, fp16-split slices)', 'f', (512, 64, 8, 12, 3),
     {'STX_CONV_ALGO': 'h2a'}, 'y', 'h2 64x8x32 split 8'),
    ('conv_mfma.hip: splitk_reduce_launch vec4, y (forward, fp32 Winograd slices)', 'f', (512, 64, 8, 12, 3),
     {'STX_CONV_ALGO': 'wino2b'}, 'y', 'wino2 16x16 split 8'),
    ('conv_mfma.hip: splitk_reduce_launch vec4, y (backward)', 'b', (64, 512, 8, 12, 3), {'STX_CONV_ALGO': 'h2a'}, 'dx',
     'h2 64x8x32 split 8'),
    ('conv_mfma.hip: splitk_reduce_launch vec4, the mask', 'b', (64, 512, 8, 12, 3), {'STX_CONV_ALGO': 'h2a'}, 'mask',
     'h2 64x8x32 split 8'),
]


@pytest.mark.parametrize('what,direction,shape,env,operand,stated', ALIGNMENT, ids=[a[0] for a in ALIGNMENT])
def test_pointer_alignment_branches(what, direction, shape, env, operand, stated, monkeypatch):
    eng = gpu_engine()
    _set_env(monkeypatch, env)
    got = {}
    for offset in (0, 4):
        if direction == 'f':
            runs = [_conv_forward(eng, shape, relu, {operand: offset}) for relu in (1, 0)]
        else:
            runs = [_conv_backward(eng, shape, masked, {operand: offset}) for masked in ((1,) if operand == 'mask' else (0, 1))]
        got[offset] = runs
    refs = _conv_ref(*shape, 'f' if direction == 'f' else 'b')
    refs = refs[1:] if operand == 'mask' else refs
    for offset, runs in got.items():
        for run, ref in zip(runs, refs):
            err = max_rel(run, ref)
            print('%s, %d bytes on: %.2e of bound 2e-5' % (what, offset, err))
            assert err < 2e-5
    for aligned, shifted in zip(got[0], got[4]):
        assert aligned.tobytes() == shifted.tobytes(), what


def test_the_reduce_pass_gives_the_same_bits_element_wise(monkeypatch):
    """STX_REDUCE_VEC=0 ("bit-identical either way") on the split shape of the alignment cases, under guard bands."""
    eng = gpu_engine()
    shape = (512, 64, 8, 12, 3)
    _set_env(monkeypatch, {'STX_CONV_ALGO': 'h2a'})
    vec = _conv_forward(eng, shape, 1)
    _set_env(monkeypatch, {'STX_CONV_ALGO': 'h2a', 'STX_REDUCE_VEC': '0'})
    assert _conv_forward(eng, shape, 1).tobytes() == vec.tobytes()
