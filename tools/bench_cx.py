"""Device time of the contextual style term (cx.hip), step by step, and beside a tile evaluation.

    python tools/bench_cx.py [--out profiles/cx_times.txt]

At the conv4_2 shape (512 x 128^2) and the conv3_2 shape (256 x 256^2) of a 1024^2 tile and at the conv4_2 shape of a
256^2 tile (512 x 32^2), with --cx-points 1024 and 4096 against banks of M = 1024, 4096 and 16384 rows where points x M
stays within 2^24, the engine's per-group event timing gives the five groups of stx_op_cx_terms: `prepare` (the unit
columns of F - mu on the sample grid), `score` (s = X B^T with the slots of the row maxima), `rows` (the row pass: k*,
tau, p), `cols` (the column pass and the second row pass: i*, CX, g) and `grad` (q = g B in K slices, then its
projection into the blob's layout, with the clearing of the gradient array where the grid skips pixels).

Floors.  The products run on the fp32 matrix cores: 2 N M C flop each -- one in `score`, one in `grad` -- at the
157.3 TFLOP/s of that pipe.  The row pass reads s, writes e, reads it and writes p: 16 N M bytes; the column pass
reads p, the second row pass reads p and writes g: 12 N M bytes; both at the 6.3 TB/s the project takes as the
achievable HBM rate; matrices that fit the Infinity Cache can come in under the floor.

For the comparison DESIGN.md 3.23 makes, the same run times selfsim_grad_kernel's group (`selfsim grad`, K = N) at
the first shape with 1024 and 4096 points against ITS floor of 2 N^2 C flop.

Then the term at its defaults (conv3_2 and conv4_2, 1024 points, a bank of 4096 rows) beside the tile evaluation
itself: stx_sc_grad_tile (conv4_2 content, five Gram layers) on a 1024^2 and a 256^2 tile, device-event time per
evaluation without and with the targets, in the same run.
"""

import argparse
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                              # noqa: E402
from style_transfer_amd import lib                                        # noqa: E402
from style_transfer_amd.config_system import (CX_H_DEFAULT, CX_LAYERS_DEFAULT, CX_MAX_CELLS, CX_POINTS_DEFAULT,  # noqa: E402
                                              CX_ROWS_DEFAULT, selfsim_grid)
from style_transfer_amd.engine import TileEngine                          # noqa: E402
from style_transfer_amd.netspec import builtin_net                        # noqa: E402
from style_transfer_amd.weights import synthetic_weights                  # noqa: E402

HBM_BYTES_PER_S = 6.3e12
FP32_MATRIX_FLOPS = 157.3e12
SHAPES = [(1024, 'conv4_2', 512, 128), (1024, 'conv3_2', 256, 256), (256, 'conv4_2', 512, 32)]
POINTS = (1024, 4096)
BANKS = (1024, 4096, 16384)
GROUPS = ('prepare', 'score', 'rows', 'cols', 'grad')


def group_ms(eng, call, reps, term='cx', groups=GROUPS):
    """Median device ms of every group of `call`."""
    for _ in range(3):
        call()
    eng.profile(True)
    times = {g: [] for g in groups}
    for _ in range(reps):
        call()
        rows = [(label.split(), ms) for label, ms, _ in eng.profile_read()]
        for g in groups:
            times[g].append(sum(ms for words, ms in rows if words[:2] == [term, g]))
    eng.profile(False)
    return {g: float(np.median(v)) for g, v in times.items()}


def fill(eng, rng, c, n):
    """A [c, n, n] device blob of rectified noise, made in slabs: the host array stays small."""
    feat = eng.empty((c, n, n))
    block = np.maximum(rng.standard_normal((c, min(n, 64), n)) + 0.3, 0).astype(np.float32)
    for y0 in range(0, n, block.shape[1]):
        slab = eng.to_device(np.ascontiguousarray(np.roll(block, y0, axis=2)))
        eng.map_place(feat, y0, 0, slab)
        eng.sync()
        slab.free()
    return feat


def device_bank(eng, rng, M, c):
    """(bank [M, c], mu [c]) on the device, by stx_cx_bank from rectified noise."""
    raw = eng.to_device(np.maximum(rng.standard_normal((M, c)) + 0.3, 0).astype(np.float32))
    bank, mu = eng.empty((M, c)), eng.empty((c,))
    lib.call('stx_cx_bank', eng.handle, raw.ptr, lib.DEVICE, c, M, mu.ptr, bank.ptr, lib.DEVICE)
    raw.free()
    return bank, mu


def tile_ms(eng, tile, grad, cl, sl, cw, sw, reps):
    times = []
    for i in range(reps + 2):
        eng.sc_grad_tile_async(tile, (0, 0), (0, 0), cl, sl, {}, cw, sw, grad_out=grad)
        eng.sync()
        if i >= 2:
            times.append(eng.last_tile_ms())
    return float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=10)
    opts = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_cx: no GPU')
    net = builtin_net('vgg19')
    eng = TileEngine(net, 0, synthetic_weights(net, 0))
    rng = np.random.RandomState(0)
    lines = ['# --cx-weight: the contextual style term (cx.hip), device-event ms',
             '# device: %s; median of %d calls after 3 warm-up calls' % (torch.cuda.get_device_name(0), opts.reps),
             '# matrix floor: 2 N M C flop per product at 157.3 TFLOP/s (fp32 MFMA); score and grad hold one each',
             '# byte floors: rows 16 N M bytes, cols 12 N M bytes, at 6.3 TB/s',
             '%5s %8s %4s %5s %6s %5s %6s %8s %8s %8s %8s %8s %8s %9s %8s %8s %8s %8s'
             % ('tile', 'blob', 'C', 'side', 'points', 'N', 'M', 'prepare', 'score', 'rows', 'cols', 'grad', 'total',
                'prod flr', 'score x', 'grad x', 'rows x', 'cols x')]
    for tile, name, c, side in SHAPES:
        feat = fill(eng, rng, c, side)
        s_out = eng.empty((c, side, side))
        for M in BANKS:
            bank, mu = device_bank(eng, rng, M, c)
            for points in POINTS:
                if points * M > CX_MAX_CELLS:
                    continue
                g, gh, gw = selfsim_grid(side, side, points)
                N = gh * gw
                out = (ctypes.c_double * 2)()
                call = lambda: lib.call('stx_op_cx_terms', eng.handle, feat.ptr, c, side, side, points, bank.ptr, mu.ptr,
                                        M, CX_H_DEFAULT, s_out.ptr, out, None, None)
                t = group_ms(eng, call, opts.reps)
                product = 2.0 * N * M * c / FP32_MATRIX_FLOPS * 1e3
                rows_floor, cols_floor = (16.0 * N * M / HBM_BYTES_PER_S * 1e3, 12.0 * N * M / HBM_BYTES_PER_S * 1e3)
                lines.append('%5d %8s %4d %5d %6d %5d %6d %8.4f %8.4f %8.4f %8.4f %8.4f %8.4f %9.4f %8.2f %8.2f %8.2f %8.2f'
                             % (tile, name, c, side, points, N, M, t['prepare'], t['score'], t['rows'], t['cols'],
                                t['grad'], sum(t.values()), product, t['score'] / product, t['grad'] / product,
                                t['rows'] / rows_floor, t['cols'] / cols_floor))
                print(lines[-1], flush=True)
            bank.free()
            mu.free()
        if (tile, name) == SHAPES[0][:2]:       # the sibling's gradient product in the same run
            lines.append('# selfsim_grad_kernel with its projection (K = N) at this shape, against 2 N^2 C flop:')
            for points in POINTS:
                N = int(np.prod(selfsim_grid(side, side, points)[1:]))
                out = (ctypes.c_double * 2)()
                call = lambda: lib.call('stx_op_selfsim_terms', eng.handle, feat.ptr, feat.ptr, c, side, side, points,
                                        s_out.ptr, out, None)
                t = group_ms(eng, call, opts.reps, 'selfsim', ('grad',))
                product = 2.0 * N * N * c / FP32_MATRIX_FLOPS * 1e3
                lines.append('#   points %d N %d: grad %.4f ms, floor %.4f ms, x %.2f' % (points, N, t['grad'], product,
                                                                                         t['grad'] / product))
                print(lines[-1], flush=True)
        for buf in (feat, s_out):
            buf.free()
    # ---- the term at its defaults beside the tile evaluation
    cl, sl = ['conv4_2'], ['conv1_1', 'conv2_1', 'conv3_1', 'conv4_1', 'conv5_1']
    cw, sw = {'conv4_2': 0.05}, {l: 0.2 for l in sl}
    lines += ['#', '# stx_sc_grad_tile (conv4_2 content, five Gram layers), device-event ms per evaluation, without and '
              'with', '# contextual targets at %s with %d points, banks of %d rows, h %g (weight 1)'
              % (' '.join(CX_LAYERS_DEFAULT), CX_POINTS_DEFAULT, CX_ROWS_DEFAULT, CX_H_DEFAULT),
              '%5s %10s %10s %10s %9s' % ('tile', 'without', 'with', 'term ms', 'of tile')]
    for size in (1024, 256):
        contents = [{l: np.abs(rng.standard_normal(eng.feature_shape(l, size, size))).astype(np.float32) for l in cl}]
        styles = [{l: np.tril(rng.standard_normal((eng.layer_info(l)[1],) * 2)).astype(np.float32) for l in sl}]
        eng.set_contents_and_styles(contents, styles)
        tile = eng.to_device(rng.uniform(-120, 120, (3, size, size)).astype(np.float32))
        grad = eng.empty((3, size, size))
        without = tile_ms(eng, tile, grad, cl, sl, cw, sw, opts.reps)
        banks = {l: np.maximum(rng.standard_normal((CX_ROWS_DEFAULT, eng.layer_info(l)[1])) + 0.3, 0).astype(np.float32)
                 for l in CX_LAYERS_DEFAULT}
        eng.set_cx_targets(banks, None, CX_POINTS_DEFAULT, CX_H_DEFAULT)
        with_term = tile_ms(eng, tile, grad, cl, sl, cw, sw, opts.reps)
        eng.set_cx_targets({})
        lines.append('%5d %10.3f %10.3f %10.3f %9.2f' % (size, without, with_term, with_term - without,
                                                        (with_term - without) / without))
        print(lines[-1], flush=True)
        tile.free()
        grad.free()
    text = '\n'.join(lines) + '\n'
    if opts.out:
        os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
        with open(opts.out, 'w') as f:
            f.write(text)
    else:
        print(text)
    eng.close()


if __name__ == '__main__':
    main()
