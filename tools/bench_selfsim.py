"""Device time of the self-similarity content term (selfsim.hip), step by step, and beside a tile evaluation.

    python tools/bench_selfsim.py [--out profiles/selfsim_times.txt]

At the conv4_2 shape (512 x 128^2) and the conv3_2 shape (256 x 256^2) of a 1024^2 tile and at the conv4_2 shape of a
256^2 tile (512 x 32^2), with --selfsim-points 1024 and 4096, the engine's per-group event timing gives the four groups
of stx_op_selfsim_terms: `prepare` (both sides' unit columns on the sample grid), `dist` (DX and DC in one launch),
`cols` (the two sweeps of the column pass) and `grad` (q = -(A + A^T) X, then its projection into the blob's layout,
with the clearing of the gradient array where the grid skips pixels).

Floors.  The products run on the fp32 matrix cores: 2 N^2 C flop each -- two of them in `dist`, one in `grad` -- at
the 157.3 TFLOP/s of that pipe.  The column pass reads DX and DC (8 N^2 bytes), writes T (N^2), reads T again and
writes A (4 N^2): 14 N^2 bytes at the 6.3 TB/s the project takes as the achievable HBM rate; at these
sizes the matrices fit the Infinity Cache, and a time under the floor is the cache's doing.

Then the term at its default (conv4_2, 1024 points) beside the tile evaluation itself: stx_sc_grad_tile (conv4_2
content, five Gram layers) on a 1024^2 and a 256^2 tile, device-event time per evaluation without and with the target,
in the same run.
"""

import argparse
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                              # noqa: E402
from style_transfer_amd import lib                                        # noqa: E402
from style_transfer_amd.config_system import SELFSIM_POINTS_DEFAULT, selfsim_grid     # noqa: E402
from style_transfer_amd.engine import TileEngine                          # noqa: E402
from style_transfer_amd.netspec import builtin_net                        # noqa: E402
from style_transfer_amd.weights import synthetic_weights                  # noqa: E402

HBM_BYTES_PER_S = 6.3e12
FP32_MATRIX_FLOPS = 157.3e12
SHAPES = [(1024, 'conv4_2', 512, 128), (1024, 'conv3_2', 256, 256), (256, 'conv4_2', 512, 32)]
POINTS = (1024, 4096)
GROUPS = ('prepare', 'dist', 'cols', 'grad')


def group_ms(eng, call, reps):
    """Median device ms of every selfsim group of `call`."""
    for _ in range(3):
        call()
    eng.profile(True)
    times = {g: [] for g in GROUPS}
    for _ in range(reps):
        call()
        rows = [(label.split(), ms) for label, ms, _ in eng.profile_read()]
        for g in GROUPS:
            times[g].append(sum(ms for words, ms in rows if words[:2] == ['selfsim', g]))
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
        sys.exit('bench_selfsim: no GPU')
    net = builtin_net('vgg19')
    eng = TileEngine(net, 0, synthetic_weights(net, 0))
    rng = np.random.RandomState(0)
    lines = ['# --selfsim-weight: the self-similarity content term (selfsim.hip), device-event ms',
             '# device: %s; median of %d calls after 3 warm-up calls' % (torch.cuda.get_device_name(0), opts.reps),
             '# matrix floor: 2 N^2 C flop per product at 157.3 TFLOP/s (fp32 MFMA); dist holds two products, grad one',
             '# byte floor of cols: 14 N^2 bytes at 6.3 TB/s',
             '%5s %8s %4s %5s %6s %2s %5s %8s %8s %8s %8s %8s %9s %8s %9s %8s %9s %8s'
             % ('tile', 'blob', 'C', 'side', 'points', 'g', 'N', 'prepare', 'dist', 'cols', 'grad', 'total', 'dist flr',
                'x floor', 'grad flr', 'x floor', 'cols flr', 'x floor')]
    for tile, name, c, side in SHAPES:
        feat, other = fill(eng, rng, c, side), fill(eng, rng, c, side)
        s_out = eng.empty((c, side, side))
        for points in POINTS:
            g, gh, gw = selfsim_grid(side, side, points)
            N = gh * gw
            out = (ctypes.c_double * 2)()
            call = lambda: lib.call('stx_op_selfsim_terms', eng.handle, feat.ptr, other.ptr, c, side, side, points,
                                    s_out.ptr, out, None)
            t = group_ms(eng, call, opts.reps)
            product = 2.0 * N * N * c / FP32_MATRIX_FLOPS * 1e3
            cols = 14.0 * N * N / HBM_BYTES_PER_S * 1e3
            lines.append('%5d %8s %4d %5d %6d %2d %5d %8.4f %8.4f %8.4f %8.4f %8.4f %9.4f %8.2f %9.4f %8.2f %9.4f %8.2f'
                         % (tile, name, c, side, points, g, N, t['prepare'], t['dist'], t['cols'], t['grad'],
                            sum(t.values()), 2 * product, t['dist'] / (2 * product), product, t['grad'] / product, cols,
                            t['cols'] / cols))
            print(lines[-1], flush=True)
        for buf in (feat, other, s_out):
            buf.free()
    # ---- the term at its default beside the tile evaluation
    cl, sl = ['conv4_2'], ['conv1_1', 'conv2_1', 'conv3_1', 'conv4_1', 'conv5_1']
    cw, sw = {'conv4_2': 0.05}, {l: 0.2 for l in sl}
    lines += ['#', '# stx_sc_grad_tile (conv4_2 content, five Gram layers), device-event ms per evaluation, without and '
              'with', '# a self-similarity target at conv4_2 with %d points (weight 1)' % SELFSIM_POINTS_DEFAULT,
              '%5s %10s %10s %10s %9s' % ('tile', 'without', 'with', 'term ms', 'of tile')]
    for size in (1024, 256):
        contents = [{l: np.abs(rng.standard_normal(eng.feature_shape(l, size, size))).astype(np.float32) for l in cl}]
        styles = [{l: np.tril(rng.standard_normal((eng.layer_info(l)[1],) * 2)).astype(np.float32) for l in sl}]
        eng.set_contents_and_styles(contents, styles)
        tile = eng.to_device(rng.uniform(-120, 120, (3, size, size)).astype(np.float32))
        grad = eng.empty((3, size, size))
        without = tile_ms(eng, tile, grad, cl, sl, cw, sw, opts.reps)
        eng.set_selfsim_targets({'conv4_2': SELFSIM_POINTS_DEFAULT})
        with_term = tile_ms(eng, tile, grad, cl, sl, cw, sw, opts.reps)
        eng.set_selfsim_targets({})
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
