"""Device time of the sliced Wasserstein style term (swd.hip), step by step, and beside a tile evaluation.

    python tools/bench_swd.py [--out profiles/swd_times.txt]

At the blob shapes of a 1024^2 tile -- conv1_1 (64 x 1024^2), conv2_1 (128 x 512^2), conv3_1 (256 x 256^2),
conv4_1 (512 x 128^2) -- and of a 256^2 tile (64 x 256^2 ... 512 x 32^2), with D = C directions (the command
line's default) and 4096 quantiles, the engine's per-group event timing gives the four groups of stx_op_swd_terms:
`project` (V F into sort records), `sort` (every launch of the bitonic network but the last), `rank` (the last
launch: the steps left inside an LDS block, then the rank pass) and `grad` (V^T G / D).

The sort's byte floor: every launch of the network reads and writes every record once, 16 bytes per record and
launch, D x N records (N: n padded to a power of two), at the 6.3 TB/s the project takes as the achievable HBM
rate.  The rank launch is counted like the others (it reads the records and writes G and nothing
else: 12 bytes).  The records of the layers from conv2_1 on at a 256^2 tile fit the Infinity Cache: a time under
the floor there is the cache's doing.  A sort that is far above its floor is bound by the LDS steps inside the
blocks, not by memory.

Then the whole term at the command line's default layers (conv2_1 conv3_1 conv4_1) beside the tile evaluation
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
from style_transfer_amd.config_system import SWD_LAYERS_DEFAULT, SWD_QUANTILES, swd_directions    # noqa: E402
from style_transfer_amd.engine import TileEngine                          # noqa: E402
from style_transfer_amd.netspec import builtin_net                        # noqa: E402
from style_transfer_amd.weights import synthetic_weights                  # noqa: E402

HBM_BYTES_PER_S = 6.3e12
BLOCK = 8192        # records per LDS block (kSwdBlock)
SHAPES = {1024: [('conv1_1', 64, 1024), ('conv2_1', 128, 512), ('conv3_1', 256, 256), ('conv4_1', 512, 128)],
          256: [('conv1_1', 64, 256), ('conv2_1', 128, 128), ('conv3_1', 256, 64), ('conv4_1', 512, 32)]}
GROUPS = ('project', 'sort', 'rank', 'grad')


def padded(n):
    N = 2
    while N < n:
        N *= 2
    return N


def sort_passes(n):
    """Launches of the bitonic network over a row of n records (swd_sort_passes)."""
    N = padded(n)
    B = min(N, BLOCK)
    passes, k = 1, 2 * B
    while k <= N:
        j = k // 2
        while j >= B:       # (up to three steps per pass over global memory)
            j //= 8 if j // 4 >= B else 4 if j // 2 >= B else 2
            passes += 1
        passes += 1
        k *= 2
    return passes


def group_ms(eng, call, reps):
    """Median device ms of every swd group of `call`."""
    for _ in range(3):
        call()
    eng.profile(True)
    times = {g: [] for g in GROUPS}
    for _ in range(reps):
        call()
        rows = [(label.split(), ms) for label, ms, _ in eng.profile_read()]
        for g in GROUPS:
            times[g].append(sum(ms for words, ms in rows if words[:2] == ['swd', g]))
    eng.profile(False)
    return {g: float(np.median(v)) for g, v in times.items()}


def fill(eng, rng, c, n):
    """A [c, n, n] device blob of rectified noise, made in slabs: the host array stays small."""
    feat = eng.empty((c, n, n))
    block = np.maximum(rng.standard_normal((c, min(n, 64), n)), 0).astype(np.float32)
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
        sys.exit('bench_swd: no GPU')
    net = builtin_net('vgg19')
    eng = TileEngine(net, 0, synthetic_weights(net, 0))
    rng = np.random.RandomState(0)
    lines = ['# --swd-weight: the sliced Wasserstein style term (swd.hip), device-event ms',
             '# device: %s; median of %d calls after 3 warm-up calls; D = C directions, Q = %d'
             % (torch.cuda.get_device_name(0), opts.reps, SWD_QUANTILES),
             '# sort floor: launches x 16 bytes x D x N records at 6.3 TB/s (sort + rank are the network: x floor is '
             'theirs together)',
             '%5s %8s %4s %8s %8s %7s %8s %8s %8s %8s %8s %9s %8s' % ('tile', 'blob', 'D', 'n', 'N', 'passes', 'project',
                                                                    'sort', 'rank', 'grad', 'total', 'floor ms',
                                                                    'x floor')]
    for tile, shapes in SHAPES.items():
        for name, c, side in shapes:
            n = side * side
            feat, other = fill(eng, rng, c, side), fill(eng, rng, c, side)
            V = swd_directions(0, name, c, c)
            tq = eng.swd_target(other, V, SWD_QUANTILES)
            other.free()
            d_v, d_tq, s_out = eng.to_device(V), eng.to_device(tq), eng.empty((c, side, side))
            out = (ctypes.c_double * 2)()
            call = lambda: lib.call('stx_op_swd_terms', eng.handle, feat.ptr, c, side, side, d_v.ptr, c, d_tq.ptr,
                                    SWD_QUANTILES, s_out.ptr, None, out)
            t = group_ms(eng, call, opts.reps)
            passes = sort_passes(n)
            floor = passes * 16.0 * c * padded(n) / HBM_BYTES_PER_S * 1e3
            lines.append('%5d %8s %4d %8d %8d %7d %8.4f %8.4f %8.4f %8.4f %8.4f %9.4f %8.2f'
                         % (tile, name, c, n, padded(n), passes, t['project'], t['sort'], t['rank'], t['grad'],
                            sum(t.values()), floor, (t['sort'] + t['rank']) / floor))
            print(lines[-1], flush=True)
            for buf in (feat, d_v, d_tq, s_out):
                buf.free()
    # ---- the term at its default layers beside the tile evaluation
    cl, sl = ['conv4_2'], ['conv1_1', 'conv2_1', 'conv3_1', 'conv4_1', 'conv5_1']
    cw, sw = {'conv4_2': 0.05}, {l: 0.2 for l in sl}
    lines += ['#', '# stx_sc_grad_tile (conv4_2 content, five Gram layers), device-event ms per evaluation, without and '
              'with', '# sliced Wasserstein targets at %s (weight 1 / 3 each)' % ' '.join(SWD_LAYERS_DEFAULT),
              '%5s %10s %10s %10s %9s' % ('tile', 'without', 'with', 'term ms', 'of tile')]
    for size in (1024, 256):
        contents = [{l: np.abs(rng.standard_normal(eng.feature_shape(l, size, size))).astype(np.float32) for l in cl}]
        styles = [{l: np.tril(rng.standard_normal((eng.layer_info(l)[1],) * 2)).astype(np.float32) for l in sl}]
        eng.set_contents_and_styles(contents, styles)
        tile = eng.to_device(rng.uniform(-120, 120, (3, size, size)).astype(np.float32))
        grad = eng.empty((3, size, size))
        without = tile_ms(eng, tile, grad, cl, sl, cw, sw, opts.reps)
        targets = {}
        for layer in SWD_LAYERS_DEFAULT:
            c = eng.layer_info(layer)[1]
            V = swd_directions(0, layer, c, c)
            targets[layer] = (V, np.sort(rng.standard_normal((c, SWD_QUANTILES)).astype(np.float32) * 50, axis=1))
        eng.set_swd_targets(targets, {layer: 1 / 3 for layer in targets})
        with_term = tile_ms(eng, tile, grad, cl, sl, cw, sw, opts.reps)
        eng.set_swd_targets({})
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
