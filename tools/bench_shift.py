"""Device time of the shifted-Gram style term (shiftgram.hip), step by step, and beside a tile evaluation.

    python tools/bench_shift.py [--out profiles/shift_times.txt]

At the conv1_1, conv2_1 and conv3_1 shapes of a 1024^2 tile (64 x 1024^2, 128 x 512^2, 256 x 256^2) and of a 256^2
tile (64 x 256^2, 128 x 128^2, 256 x 64^2), with the default offsets (--shift-offsets 2 4 8: six offsets), the
engine's per-group event timing gives the three groups of stx_op_shift_terms: `cross` (the slices' partials of every
offset's cross-Gram), `merge` (their sum in slice order against the targets: the gradient's weights and the partials
of E) and `grad` (S as one product over K = 2 |Delta| C with the partials of sum |S|).

Floors.  The products run on the fp32 matrix cores: 2 |Delta| C^2 n flop in `cross`, 4 |Delta| C^2 n in `grad`, at the
157.3 TFLOP/s of that pipe.  `merge` reads the partials and writes the weights: a few MB, launch-bound.

Then the term at its defaults (conv1_1 conv2_1 conv3_1, six offsets) beside the tile evaluation itself:
stx_sc_grad_tile (conv4_2 content, five Gram layers) on a 1024^2 and a 256^2 tile, device-event time per evaluation
without and with the targets, in the same run.
"""

import argparse
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                              # noqa: E402
from style_transfer_amd import lib                                        # noqa: E402
from style_transfer_amd.config_system import SHIFT_LAYERS_DEFAULT, shift_offsets      # noqa: E402
from style_transfer_amd.engine import TileEngine                          # noqa: E402
from style_transfer_amd.netspec import builtin_net                        # noqa: E402
from style_transfer_amd.weights import synthetic_weights                  # noqa: E402

FP32_MATRIX_FLOPS = 157.3e12
SHAPES = [(1024, 'conv1_1', 64, 1024), (1024, 'conv2_1', 128, 512), (1024, 'conv3_1', 256, 256),
          (256, 'conv1_1', 64, 256), (256, 'conv2_1', 128, 128), (256, 'conv3_1', 256, 64)]
GROUPS = ('cross', 'merge', 'grad')


def group_ms(eng, call, reps):
    """Median device ms of every shift group of `call`."""
    for _ in range(3):
        call()
    eng.profile(True)
    times = {g: [] for g in GROUPS}
    for _ in range(reps):
        call()
        rows = [(label.split(), ms) for label, ms, _ in eng.profile_read()]
        for g in GROUPS:
            times[g].append(sum(ms for words, ms in rows if words[:2] == ['shift', g]))
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
        sys.exit('bench_shift: no GPU')
    net = builtin_net('vgg19')
    eng = TileEngine(net, 0, synthetic_weights(net, 0))
    rng = np.random.RandomState(0)
    offsets = shift_offsets(argparse.Namespace())
    flat = (ctypes.c_int * (2 * len(offsets)))(*[v for o in offsets for v in o])
    lines = ['# --shift-weight: the shifted-Gram style term (shiftgram.hip), device-event ms',
             '# device: %s; median of %d calls after 3 warm-up calls' % (torch.cuda.get_device_name(0), opts.reps),
             '# offsets %s' % ' '.join('(%d,%d)' % o for o in offsets),
             '# matrix floor at 157.3 TFLOP/s (fp32 MFMA): cross 2 |Delta| C^2 n flop, grad 4 |Delta| C^2 n flop',
             '%5s %8s %4s %5s %8s %8s %8s %8s %9s %8s %9s %8s'
             % ('tile', 'blob', 'C', 'side', 'cross', 'merge', 'grad', 'total', 'cross flr', 'x floor', 'grad flr',
                'x floor')]
    for tile, name, c, side in SHAPES:
        feat = fill(eng, rng, c, side)
        grams = eng.to_device((rng.standard_normal((len(offsets), c, c)) * 0.01).astype(np.float32))
        s_out = eng.empty((c, side, side))
        out = (ctypes.c_double * 2)()
        call = lambda: lib.call('stx_op_shift_terms', eng.handle, feat.ptr, c, side, side, flat, len(offsets),
                                grams.ptr, s_out.ptr, out)
        t = group_ms(eng, call, opts.reps)
        cross = 2.0 * len(offsets) * c * c * side * side / FP32_MATRIX_FLOPS * 1e3
        lines.append('%5d %8s %4d %5d %8.4f %8.4f %8.4f %8.4f %9.4f %8.2f %9.4f %8.2f'
                     % (tile, name, c, side, t['cross'], t['merge'], t['grad'], sum(t.values()), cross,
                        t['cross'] / cross, 2 * cross, t['grad'] / (2 * cross)))
        print(lines[-1], flush=True)
        for buf in (feat, grams, s_out):
            buf.free()
    # ---- the term at its defaults beside the tile evaluation
    cl, sl = ['conv4_2'], ['conv1_1', 'conv2_1', 'conv3_1', 'conv4_1', 'conv5_1']
    cw, sw = {'conv4_2': 0.05}, {l: 0.2 for l in sl}
    lines += ['#', '# stx_sc_grad_tile (conv4_2 content, five Gram layers), device-event ms per evaluation, without and '
              'with', '# shifted-Gram targets at %s, six offsets (weight 1)' % ' '.join(SHIFT_LAYERS_DEFAULT),
              '%5s %10s %10s %10s %9s' % ('tile', 'without', 'with', 'term ms', 'of tile')]
    for size in (1024, 256):
        contents = [{l: np.abs(rng.standard_normal(eng.feature_shape(l, size, size))).astype(np.float32) for l in cl}]
        styles = [{l: np.tril(rng.standard_normal((eng.layer_info(l)[1],) * 2)).astype(np.float32) for l in sl}]
        eng.set_contents_and_styles(contents, styles)
        tile = eng.to_device(rng.uniform(-120, 120, (3, size, size)).astype(np.float32))
        grad = eng.empty((3, size, size))
        without = tile_ms(eng, tile, grad, cl, sl, cw, sw, opts.reps)
        eng.set_shift_targets({l: (offsets, (rng.standard_normal((len(offsets),) + (eng.layer_info(l)[1],) * 2) * 0.01)
                                   .astype(np.float32)) for l in SHIFT_LAYERS_DEFAULT})
        with_term = tile_ms(eng, tile, grad, cl, sl, cw, sw, opts.reps)
        eng.set_shift_targets({})
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
