"""Device time of the --style-masks passes (style_mask.hip) and of a masked tile evaluation.

    python tools/bench_style_mask.py [--out profiles/style_mask_times.txt]

Part 1: the masked style term on given arrays (stx_op_masked_style_terms) at the blob shapes of a 1024^2
tile -- conv1_1 (64 x 1024^2), conv2_1 (128 x 512^2), conv3_1 (256 x 256^2) -- with the engine's per-group
event timing on: group `mask` is Fm = F . m with the partials of sum m^2 plus the C x C pass T' = a Gs (two
launches), group `smask` is S <- a m . S with the partials of sum |m . S| plus the one-workgroup final sum the
stand-alone call launches behind it (two launches; the tile path defers that sum).  Beside each time the
byte floor of the blob pass alone (read + write of the blob, 8 C HW bytes) at the 6.3 TB/s the project takes
as the achievable HBM rate.  The 134 MB blob of conv2_1 and the 67 MB blob of conv3_1 fit the
256 MiB Infinity Cache, so a time near or under the HBM floor there is the cache's doing.

Part 2: one 1024^2 VGG-19 tile evaluation (styles conv1_1 .. conv5_1, content conv4_2) with two style
sets under complementary masks against the same evaluation with the two sets unmasked: device ms between the
call's own events (stx_last_tile_ms), and the `mask` / `smask` groups of one profiled evaluation.
"""

import argparse
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                              # noqa: E402
from style_transfer_amd import lib                                        # noqa: E402
from style_transfer_amd.engine import TileEngine                          # noqa: E402
from style_transfer_amd.netspec import builtin_net                        # noqa: E402
from style_transfer_amd.weights import synthetic_weights                  # noqa: E402

HBM_BYTES_PER_S = 6.3e12
SHAPES = [('conv1_1', 64, 1024), ('conv2_1', 128, 512), ('conv3_1', 256, 256)]
STYLE_LAYERS = ['conv1_1', 'conv2_1', 'conv3_1', 'conv4_1', 'conv5_1']


def smooth_mask(n):
    y, x = np.mgrid[:n, :n]
    return np.float32(0.5 + 0.5 * np.sin(0.011 * x + 0.007 * y) * np.cos(0.005 * y - 0.003 * x))


def kernel_times(eng, opts, lines):
    rng = np.random.RandomState(0)
    lines += ['# part 1: groups of stx_op_masked_style_terms, device-event ms (median of %d after 3 warm-up calls)'
              % opts.reps,
              '# floor = read + write of the blob (8 C HW bytes) at 6.3 TB/s',
              '%8s %6s %9s %9s %9s' % ('blob', 'group', 'ms', 'floor ms', 'x floor')]
    for name, c, n in SHAPES:
        feat = eng.empty((c, n, n))
        block = np.maximum(rng.standard_normal((c, 64, n)), 0).astype(np.float32)
        for y0 in range(0, n, 64):          # (filled on the device side in slabs: the host array stays small)
            slab = eng.to_device(np.ascontiguousarray(np.roll(block, y0, axis=2)))
            eng.map_place(feat, y0, 0, slab)
            eng.sync()
            slab.free()
        target = eng.to_device(np.tril(rng.standard_normal((c, c))).astype(np.float32))
        d_map = eng.to_device(smooth_mask(n))
        s_out = eng.empty((c, n, n))
        out = (ctypes.c_double * 3)()
        roll = (ctypes.c_int * 2)(0, 0)
        call = lambda: lib.call('stx_op_masked_style_terms', eng.handle, feat.ptr, c, n, n, d_map.ptr, n, n, 0, 0,
                                roll, target.ptr, s_out.ptr, out)
        for _ in range(3):
            call()
        times = {'mask': [], 'smask': []}
        eng.profile(True)
        for _ in range(opts.reps):
            call()
            for label, ms, _ in eng.profile_read():
                group = label.split()[0]
                if group in times:
                    times[group].append(ms)
        eng.profile(False)
        floor_ms = 8.0 * c * n * n / HBM_BYTES_PER_S * 1e3
        for group in ('mask', 'smask'):
            ms = float(np.median(times[group]))
            lines.append('%8s %6s %9.4f %9.4f %9.2f' % (name, group, ms, floor_ms, ms / floor_ms))
            print(lines[-1], flush=True)
        for buf in (feat, target, d_map, s_out):
            buf.free()


def tile_times(eng, opts, lines):
    rng = np.random.RandomState(1)
    n = 1024
    cl, cw = ['conv4_2'], {'conv4_2': 0.05}
    sw = {l: 1.0 / len(STYLE_LAYERS) for l in STYLE_LAYERS}
    tile = eng.to_device(rng.uniform(-110, 120, (3, n, n)).astype(np.float32))
    grad = eng.empty((3, n, n))
    contents = [{l: np.abs(rng.standard_normal(eng.feature_shape(l, n, n))).astype(np.float32) for l in cl}]
    styles = [{l: np.tril(rng.standard_normal((eng.layer_info(l)[1],) * 2)).astype(np.float32)
               for l in STYLE_LAYERS} for _ in range(2)]
    m0 = smooth_mask(n)
    run = lambda: eng.sc_grad_tile_async(tile, (0, 0), (0, 0), cl, STYLE_LAYERS, {}, cw, sw, grad_out=grad)
    lines += ['# part 2: one 1024^2 VGG-19 tile evaluation, two style sets, device ms (median of %d after 3 warm-up)'
              % opts.reps]
    result = {}
    for name, masks in (('unmasked', []), ('masked', [m0, 1 - m0]), ('unmasked again', [])):
        eng.set_contents_and_styles(contents, styles)
        eng.set_style_masks(masks)
        for _ in range(3):
            run()
        eng.sync()
        times = []
        for _ in range(opts.reps):
            run()
            eng.sync()
            times.append(eng.last_tile_ms())
        result[name] = float(np.median(times))
        lines.append('%16s %9.3f ms  (min %.3f, max %.3f)' % (name, result[name], min(times), max(times)))
        print(lines[-1], flush=True)
        if masks:
            eng.profile(True)
            run()
            eng.sync()
            rows = eng.profile_read()
            eng.profile(False)
            for group in ('mask', 'smask'):
                part = [(label, ms) for label, ms, _ in rows if label.split()[0] == group]
                lines.append('%16s %9.3f ms in %d groups: %s' % (group, sum(ms for _, ms in part), len(part),
                                                                 ', '.join('%s %.3f' % (l.split()[1], ms)
                                                                           for l, ms in part)))
                print(lines[-1], flush=True)
    lines.append('%16s %9.3f ms over the unmasked evaluation (%.1f %%)'
                 % ('masks cost', result['masked'] - result['unmasked'],
                    100 * (result['masked'] / result['unmasked'] - 1)))
    print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=20)
    opts = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_style_mask: no GPU')
    net = builtin_net('vgg19')
    eng = TileEngine(net, 0, synthetic_weights(net, 0))
    lines = ['# --style-masks: the passes of style_mask.hip and a masked tile evaluation',
             '# device: %s' % torch.cuda.get_device_name(0)]
    kernel_times(eng, opts, lines)
    tile_times(eng, opts, lines)
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
