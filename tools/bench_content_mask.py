"""Device time of the --content-mask term (content_mask.hip) and of a masked tile evaluation.

    python tools/bench_content_mask.py [--out profiles/content_mask_times.txt]

Part 1: the masked content term on given arrays (stx_op_masked_content_terms) at the blob shapes of a 1024^2
tile -- conv4_2 (512 x 128^2), conv3_2 (256 x 256^2) -- with the engine's per-group event timing on: group
`cmask` is the window's mean weight, the pass that writes S = a (m d) with the partials of its two sums, and
the final sums the stand-alone call launches behind it (three launches; the tile path defers the last).
Beside each time the byte floor of the pass -- feat, content window and S (12 C HW bytes) and the mask map
once (4 HW) -- at the 6.3 TB/s the project takes as the achievable HBM rate.  Blobs of this size
fit the 256 MiB Infinity Cache, so a time near or under the HBM floor is the cache's doing.

Part 2: what the term replaces.  A 1024^2 VGG-19 tile evaluation with that layer as its only tap, profiled:
unmasked it is group `content` (content_sums + its final sums) and group `inject` (the difference recomputed
and added); masked it is group `cmask` and group `inject` (S added).

Part 3: one 1024^2 tile evaluation (styles conv1_1 .. conv5_1, content conv4_2) with and without a mask:
device ms between the call's own events (stx_last_tile_ms).
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
SHAPES = [('conv4_2', 512, 128), ('conv3_2', 256, 256)]
STYLE_LAYERS = ['conv1_1', 'conv2_1', 'conv3_1', 'conv4_1', 'conv5_1']
N = 1024


def smooth_mask(n):
    y, x = np.mgrid[:n, :n]
    return np.float32(0.5 + 0.5 * np.sin(0.011 * x + 0.007 * y) * np.cos(0.005 * y - 0.003 * x))


def device_blob(eng, rng, c, n):
    """A [c, n, n] array of rectified noise, filled on the device in slabs: the host array stays small."""
    blob = eng.empty((c, n, n))
    block = np.maximum(rng.standard_normal((c, 64, n)), 0).astype(np.float32)
    for y0 in range(0, n, 64):
        slab = eng.to_device(np.ascontiguousarray(np.roll(block, y0, axis=2)))
        eng.map_place(blob, y0, 0, slab)
        eng.sync()
        slab.free()
    return blob


def kernel_times(eng, opts, lines):
    rng = np.random.RandomState(0)
    lines += ['# part 1: group cmask of stx_op_masked_content_terms, device-event ms (median of %d after 3 warm-up calls)'
              % opts.reps,
              '# floor = feat + content window + S (12 C HW bytes) + the mask map (4 HW) at 6.3 TB/s',
              '%8s %6s %9s %9s %9s' % ('blob', 'group', 'ms', 'floor ms', 'x floor')]
    for name, c, n in SHAPES:
        feat, content = device_blob(eng, rng, c, n), device_blob(eng, rng, c, n)
        d_map = eng.to_device(smooth_mask(n))
        s_out = eng.empty((c, n, n))
        out = (ctypes.c_double * 3)()
        roll = (ctypes.c_int * 2)(0, 0)
        call = lambda: lib.call('stx_op_masked_content_terms', eng.handle, feat.ptr, c, n, n, content.ptr, n, n,
                                d_map.ptr, 0, 0, roll, s_out.ptr, out)
        for _ in range(3):
            call()
        times = []
        eng.profile(True)
        for _ in range(opts.reps):
            call()
            times += [ms for label, ms, _ in eng.profile_read() if label.split()[0] == 'cmask']
        eng.profile(False)
        floor_ms = (12.0 * c + 4.0) * n * n / HBM_BYTES_PER_S * 1e3
        ms = float(np.median(times))
        lines.append('%8s %6s %9.4f %9.4f %9.2f' % (name, 'cmask', ms, floor_ms, ms / floor_ms))
        print(lines[-1], flush=True)
        for buf in (feat, content, d_map, s_out):
            buf.free()


def median_groups(eng, run, reps, groups):
    """Median device ms of the named profile groups over `reps` profiled evaluations."""
    times = {g: [] for g in groups}
    eng.profile(True)
    for _ in range(reps):
        run()
        eng.sync()
        rows = eng.profile_read()
        for g in groups:
            times[g].append(sum(ms for label, ms, _ in rows if label.split()[0] == g))
    eng.profile(False)
    return {g: float(np.median(v)) for g, v in times.items()}


def replaced_times(eng, opts, lines):
    rng = np.random.RandomState(2)
    tile = eng.to_device(rng.uniform(-110, 120, (3, N, N)).astype(np.float32))
    grad = eng.empty((3, N, N))
    lines += ['# part 2: the layer as the only tap of a 1024^2 tile evaluation, profiled groups, device-event ms '
              '(median of %d)' % opts.reps,
              '%8s %28s %28s' % ('blob', 'unmasked: content + inject', 'masked: cmask + inject')]
    for name, c, n in SHAPES:
        cl, cw = [name], {name: 0.05}
        contents = [{name: np.abs(rng.standard_normal((c, n, n))).astype(np.float32)}]
        run = lambda: eng.sc_grad_tile_async(tile, (0, 0), (0, 0), cl, [], {}, cw, {}, grad_out=grad)
        eng.set_contents_and_styles(contents, [])
        for _ in range(3):
            run()
        eng.sync()
        plain = median_groups(eng, run, opts.reps, ('content', 'inject'))
        eng.set_content_mask(smooth_mask(N))
        for _ in range(3):
            run()
        eng.sync()
        masked = median_groups(eng, run, opts.reps, ('cmask', 'inject'))
        eng.set_content_mask(None)
        lines.append('%8s %10.4f + %.4f = %.4f %10.4f + %.4f = %.4f'
                     % (name, plain['content'], plain['inject'], plain['content'] + plain['inject'],
                        masked['cmask'], masked['inject'], masked['cmask'] + masked['inject']))
        print(lines[-1], flush=True)
    for buf in (tile, grad):
        buf.free()


def tile_times(eng, opts, lines):
    rng = np.random.RandomState(1)
    cl, cw = ['conv4_2'], {'conv4_2': 0.05}
    sw = {l: 1.0 / len(STYLE_LAYERS) for l in STYLE_LAYERS}
    tile = eng.to_device(rng.uniform(-110, 120, (3, N, N)).astype(np.float32))
    grad = eng.empty((3, N, N))
    contents = [{l: np.abs(rng.standard_normal(eng.feature_shape(l, N, N))).astype(np.float32) for l in cl}]
    styles = [{l: np.tril(rng.standard_normal((eng.layer_info(l)[1],) * 2)).astype(np.float32)
               for l in STYLE_LAYERS}]
    run = lambda: eng.sc_grad_tile_async(tile, (0, 0), (0, 0), cl, STYLE_LAYERS, {}, cw, sw, grad_out=grad)
    lines += ['# part 3: one 1024^2 VGG-19 tile evaluation, device ms (median of %d after 3 warm-up)' % opts.reps]
    result = {}
    for name, mask in (('unmasked', None), ('masked', smooth_mask(N)), ('unmasked again', None)):
        eng.set_contents_and_styles(contents, styles)
        eng.set_content_mask(mask)
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
    lines.append('%16s %9.3f ms over the unmasked evaluation (%.1f %%)'
                 % ('the mask costs', result['masked'] - result['unmasked'],
                    100 * (result['masked'] / result['unmasked'] - 1)))
    print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=20)
    opts = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_content_mask: no GPU')
    net = builtin_net('vgg19')
    eng = TileEngine(net, 0, synthetic_weights(net, 0))
    lines = ['# --content-mask: the passes of content_mask.hip and a masked tile evaluation',
             '# device: %s' % torch.cuda.get_device_name(0)]
    kernel_times(eng, opts, lines)
    replaced_times(eng, opts, lines)
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
