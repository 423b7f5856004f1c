"""Device time of the temporal-consistency term at 1024^2, 2048^2 and 4096^2, from device events on the
engine's stream: stx_image_temporal (the kernel and the finish of its partials) at a weight of all ones
and on the composite a mild affine flow leaves (96 % held), stx_image_flow_warp with a forward flow (first = 1),
and -- the yardstick -- stx_image_regularizers with only the auxiliary-image term on, existing code that
does the same arithmetic without the weight.

    python tools/bench_temporal.py [--out profiles/temporal_times.txt] [--sizes 1024 2048 4096]

Beside each time its byte floor at the 6.3 TB/s the project takes as the achievable HBM rate
(VERDICT.md): the term 52 HW bytes (img 12, target 12, weight 4, gradient read and written 24), the
yardstick 36 HW bytes, the warp 44 HW bytes (flow_b 8, flow_f 8, prev 12, target 12 and weight 4 written;
include/stx.h).  The pictures of the smaller sizes fit the 256 MiB Infinity Cache, so a time under the
HBM floor there is the cache's doing.  The last line is the term's time per pixel at 2048^2 over the
yardstick's, which should be at most 1.7 (the byte ratio 52 / 36 = 1.44 plus 15 % for the extra stream).
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
RATIO_BOUND = 1.7


def affine_flows(size):
    """The mild affine map of the GPU tests (rotation 0.03 rad, zoom 1.02, shift (2.3, -1.7) about the centre)
    as a backward flow, and the inverse map's displacement as the forward flow."""
    y, x = np.mgrid[:size, :size].astype(np.float64)
    c = (size - 1) / 2.0
    co, si, zoom = np.cos(0.03), np.sin(0.03), 1.02
    dx, dy = x - c, y - c
    back = np.stack([c + zoom * (co * dx - si * dy) + 2.3 - x, c + zoom * (si * dx + co * dy) - 1.7 - y])
    ex, ey = dx - 2.3, dy + 1.7
    fwd = np.stack([c + (co * ex + si * ey) / zoom - x, c + (-si * ex + co * ey) / zoom - y])
    return np.float32(back), np.float32(fwd)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--sizes', type=int, nargs='+', default=[1024, 2048, 4096])
    ap.add_argument('--reps', type=int, default=30)
    opts = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_temporal: no GPU')
    net = builtin_net('vgg19')
    eng = TileEngine(net, 0, synthetic_weights(net, 0))
    raw = ctypes.c_void_p()
    lib.call('stx_engine_stream', eng.handle, ctypes.byref(raw))
    stream = torch.cuda.ExternalStream(raw.value)
    lines = ['# temporal-consistency term, device-event ms per call (median of %d after 5 warm-up calls)' % opts.reps,
             '# floor = bytes moved at 6.3 TB/s: temporal 52 HW, aux (stx_image_regularizers, auxiliary term only) '
             '36 HW, warp 44 HW',
             '# device: %s' % torch.cuda.get_device_name(0),
             '%6s %16s %9s %9s %9s %12s' % ('size', 'call', 'ms', 'floor ms', 'x floor', 'ns / pixel')]
    rng = np.random.RandomState(0)
    loss = ctypes.c_double()
    mean = (ctypes.c_float * 3)(0, 0, 0)
    per_pixel = {}
    for size in opts.sizes:
        hw = size * size
        img = eng.to_device(rng.uniform(-120, 130, (3, size, size)).astype(np.float32))
        prev = eng.to_device(rng.uniform(-120, 130, (3, size, size)).astype(np.float32))
        grad = eng.empty((3, size, size)).zero()
        ones = eng.to_device(np.ones((size, size), np.float32))
        target, weight = eng.empty((3, size, size)), eng.empty((size, size))
        back, fwd = (eng.to_device(flow) for flow in affine_flows(size))

        def warp():
            lib.call('stx_image_flow_warp', eng.handle, prev.ptr, back.ptr, fwd.ptr, size, size, 1.0, 1.0, 1,
                     target.ptr, weight.ptr)
        warp()                      # (the composite the second temporal row runs on)
        held = float(weight.get().mean())
        calls = [
            ('aux', 36 * hw, lambda: lib.call('stx_image_regularizers', eng.handle, img.ptr, grad.ptr, size, size, mean,
                                              0.0, 2.0, 0.0, 6.0, prev.ptr, 1e-3, None, ctypes.byref(loss))),
            ('temporal w=1', 52 * hw, lambda: lib.call('stx_image_temporal', eng.handle, img.ptr, grad.ptr, prev.ptr,
                                                       ones.ptr, size, size, 1e-3, ctypes.byref(loss))),
            ('temporal %.0f%%' % (100 * held), 52 * hw,
             lambda: lib.call('stx_image_temporal', eng.handle, img.ptr, grad.ptr, target.ptr, weight.ptr, size, size,
                              1e-3, ctypes.byref(loss))),
            ('warp fwd', 44 * hw, warp)]
        for name, nbytes, call in calls:
            for _ in range(5):
                call()
            eng.sync()
            times = []
            for _ in range(opts.reps):
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record(stream)
                call()
                stop.record(stream)
                eng.sync()
                times.append(start.elapsed_time(stop))
            ms = float(np.median(times))
            floor_ms = nbytes / HBM_BYTES_PER_S * 1e3
            per_pixel[size, name] = ms * 1e6 / hw
            lines.append('%6d %16s %9.4f %9.4f %9.2f %12.5f' % (size, name, ms, floor_ms, ms / floor_ms, ms * 1e6 / hw))
            print(lines[-1], flush=True)
        for buf in (img, prev, grad, ones, target, weight, back, fwd):
            buf.free()
    if 2048 in opts.sizes:
        ratio = per_pixel[2048, 'temporal w=1'] / per_pixel[2048, 'aux']
        lines.append('# 2048^2: temporal (w = 1) %.5f ns / pixel, aux %.5f ns / pixel, ratio %.3f (bound %.1f: %s)'
                     % (per_pixel[2048, 'temporal w=1'], per_pixel[2048, 'aux'], ratio, RATIO_BOUND,
                        'met' if ratio <= RATIO_BOUND else 'MISSED'))
        print(lines[-1], flush=True)
    text = '\n'.join(lines) + '\n'
    if opts.out:
        os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
        with open(opts.out, 'w') as f:
            f.write(text)
    else:
        print(text)


if __name__ == '__main__':
    main()
