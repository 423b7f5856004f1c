"""Device time of the three --preserve-color kernels at 1024^2, 2048^2 and 4096^2, from device
events on the engine's stream: stx_image_color_stats (the pass, its finish and the read-back of
the nine sums the call waits for), stx_image_color_affine (in place) and stx_image_to_u8_luma.

    python tools/bench_color.py [--out profiles/preserve_color_times.txt] [--sizes 1024 2048 4096]

Beside each time its byte floor at the 6.3 TB/s the project takes as the achievable HBM rate
(VERDICT.md): stats 12 HW bytes read, affine 24 HW (read and write three planes), luma 24 HW read
and 3 HW written.  The pictures of the smaller sizes fit the 256 MiB Infinity Cache, so a time under
the HBM floor there is the cache's doing.
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
MEAN = (103.939, 116.779, 123.68)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--sizes', type=int, nargs='+', default=[1024, 2048, 4096])
    ap.add_argument('--reps', type=int, default=30)
    opts = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_color: no GPU')
    net = builtin_net('vgg19')
    eng = TileEngine(net, 0, synthetic_weights(net, 0))
    raw = ctypes.c_void_p()
    lib.call('stx_engine_stream', eng.handle, ctypes.byref(raw))
    stream = torch.cuda.ExternalStream(raw.value)
    lines = ['# --preserve-color kernels, device-event ms per call (median of %d after 5 warm-up calls)'
             % opts.reps,
             '# floor = bytes moved at 6.3 TB/s: stats 12 HW read, affine 24 HW, luma 24 HW read + 3 HW written',
             '# device: %s' % torch.cuda.get_device_name(0),
             '%6s %8s %9s %9s %9s' % ('size', 'kernel', 'ms', 'floor ms', 'x floor')]
    rng = np.random.RandomState(0)
    mean = (ctypes.c_float * 3)(*MEAN)
    A = (ctypes.c_double * 9)(*(np.eye(3) * 0.9 + 0.05).ravel())
    b = (ctypes.c_double * 3)(1.0, -2.0, 3.0)
    sums = (ctypes.c_double * 9)()
    for size in opts.sizes:
        img = eng.to_device(rng.uniform(-120, 130, (3, size, size)).astype(np.float32))
        content = eng.to_device(rng.uniform(-100, 110, (3, size, size)).astype(np.float32))
        out = eng.empty((size, size, 3), np.uint8)
        hw = size * size
        calls = [
            ('stats', 12 * hw, lambda: lib.call('stx_image_color_stats', eng.handle, img.ptr, size, size, sums)),
            ('affine', 24 * hw, lambda: lib.call('stx_image_color_affine', eng.handle, img.ptr, img.ptr, size,
                                                size, A, b, mean)),
            ('luma', 27 * hw, lambda: lib.call('stx_image_to_u8_luma', eng.handle, img.ptr, content.ptr, size,
                                              size, mean, out.ptr)),
        ]
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
            lines.append('%6d %8s %9.4f %9.4f %9.2f' % (size, name, ms, floor_ms, ms / floor_ms))
            print(lines[-1], flush=True)
        for buf in (img, content, out):
            buf.free()
    text = '\n'.join(lines) + '\n'
    if opts.out:
        os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
        with open(opts.out, 'w') as f:
            f.write(text)
    else:
        print(text)


if __name__ == '__main__':
    main()
