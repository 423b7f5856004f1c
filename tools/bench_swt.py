"""Device time of the SWT term at 1024^2, 2048^2 and 4096^2, from device events on the engine's
stream: the Haar kernels (stx_image_swt_haar_levels; order 1) and the table-driven kernels of
dbN / symN (stx_image_swt_daub_levels; --orders N ...) in the same run.  One level of order 1 is
the shipped one-level kernel (stx_image_swt_haar).

    python tools/bench_swt.py --orders 1 --levels 6 [--out profiles/swt_levels_times.txt]
    python tools/bench_swt.py --levels 4 [--out profiles/swt_wavelet_times.txt] [--sizes 1024 2048 4096]

Beside each time: the taps per axis (2 (2 order - 1)(2^levels - 1) + 1, at most the padded side),
the multiple of the two-pass byte floor -- 20 bytes per pixel and channel (read the image, write and
read the row-filtered image, read and write the gradient) at the 6.3 TB/s the project takes as the
achievable HBM rate -- the ratio to the level below and the ratio to the Haar kernel at
the same level count (when order 1 is among --orders).
"""

import argparse
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                              # noqa: E402
from style_transfer_amd import image_ops, lib                             # noqa: E402
from style_transfer_amd.engine import TileEngine                          # noqa: E402
from style_transfer_amd.netspec import builtin_net                        # noqa: E402
from style_transfer_amd.weights import synthetic_weights                  # noqa: E402

HBM_BYTES_PER_S = 6.3e12
FLOOR_BYTES = 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--sizes', type=int, nargs='+', default=[1024, 2048, 4096])
    ap.add_argument('--levels', type=int, default=6)
    ap.add_argument('--orders', type=int, nargs='+', default=[1, 2, 4, 8])
    ap.add_argument('--reps', type=int, default=30)
    opts = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_swt: no GPU')
    net = builtin_net('vgg19')
    eng = TileEngine(net, 0, synthetic_weights(net, 0))
    raw = ctypes.c_void_p()
    lib.call('stx_engine_stream', eng.handle, ctypes.byref(raw))
    stream = torch.cuda.ExternalStream(raw.value)
    lines = ['# SWT term, device-event ms per call (median of %d after 5 warm-up calls), power 2,'
             % opts.reps,
             '# roll (8, -16); order 1 = the Haar kernels (1 level: the shipped one-level kernel), order N ='
             ' dbN / symN',
             '# through the table-driven kernels; floor = 20 B/pixel/channel at 6.3 TB/s',
             '# device: %s' % torch.cuda.get_device_name(0),
             '%6s %6s %6s %6s %9s %9s %9s %9s' % ('size', 'order', 'levels', 'taps', 'ms', 'x floor',
                                                  'x prev', 'x haar')]
    rng = np.random.RandomState(0)
    for size in opts.sizes:
        img = eng.to_device(rng.uniform(-120, 130, (3, size, size)).astype(np.float32))
        grad = eng.empty((3, size, size)).zero()
        floor_ms = FLOOR_BYTES * 3 * size * size / HBM_BYTES_PER_S * 1e3
        side = image_ops.swt_padded_side(size, size)
        haar = {}
        for order in opts.orders:
            prev = None
            for levels in range(1, opts.levels + 1):
                def call():
                    if order == 1:
                        image_ops.swt_haar(eng, img, grad, 0.37, 2.0, roll=(8, -16), levels=levels)
                    else:
                        image_ops.swt_wavelet(eng, img, grad, 0.37, 2.0, 'db%d' % order,
                                              levels=levels, roll=(8, -16))
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
                if order == 1:
                    haar[levels] = ms
                taps = min(2 * (2 * order - 1) * (2 ** levels - 1) + 1, side)
                lines.append('%6d %6d %6d %6d %9.4f %9.2f %9s %9s'
                             % (size, order, levels, taps, ms, ms / floor_ms,
                                '-' if prev is None else '%.2f' % (ms / prev),
                                '%.2f' % (ms / haar[levels]) if levels in haar else '-'))
                print(lines[-1], flush=True)
                prev = ms
        img.free()
        grad.free()
    text = '\n'.join(lines) + '\n'
    if opts.out:
        os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
        with open(opts.out, 'w') as f:
            f.write(text)
    else:
        print(text)


if __name__ == '__main__':
    main()
