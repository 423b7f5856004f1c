"""Device time of the Laplacian loss at 1024^2, 2048^2 and 4096^2, from device events on the
engine's stream: stx_image_lap with pools {4} and {4, 16} (pool, error, back-projection, finish and
scatter launches of one call) and stx_image_lap_target with {4, 16} (pool and one grid launch).

    python tools/bench_lap.py [--out profiles/lap_times.txt] [--sizes 1024 2048 4096]

Beside each time its byte floor at the 6.3 TB/s the project takes as the achievable HBM rate
(VERDICT.md): the loss 36 HW bytes (12 to read the image, 24 to read and write the gradient), the
target 12 HW bytes; the pooled grids (1/16 of a plane and less) are left out of the floor.  The
pictures of the smaller sizes fit the 256 MiB Infinity Cache, so a time under the HBM floor there is
the cache's doing.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--sizes', type=int, nargs='+', default=[1024, 2048, 4096])
    ap.add_argument('--reps', type=int, default=30)
    opts = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_lap: no GPU')
    net = builtin_net('vgg19')
    eng = TileEngine(net, 0, synthetic_weights(net, 0))
    raw = ctypes.c_void_p()
    lib.call('stx_engine_stream', eng.handle, ctypes.byref(raw))
    stream = torch.cuda.ExternalStream(raw.value)
    lines = ['# Laplacian loss, device-event ms per call (median of %d after 5 warm-up calls)' % opts.reps,
             '# floor = bytes moved at 6.3 TB/s: lap 12 HW read + 24 HW gradient read and written, target 12 HW read',
             '# device: %s' % torch.cuda.get_device_name(0),
             '%6s %14s %9s %9s %9s' % ('size', 'call', 'ms', 'floor ms', 'x floor')]
    rng = np.random.RandomState(0)
    loss = ctypes.c_double()
    for size in opts.sizes:
        img = eng.to_device(rng.uniform(-120, 130, (3, size, size)).astype(np.float32))
        content = eng.to_device(rng.uniform(-120, 130, (3, size, size)).astype(np.float32))
        grad = eng.empty((3, size, size)).zero()
        hw = size * size
        calls = []
        keep = []
        for pools, weights in (([4], [1.0]), ([4, 16], [0.25, 0.75])):
            target = image_ops.lap_target(eng, content, pools)
            keep.append(target)
            n, arr = len(pools), (ctypes.c_int * len(pools))(*pools)
            w = (ctypes.c_double * n)(*weights)
            calls.append(('lap %s' % '+'.join(map(str, pools)), 36 * hw,
                          lambda n=n, arr=arr, w=w, target=target: lib.call(
                              'stx_image_lap', eng.handle, img.ptr, grad.ptr, size, size, n, arr, w, target.ptr,
                              1e-3, ctypes.byref(loss))))
        arr2 = (ctypes.c_int * 2)(4, 16)
        calls.append(('target 4+16', 12 * hw,
                      lambda: lib.call('stx_image_lap_target', eng.handle, content.ptr, size, size, 2, arr2,
                                       keep[1].ptr)))
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
            lines.append('%6d %14s %9.4f %9.4f %9.2f' % (size, name, ms, floor_ms, ms / floor_ms))
            print(lines[-1], flush=True)
        for buf in [img, content, grad] + keep:
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
