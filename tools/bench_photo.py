"""Device time of the photorealism regulariser (stx_image_photo: the matting-Laplacian kernel and the
finish of its partials) at 1024^2, 2048^2 and 4096^2, from device events on the engine's stream.

    python tools/bench_photo.py [--out profiles/photo_times.txt] [--sizes 1024 2048 4096]

Beside each time its byte floor at the 6.3 TB/s the project takes as the achievable HBM rate
(VERDICT.md): 48 HW bytes, 12 to read the image, 12 to read the content picture, 24 to read and write
the gradient.  The pictures of the smaller sizes fit the 256 MiB Infinity Cache, so a time near or
under the HBM floor there is the cache's doing.  The content picture is a colour-line picture under
noise and the iterate is noise: the kernel's work does not depend on the values.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--sizes', type=int, nargs='+', default=[1024, 2048, 4096])
    ap.add_argument('--reps', type=int, default=30)
    opts = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_photo: no GPU')
    net = builtin_net('vgg19')
    eng = TileEngine(net, 0, synthetic_weights(net, 0))
    raw = ctypes.c_void_p()
    lib.call('stx_engine_stream', eng.handle, ctypes.byref(raw))
    stream = torch.cuda.ExternalStream(raw.value)
    lines = ['# photorealism regulariser, device-event ms per call (median of %d after 5 warm-up calls)' % opts.reps,
             '# floor = 48 HW bytes at 6.3 TB/s: 12 image read + 12 content read + 24 gradient read and written',
             '# device: %s' % torch.cuda.get_device_name(0),
             '%6s %9s %9s %9s %9s %12s' % ('size', 'eps', 'ms', 'floor ms', 'x floor', 'ns / pixel')]
    rng = np.random.RandomState(0)
    loss = ctypes.c_double()
    for size in opts.sizes:
        y, x = np.mgrid[:size, :size]
        base = np.sin(x / 9.0) * np.cos(y / 7.0)
        picture = np.stack([0.4 * base + 0.5, 0.3 * base + 0.4, 0.5 - 0.2 * base]) * 255 - 110
        content = eng.to_device(np.float32(np.round(picture + rng.uniform(-2, 2, picture.shape))))
        img = eng.to_device(rng.uniform(-120, 130, (3, size, size)).astype(np.float32))
        grad = eng.empty((3, size, size)).zero()
        hw = size * size
        for eps in (1e-7, 1e-4):
            call = lambda: lib.call('stx_image_photo', eng.handle, img.ptr, content.ptr, grad.ptr, size, size,
                                    eps, 1e-3, ctypes.byref(loss))
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
            floor_ms = 48 * hw / HBM_BYTES_PER_S * 1e3
            lines.append('%6d %9g %9.4f %9.4f %9.2f %12.4f' % (size, eps, ms, floor_ms, ms / floor_ms,
                                                               ms * 1e6 / hw))
            print(lines[-1], flush=True)
        for buf in (img, content, grad):
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
