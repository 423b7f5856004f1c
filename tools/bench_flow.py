"""Device time of the optical-flow estimator (stx_image_flow_estimate, csrc/flow.hip; --prev-contents) at 1024^2,
2048^2 and 256^2, from device events on the engine's stream (median of --reps calls after warm-up):

  * one whole estimate at the defaults, with its launch count (flow.launch_count);
  * the half-sweep alone: with levels = outer = inner = 1 the call is one linear solve, and the difference of a call
    with sor = 60 and one with sor = 10 is 100 half-sweeps at the full size.  Beside it the byte floor at the 6.3 TB/s
    the project takes as the achievable HBM rate: a half-sweep touches every line of 17 float64 planes
    and writes four of them back, 168 B per pixel of the level (csrc/flow.hip has the count);
  * the split of the estimate's time by level: the call with k levels less the call with k - 1.

    python tools/bench_flow.py [--out profiles/flow_times.txt] [--sizes 1024 2048 256] [--yardstick-tree DIR]

With --yardstick-tree (a built checkout of the parent commit) the cost condition of DESIGN.md 3.25 is measured too:
the wall-clock of both flows for one earlier frame at 1024^2 (upload, two estimates, sync) against that tree's
`--size 1024 --tile-size 1024` run on synthetic pictures and weights (tools/time_cli.sh), each started as a fresh
process, alternating, three times.  The bound is 0.2.
"""

import argparse
import ctypes
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                              # noqa: E402
from PIL import Image                                                     # noqa: E402
from style_transfer_amd import image_ops, lib                            # noqa: E402
from style_transfer_amd.engine import TileEngine                          # noqa: E402
from style_transfer_amd.flow import estimate_flow, launch_count, pyramid_sizes    # noqa: E402
from style_transfer_amd.netspec import builtin_net                        # noqa: E402

HBM_BYTES_PER_S = 6.3e12
SWEEP_BYTES = 168
COST_BOUND = 0.2


def frames(size, seed=0):
    """Two grey frames [size, size] in 0 ... 255: smooth noise, and the same moved by a mild affine map."""
    rng = np.random.RandomState(seed)
    small = rng.uniform(0, 255, (max(2, size // 16) + 4, max(2, size // 16) + 4)).astype(np.float32)
    big = np.asarray(Image.fromarray(small).resize((size + 64, size + 64), Image.BICUBIC), np.float32)
    return (np.ascontiguousarray(np.clip(big[32:32 + size, 32:32 + size], 0, 255)),
            np.ascontiguousarray(np.clip(big[30:30 + size, 35:35 + size], 0, 255)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--sizes', type=int, nargs='+', default=[1024, 2048, 256])
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--level-reps', type=int, default=10)
    ap.add_argument('--yardstick-tree', default=None)
    opts = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_flow: no GPU')
    eng = TileEngine(builtin_net('vgg19'), 0)
    raw = ctypes.c_void_p()
    lib.call('stx_engine_stream', eng.handle, ctypes.byref(raw))
    stream = torch.cuda.ExternalStream(raw.value)
    lines = ['# optical-flow estimator, device-event ms per call (median of %d after 3 warm-up calls; per level: of %d)'
             % (opts.reps, opts.level_reps),
             '# half-sweep floor = %d B per pixel at 6.3 TB/s' % SWEEP_BYTES,
             '# device: %s' % torch.cuda.get_device_name(0)]

    def timed(d1, d2, out, params, reps):
        c_params = image_ops.flow_params(params)
        size = d1.shape[0]

        def call():
            lib.call('stx_image_flow_estimate', eng.handle, d1.ptr, d2.ptr, size, size, ctypes.byref(c_params), out.ptr)
        for _ in range(3):
            call()
        eng.sync()
        times = []
        for _ in range(reps):
            # (a sync gives the workspace back: the call before the events allocates it again, so that the host's
            # hipMalloc is not on the timed stretch; the timed call is queued while that one runs)
            call()
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record(stream)
            call()
            stop.record(stream)
            eng.sync()
            times.append(start.elapsed_time(stop))
        return float(np.median(times))

    for size in opts.sizes:
        i1, i2 = frames(size)
        d1, d2, out = eng.to_device(i1), eng.to_device(i2), eng.empty((2, size, size))
        whole = timed(d1, d2, out, None, opts.reps)
        n_launch = launch_count(size, size)
        lines.append('%5d^2 whole estimate (defaults): %9.3f ms, %d launches, %.2f us per launch, %.2f ns per pixel'
                     % (size, whole, n_launch, whole * 1e3 / n_launch, whole * 1e6 / size ** 2))
        print(lines[-1], flush=True)
        one = dict(levels=1, outer=1, inner=1)
        long_ms, short_ms = timed(d1, d2, out, dict(one, sor=60), opts.reps), timed(d1, d2, out, dict(one, sor=10), opts.reps)
        sweep = (long_ms - short_ms) / 100
        floor = SWEEP_BYTES * size ** 2 / HBM_BYTES_PER_S * 1e3
        lines.append('%5d^2 half-sweep at the full size: %9.4f ms, floor %.4f ms, x %.2f of the floor'
                     % (size, sweep, floor, sweep / floor))
        print(lines[-1], flush=True)
        sizes = pyramid_sizes(size, size)
        before = 0.0
        for k in range(1, len(sizes) + 1):
            ms = timed(d1, d2, out, dict(levels=k), opts.level_reps)
            h, w = sizes[k - 1]
            lines.append('%5d^2   level %2d (%4d x %4d): %8.3f ms' % (size, k - 1, w, h, ms - before))
            print(lines[-1], flush=True)
            before = ms
        for buf in (d1, d2, out):
            buf.free()

    if opts.yardstick_tree:
        tree = os.path.abspath(opts.yardstick_tree)
        work = tempfile.mkdtemp(prefix='stx_flow_cost_')
        subprocess.run([sys.executable, os.path.join(tree, 'tools', 'make_inputs.py'), work, '2048'], check=True,
                       stdout=subprocess.DEVNULL)
        a, b = (Image.fromarray(np.uint8(f)).convert('RGB') for f in frames(1024))
        flow_s, cli_s = [], []
        for _ in range(3):
            start = time.perf_counter()
            flows = [estimate_flow(eng, a, b), estimate_flow(eng, b, a)]
            eng.sync()
            flow_s.append(time.perf_counter() - start)
            for flow in flows:
                flow.free()
            start = time.perf_counter()
            subprocess.run([sys.executable, os.path.join(tree, 'style_transfer.py'), '-ci', os.path.join(work, 'content.png'),
                            '-si', os.path.join(work, 'style.png'), '--devices', '0', '--weights', 'synthetic', '--size',
                            '1024', '--tile-size', '1024', '-oi', os.path.join(work, 'out.png')], check=True, cwd=work,
                           stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=120)
            cli_s.append(time.perf_counter() - start)
        ratio = float(np.median(flow_s) / np.median(cli_s))
        lines.append('# cost condition at 1024^2, wall-clock, alternating: both flows %s s; the parent\'s --size 1024 '
                     '--tile-size 1024 run %s s' % (' / '.join('%.4f' % s for s in flow_s), ' / '.join('%.3f' % s for s in cli_s)))
        lines.append('# medians %.4f s against %.3f s: ratio %.4f (bound %.1f: %s)'
                     % (np.median(flow_s), np.median(cli_s), ratio, COST_BOUND, 'met' if ratio <= COST_BOUND else 'MISSED'))
        print('\n'.join(lines[-2:]), flush=True)
    eng.close()
    text = '\n'.join(lines) + '\n'
    if opts.out:
        os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
        with open(opts.out, 'w') as f:
            f.write(text)
    else:
        print(text)


if __name__ == '__main__':
    main()
