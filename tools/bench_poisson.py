"""Device time of the screened-Poisson output stage (stx_image_poisson, csrc/poisson.hip; --poisson-lambda) at
1024^2, 2048^2 and 4096^2, from device events on the engine's stream (median of --reps calls after warm-up):

  * one whole solve at the default cycles for lambda 5 and 500, with its launch count (poisson.launch_count);
  * the half-sweep alone: with lambda 0.04 the problem has one level and a cycle is 40 half-sweeps at the full size,
    so the difference of a call with 3 cycles and one with 1 is 80 of them.  Beside it the byte floor at the 6.3 TB/s
    the project takes as the achievable HBM rate: a half-sweep reads and writes every line of e and reads
    every line of b, 24 B per pixel and channel (csrc/poisson.hip has the count).  Reported, not bounded.

    python tools/bench_poisson.py [--out profiles/poisson_times.txt] [--sizes 1024 2048 4096] [--yardstick-tree DIR]

With --yardstick-tree (a built checkout of the parent commit) the cost condition of DESIGN.md 3.26 is measured too:
the wall-clock of one solve at 2048^2 with lambda 5 and the default cycles (the call, the sync, the result freed: what
a written picture adds) against that tree's `--size 2048 --tile-size 1024` run on synthetic pictures and weights
(tools/time_cli.sh), started as a fresh process, alternating, three times.  The bound is 0.05.
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
from style_transfer_amd import image_ops, lib                            # noqa: E402
from style_transfer_amd.engine import TileEngine                          # noqa: E402
from style_transfer_amd.netspec import builtin_net                        # noqa: E402
from style_transfer_amd.poisson import POISSON_CYCLES_DEFAULT, launch_count, levels      # noqa: E402

HBM_BYTES_PER_S = 6.3e12
SWEEP_BYTES = 24            # per pixel and channel
COST_BOUND = 0.05


def pictures(size, seed=0):
    """(s, c) [3, size, size]: a noisy result against a content picture with a step, in the pipeline's frame."""
    rng = np.random.RandomState(seed)
    s = rng.uniform(-120, 130, (3, size, size)).astype(np.float32)
    c = rng.uniform(-120, -20, (3, size, size)).astype(np.float32)
    c[:, :, size // 2:] += 150
    return s, c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--sizes', type=int, nargs='+', default=[1024, 2048, 4096])
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--yardstick-tree', default=None)
    opts = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_poisson: no GPU')
    eng = TileEngine(builtin_net('vgg19'), 0)
    raw = ctypes.c_void_p()
    lib.call('stx_engine_stream', eng.handle, ctypes.byref(raw))
    stream = torch.cuda.ExternalStream(raw.value)
    lines = ['# screened-Poisson stage, device-event ms per call (median of %d after 2 warm-up calls), %d cycles'
             % (opts.reps, POISSON_CYCLES_DEFAULT),
             '# half-sweep floor = %d B per pixel and channel at 6.3 TB/s' % SWEEP_BYTES,
             '# device: %s' % torch.cuda.get_device_name(0)]

    def timed(d_s, d_c, out, lam, cycles, reps):
        size = d_s.shape[1]

        def call():
            lib.call('stx_image_poisson', eng.handle, d_s.ptr, d_c.ptr, out.ptr, size, size, float(lam), int(cycles))
        for _ in range(2):
            call()
        eng.sync()
        times = []
        for _ in range(reps):
            # (a sync gives the workspace back: a short call before the events allocates it again, so that the host's
            # hipMalloc is not on the timed stretch; the timed call is queued while that one runs)
            lib.call('stx_image_poisson', eng.handle, d_s.ptr, d_c.ptr, out.ptr, size, size, float(lam), 1)
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record(stream)
            call()
            stop.record(stream)
            eng.sync()
            times.append(start.elapsed_time(stop))
        return float(np.median(times))

    for size in opts.sizes:
        s, c = pictures(size)
        d_s, d_c, out = eng.to_device(s), eng.to_device(c), eng.empty((3, size, size))
        for lam in (5.0, 500.0):
            whole = timed(d_s, d_c, out, lam, POISSON_CYCLES_DEFAULT, opts.reps)
            n_launch = launch_count(size, size, lam)
            lines.append('%5d^2 whole solve, lambda %5g (%d levels): %9.3f ms, %6d launches, %.2f us per launch, '
                         '%.2f ns per pixel' % (size, lam, len(levels(size, size, lam)), whole, n_launch,
                                                whole * 1e3 / n_launch, whole * 1e6 / size ** 2))
            print(lines[-1], flush=True)
        long_ms, short_ms = timed(d_s, d_c, out, 0.04, 3, opts.reps), timed(d_s, d_c, out, 0.04, 1, opts.reps)
        sweep = (long_ms - short_ms) / 80
        floor = SWEEP_BYTES * 3 * size ** 2 / HBM_BYTES_PER_S * 1e3
        lines.append('%5d^2 half-sweep at the full size: %9.4f ms, floor %.4f ms, x %.2f of the floor'
                     % (size, sweep, floor, sweep / floor))
        print(lines[-1], flush=True)
        for buf in (d_s, d_c, out):
            buf.free()

    if opts.yardstick_tree:
        tree = os.path.abspath(opts.yardstick_tree)
        work = tempfile.mkdtemp(prefix='stx_poisson_cost_')
        subprocess.run([sys.executable, os.path.join(tree, 'tools', 'make_inputs.py'), work, '2048'], check=True,
                       stdout=subprocess.DEVNULL)
        s, c = pictures(2048)
        d_s, d_c = eng.to_device(s), eng.to_device(c)
        solve_s, cli_s = [], []
        for _ in range(3):
            start = time.perf_counter()
            solved = image_ops.poisson(eng, d_s, d_c, 5.0)
            eng.sync()
            solved.free()
            solve_s.append(time.perf_counter() - start)
            start = time.perf_counter()
            subprocess.run([sys.executable, os.path.join(tree, 'style_transfer.py'), '-ci', os.path.join(work, 'content.png'),
                            '-si', os.path.join(work, 'style.png'), '--devices', '0', '--weights', 'synthetic', '--size',
                            '2048', '--tile-size', '1024', '-oi', os.path.join(work, 'out.png')], check=True, cwd=work,
                           stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=240)
            cli_s.append(time.perf_counter() - start)
        ratio = float(np.median(solve_s) / np.median(cli_s))
        lines.append('# cost condition at 2048^2, lambda 5, wall-clock, alternating: one solve %s s; the parent\'s --size 2048 '
                     '--tile-size 1024 run %s s' % (' / '.join('%.4f' % t for t in solve_s), ' / '.join('%.3f' % t for t in cli_s)))
        lines.append('# medians %.4f s against %.3f s: ratio %.4f (bound %.2f: %s)'
                     % (np.median(solve_s), np.median(cli_s), ratio, COST_BOUND, 'met' if ratio <= COST_BOUND else 'MISSED'))
        print('\n'.join(lines[-2:]), flush=True)
        for buf in (d_s, d_c):
            buf.free()
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
