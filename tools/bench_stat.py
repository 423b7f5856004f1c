"""Device time of the mean / std style term (stat.hip) beside the Gram / SYMM block of the same layer.

    python tools/bench_stat.py [--out profiles/stat_times.txt]

At the blob shapes of a 1024^2 tile -- conv1_1 (64 x 1024^2), conv2_1 (128 x 512^2), conv3_1 (256 x 256^2),
conv4_1 (512 x 128^2), conv5_1 (512 x 64^2) -- the engine's per-group event timing gives group `stat` of
stx_op_stat_terms (the three launches of the term and the one-workgroup final sum the stand-alone call
launches behind them; the tile path defers that sum) and groups `gram` + `symm` of stx_op_style_terms
(launch_style_terms as the tile path runs it).

Byte floors, at the 6.3 TB/s the project takes as the achievable HBM rate.  The statistics term
makes three passes over F -- the sum, the centred second sweep, the gradient -- and writes S once: 16 C HW
bytes; the second sweep re-reads a 64 KB slice its workgroup has just read, so 12 C HW is what has to come
from further away than L2.  The Gram / SYMM block reads F for the Gram, reads it again for S = sym(D) F and
writes S: 12 C HW bytes at the least, beside its 4 C^2 HW floating-point operations.  The blobs from conv2_1
on fit the 256 MiB Infinity Cache: a time under an HBM floor there is the cache's doing.
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
SHAPES = [('conv1_1', 64, 1024), ('conv2_1', 128, 512), ('conv3_1', 256, 256), ('conv4_1', 512, 128),
          ('conv5_1', 512, 64)]


def group_ms(eng, call, groups, reps):
    """Median device ms of the named profile groups of `call`, summed per call."""
    for _ in range(3):
        call()
    eng.profile(True)
    times = []
    for _ in range(reps):
        call()
        times.append(sum(ms for label, ms, _ in eng.profile_read() if label.split()[0] in groups))
    eng.profile(False)
    return float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=20)
    opts = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_stat: no GPU')
    net = builtin_net('vgg19')
    eng = TileEngine(net, 0, synthetic_weights(net, 0))
    rng = np.random.RandomState(0)
    lines = ['# --stat-weight: the mean / std style term (stat.hip) beside launch_style_terms, device-event ms',
             '# device: %s; median of %d calls after 3 warm-up calls' % (torch.cuda.get_device_name(0), opts.reps),
             '# floors at 6.3 TB/s: stat 16 C HW bytes (3 reads of F + 1 write of S), gram+symm 12 C HW bytes',
             '%8s %9s %9s %8s %11s %9s %8s' % ('blob', 'stat ms', 'floor ms', 'x floor', 'gram+symm', 'floor ms',
                                              'x floor')]
    for name, c, n in SHAPES:
        feat = eng.empty((c, n, n))
        block = np.maximum(rng.standard_normal((c, min(n, 64), n)), 0).astype(np.float32)
        for y0 in range(0, n, block.shape[1]):  # (filled on the device side in slabs: the host array stays small)
            slab = eng.to_device(np.ascontiguousarray(np.roll(block, y0, axis=2)))
            eng.map_place(feat, y0, 0, slab)
            eng.sync()
            slab.free()
        mu, sd = eng.feature_stats(feat)
        d_mu = eng.to_device((mu * rng.uniform(0.5, 1.5, c)).astype(np.float32))
        d_sd = eng.to_device((sd * rng.uniform(0.5, 1.5, c)).astype(np.float32))
        target = eng.to_device(np.tril(rng.standard_normal((c, c))).astype(np.float32))
        s_out = eng.empty((c, n, n))
        out = (ctypes.c_double * 2)()
        half, asum = ctypes.c_double(), ctypes.c_double()
        stat = lambda: lib.call('stx_op_stat_terms', eng.handle, feat.ptr, c, n, n, d_mu.ptr, d_sd.ptr, s_out.ptr, out)
        gram = lambda: lib.call('stx_op_style_terms', eng.handle, feat.ptr, c, n, n, target.ptr, s_out.ptr, None,
                                ctypes.byref(half), ctypes.byref(asum))
        stat_ms = group_ms(eng, stat, ('stat',), opts.reps)
        gram_ms = group_ms(eng, gram, ('gram', 'symm'), opts.reps)
        stat_floor = 16.0 * c * n * n / HBM_BYTES_PER_S * 1e3
        gram_floor = 12.0 * c * n * n / HBM_BYTES_PER_S * 1e3
        lines.append('%8s %9.4f %9.4f %8.2f %11.4f %9.4f %8.2f' % (name, stat_ms, stat_floor, stat_ms / stat_floor,
                                                                   gram_ms, gram_floor, gram_ms / gram_floor))
        print(lines[-1], flush=True)
        for buf in (feat, d_mu, d_sd, target, s_out):
            buf.free()
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
