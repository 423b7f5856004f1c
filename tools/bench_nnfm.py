"""Device time of the nearest-neighbour feature matching term (nnfm.hip) on given arrays.

    python tools/bench_nnfm.py [--out profiles/nnfm_times.txt]
    python tools/bench_nnfm.py --patch 3 [--out profiles/nnfm_patch_times.txt]
    python tools/bench_nnfm.py --k 1 2 4 [--out profiles/nnfm_knn_times.txt]
    python tools/bench_nnfm.py --cover [--out profiles/nnfm_cover_times.txt]
    python tools/bench_nnfm.py --masks 2 [--out ...]; --masks 4 (both tables: profiles/nnfm_guided_times.txt)

stx_op_nnfm_terms at the blob shapes of a 1024^2 tile -- conv3_1 (256 x 256^2) and conv4_1 (512 x 128^2) --
against the banks of a 512^2 and of a 1024^2 style picture at --nnfm-stride 1 and 2, and at the shapes of a
256^2 tile (conv3_1 256 x 64^2, conv4_1 512 x 32^2), where the bank is cut into slices.  The engine's
per-group event timing is on: `prepare` (1 / |f_i| and the fp16 pieces of the unit columns), `search` (the
n x M x C product with its argmax, and the slices' merge when there is one), `grad` (S with the partials, and
the one-workgroup final sums the stand-alone call launches behind it).  Median of --reps calls after two
warm-up calls.  The pieces of the bank are made once when the targets are set (stx_set_nnfm_patch_targets) and
are not part of a tile's term: their pass is outside the three groups.

The search is priced against the matrix floor 3 x 2 n M C flop (three fp16 products per fp32-class product)
at 2.5 PFLOP/s, the dense fp16 rate of the MI355X.

--patch 3: stx_op_nnfm_patch_terms (--nnfm-patch 3) at the same shapes, K = 9 C.  Its yardstick is the plain
search run in the same call on a synthetic blob of 9 C channels with the same n and M: the same flops, and what
a materialised [n][9 C] query array would cost the search (`plain 9C`, with the ratio patch / plain).

--k 1 2 4: the k-nearest term (--nnfm-k, stx_op_nnfm_knn_terms) at the same shapes, one row per K, every K in the
same run as K = 1 (which is the call of the table without --k): `search x` and `grad x` are the group's time over
that of the K = 1 row above it.

--cover: the coverage part (--nnfm-cover, stx_op_nnfm_cover_terms with factor 1, K = 1) at the same shapes.  Beside
the forward search and gradient of the same call: `rsearch` (the reverse search: the same kernel with the operands
exchanged, the same 6 n M C flop, under nnfm_plan(M, n) -- `rslices`), `index` (c'_j with the row counts, the
prefix sums, the cursor fill and the pass that puts every list in order) and `cgrad` (the pass that adds the
lists' rows to S), each with its ratio to the forward group it stands beside (index and cgrad: to the forward
gradient).  Two rows per shape: random unit rows, whose winners spread over the columns (`longest` = the longest
list), and `one list` -- every bank row a noisy copy of column 0's direction, so that ONE column owns all M rows:
the worst case of the index's ordering pass and of the gradient's walk (fewer repetitions).

--masks S: the guided term (--nnfm-masks, stx_op_nnfm_guided_terms, K = 1) at the same shapes against a bank of S
equal segments, M rows each, under hard stripe masks that partition the map -- `v`: S vertical stripes, `h`: S
horizontal ones.  `window` is the mask pass with the launch that gives a, `gsearch` and `ggrad` the guided search
(with its merge) and gradient.  Beside them, in the same run, the unguided search (stx_op_nnfm_terms) against ONE
segment's rows (`one`) and against the whole bank of S M rows (`whole`), with the ratios gsearch / one and gsearch /
whole, and the unguided gradient over the whole bank (`grad`).  `pairs` is the share of the (segment, 128-column
block) pairs that are searched: a query block is 128 consecutive columns in row-major order, so a horizontal stripe
gives every block to one segment (1 / S), while a vertical stripe does so only where it is at least 128 columns
wide -- on a map of 128 columns or fewer every block crosses all S stripes and nothing is left out.
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

FP16_FLOPS = 2.5e15
# (blob, C, side of the blob's map, side of the style picture's map at that layer)
TILE_1024 = [('conv3_1', 256, 256, s) for s in (128, 256)] + [('conv4_1', 512, 128, s) for s in (64, 128)]
TILE_256 = [('conv3_1', 256, 64, s) for s in (128, 256)] + [('conv4_1', 512, 32, s) for s in (64, 128)]


def unit_rows(rng, m, c):
    b = rng.standard_normal((m, c)).astype(np.float32)
    return b / np.linalg.norm(b, axis=1, keepdims=True)


def measure(eng, rng, c, side, rows, reps, patch=1, k=1):
    """Median ms of the term's three groups; ``patch`` 3: the patch term of a c-channel blob (bank rows of 9 c);
    ``k`` above 1: the k-nearest term."""
    feat = eng.to_device(np.maximum(rng.standard_normal((c, side, side)), 0).astype(np.float32) + np.float32(1e-3))
    bank = eng.to_device(unit_rows(rng, rows, patch * patch * c))
    s_out = eng.empty((c, side, side))
    idx = eng.empty((k * side * side,), np.int32)
    out = (ctypes.c_double * 2)()
    if k > 1:
        call = lambda: lib.call('stx_op_nnfm_knn_terms', eng.handle, feat.ptr, c, side, side, patch, k, bank.ptr, rows,
                                s_out.ptr, idx.ptr, out)
    elif patch == 1:
        call = lambda: lib.call('stx_op_nnfm_terms', eng.handle, feat.ptr, c, side, side, bank.ptr, rows, s_out.ptr,
                                idx.ptr, out)
    else:
        call = lambda: lib.call('stx_op_nnfm_patch_terms', eng.handle, feat.ptr, c, side, side, patch, bank.ptr, rows,
                                s_out.ptr, idx.ptr, out)
    for _ in range(2):
        call()
    times = {'prepare': [], 'search': [], 'grad': []}
    slices = 1
    eng.profile(True)
    for _ in range(reps):
        call()
        for label, ms, _ in eng.profile_read():
            words = [word for word in label.split() if word != 'patch' and word != 'k%d' % k]
            if words[0] == 'nnfm' and words[1] in times:
                times[words[1]].append(ms)
                if words[1] == 'search':
                    slices = int(words[-1][1:])
    eng.profile(False)
    for buf in (feat, bank, s_out, idx):
        buf.free()
    return {k: float(np.median(v)) for k, v in times.items()}, slices


def measure_cover(eng, rng, c, side, rows, reps, one_list):
    """Median ms of the six groups of a call with a coverage part, the two slice counts and the longest list."""
    f = np.maximum(rng.standard_normal((c, side, side)), 0).astype(np.float32) + np.float32(1e-3)
    b = unit_rows(rng, rows, c)
    if one_list:        # every row leans towards column 0, far more than towards any other column
        d = unit_rows(rng, 1, c)[0]
        f[:, 0, 0] = 5 * d
        b = d[None, :] + np.float32(0.3) * b
        b /= np.linalg.norm(b, axis=1, keepdims=True)
    feat, bank = eng.to_device(f), eng.to_device(b.astype(np.float32))
    s_out = eng.empty((c, side, side))
    idx, win = eng.empty((side * side,), np.int32), eng.empty((rows,), np.int32)
    out = (ctypes.c_double * 3)()
    call = lambda: lib.call('stx_op_nnfm_cover_terms', eng.handle, feat.ptr, c, side, side, 1, 1, 1.0, bank.ptr, rows,
                            s_out.ptr, idx.ptr, win.ptr, out)
    for _ in range(2):
        call()
    names = {'nnfm prepare': 'prepare', 'nnfm search': 'search', 'nnfm grad': 'grad', 'nnfm cover search': 'rsearch',
             'nnfm cover index': 'index', 'nnfm cover grad': 'cgrad'}
    times = {name: [] for name in names.values()}
    slices = {}
    eng.profile(True)
    for _ in range(reps):
        call()
        for label, ms, _ in eng.profile_read():
            words = label.split()
            head = ' '.join(words[:3 if words[1] == 'cover' else 2])
            if head in names:
                times[names[head]].append(ms)
                if names[head].endswith('search'):
                    slices[names[head]] = int(words[-1][1:])
    eng.profile(False)
    longest = int(np.bincount(win.get(), minlength=side * side).max())
    for buf in (feat, bank, s_out, idx, win):
        buf.free()
    return {k: float(np.median(v)) for k, v in times.items()}, slices, longest


def stripe_maps(side, segments, kind):
    """[segments, side, side]: hard stripes that partition the map, vertical (`v`) or horizontal (`h`)."""
    owner = np.arange(side) * segments // side
    line = (np.arange(segments)[:, None] == owner[None, :]).astype(np.float32)      # [segments, side]
    maps = np.empty((segments, side, side), np.float32)
    maps[:] = line[:, None, :] if kind == 'v' else line[:, :, None]
    return maps


def measure_guided(eng, rng, c, side, rows, segments, kind, reps):
    """Median ms of the guided call's groups, its slice count and the share of searched pairs."""
    feat = eng.to_device(np.maximum(rng.standard_normal((c, side, side)), 0).astype(np.float32) + np.float32(1e-3))
    bank = eng.to_device(unit_rows(rng, segments * rows, c))
    maps_host = stripe_maps(side, segments, kind)
    maps = eng.to_device(maps_host)
    n = side * side
    s_out = eng.empty((c, side, side))
    idx = eng.empty((segments * n,), np.int32)
    out = (ctypes.c_double * 3)()
    seg_rows, roll = (ctypes.c_int * segments)(*[rows] * segments), (ctypes.c_int * 2)(0, 0)
    call = lambda: lib.call('stx_op_nnfm_guided_terms', eng.handle, feat.ptr, c, side, side, 1, bank.ptr, seg_rows,
                            segments, maps.ptr, side, side, 0, 0, roll, s_out.ptr, idx.ptr, out)
    for _ in range(2):
        call()
    times = {'prepare': [], 'window': [], 'search': [], 'grad': []}
    slices = 1
    eng.profile(True)
    for _ in range(reps):
        call()
        for label, ms, _ in eng.profile_read():
            words = label.split()
            if words[:2] == ['nnfm', 'guided'] and words[2] in times:
                times[words[2]].append(ms)
                if words[2] == 'search':
                    slices = int(words[-2][1:])
    eng.profile(False)
    for buf in (feat, bank, maps, s_out, idx):
        buf.free()
    blocks = -(-n // 128)
    padded = np.zeros((segments, blocks * 128), np.float32)
    padded[:, :n] = maps_host.reshape(segments, n)
    pairs = float((padded.reshape(segments, blocks, 128) > 0).any(axis=2).mean())
    return {k: float(np.median(v)) for k, v in times.items()}, slices, pairs


def guided_lines(eng, rng, opts):
    S = opts.masks
    lines = ['# --nnfm-masks: stx_op_nnfm_guided_terms (K = 1), %d equal segments of M rows under hard stripe masks, '
             'device-event ms per group (median of %d after 2 warm-up calls)' % (S, opts.reps),
             '# device: %s' % torch.cuda.get_device_name(0),
             '# one, whole = the search of stx_op_nnfm_terms against M and against %d M rows, grad = its gradient over the '
             'whole bank; all of one run' % S,
             '# pairs = searched (segment, 128-column block) pairs / all; g/one = gsearch / one; g/whole = gsearch / whole',
             '%6s %8s %4s %7s %7s %6s %2s %4s %6s %6s %8s %9s %9s %9s %9s %9s %9s %7s %7s'
             % ('tile', 'blob', 'C', 'n', 'M', 'stride', 'S', 'mask', 'slices', 'pairs', 'prepare', 'window', 'gsearch',
                'ggrad', 'one', 'whole', 'grad', 'g/one', 'g/whole')]
    for tile, shapes in ((1024, TILE_1024), (256, TILE_256)):
        for blob, c, side, style_side in shapes:
            for stride in (1, 2):
                rows = (-(-style_side // stride)) ** 2
                one, _ = measure(eng, rng, c, side, rows, opts.reps)
                whole, _ = measure(eng, rng, c, side, S * rows, opts.reps)
                for kind in ('v', 'h'):
                    t, slices, pairs = measure_guided(eng, rng, c, side, rows, S, kind, opts.reps)
                    line = ('%6d %8s %4d %7d %7d %6d %2d %4s %6d %6.3f %8.4f %9.4f %9.4f %9.4f %9.4f %9.4f %9.4f %7.3f %7.3f'
                            % (tile, blob, c, side * side, rows, stride, S, kind, slices, pairs, t['prepare'], t['window'],
                               t['search'], t['grad'], one['search'], whole['search'], whole['grad'],
                               t['search'] / one['search'], t['search'] / whole['search']))
                    lines.append(line)
                    print(line, flush=True)
    return lines


def cover_lines(eng, rng, opts):
    lines = ['# --nnfm-cover: stx_op_nnfm_cover_terms (cover 1, K = 1), device-event ms per group (median of %d, `one '
             'list` rows of %d, after 2 warm-up calls)' % (opts.reps, min(opts.reps, 5)),
             '# device: %s' % torch.cuda.get_device_name(0),
             '# rsearch x = rsearch / search; index x, cgrad x = the group over the forward grad; all of one call',
             '%6s %8s %4s %7s %7s %6s %6s %7s %8s %8s %9s %9s %9s %9s %9s %9s %9s %8s %7s  %s'
             % ('tile', 'blob', 'C', 'n', 'M', 'stride', 'slices', 'rslices', 'longest', 'prepare', 'search', 'grad', 'rsearch',
                'index', 'cgrad', 'rsearch x', 'index x', 'cgrad x', 'added', 'bank')]
    for tile, shapes in ((1024, TILE_1024), (256, TILE_256)):
        for blob, c, side, style_side in shapes:
            for stride in (1, 2):
                rows = (-(-style_side // stride)) ** 2
                for one_list in (False, True):
                    t, slices, longest = measure_cover(eng, rng, c, side, rows, min(opts.reps, 5) if one_list else opts.reps,
                                                       one_list)
                    added = t['rsearch'] + t['index'] + t['cgrad']
                    line = ('%6d %8s %4d %7d %7d %6d %6d %7d %8d %8.4f %9.4f %9.4f %9.4f %9.4f %9.4f %9.3f %9.3f %8.3f %7.4f  %s'
                            % (tile, blob, c, side * side, rows, stride, slices['search'], slices['rsearch'], longest, t['prepare'],
                               t['search'], t['grad'], t['rsearch'], t['index'], t['cgrad'], t['rsearch'] / t['search'],
                               t['index'] / t['grad'], t['cgrad'] / t['grad'], added, 'one list' if one_list else 'random'))
                    lines.append(line)
                    print(line, flush=True)
    return lines


def table_lines(eng, rng, opts):
    """The table of one mode: the plain columns, and for --patch 3 the plain search at 9 C and the ratio to it."""
    p3 = opts.patch == 3
    name, width = ('stx_op_nnfm_patch_terms', '9C') if p3 else ('stx_op_nnfm_terms', 'C')
    lines = ['# --nnfm-%s: %s, device-event ms per group (median of %d after 2 warm-up calls)'
             % ('patch 3' if p3 else 'weight', name, opts.reps),
             '# device: %s' % torch.cuda.get_device_name(0),
             '# floor = 3 x 2 n M %s flop at 2.5 PFLOP/s; of floor = floor / search' % width]
    if p3:
        lines.append('# plain 9C = the search of stx_op_nnfm_terms on a blob of 9 C channels, same n and M; '
                     'ratio = search / plain 9C')
    many = opts.k != [1]
    if many:
        lines.append('# --nnfm-k: one row per K (K > 1: stx_op_nnfm_knn_terms); search x, grad x = the time over the '
                     'K = 1 row of the same shape, same run')
    head = ('tile', 'blob', 'C', 'n', 'M', 'stride', 'slices', 'prepare', 'search', 'grad', 'total', 'floor ms', 'of floor')
    lines.append('%6s %8s %4s %7s %7s %6s %6s %9s %9s %9s %9s %9s %8s' % head
                 + (' %9s %6s' % ('plain 9C', 'ratio') if p3 else '') + (' %2s %8s %7s' % ('K', 'search x', 'grad x') if many else ''))
    for tile, shapes in ((1024, TILE_1024), (256, TILE_256)):
        for blob, c, side, style_side in shapes:
            for stride in (1, 2):
                rows = (-(-style_side // stride)) ** 2
                n = side * side
                floor_ms = 6.0 * n * rows * opts.patch ** 2 * c / FP16_FLOPS * 1e3
                one = None
                for k in opts.k:
                    t, slices = measure(eng, rng, c, side, rows, opts.reps, opts.patch, k)
                    one = t if k == 1 else one
                    line = ('%6d %8s %4d %7d %7d %6d %6d %9.4f %9.4f %9.4f %9.4f %9.4f %8.3f'
                            % (tile, blob, c, n, rows, stride, slices, t['prepare'], t['search'], t['grad'],
                               sum(t.values()), floor_ms, floor_ms / t['search']))
                    if p3:
                        plain, _ = measure(eng, rng, 9 * c, side, rows, opts.reps)
                        line += ' %9.4f %6.3f' % (plain['search'], t['search'] / plain['search'])
                    if many:
                        line += ' %2d %8.3f %7.3f' % (k, t['search'] / one['search'], t['grad'] / one['grad'])
                    lines.append(line)
                    print(line, flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--patch', type=int, default=1, choices=(1, 3))
    ap.add_argument('--k', type=int, nargs='+', default=[1], choices=(1, 2, 3, 4),
                    help='rows per query, K = 1 first: every K is set beside the K = 1 of the same run')
    ap.add_argument('--cover', action='store_true',
                    help='the coverage part (--nnfm-cover): reverse search, index and gradient beside the forward groups')
    ap.add_argument('--masks', type=int, default=0, choices=(2, 4),
                    help='the guided term (--nnfm-masks) over S equal segments under stripe masks, beside the unguided '
                         'search against one segment and against the whole bank')
    opts = ap.parse_args()
    if (opts.cover or opts.masks) and (opts.patch != 1 or opts.k != [1]):
        ap.error('--cover, --masks: the table is that of patch 1 and K = 1')
    if opts.cover and opts.masks:
        ap.error('--cover and --masks are two tables')
    if opts.k[0] != 1:
        ap.error('--k: the list begins with 1, the row the others are set beside')
    if not torch.cuda.is_available():
        sys.exit('bench_nnfm: no GPU')
    net = builtin_net('vgg19')
    eng = TileEngine(net, 0, synthetic_weights(net, 0))
    lines = (cover_lines if opts.cover else guided_lines if opts.masks else table_lines)(eng, np.random.RandomState(0), opts)
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
