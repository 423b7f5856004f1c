"""Which kernel, tiling and K split a stx_op_conv_* hook call takes: the launchers' own arithmetic restated in
Python, shape and switches in, a branch name out.  Nothing here measures; every line has its source beside it.  The
default switches are assumed but for STX_CONV_ALGO (`algo`); plane sets stay far below the 2 GiB addressing limits.

A branch is 'family tiling split':
  'first'                                   conv_first_kernel (op_hooks.cpp: conv_first_usable)
  'm4'                                      conv3x3_m4_kernel (op_hooks.cpp: ksize 3, Cin <= 4 backward)
  'h2 64x8x32 | 128x8x32 | 64x16x32 ...'    conv_h2.hip, channels x patch rows x patch columns
  'wino2 4x64 | 16x16 | 8x32 ...'           conv_wino2.hip, patch rows x columns
  'direct v<id> ...'                        conv_mfma.hip, the variant of kVariants
and the split 'unsplit', 'split <f>' (every workgroup stores a K slice into the engine's workspace and
splitk_reduce_launch writes y) or 'tail <items>x<slices>' (wino2_launch_tail: only the last items are sliced)."""


def _cdiv(a, b):
    return -(-a // b)


# conv_mfma.hip kVariants: id -> (ks, kc, bm, pr, pc, inject)
DIRECT = {3: (3, 8, 32, 8, 32, False), 5: (3, 8, 64, 4, 32, True), 2: (3, 8, 64, 8, 32, True), 8: (3, 4, 64, 4, 32, False),
          12: (1, 32, 64, 4, 32, False), 6: (1, 16, 128, 8, 32, False), 7: (1, 16, 64, 8, 64, False)}
H2 = {0: ('64x8x32', 64, 8, 2.0, 8.5), 1: ('128x8x32', 128, 8, 2.75, 17.0), 2: ('64x16x32', 64, 16, 3.5, 17.0)}
WINO2 = {0: ('4x64', 4, 64), 1: ('16x16', 16, 16), 2: ('8x32', 8, 32)}


def h2_plan(cfg, K, M, H, W):
    """conv_h2.hip h2_plan -> (factor, cost); KC = 16, PC = 32."""
    _, bm, pr, t_chunk, t_fixed = H2[cfg]
    n_pairs = K // 32
    n = _cdiv(M, bm) * _cdiv(H, pr) * _cdiv(W, 32)
    out_mb = 4e-6 * M * H * W
    best, best_cost = 1, 0.0
    f = 1
    while f <= 8 and (f == 1 or n_pairs // f >= 2):
        rounds = _cdiv(n * f, 256)
        c = rounds * (2.0 * _cdiv(n_pairs, f) * t_chunk + t_fixed)
        if f > 1:
            c += (f + 1) * out_mb / 3.0 + 5.0
        if f == 1 or c < best_cost:
            best, best_cost = f, c
        f += 1
    return best, best_cost


def h2_pick(K, M, H, W):
    """conv_h2.hip h2_pick_config: the cheapest tiling, 128 channels only where M % 128 == 0."""
    best, best_cost = 0, h2_plan(0, K, M, H, W)[1]
    for cfg in (1, 2):
        if cfg == 1 and M % 128:
            continue
        c = h2_plan(cfg, K, M, H, W)[1]
        if c < best_cost:
            best, best_cost = cfg, c
    return best


def wino2_geometry(H, W):
    """conv_wino2.hip wino2_pick_geometry."""
    if W <= 40:
        return 1
    wide, mid = _cdiv(H, 4) * _cdiv(W, 64), _cdiv(H, 8) * _cdiv(W, 32)
    return 2 if mid * 10 <= wide * 9 else 0


def wino2_uniform(geo, K, M, H, W):
    """conv_wino2.hip wino2_uniform_plan -> (factor, cost); KC = 8, BM = 64."""
    _, pr, pc = WINO2[geo]
    n_chunks = _cdiv(K, 8)
    n = _cdiv(M, 64) * _cdiv(H, pr) * _cdiv(W, pc)
    out_mb = 4e-6 * M * H * W
    best, best_cost = 1, 0.0
    f = 1
    while f <= 8 and n_chunks // f >= 4:
        rounds = _cdiv(n * f, 256)
        c = rounds * (n_chunks / f * 2.05 + 6.0)
        if f > 1:
            c += (f + 1) * out_mb / 3.0 + 5.0
        if f == 1 or c < best_cost:
            best, best_cost = f, c
        f += 1
    return best, best_cost


def wino2_tail(geo, K, M, H, W):
    """conv_wino2.hip wino2_tail_plan / wino2_tail_choice -> (items, slices, cost) or None."""
    _, pr, pc = WINO2[geo]
    n_chunks = _cdiv(K, 8)
    n = _cdiv(M, 64) * _cdiv(H, pr) * _cdiv(W, pc)
    q, r = divmod(n, 256)
    if q < 1 or r == 0:
        return None
    f = min(8, 256 // r, n_chunks // 4)
    if f < 2:
        return None
    round_us = lambda chunks: chunks * 2.05 + 6.0
    cost = q * round_us(n_chunks) + round_us(_cdiv(n_chunks, f)) + (f + 1) * r * (4e-6 * 64 * pr * pc) / 3.0 + 5.0 + 6.0
    return (r, f, cost) if cost < wino2_uniform(geo, K, M, H, W)[1] else None


def direct_config(ks, K, M, H, W):
    """conv_mfma.hip conv_pick_config."""
    if ks == 1:
        return 12 if H * W <= 128 * 128 else (6 if M >= 128 else 7)
    if K <= 4:
        return 8
    if M <= 32:
        return 3
    if _cdiv(M, 64) * _cdiv(H, 8) * _cdiv(W, 32) >= 2048 and K >= 128:
        return 2
    return 5


def direct_split(cfg, K, M, H, W):
    """conv_mfma.hip direct_splitk_factor (packed weights, forward or backward-data)."""
    ks, kc, bm, pr, pc, inject = DIRECT[cfg]
    if ks != 3 or not inject:
        return 1
    n_wg = _cdiv(M, bm) * _cdiv(H, pr) * _cdiv(W, pc)
    max_split = min(16, _cdiv(K, kc) // 4)
    for f in range(1, max_split + 1):
        n = n_wg * f
        if n > 5 * 256:
            return f
        if n >= 512 and (n / 256) / _cdiv(n, 256) >= 0.9:
            return f
    return max(max_split, 1)


def _split(f):
    return 'unsplit' if f == 1 else 'split %d' % f


def branch(direction, cin, cout, h, w, ks=3, algo=None):
    """The branch of stx_op_conv_forward ('f') or stx_op_conv_backward_data ('b') for a Caffe layer cin -> cout."""
    if direction == 'f' and ks == 3 and 1 <= cin <= 3 and cout == 64:        # op_hooks.cpp: conv_first_usable
        return 'first'
    if direction == 'b' and ks == 3 and cin <= 4:                            # op_hooks.cpp: conv_small_launch
        return 'm4'
    K, M = (cin, cout) if direction == 'f' else (cout, cin)
    # conv_dispatch.cpp h2_choice: forced by STX_CONV_ALGO=h2*, else from 64 channels on both sides; h2_usable
    force = {'h2a': 0, 'h2b': 1, 'h2c': 2}.get(algo)
    h2 = (force is not None or (not algo and K >= 64 and M >= 64)) and ks == 3 and K % 32 == 0 and K >= 32
    if h2:
        cfg = force if force is not None else h2_pick(K, M, h, w)
        return 'h2 %s %s' % (H2[cfg][0], _split(h2_plan(cfg, K, M, h, w)[0]))
    # conv_dispatch.cpp wino_choice (the engine's winograd flag is on by default)
    if ks == 3 and K >= 8 and M > 4 and algo != 'direct':
        geo = {'wino2a': 0, 'wino2b': 1, 'wino2c': 2}.get(algo)
        if geo is None and M > 32:
            geo = wino2_geometry(h, w)
        if geo is not None:
            tail = wino2_tail(geo, K, M, h, w)
            if tail:
                return 'wino2 %s tail %dx%d' % (WINO2[geo][0], tail[0], tail[1])
            return 'wino2 %s %s' % (WINO2[geo][0], _split(wino2_uniform(geo, K, M, h, w)[0]))
    cfg = direct_config(ks, K, M, h, w)
    return 'direct v%d %s' % (cfg, _split(direct_split(cfg, K, M, h, w)))
