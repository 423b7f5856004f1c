"""The screened-Poisson output stage (stx_image_poisson, include/stx.h) in float64 numpy: the multigrid restated
operation for operation -- every sum in the order the kernels of csrc/poisson.hip take it, one rounding per
operation -- its level-count function, and an exact direct solve (the operator is diagonalised by the orthonormal
DCT-II) that the multigrid's convergence is measured against.

Per channel, with d = c - s and N(p) the 4-neighbours of p inside the picture, n(p) = |N(p)|:

    e_p + lam sum_{q in N(p)} (e_p - e_q) = lam (n(p) d_p - sum_{q in N(p)} d_q)          (A e = b)

and the output is float32(double(s) + e).  A neighbour outside the picture enters every sum as +0.0, and every
neighbour sum is ((left + right) + up) + down.
"""

import functools

import numpy as np

POISSON_CYCLES_DEFAULT = 9     # (the smallest count that meets the cap on every case, plus 2)
POISSON_LAMBDA_MAX = 1000.0
POISSON_COARSEST_LAMBDA = 0.05
POISSON_PRE, POISSON_POST, POISSON_COARSEST = 2, 2, 20


def levels(height, width, lam):
    """[(h, w, lambda)] from the picture down: h' = ceil(h / 2), w' = ceil(w / 2), lambda' = lambda / 4; a level is
    the coarsest when min(h, w) <= 2 or lambda <= 0.05."""
    out = [(int(height), int(width), float(lam))]
    while not (min(out[-1][0], out[-1][1]) <= 2 or out[-1][2] <= POISSON_COARSEST_LAMBDA):
        h, w, l = out[-1]
        out.append(((h + 1) // 2, (w + 1) // 2, l / 4.0))
    return out


def level_count(height, width, lam):
    return len(levels(height, width, lam))


def launch_count(height, width, lam, cycles=POISSON_CYCLES_DEFAULT):
    """Kernel launches of one solve: the right-hand side and the output, and per W-cycle, with 2^l visits of level
    l, 40 half-sweeps at a visit of the coarsest level and 8 half-sweeps, one residual + restriction and one
    prolongation + add at a visit of any other."""
    n = level_count(height, width, lam)
    per_cycle = sum((2 ** l) * (2 * POISSON_COARSEST if l == n - 1 else 2 * (POISSON_PRE + POISSON_POST) + 2)
                    for l in range(n))
    return 2 + cycles * per_cycle


def neighbour_sum(a):
    """((left + right) + up) + down over [..., H, W], +0.0 for a neighbour outside."""
    p = np.zeros(a.shape[:-2] + (a.shape[-2] + 2, a.shape[-1] + 2), np.float64)
    p[..., 1:-1, 1:-1] = a
    return ((p[..., 1:-1, :-2] + p[..., 1:-1, 2:]) + p[..., :-2, 1:-1]) + p[..., 2:, 1:-1]


@functools.lru_cache(maxsize=None)
def neighbour_count(height, width):
    out = neighbour_sum(np.ones((height, width), np.float64))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def colour_mask(height, width, colour):
    yy, xx = np.mgrid[0:height, 0:width]
    return ((yy + xx) & 1) == colour


def rhs(s, c, lam):
    """b = lam * (n d - sum_q d_q) with d = double(c) - double(s)."""
    d = np.asarray(c, np.float64) - np.asarray(s, np.float64)
    return lam * (neighbour_count(*d.shape[-2:]) * d - neighbour_sum(d))


def half_sweep(e, b, lam, colour):
    """e_p = (b_p + lam S_p) / (1 + lam n(p)) at the pixels with (y + x) & 1 == colour, in place."""
    h, w = e.shape[-2:]
    mask = colour_mask(h, w, colour)
    new = (b + lam * neighbour_sum(e)) / (1.0 + lam * neighbour_count(h, w))
    e[..., mask] = new[..., mask]


def sweeps(e, b, lam, count, first):
    for _ in range(count):
        half_sweep(e, b, lam, first)
        half_sweep(e, b, lam, first ^ 1)


def residual(e, b, lam):
    """r_p = (b_p + lam S_p) - (1 + lam n(p)) e_p."""
    return (b + lam * neighbour_sum(e)) - (1.0 + lam * neighbour_count(*e.shape[-2:])) * e


def restrict(r):
    """The mean over the existing children (2Y + dy, 2X + dx) of a coarse cell: (((r00 + r01) + r10) + r11) / count
    with +0.0 for a child outside."""
    h, w = r.shape[-2:]
    hc, wc = (h + 1) // 2, (w + 1) // 2
    p = np.zeros(r.shape[:-2] + (2 * hc, 2 * wc), np.float64)
    p[..., :h, :w] = r
    ones = np.zeros((2 * hc, 2 * wc), np.float64)
    ones[:h, :w] = 1.0
    total = ((p[..., 0::2, 0::2] + p[..., 0::2, 1::2]) + p[..., 1::2, 0::2]) + p[..., 1::2, 1::2]
    count = ((ones[0::2, 0::2] + ones[0::2, 1::2]) + ones[1::2, 0::2]) + ones[1::2, 1::2]
    return total / count


def prolong(ec, height, width):
    """Cell-centred bilinear: with (Y, X) = (y >> 1, x >> 1) and (Yn, Xn) the parent's neighbour on the child's side
    (+1 for an odd coordinate, -1 for an even one), clamped to the level,
    0.75 (0.75 E[Y,X] + 0.25 E[Y,Xn]) + 0.25 (0.75 E[Yn,X] + 0.25 E[Yn,Xn])."""
    hc, wc = ec.shape[-2:]
    y, x = np.arange(height), np.arange(width)
    Y, X = y >> 1, x >> 1
    Yn = np.clip(Y + np.where(y & 1, 1, -1), 0, hc - 1)
    Xn = np.clip(X + np.where(x & 1, 1, -1), 0, wc - 1)
    top = 0.75 * ec[..., Y[:, None], X[None, :]] + 0.25 * ec[..., Y[:, None], Xn[None, :]]
    other = 0.75 * ec[..., Yn[:, None], X[None, :]] + 0.25 * ec[..., Yn[:, None], Xn[None, :]]
    return 0.75 * top + 0.25 * other


def w_cycle(es, bs, lv, l):
    """One visit of level l: es[l] is improved in place for the right-hand side bs[l]."""
    lam = lv[l][2]
    if l == len(lv) - 1:
        sweeps(es[l], bs[l], lam, POISSON_COARSEST, 0)
        return
    sweeps(es[l], bs[l], lam, POISSON_PRE, 0)
    bs[l + 1] = restrict(residual(es[l], bs[l], lam))
    es[l + 1] = np.zeros_like(bs[l + 1])
    w_cycle(es, bs, lv, l + 1)
    w_cycle(es, bs, lv, l + 1)
    es[l] += prolong(es[l + 1], lv[l][0], lv[l][1])
    sweeps(es[l], bs[l], lam, POISSON_POST, 1)


def correction(s, c, lam, cycles=POISSON_CYCLES_DEFAULT):
    """The multigrid's e [..., H, W] in float64 after ``cycles`` W-cycles from e = 0."""
    s, c = np.asarray(s), np.asarray(c)
    lv = levels(s.shape[-2], s.shape[-1], lam)
    bs, es = [None] * len(lv), [None] * len(lv)
    bs[0] = rhs(s, c, float(lam))
    es[0] = np.zeros_like(bs[0])
    for _ in range(cycles):
        w_cycle(es, bs, lv, 0)
    return es[0]


def solve(s, c, lam, cycles=POISSON_CYCLES_DEFAULT):
    """What stx_image_poisson writes: float32(double(s) + e)."""
    return (np.asarray(s, np.float64) + correction(s, c, lam, cycles)).astype(np.float32)


def apply_operator(e, lam):
    """A e = e_p + lam sum_q (e_p - e_q)."""
    return e + lam * (neighbour_count(*e.shape[-2:]) * e - neighbour_sum(e))


def dct_matrix(n):
    """The orthonormal DCT-II as an [n, n] matrix: rows are the eigenvectors of the 1-D Neumann Laplacian."""
    k, i = np.arange(n)[:, None], np.arange(n)[None, :]
    m = np.cos(np.pi * k * (2 * i + 1) / (2.0 * n)) * np.sqrt(2.0 / n)
    m[0] /= np.sqrt(2.0)
    return m


def direct(s, c, lam):
    """The exact e: A has the eigenvalues 1 + lam (4 - 2 cos(pi i / H) - 2 cos(pi j / W)) on the DCT-II basis."""
    b = rhs(s, c, float(lam))
    h, w = b.shape[-2:]
    ch, cw = dct_matrix(h), dct_matrix(w)
    eig = 1.0 + lam * ((2.0 - 2.0 * np.cos(np.pi * np.arange(h) / h))[:, None]
                       + (2.0 - 2.0 * np.cos(np.pi * np.arange(w) / w))[None, :])
    return ch.T @ ((ch @ b @ cw.T) / eig) @ cw


def energy(f, s, c, lam):
    """sum (f - s)^2 + lam sum over edges ((f_p - f_q) - (c_p - c_q))^2."""
    f, s, c = (np.asarray(a, np.float64) for a in (f, s, c))
    g = f - c
    return float(((f - s) ** 2).sum() + lam * ((np.diff(g, axis=-1) ** 2).sum() + (np.diff(g, axis=-2) ** 2).sum()))


def case(height, width, seed=0, channels=None):
    """Uniform-noise s against noise-plus-step c, both in 0 ... 255 (float32): the convergence cases' pictures."""
    rng = np.random.RandomState(seed + 1000 * height + width)
    shape = (height, width) if channels is None else (channels, height, width)
    s = rng.uniform(0, 255, shape).astype(np.float32)
    c = rng.uniform(0, 100, shape)
    c[..., :, width // 2:] += 155.0
    return s, c.astype(np.float32)
