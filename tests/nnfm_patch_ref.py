"""Reference arithmetic of the 3 x 3 patch form of the nearest-neighbour term (--nnfm-patch 3,
stx_set_nnfm_patch_targets) for the tests, in float64.  For a blob F [C, h, w] with n = h w pixels p = (y, x)
and a bank B [M, 9 C] of unit or zero rows b_j:

    P_p[t, c] = F[c][y + dy][x + dx]               t = (dy, dx), dy outer, dx inner, (-1, -1) first; 0 outside
    R_p = |P_p|,  X_p = P_p / R_p                  (R_p = 0: X_p = 0, c_p = 0, j_p = 0, G_p = 0)
    j_p = argmax_j P_p . b_j                       (the lowest j among equal scores)
    c_p = X_p . b_{j_p}
    E   = (2/n) sum_p (1 - c_p)
    G_p = -(b_{j_p} - c_p X_p) / R_p               (9 C: n d(E/2)/dP_p with j_p held fixed)
    S[c][p] = sum_t G_{p - t}[t, c]                over the taps whose centre p - t lies in the map

Every function takes ``patch`` (3 by default); with ``patch=1`` it IS tests/nnfm_ref.py's.  ``emulated_scores``
restates the GPU's search: fp16 hi / lo pieces of the columns under ONE power of two for the blob (the largest
column norm into (2^12, 2^13]) and of b 2^13, stages in the order tap, then channel.  ``NnfmPatchOracleModel`` is
the oracle's tile evaluation with this term where ``NnfmOracleModel`` has its own."""

import math

import numpy as np

from tests import nnfm_ref
from tests.nnfm_ref import bank_rows, concat_banks, normalized      # noqa: F401  (the same for both forms)

TAPS = [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]


def patches(F, patch=3):
    """P [n, patch^2 C] of F [C, h, w] in float64, tap-major, zero-padded."""
    F = np.asarray(F, np.float64)
    c, h, w = F.shape
    if patch == 1:
        return F.reshape(c, -1).T.copy()
    padded = np.zeros((c, h + 2, w + 2))
    padded[:, 1:-1, 1:-1] = F
    return np.concatenate([padded[:, 1 + dy:1 + dy + h, 1 + dx:1 + dx + w].reshape(c, -1).T for dy, dx in TAPS], axis=1)


def unit_patches(F, patch=3):
    """(X [n, patch^2 C], R [n]); a zero patch gives a zero row."""
    p = patches(F, patch)
    r = np.sqrt((p * p).sum(axis=1))
    return np.divide(p, r[:, None], out=np.zeros_like(p), where=r[:, None] > 0), r


def patch_bank_of(F, stride=1, patch=3):
    """The bank of one feature map: its unit patches centred at y % stride == 0 and x % stride == 0, raster
    order, [rows, patch^2 C].  The stride thins the centres only."""
    if patch == 1:
        return nnfm_ref.bank_of(F, stride)
    _, h, w = np.shape(F)
    x = unit_patches(F, patch)[0]
    return x.reshape(h, w, -1)[::stride, ::stride].reshape(-1, x.shape[1])


def scores64(F, B, patch=3):
    if patch == 1:
        return nnfm_ref.scores64(F, B)
    return unit_patches(F, patch)[0] @ np.asarray(B, np.float64).T


def nearest(F, B, patch=3):
    """j [n]: the float64 argmax, lowest index among equals."""
    if patch == 1:
        return nnfm_ref.nearest(F, B)
    return np.argmax(scores64(F, B, patch), axis=1).astype(np.int64)


def fold(G, shape):
    """S [C, h, w] of the patch gradients G [n, 9 C]: patch p's tap t goes to pixel p + t, where it was read."""
    c, h, w = shape
    g = np.asarray(G, np.float64).reshape(h, w, 9, c)
    padded = np.zeros((c, h + 2, w + 2))
    for t, (dy, dx) in enumerate(TAPS):
        padded[:, 1 + dy:1 + dy + h, 1 + dx:1 + dx + w] += g[:, :, t, :].transpose(2, 0, 1)
    return padded[:, 1:-1, 1:-1].copy()


def terms_at(F, B, j, patch=3):
    """(E, S [like F], sum |S|, c [n]) with the rows j [n] given."""
    if patch == 1:
        return nnfm_ref.terms_at(F, B, j)
    x, r = unit_patches(F, patch)
    b = np.asarray(B, np.float64)[np.asarray(j, np.int64)]
    c = np.where(r > 0, (x * b).sum(axis=1), 0.0)
    inv = np.divide(1.0, r, out=np.zeros_like(r), where=r > 0)
    S = fold(-(b - c[:, None] * x) * inv[:, None], np.shape(F))
    return 2.0 * float((1.0 - c).sum()) / len(r), S, float(np.abs(S).sum()), c


def terms(F, B, patch=3):
    """(E, S, sum |S|, c, j) at the reference's own rows."""
    if patch == 1:
        return nnfm_ref.terms(F, B)
    j = nearest(F, B, patch)
    return terms_at(F, B, j, patch) + (j,)


def half_e_unit(F, B, patch=3):
    """E / 2 as (1 / 2n) sum_p |X_p - b_{j_p}|^2 (unit rows, no zero patch): without the cancelled 1 - c_p."""
    if patch == 1:
        return nnfm_ref.half_e_unit(F, B)
    x, _ = unit_patches(F, patch)
    b = np.asarray(B, np.float64)[nearest(F, B, patch)]
    return float(((x - b) ** 2).sum()) / (2 * x.shape[0])


def finite_difference(F, B, index, h, patch=3):
    """Central difference of E / 2 along element ``index`` of F; the rows are searched anew on both sides."""
    if patch == 1:
        return nnfm_ref.finite_difference(F, B, index, h)
    plus, minus = np.array(F, np.float64), np.array(F, np.float64)
    plus[index] += h
    minus[index] -= h
    return (half_e_unit(plus, B, patch) - half_e_unit(minus, B, patch)) / (2 * h)


def common_scale(F):
    """The power of two that puts the largest column norm of F into (2^12, 2^13] (1 for a zero blob)."""
    f = np.asarray(F, np.float64).reshape(np.shape(F)[0], -1)
    m = math.sqrt(float((f * f).sum(axis=0).max()))
    if m == 0:
        return 1.0
    frac, e = math.frexp(m)         # m = frac 2^e, frac in [0.5, 1)
    return 2.0 ** ((14 if frac == 0.5 else 13) - e)


def emulated_scores(F, B, patch=3):
    """The search's scores [n, M] as the GPU forms them, in cosine units (over scale 2^13 R_p): float32 inputs,
    the pieces of f scale gathered into patches and of b 2^13, per 16-channel step lo hi + hi lo + hi hi added
    to a float32 accumulator, the steps in the order tap, then channel."""
    if patch == 1:
        return nnfm_ref.emulated_scores(F, B)
    shape = np.shape(F)
    scale = common_scale(np.asarray(F, np.float32))
    fh, fl = nnfm_ref._split((np.asarray(F, np.float32) * np.float32(scale)).astype(np.float32))
    xh, xl = patches(fh.reshape(shape)), patches(fl.reshape(shape))
    bh, bl = nnfm_ref._split(np.asarray(B, np.float32) * np.float32(nnfm_ref.SCALE))
    acc = np.zeros((xh.shape[0], bh.shape[0]), np.float32)
    for k in range(0, xh.shape[1], 16):
        s = slice(k, k + 16)
        for a, b in ((bl, xh), (bh, xl), (bh, xh)):
            acc = (acc.astype(np.float64) + b[:, s] @ a[:, s].T).astype(np.float32)
    r = unit_patches(np.asarray(F, np.float32))[1]
    inv = np.divide(1.0, r, out=np.zeros_like(r), where=r > 0)
    return acc.astype(np.float64) / (scale * nnfm_ref.SCALE) * inv[:, None]


def search_error(F, B, patch=3):
    """The emulation's worst |score - float64 score| over all pairs, in cosine units."""
    return float(np.abs(emulated_scores(F, B, patch) - scores64(F, B, patch)).max())


class NnfmPatchOracleModel(nnfm_ref.NnfmOracleModel):
    """``NnfmOracleModel`` whose banks are patch banks: ``nnfm_banks`` = {layer: B [M, 9 C]}.  The term stands
    where the parent's stands -- the parent's evaluation runs with this module's ``terms`` in place of its own."""

    def nnfm_loss64(self, acts, layer_weights):
        return sum(layer_weights.get(b, 1.0) * self.nnfm_weights.get(b, 1.0) * terms(acts[b], self.nnfm_banks[b])[0] / 2
                   for b in self.nnfm_banks)

    def sc_grad_tile(self, *args, **kwargs):
        plain = nnfm_ref.terms
        nnfm_ref.terms = terms
        try:
            return super().sc_grad_tile(*args, **kwargs)
        finally:
            nnfm_ref.terms = plain
