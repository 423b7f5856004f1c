"""The SWT regularizer of the reference (num_utils.py:179-196, style_transfer.py:716-720) for the
orthogonal Daubechies / symlet wavelets (``dbN``, ``symN``) at any level count, restated in numpy
float64.  tests/swt_levels_ref.py has the argument for Haar; this is the same argument for a longer
filter.  PyWavelets is in neither tree: PARITY UNPINNED, as for Haar.

For an orthonormal low-pass filter h (sum h = sqrt 2) and g[k] = (-1)^k h[len-1-k], level j of the
stationary transform filters with h and g dilated by d = 2^(j-1), periodic on the padded square, and
the inverse -- the mean of the reconstructions from the two cosets of shifts -- is half the adjoint
of that per level and axis (H'H + G'G = 2 I).  num_utils.py:191-192 zeroes every approximation band,
the inverse reads only the deepest one, so what is removed is the path through a_L alone:
    D = x - B_L x,   B_L = product over j of (r/2 at stride 2^(j-1)) along rows and columns,
with r the autocorrelation of h.  r depends on |H(w)|^2 alone, and dbN and symN differ only in which
roots of it go to H: both have
    |H(w)|^2 = 2 cos^2N(w/2) * sum over k < N of C(N-1+k, k) sin^2k(w/2)
(Daubechies 1988), which ``autocorrelation`` expands exactly in rationals -- a route that shares
nothing with the Lagrange-interpolation product the library builds its taps from.
``swt_filterbank`` does the transform and its inverse band by band for ANY orthonormal h, with no
closed form; tests/test_swt_wavelet_host.py holds the two against each other, with filters obtained
there by spectral factorisation.
"""

from fractions import Fraction
from math import comb

import numpy as np

from oracle import num_ops
from tests.swt_levels_ref import padded_side


def _mul(a, b):
    out = [Fraction(0)] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            out[i + j] += x * y
    return out


def autocorrelation_exact(order):
    """r[-(2N-1) .. 2N-1] of dbN / symN as Fractions: the coefficients of |H|^2 as a Laurent
    polynomial in z = e^{iw}, with cos^2(w/2) = (z + 2 + 1/z)/4 and sin^2(w/2) = (-z + 2 - 1/z)/4."""
    n = int(order)
    cos2 = [Fraction(1, 4), Fraction(1, 2), Fraction(1, 4)]
    sin2 = [Fraction(-1, 4), Fraction(1, 2), Fraction(-1, 4)]
    total = [Fraction(0)] * (2 * (n - 1) + 1)               # centred: index n - 1 is z^0
    power = [Fraction(1)]
    for k in range(n):
        for i, c in enumerate(power):                       # power = sin2^k, centred at index k
            total[n - 1 - k + i] += comb(n - 1 + k, k) * c
        power = _mul(power, sin2)
    front = [Fraction(2)]
    for _ in range(n):
        front = _mul(front, cos2)
    return _mul(front, total)                               # length 4 n - 1, centre at 2 n - 1


def autocorrelation(order):
    return np.array([float(c) for c in autocorrelation_exact(order)])


def swt_wavelet_detail(x, order, levels):
    """Detail part (deepest approximation band zeroed) of the ``levels``-level stationary transform
    with dbN / symN, N = ``order``, of every channel of x [C,H,W], on the symmetric padding to a
    power-of-two square, cropped back; float64."""
    x = np.asarray(x, np.float64)
    div = padded_side(*x.shape[1:])
    if not 1 <= levels <= int(np.log2(div)):
        raise ValueError('%d levels on a padded side of %d' % (levels, div))
    pw = num_ops._pad_width(x.shape, (1, div, div))
    xp = np.pad(x, pw, 'symmetric')
    r = autocorrelation(order)
    half = len(r) // 2
    blur = xp
    for j in range(levels):
        for axis in (1, 2):
            nxt = np.zeros_like(blur)
            for k in range(-half, half + 1):
                if r[k + half] != 0:
                    nxt += (0.5 * r[k + half]) * np.roll(blur, k * 2 ** j, axis)
            blur = nxt
    d = xp - blur
    return d[:, pw[1][0]:pw[1][0] + x.shape[1], pw[2][0]:pw[2][0] + x.shape[2]]


def swt_filterbank(ch, h, levels):
    """The same for ONE square 2-D array whose side is a power of two and any orthonormal low-pass
    filter h, band by band: dilated analysis along both axes with every detail band kept, the
    deepest low-low band zeroed, synthesis as half the adjoint (float64)."""
    a = np.asarray(ch, np.float64)
    h = np.asarray(h, np.float64)
    g = np.array([(-1) ** k * h[len(h) - 1 - k] for k in range(len(h))])

    def analysis(v, axis, d):
        lo, hi = np.zeros_like(v), np.zeros_like(v)
        for k in range(len(h)):
            shifted = np.roll(v, -k * d, axis)              # v[n + k d]
            lo += h[k] * shifted
            hi += g[k] * shifted
        return lo, hi

    def synthesis(lo, hi, axis, d):
        v = np.zeros_like(lo)
        for k in range(len(h)):                             # the adjoint: v[n] += f[k] band[n - k d]
            v += h[k] * np.roll(lo, k * d, axis) + g[k] * np.roll(hi, k * d, axis)
        return 0.5 * v

    details = []
    for j in range(levels):
        d = 2 ** j
        lo, hi = analysis(a, 0, d)
        a, lh = analysis(lo, 1, d)
        hl, hh = analysis(hi, 1, d)
        details.append((lh, hl, hh))
    a = np.zeros_like(a)
    for j in reversed(range(levels)):
        d = 2 ** j
        lh, hl, hh = details[j]
        a = synthesis(synthesis(a, lh, 1, d), synthesis(hl, hh, 1, d), 0, d)
    return a


def swt_norm_wavelet(x, order, levels, p=2):
    """(loss, grad) of num_utils.swt_norm(x, 'db<order>', levels, p): the p-norm and its own
    gradient at the detail image, not chained through the transform."""
    return num_ops.p_norm_loss_grad(swt_wavelet_detail(x, order, levels), p)
