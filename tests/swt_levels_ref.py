"""The SWT regularizer of the reference (num_utils.py:179-196, style_transfer.py:716-720) for the
Haar wavelet at any level count, restated in numpy float64.  oracle/num_ops.py has the one-level
form and the reasons for restating it (PyWavelets is in neither tree: PARITY UNPINNED); this is the
same argument carried through L levels.

Level j = 1..L of the stationary transform uses the two-tap Haar filters dilated by d = 2^(j-1),
periodic on the padded square:
    a_j[n] = (a_{j-1}[n] + a_{j-1}[n+d]) / sqrt 2,   d_j[n] = (a_{j-1}[n] - a_{j-1}[n+d]) / sqrt 2
The inverse averages, level by level, the two reconstructions that a decimated transform would give
from the two cosets of shifts.  num_utils.py:191-192 zeroes the approximation band of every level,
but the inverse reads only the deepest one, so what is removed is the path through a_L alone: per
axis and level, analysis followed by the synthesis of the low band is [1 2 1]/4 at stride d, hence
    D = x - B_L x,   B_L = product over j of ([1 2 1]/4 at stride 2^(j-1)) along rows and columns.
``swt_haar_filterbank`` does the transform and its inverse band by band, with no closed form, and
tests/test_swt_levels_host.py holds the two against each other.
"""

import numpy as np

from oracle import num_ops


def padded_side(h, w):
    return 2 ** int(np.ceil(np.log2(max(h, w))))


def swt_haar_detail(x, levels):
    """Detail part (deepest approximation band zeroed) of the ``levels``-level stationary Haar
    transform of every channel of x [C,H,W], on the symmetric padding to a power-of-two square,
    cropped back; float64."""
    x = np.asarray(x, np.float64)
    div = padded_side(*x.shape[1:])
    if not 1 <= levels <= int(np.log2(div)):
        raise ValueError('%d levels on a padded side of %d' % (levels, div))
    pw = num_ops._pad_width(x.shape, (1, div, div))
    xp = np.pad(x, pw, 'symmetric')
    blur = xp
    for j in range(levels):
        for axis in (1, 2):
            blur = (np.roll(blur, 2 ** j, axis) + 2 * blur + np.roll(blur, -2 ** j, axis)) / 4
    d = xp - blur
    return d[:, pw[1][0]:pw[1][0] + x.shape[1], pw[2][0]:pw[2][0] + x.shape[2]]


def swt_haar_filterbank(ch, levels):
    """The same for ONE square 2-D array whose side is a power of two, band by band: dilated
    analysis along both axes with every detail band kept, the deepest low-low band zeroed,
    synthesis as the mean of the two shifted reconstructions (float64)."""
    a = np.asarray(ch, np.float64)
    s = np.sqrt(0.5)

    def analysis(v, axis, d):
        nxt = np.roll(v, -d, axis)
        return s * (v + nxt), s * (v - nxt)

    def synthesis(lo, hi, axis, d):
        # v[n] from (lo[n], hi[n]) = s (v[n] +- v[n+d]) and from (lo[n-d], hi[n-d]); mean of both
        from_n = s * (lo + hi)
        from_prev = s * (np.roll(lo, d, axis) - np.roll(hi, d, axis))
        return 0.5 * (from_n + from_prev)

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


def swt_norm_haar(x, levels, p=2):
    """(loss, grad) of num_utils.swt_norm(x, 'haar', levels, p): the p-norm and its own gradient
    at the detail image, not chained through the transform."""
    return num_ops.p_norm_loss_grad(swt_haar_detail(x, levels), p)
