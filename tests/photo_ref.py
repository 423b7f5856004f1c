"""The photorealism regulariser (Luan, Paris, Shechtman, Bala, "Deep Photo Style Transfer", 2017) in float64
numpy -- there is no reference implementation of this term --, in two forms that share no code path:

  * matrix-free (``photo_loss`` / ``apply_l``): per 3 x 3 window the affine fit of a plane of the iterate to
    the content picture's colours and its nine residuals, gathered per pixel;
  * dense (``dense_l``): the matting Laplacian of Levin, Lischinski and Weiss, built window by window,
        L_ij = sum over windows k holding i and j of [ delta_ij - (1 + (I_i - mu_k)^T (S_k + eps/9 Id)^-1 (I_j - mu_k)) / 9 ]
    for pictures of up to about 12 x 12.

Pictures are [3, H, W] in the library's units (0..255 scale; a constant offset changes nothing).  Also here:
the test pictures, and the emulations of what a device may round (``emulate``), which price the GPU tests'
bounds without a GPU."""

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

UNIT = 255.0
# the nine pixels of a window in row-major order: (dy, dx) of pixel j relative to the window's first pixel
OFFSETS = [(j // 3, j % 3) for j in range(9)]


def _windows(planes):
    """[C, H, W] -> [H - 2, W - 2, 9, C]: the pixels of every window, row-major inside a window."""
    view = sliding_window_view(planes, (3, 3), axis=(1, 2))            # [C, H-2, W-2, 3, 3]
    return np.ascontiguousarray(view.reshape(view.shape[:3] + (9,)).transpose(1, 2, 3, 0))


def window_fit(img, content, eps, dtype=np.float64):
    """Per window and plane: the residuals r [H-2, W-2, 9, 3 planes] and the coefficients a [H-2, W-2, 3
    planes, 3].  ``dtype`` is the precision of the window algebra (the inputs are converted to it first)."""
    I = _windows(np.asarray(content, dtype) / dtype(UNIT))
    v = _windows(np.asarray(img, dtype) / dtype(UNIT))
    dI = I - I.mean(axis=2, keepdims=True)
    dv = v - v.mean(axis=2, keepdims=True)
    dIt = dI.transpose(0, 1, 3, 2)
    S = np.matmul(dIt, dI) / dtype(9) + dtype(eps) / dtype(9) * np.eye(3, dtype=dtype)
    q = np.matmul(dIt, dv) / dtype(9)                                  # [.., 3 colours, 3 planes]
    a = np.linalg.solve(S, q)                                          # [.., 3 colours, 3 planes]
    r = dv - np.matmul(dI, a)
    return r, a.transpose(0, 1, 3, 2)


def gather(r, H, W, dtype=np.float64, order=range(9)):
    """(L v)_i: the sum over the windows holding pixel i of its residual there.  r: [H-2, W-2, 9, C] ->
    [C, H, W].  ``order``: the order in which a pixel's (up to) nine terms are added, by window offset."""
    out = np.zeros((r.shape[3], H, W), dtype)
    for j in order:
        dy, dx = OFFSETS[j]
        out[:, dy:dy + H - 2, dx:dx + W - 2] += r[:, :, j, :].transpose(2, 0, 1).astype(dtype)
    return out


def photo_loss(img, content, eps, scale=1.0, fit=None):
    """(loss, grad [3, H, W]) of scale * sum_c v_c^T L v_c in float64: the loss as the sum of non-negatives
    sum r^2 + eps |a|^2, the gradient as scale * 2 * (L v_c) / 255.  ``fit``: window_fit of the same
    arguments, where the caller has it already."""
    _, H, W = np.shape(img)
    assert H >= 3 and W >= 3, (H, W)
    r, a = window_fit(img, content, eps) if fit is None else fit
    loss = scale * (np.sum(r * r) + eps * np.sum(a * a))
    return loss, scale * 2.0 * gather(r, H, W) / UNIT


def apply_l(plane, content, eps):
    """L v for one plane v [H, W] (already divided by 255, or anything else: L is linear)."""
    H, W = plane.shape
    r, _ = window_fit(np.stack([plane] * 3) * UNIT, content, eps)
    return gather(r, H, W)[0]


def dense_l(content, eps):
    """The matting Laplacian [H W, H W] of a small content picture, window by window."""
    I = np.float64(content) / UNIT
    _, H, W = I.shape
    assert H * W <= 200, 'dense_l is for small pictures'
    L = np.zeros((H * W, H * W))
    for cy in range(1, H - 1):
        for cx in range(1, W - 1):
            idx = [(cy - 1 + dy) * W + cx - 1 + dx for dy, dx in OFFSETS]
            pix = np.stack([I[:, cy - 1 + dy, cx - 1 + dx] for dy, dx in OFFSETS])     # [9, 3]
            d = pix - pix.mean(axis=0)
            S = d.T @ d / 9.0 + eps / 9.0 * np.eye(3)
            L[np.ix_(idx, idx)] += np.eye(9) - (1.0 + d @ np.linalg.inv(S) @ d.T) / 9.0
    return L


# ------------------------------------------------------------------------------ what a device may round
ORDERS = (tuple(range(9)), tuple(range(8, -1, -1)), (4, 0, 8, 2, 6, 1, 7, 3, 5), (0, 2, 4, 6, 8, 1, 3, 5, 7))


def emulate(img, content, eps, scale, order=range(9), fit=None):
    """The gradient with float64 window algebra, each residual rounded to float32 and a pixel's nine
    residuals added in float32 in ``order``; the factor 2 scale / 255 is applied in float64 and the result
    rounded to float32 once.  Anything that keeps more in float64 is at least as close to the reference."""
    _, H, W = np.shape(img)
    r, _ = window_fit(img, content, eps) if fit is None else fit
    return np.float32(np.float64(gather(r.astype(np.float32, copy=False), H, W, np.float32, order)) *
                      (2.0 * scale / UNIT))


def emulated_k(img, content, eps, scale, grad_ref, fit=None):
    """The worst error of ``emulate`` over ORDERS against the float64 gradient, in ``spread_unit``s."""
    fit = window_fit(img, content, eps) if fit is None else fit
    fit = (np.float32(fit[0]), fit[1])                       # (rounded once, for every order)
    worst = max(np.abs(np.float64(emulate(img, content, eps, scale, order, fit)) - grad_ref).max()
                for order in ORDERS)
    return worst / spread_unit(img, scale)


def all_float32(img, content, eps, scale):
    """The gradient with the whole window algebra in float32 (what the kernel must not do)."""
    _, H, W = np.shape(img)
    r, _ = window_fit(img, content, eps, np.float32)
    return np.float32(gather(r, H, W, np.float32)) * np.float32(2.0 * scale / UNIT)


def spread_unit(img, scale):
    """2^-24 * 9 * (max over windows and planes of |v - m_k|) / 255 * 2 scale: one float32 rounding of each
    of a pixel's nine residuals at their largest, in the gradient's units -- the unit of the budget where
    the reference gradient itself is of the order of eps."""
    v = _windows(np.float64(img))
    return 2.0 ** -24 * 9 * np.abs(v - v.mean(axis=2, keepdims=True)).max() / UNIT * 2.0 * scale


# ------------------------------------------------------------------------------ pictures
def noise(hw, seed):
    """(iterate, content): seeded noise over the library's range."""
    rng = np.random.RandomState(seed)
    return (rng.uniform(-120, 130, (3,) + tuple(hw)).astype(np.float32),
            rng.uniform(-120, 130, (3,) + tuple(hw)).astype(np.float32))


def colour_line(hw, seed=0, mean=(103.939, 116.779, 123.68)):
    """(iterate, content).  The content picture's colours lie on one line up to the rounding to 8 bits, so the
    window covariances have one large and two tiny eigenvalues, and a 30 x 40 corner is flat where the size
    allows: base = sin(x / 9) cos(y / 7), planes 0.4 base + 0.5, 0.3 base + 0.4, 0.5 - 0.2 base, rounded to
    u8, minus the mean.  The iterate is its first plane on every plane plus noise of 0.2 * 255."""
    H, W = hw
    y, x = np.mgrid[:H, :W]
    base = np.sin(x / 9.0) * np.cos(y / 7.0)
    planes = np.stack([0.4 * base + 0.5, 0.3 * base + 0.4, 0.5 - 0.2 * base])
    u8 = np.round(planes * 255.0)
    if H > 30 and W > 40:
        u8[:, :30, :40] = u8[:, :1, :1]
    content = np.float32(u8 - np.float64(mean).reshape(3, 1, 1))
    rng = np.random.RandomState(seed)
    img = np.float32(content[:1] + 0.2 * 255.0 * rng.standard_normal((3, H, W)))
    return img, content


def flat(hw, seed=0):
    """(iterate, content): a content picture of one colour under a noise iterate."""
    img, _ = noise(hw, seed)
    content = np.empty((3,) + tuple(hw), np.float32)
    content[:] = np.float32([-20.5, 31.25, 7.0]).reshape(3, 1, 1)
    return img, content
