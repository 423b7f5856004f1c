"""Device-resident full-image operations (thin wrappers over the stx_image_* / stx_vec_* ABI).

These replace the host-side numpy of the reference's step loop: ``roll2`` + tile slicing
(``num_utils.py:136-140``, ``style_transfer.py:632,642``), ``tv_norm`` / ``p_norm`` / aux term
(``style_transfer.py:709-733``), the statistics of ``transfer`` (``style_transfer.py:808-815``)
and ``get_image`` (``style_transfer.py:378-386``).  Images are ``DeviceArray`` [3,H,W] on the
engine's GPU and stay UN-rolled: the per-iteration shift is an index offset in cut / put.
"""

import ctypes
import re

import numpy as np

from . import lib


def _xy(roll):
    if roll is None:
        return (ctypes.c_int * 2)(0, 0)
    return (ctypes.c_int * 2)(int(roll[0]), int(roll[1]))


def cut_tile(engine, img, roll_xy, rect, tile):
    """tile <- window rect=(y0,y1,x0,x1) of roll2(img, roll_xy)."""
    y0, y1, x0, x1 = rect
    _, H, W = img.shape
    lib.call('stx_image_cut_tile', engine.handle, img.ptr, H, W, _xy(roll_xy), y0, x0, y1 - y0,
             x1 - x0, tile.ptr)


def put_tile(engine, grad, roll_xy, rect, tile_grad):
    """Places a tile gradient back into the un-rolled full gradient."""
    y0, y1, x0, x1 = rect
    _, H, W = grad.shape
    lib.call('stx_image_put_tile', engine.handle, grad.ptr, H, W, _xy(roll_xy), y0, x0, y1 - y0,
             x1 - x0, tile_grad.ptr)


class PendingScalar:
    def __init__(self):
        self._v = ctypes.c_double(float('nan'))

    @property
    def value(self):
        return self._v.value


def regularizers(engine, img, grad, mean_bgr, tv_scale, tv_power, p_scale, p_power, aux=None,
                 aux_scale=0.0, aux_roll=None):
    """grad += regularizer gradients; returns a PendingScalar with the loss (valid after sync).
    ``aux_roll``: the iteration's shift (x, y) -- the reference rolls the image, not the auxiliary
    image, so the un-rolled image meets the auxiliary image displaced by it."""
    _, H, W = img.shape
    mean = (ctypes.c_float * 3)(*[float(m) for m in np.ravel(mean_bgr)])
    out = engine.keep_until_sync(PendingScalar())
    lib.call('stx_image_regularizers', engine.handle, img.ptr, grad.ptr, H, W, mean,
             float(tv_scale), float(tv_power), float(p_scale), float(p_power),
             aux.ptr if aux is not None else None, float(aux_scale),
             _xy(aux_roll) if aux_roll is not None else None, ctypes.byref(out._v))
    return out


def swt_padded_side(h, w):
    """Side of the power-of-two square the SWT term pads an h x w image to (num_utils.py:186-188);
    the level count may not exceed its log2."""
    return 1 << max(0, (max(h, w) - 1).bit_length())


def swt_wavelet_order(wavelet):
    """Vanishing moments of an orthogonal Daubechies / symlet wavelet by its PyWavelets name: haar
    and db1 -> 1, dbN (1..38) and symN (2..20) -> N.  The SWT term depends on the filter through
    |H|^2 alone, which dbN and symN share.  Any other name raises NotImplementedError."""
    name = str(wavelet)
    if name == 'haar':
        return 1
    m = re.fullmatch(r'(db|sym)([1-9][0-9]?)', name)
    if m:
        order = int(m.group(2))
        if (1 if m.group(1) == 'db' else 2) <= order <= (38 if m.group(1) == 'db' else 20):
            return order
    raise NotImplementedError('SWT wavelet %r: only haar, db1..db38 and sym2..sym20 are '
                              'implemented' % (wavelet,))


def _swt(engine, img, grad, scale, power, order, levels, roll):
    """The SWT term through the entry point of its own form: the one-level Haar kernel, Haar at
    several levels, or the dbN / symN table (the library delegates the same way, bit for bit)."""
    _, H, W = img.shape
    out = engine.keep_until_sync(PendingScalar())
    if order == 1 and levels == 1:
        name, form = 'stx_image_swt_haar', ()
    elif order == 1:
        name, form = 'stx_image_swt_haar_levels', (int(levels),)
    else:
        name, form = 'stx_image_swt_daub_levels', (int(order), int(levels))
    lib.call(name, engine.handle, img.ptr, grad.ptr, H, W, *form,
             _xy(roll) if roll is not None else None, float(scale), float(power),
             ctypes.byref(out._v))
    return out


def swt_wavelet(engine, img, grad, scale, power, wavelet, levels=1, roll=None):
    """grad += scale * (p-norm gradient at the SWT detail image of the rolled picture / 127.5) for
    the wavelets of ``swt_wavelet_order`` (style_transfer.py:716-720; num_utils.py:184-196 passes
    any PyWavelets name on); returns a PendingScalar with scale * sum |detail|^power.  A level count
    outside 1 .. log2 of ``swt_padded_side`` raises ValueError, as PyWavelets would."""
    order = swt_wavelet_order(wavelet)
    _, H, W = img.shape
    levels = int(levels)
    if levels < 1 or 2 ** levels > swt_padded_side(H, W):
        raise ValueError('%d SWT levels: a %d x %d image is padded to a square of side %d, which '
                         'takes 1 to %d levels' % (levels, W, H, swt_padded_side(H, W),
                                                   swt_padded_side(H, W).bit_length() - 1))
    return _swt(engine, img, grad, scale, power, order, levels, roll)


def swt_haar(engine, img, grad, scale, power, roll=None, levels=1):
    """``swt_wavelet`` for the Haar wavelet (``levels`` is --swt-levels), except that a level count
    outside the range is left to the library to refuse (lib.StxError)."""
    return _swt(engine, img, grad, scale, power, 1, levels, roll)


# ---------------------------------------------------------------------- --lap-weight
def _pools(pools):
    return len(pools), (ctypes.c_int * len(pools))(*[int(p) for p in pools])


def lap_floats(h, w, pools):
    """Floats of the Laplacian term's target for an h x w picture: the cells of the pooled grids,
    sum over pools of ceil(h / p) * ceil(w / p) (0 when the library refuses the pool sizes)."""
    return int(lib.load().stx_image_lap_floats(int(h), int(w), *_pools(pools)))


def lap_target(engine, content, pools):
    """The Laplacian term's target for the content picture [3,H,W] on the engine's GPU: a
    DeviceArray holding, map after map, D P_p u(content) for every pool size p (include/stx.h has the
    definition).  ``pools``: one to four distinct powers of two in 1..64."""
    _, H, W = content.shape
    n = lap_floats(H, W, pools)
    target = engine.empty((max(n, 1),))
    try:
        lib.call('stx_image_lap_target', engine.handle, content.ptr, H, W, *_pools(pools), target.ptr)
    except lib.StxError:
        target.free()
        raise
    return target


def lap_loss(engine, img, grad, target, pools, weights, scale):
    """grad += the gradient of scale * sum_p weights[p] * sum |D P_p u(img) - T_p|^2 (the Laplacian
    loss; ``target`` is ``lap_target`` of the same size and pools); returns a PendingScalar with
    the loss (valid after sync)."""
    _, H, W = img.shape
    assert len(weights) == len(pools), (weights, pools)
    n = lap_floats(H, W, pools)         # 0: the library refuses the pools below, in its own words
    if n and target.size != n:
        raise ValueError('lap_loss: a target of %d floats, but a %d x %d picture with pools %s has %d cells'
                         % (target.size, H, W, list(pools), n))
    out = engine.keep_until_sync(PendingScalar())
    w = (ctypes.c_double * len(weights))(*[float(v) for v in weights])
    lib.call('stx_image_lap', engine.handle, img.ptr, grad.ptr, H, W, *_pools(pools), w, target.ptr,
             float(scale), ctypes.byref(out._v))
    return out


# ---------------------------------------------------------------------- --photo-weight
def photo_loss(engine, img, grad, content, eps, scale):
    """grad += the gradient of scale * sum_c v_c^T L v_c, the photorealism regulariser: L is the matting
    Laplacian of ``content`` / 255 over 3 x 3 windows with regularisation ``eps``, v_c a plane of ``img`` / 255
    (include/stx.h has the definition).  ``img``, ``grad``, ``content``: DeviceArrays [3,H,W] with H, W >= 3.
    Returns a PendingScalar with the loss (valid after sync)."""
    _, H, W = img.shape
    if content.shape != img.shape:
        raise ValueError('photo_loss: a content picture of %dx%d for an image of %dx%d'
                         % (content.shape[2], content.shape[1], W, H))
    out = engine.keep_until_sync(PendingScalar())
    lib.call('stx_image_photo', engine.handle, img.ptr, content.ptr, grad.ptr, H, W, float(eps), float(scale),
             ctypes.byref(out._v))
    return out


# ---------------------------------------------------------------------- --temporal-weight
def flow_warp(engine, prev, flow_b, flow_f, su, sv, first, target, weight):
    """Composites one earlier frame ``prev`` [3,H,W], warped by the backward flow ``flow_b`` [2,H,W], into
    ``target`` [3,H,W] / ``weight`` [H,W] wherever the flow is reliable and no closer frame has the pixel
    (include/stx.h has the definition).  ``flow_f``: the forward flow for the consistency test, or None; (su,
    sv): what scales the flows' components to pixels of this size; ``first``: the accumulators count as zero."""
    _, H, W = prev.shape
    for name, arr, shape in (('flow_b', flow_b, (2, H, W)), ('flow_f', flow_f, (2, H, W)),
                             ('target', target, (3, H, W)), ('weight', weight, (H, W))):
        if arr is not None and tuple(arr.shape) != shape:
            raise ValueError('flow_warp: %s of shape %s for a picture of %dx%d' % (name, tuple(arr.shape), W, H))
    lib.call('stx_image_flow_warp', engine.handle, prev.ptr, flow_b.ptr, flow_f.ptr if flow_f is not None else None,
             H, W, float(su), float(sv), int(bool(first)), target.ptr, weight.ptr)


def flow_params(params=None):
    """A lib.FlowParams from a dict of the estimator's parameters (alpha, gamma, eta, omega, eps, levels, outer,
    inner, sor); what is missing or None takes its default, an unknown name is a ValueError."""
    params = dict(params or {})
    unknown = sorted(set(params) - set(lib.FLOW_DEFAULTS))
    if unknown:
        raise ValueError('flow_estimate: unknown parameter(s) %s; there are %s'
                         % (', '.join(unknown), ', '.join(lib.FLOW_DEFAULTS)))
    values = {name: default if params.get(name) is None else params[name] for name, default in lib.FLOW_DEFAULTS.items()}
    return lib.FlowParams(*[(int if isinstance(lib.FLOW_DEFAULTS[name], int) else float)(values[name])
                            for name, _ in lib.FlowParams._fields_])


def flow_estimate(engine, i1, i2, params=None):
    """The optical flow [2,H,W] from the grey frame ``i1`` [H,W] into ``i2`` [H,W] (0 ... 255): the displacement w
    with i1(p) ~ i2(p + w(p)), which ``flow_warp`` takes as ``flow_b`` when ``i1`` is the current frame (include/stx.h
    has the definition).  ``params``: a dict of the estimator's parameters, see ``flow_params``.  Asynchronous; the
    result is a new DeviceArray."""
    if len(i1.shape) != 2 or tuple(i2.shape) != tuple(i1.shape):
        raise ValueError('flow_estimate: frames of shape %s and %s, but two [H, W] pictures of one size are needed'
                         % (tuple(i1.shape), tuple(i2.shape)))
    H, W = i1.shape
    c_params = flow_params(params)
    out = engine.empty((2, H, W))
    try:
        lib.call('stx_image_flow_estimate', engine.handle, i1.ptr, i2.ptr, H, W, ctypes.byref(c_params), out.ptr)
    except lib.StxError:
        out.free()
        raise
    return out


def poisson(engine, img, content, lam, cycles=None):
    """The screened-Poisson output stage: a new DeviceArray [3,H,W] with the colours of ``img`` and the gradients of
    ``content`` (both [3,H,W] on the engine's GPU, one frame), the minimiser of sum (f - img)^2 + ``lam`` sum over
    edges ((f_p - f_q) - (c_p - c_q))^2 per channel after ``cycles`` multigrid W-cycles (None: the default;
    include/stx.h has the definition).  Asynchronous; the sync that waits for it gives the workspace back."""
    from .config_system import POISSON_CYCLES_DEFAULT
    if len(img.shape) != 3 or img.shape[0] != 3 or tuple(content.shape) != tuple(img.shape):
        raise ValueError('poisson: pictures of shape %s and %s, but two [3, H, W] pictures of one size are needed'
                         % (tuple(img.shape), tuple(content.shape)))
    _, H, W = img.shape
    out = engine.empty((3, H, W))
    try:
        lib.call('stx_image_poisson', engine.handle, img.ptr, content.ptr, out.ptr, H, W, float(lam),
                 int(POISSON_CYCLES_DEFAULT if cycles is None else cycles))
    except lib.StxError:
        out.free()
        raise
    return out


def temporal_loss(engine, img, grad, target, weight, scale):
    """grad += the gradient of scale * 63.75 * sum w' ((img - target) / 127.5)^2 with w' = ``weight`` [H,W]
    clipped to [0, 1] (the temporal-consistency term; include/stx.h has the definition).  ``img``, ``grad``,
    ``target``: DeviceArrays [3,H,W].  Returns a PendingScalar with the loss (valid after sync)."""
    _, H, W = img.shape
    if tuple(target.shape) != tuple(img.shape) or tuple(weight.shape) != (H, W):
        raise ValueError('temporal_loss: a target of shape %s and a weight of shape %s for an image of %dx%d'
                         % (tuple(target.shape), tuple(weight.shape), W, H))
    out = engine.keep_until_sync(PendingScalar())
    lib.call('stx_image_temporal', engine.handle, img.ptr, grad.ptr, target.ptr, weight.ptr, H, W, float(scale),
             ctypes.byref(out._v))
    return out


def adam_step(engine, params, grad, g1, g2, p1, avg, lr, b1, b2, bp1, corr1, corr2, corrp):
    lib.call('stx_adam_step', engine.handle, params.ptr, grad.ptr, g1.ptr, g2.ptr, p1.ptr, avg.ptr,
             params.size, float(lr), float(b1), float(b2), float(bp1), float(corr1), float(corr2),
             float(corrp))


def dot(engine, x, y):
    out = ctypes.c_double(0)
    lib.call('stx_vec_dot', engine.handle, x.ptr, y.ptr, x.size, ctypes.byref(out))
    return out.value


def mean_abs(engine, x):
    out = ctypes.c_double(0)
    lib.call('stx_vec_mean_abs', engine.handle, x.ptr, x.size, ctypes.byref(out))
    return out.value


def axpy(engine, a, x, y):
    lib.call('stx_vec_axpy', engine.handle, float(a), x.ptr, y.ptr, x.size)


class DeviceScalars:
    """A few float64 slots on the engine's GPU for scalars that never need to visit the host."""

    def __init__(self, engine, n):
        self.engine, self.n = engine, n
        self.array = engine.empty((n,), np.float64)

    def ptr(self, i):
        assert 0 <= i < self.n
        return self.array.ptr + 8 * i

    def free(self):
        self.array.free()


def dot_async(engine, x, y, out_ptr):
    """*out_ptr (device double) = <x, y>; no synchronisation."""
    lib.call('stx_vec_dot_async', engine.handle, x.ptr, y.ptr, x.size, out_ptr)


def abs_sum_async(engine, x, out_ptr):
    lib.call('stx_vec_abs_sum_async', engine.handle, x.ptr, x.size, out_ptr)


def axpy_dev(engine, c1, a_ptr, da, x, y, c2=0.0, b_ptr=None, db=1.0):
    """y += float(*a / da * c1 [+ *b / db * c2]) * x with a, b device doubles."""
    lib.call('stx_vec_axpy_dev', engine.handle, float(c1), a_ptr, float(da), float(c2), b_ptr,
             float(db), x.ptr, y.ptr, x.size)


def scale_dev(engine, c, den_ptr, x, den_div=1.0):
    """x *= float(c / (*den / den_div)) with den a device double."""
    lib.call('stx_vec_scale_dev', engine.handle, float(c), den_ptr, float(den_div), x.ptr, x.size)


def axpy_dot_dev(engine, c1, a_ptr, da, x, y, z, out_ptr, c2=0.0, b_ptr=None, db=1.0, src=None,
                 scale_c=0.0, scale_den_ptr=None, scale_div=1.0):
    """y = coef * x + src (coef as axpy_dev; src defaults to y), then -- with scale_den_ptr -- y *=
    float(scale_c / (*scale_den / scale_div)); *out_ptr = <z, y>: the axpy of one iteration of the
    two-loop recursion (and the scaling between the loops) with the dot product of the next, one pass."""
    lib.call('stx_vec_axpy_dot_dev', engine.handle, float(c1), a_ptr, float(da), float(c2), b_ptr,
             float(db), float(scale_c), scale_den_ptr, float(scale_div), x.ptr,
             (y if src is None else src).ptr, y.ptr, z.ptr, x.size, out_ptr)


def lbfgs_pair(engine, g_new, g_old, s, y, out_ptr2):
    """y = g_new - g_old, g_old = g_new, out_ptr2[0] = <s, y>, out_ptr2[1] = <y, y>; returns <s, y>
    (one host synchronisation)."""
    sy = ctypes.c_double()
    lib.call('stx_vec_lbfgs_pair', engine.handle, g_new.ptr, g_old.ptr, s.ptr, y.ptr, s.size, out_ptr2,
             ctypes.byref(sy))
    return sy.value


def scale2_axpy(engine, c1, c2, s, params):
    """s = c2 * (c1 * s); params += s."""
    lib.call('stx_vec_scale2_axpy', engine.handle, float(c1), float(c2), s.ptr, params.ptr, s.size)


def scale(engine, a, x):
    lib.call('stx_vec_scale', engine.handle, float(a), x.ptr, x.size)


def step_stats(engine, avg, old):
    """(mean|avg-old|, sqrt(mean(xdiff^2+ydiff^2))); old <- avg."""
    _, H, W = avg.shape
    out = (ctypes.c_double * 2)()
    lib.call('stx_image_step_stats', engine.handle, avg.ptr, old.ptr, H, W, out)
    return out[0], out[1]


class PendingStats:
    """step_stats whose two sums are still on their way: ``values()`` after the engine's pending
    values were published (sync, or wait_fence on a later fence)."""

    def __init__(self, n):
        self._raw = (ctypes.c_double * 2)(float('nan'), float('nan'))
        self._n = n

    def values(self):
        return self._raw[0] / self._n, float(np.sqrt(self._raw[1] / self._n))


def step_stats_async(engine, avg, old):
    """step_stats without the host wait (stx_image_step_stats_async); old <- avg in stream order."""
    _, H, W = avg.shape
    out = engine.keep_until_sync(PendingStats(3.0 * H * W))
    lib.call('stx_image_step_stats_async', engine.handle, avg.ptr, old.ptr, H, W, out._raw)
    return out


def to_u8(engine, img, mean_bgr):
    """RGB HWC uint8 ndarray of img + mean, clipped and truncated like the reference."""
    _, H, W = img.shape
    mean = (ctypes.c_float * 3)(*[float(m) for m in np.ravel(mean_bgr)])
    out = engine.empty((H, W, 3), np.uint8)
    lib.call('stx_image_to_u8', engine.handle, img.ptr, H, W, mean, out.ptr)
    host = out.get()
    out.free()
    return host


# ---------------------------------------------------------------------- --preserve-color
def _mean3(mean_bgr):
    return (ctypes.c_float * 3)(*[float(m) for m in np.ravel(mean_bgr)])


def to_u8_luma(engine, img, content, mean_bgr):
    """RGB HWC uint8 ndarray with the luminance of ``img`` and the chroma of ``content`` (both
    [3,H,W] on the engine's GPU): clip(c + (Y(x) - Y(c)), 0, 255) truncated, where x and c are the
    two pictures with the mean added and clipped and Y is the Rec. 601 luma."""
    _, H, W = img.shape
    assert content.shape == img.shape, (content.shape, img.shape)
    out = engine.empty((H, W, 3), np.uint8)
    lib.call('stx_image_to_u8_luma', engine.handle, img.ptr, content.ptr, H, W, _mean3(mean_bgr),
             out.ptr)
    host = out.get()
    out.free()
    return host


def color_stats(engine, img):
    """(mean[3], cov[3,3]) in float64 of the stored BGR values of a device picture [3,H,W], from the
    nine sums of stx_image_color_stats (the covariance is the population one)."""
    _, H, W = img.shape
    raw = (ctypes.c_double * 9)()
    lib.call('stx_image_color_stats', engine.handle, img.ptr, H, W, raw)
    n = float(H) * W
    mean = np.array(raw[:3], np.float64) / n
    second = np.empty((3, 3), np.float64)
    for k, (i, j) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        second[i, j] = second[j, i] = raw[3 + k] / n
    return mean, second - np.outer(mean, mean)


def color_affine(engine, src, dst, A, b, mean_bgr):
    """dst = clip(A src + b + mean, 0, 255) - mean per pixel (A [3,3], b [3] over the BGR channels,
    used as float32); ``dst`` may be ``src``."""
    _, H, W = src.shape
    assert dst.shape == src.shape, (dst.shape, src.shape)
    A = np.ascontiguousarray(A, np.float64).reshape(9)
    b = np.ascontiguousarray(b, np.float64).reshape(3)
    lib.call('stx_image_color_affine', engine.handle, src.ptr, dst.ptr, H, W,
             A.ctypes.data_as(lib.c_double_p), b.ctypes.data_as(lib.c_double_p), _mean3(mean_bgr))
    return dst


def _sym_power(cov, power):
    """cov^power of a symmetric positive semi-definite matrix; eigenvalues are floored at 1e-8 of
    the trace, so that a flat-colour picture does not divide by zero."""
    w, v = np.linalg.eigh(np.asarray(cov, np.float64))
    trace = float(np.trace(cov))
    w = np.maximum(w, 1e-8 * trace if trace > 0 else 1.0)
    return (v * w ** power) @ v.T


def color_match_transform(stats_style, stats_content):
    """(A, b) of the affine colour map that gives a picture with statistics ``stats_style`` =
    (mean, cov) those of ``stats_content``: A = cov_c^(1/2) cov_s^(-1/2), b = mean_c - A mean_s
    (symmetric square roots, float64)."""
    mean_s, cov_s = stats_style
    mean_c, cov_c = stats_content
    A = _sym_power(cov_c, 0.5) @ _sym_power(cov_s, -0.5)
    return A, np.asarray(mean_c, np.float64) - A @ np.asarray(mean_s, np.float64)
