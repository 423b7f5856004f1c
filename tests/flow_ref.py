"""The optical-flow estimator (Brox, Bruhn, Papenberg, Weickert, ECCV 2004, in the discretisation of Sanchez,
Monzon, Salgado, IPOL 2013) in float64 numpy: the statement that include/stx.h makes of stx_image_flow_estimate,
operation for operation, and the analytic scenes its tests use.  There is no reference implementation of this
estimator.

Every sum is written in the order the header gives and nothing goes through a library routine whose summation
order is its own, so that a device that rounds each float64 operation once computes the same values.  The Gaussian
weights go through ``math.exp`` -- the C library's exp, which the host side of the library calls too."""

import math

import numpy as np

DEFAULTS = dict(alpha=18.0, gamma=6.0, eta=0.75, omega=1.8, eps=0.001, levels=None, outer=5, inner=1, sor=10)
MIN_SIDE = 16


# ----------------------------------------------------------------------------------------- the pyramid
def pyramid_sizes(H, W, eta=0.75, levels=None):
    """[(h, w)] from level 0 (the input) up: h' = floor(h eta + 0.5); a level is added while min(h, w) >= 16, up to
    ``levels`` (None: as many as fit)."""
    sizes = [(int(H), int(W))]
    while levels is None or len(sizes) < levels:
        h, w = (int(math.floor(n * eta + 0.5)) for n in sizes[-1])
        if min(h, w) < MIN_SIDE:
            break
        sizes.append((h, w))
    return sizes


def gauss_weights(eta):
    """The 2 r + 1 normalised weights of the Gaussian before a step down: sigma = 0.6 sqrt(eta^-2 - 1), r =
    ceil(3 sigma)."""
    sigma = 0.6 * math.sqrt(1.0 / (eta * eta) - 1.0)
    r = int(math.ceil(3.0 * sigma))
    raw = [math.exp(-float(i * i) / (2.0 * sigma * sigma)) for i in range(-r, r + 1)]
    total = 0.0
    for value in raw:
        total = total + value
    return [value / total for value in raw]


def smooth(img, weights):
    """Rows first, then columns; replicated border; the taps are added from -r to r."""
    H, W = img.shape
    r = len(weights) // 2
    x, y = np.arange(W), np.arange(H)
    rows = np.zeros((H, W))
    for i in range(-r, r + 1):
        rows = rows + weights[i + r] * img[:, np.clip(x + i, 0, W - 1)]
    out = np.zeros((H, W))
    for i in range(-r, r + 1):
        out = out + weights[i + r] * rows[np.clip(y + i, 0, H - 1)]
    return out


def mix(p, y0, x0, fx, fy):
    """The bilinear mix, exact at fx, fy in {0, 1}."""
    top = (1.0 - fx) * p[y0, x0] + fx * p[y0, x0 + 1]
    bottom = (1.0 - fx) * p[y0 + 1, x0] + fx * p[y0 + 1, x0 + 1]
    return (1.0 - fy) * top + fy * bottom


def taps(qx, qy, H, W):
    """Clamped coordinates -> (y0, x0, fx, fy), the taps of stx_image_flow_warp: x0 = min(floor(qx), W - 2)."""
    qx, qy = np.minimum(np.maximum(qx, 0.0), float(W - 1)), np.minimum(np.maximum(qy, 0.0), float(H - 1))
    x0 = np.minimum(np.floor(qx), W - 2).astype(np.int64)
    y0 = np.minimum(np.floor(qy), H - 2).astype(np.int64)
    return y0, x0, qx - x0, qy - y0


def resample(src, hw):
    """``src`` [H, W] sampled bilinearly on an h x w grid at ((x + 0.5) W / w - 0.5, (y + 0.5) H / h - 0.5)."""
    H, W = src.shape
    h, w = hw
    sx, sy = float(W) / float(w), float(H) / float(h)
    y, x = np.mgrid[:h, :w].astype(np.float64)
    y0, x0, fx, fy = taps((x + 0.5) * sx - 0.5, (y + 0.5) * sy - 0.5, H, W)
    return mix(src, y0, x0, fx, fy)


def ddx(p):
    W = p.shape[1]
    x = np.arange(W)
    return (p[:, np.minimum(x + 1, W - 1)] - p[:, np.maximum(x - 1, 0)]) / 2.0


def ddy(p):
    H = p.shape[0]
    y = np.arange(H)
    return (p[np.minimum(y + 1, H - 1)] - p[np.maximum(y - 1, 0)]) / 2.0


# ------------------------------------------------------------------------------------------- one level
def _neighbours(p):
    """(left, right, up, down) with clamped indices (a neighbour outside the picture has weight 0)."""
    H, W = p.shape
    x, y = np.arange(W), np.arange(H)
    return p[:, np.maximum(x - 1, 0)], p[:, np.minimum(x + 1, W - 1)], p[np.maximum(y - 1, 0)], p[np.minimum(y + 1, H - 1)]


def level_solve(A, B, u, v, p):
    """``outer`` warps at one level, from (u, v); returns the new (u, v)."""
    H, W = A.shape
    alpha, gamma, omega = p['alpha'], p['gamma'], p['omega']
    eps2, om1 = p['eps'] * p['eps'], 1.0 - p['omega']
    yy, xx = np.mgrid[:H, :W]
    colours = [((xx + yy) & 1) == 0, ((xx + yy) & 1) == 1]
    inside = [xx > 0, xx < W - 1, yy > 0, yy < H - 1]
    Ax, Ay, Bx, By = ddx(A), ddy(A), ddx(B), ddy(B)
    Bxx, Bxy, Byy = ddx(Bx), ddy(Bx), ddy(By)
    for _ in range(p['outer']):
        y0, x0, fx, fy = taps(xx + u, yy + v, H, W)
        Iz = mix(B, y0, x0, fx, fy) - A
        Ix, Iy = mix(Bx, y0, x0, fx, fy), mix(By, y0, x0, fx, fy)
        Ixz, Iyz = Ix - Ax, Iy - Ay
        Ixx, Ixy, Iyy = mix(Bxx, y0, x0, fx, fy), mix(Bxy, y0, x0, fx, fy), mix(Byy, y0, x0, fx, fy)
        du, dv = np.zeros((H, W)), np.zeros((H, W))
        Su, Sv = u + du, v + dv
        for _ in range(p['inner']):
            b = (Iz + Ix * du) + Iy * dv
            gx = (Ixz + Ixx * du) + Ixy * dv
            gy = (Iyz + Ixy * du) + Iyy * dv
            psi_d = 0.5 / np.sqrt((b * b + gamma * (gx * gx + gy * gy)) + eps2)
            ux, uy, vx, vy = ddx(Su), ddy(Su), ddx(Sv), ddy(Sv)
            psi_s = 0.5 / np.sqrt((((ux * ux + uy * uy) + vx * vx) + vy * vy) + eps2)
            g = [np.where(ok, (alpha * (psi_s + n)) / 2.0, 0.0) for ok, n in zip(inside, _neighbours(psi_s))]
            gs = ((g[0] + g[1]) + g[2]) + g[3]
            A11 = psi_d * (Ix * Ix + gamma * (Ixx * Ixx + Ixy * Ixy))
            A12 = psi_d * (Ix * Iy + gamma * (Ixx * Ixy + Ixy * Iyy))
            A22 = psi_d * (Iy * Iy + gamma * (Ixy * Ixy + Iyy * Iyy))
            c1 = psi_d * (Ix * Iz + gamma * (Ixx * Ixz + Ixy * Iyz))
            c2 = psi_d * (Iy * Iz + gamma * (Ixy * Ixz + Iyy * Iyz))
            for _ in range(p['sor']):
                for colour in colours:
                    n = _neighbours(Su)
                    s = ((g[0] * n[0] + g[1] * n[1]) + g[2] * n[2]) + g[3] * n[3]
                    new_du = om1 * du + omega * ((((s - gs * u) - A12 * dv) - c1) / (A11 + gs))
                    n = _neighbours(Sv)
                    s = ((g[0] * n[0] + g[1] * n[1]) + g[2] * n[2]) + g[3] * n[3]
                    new_dv = om1 * dv + omega * ((((s - gs * v) - A12 * new_du) - c2) / (A22 + gs))
                    du, dv = np.where(colour, new_du, du), np.where(colour, new_dv, dv)
                    Su, Sv = np.where(colour, u + du, Su), np.where(colour, v + dv, Sv)
        u, v = u + du, v + dv
    return u, v


def estimate(I1, I2, **params):
    """The flow w [2, H, W] float32 with I1(p) ~ I2(p + w(p)); ``I1``, ``I2`` [H, W] (rounded to float32 first)."""
    p = dict(DEFAULTS, **{k: val for k, val in params.items() if val is not None})
    A, B = np.float64(np.float32(I1)), np.float64(np.float32(I2))
    sizes = pyramid_sizes(*A.shape, eta=p['eta'], levels=p['levels'])
    weights = gauss_weights(p['eta'])
    pyramid = [(A, B)]
    for hw in sizes[1:]:
        pyramid.append(tuple(resample(smooth(img, weights), hw) for img in pyramid[-1]))
    u = v = None
    for k in range(len(sizes) - 1, -1, -1):
        h, w = sizes[k]
        if u is None:
            u, v = np.zeros((h, w)), np.zeros((h, w))
        else:
            ch, cw = sizes[k + 1]
            u, v = resample(u, (h, w)) * (float(w) / float(cw)), resample(v, (h, w)) * (float(h) / float(ch))
        u, v = level_solve(pyramid[k][0], pyramid[k][1], u, v, p)
    return np.float32(np.stack([u, v]))


# ------------------------------------------------------------------------------------ analytic scenes
def texture(x, y, seed=0):
    """A smooth texture as a formula: 60 sinusoids with frequencies up to 0.12 cycles per pixel around 127.5,
    clipped to 0...255 (clipping commutes with warping).  ``x``, ``y``: real coordinates of any shape."""
    x, y = np.float64(x), np.float64(y)
    total = np.zeros(np.broadcast(x, y).shape)
    for k in range(60):
        radius = 0.12 * math.sqrt((k + 0.5) / 60.0)                 # (frequencies fill the disc evenly)
        angle = 2.399963229728653 * k + 0.7 * seed                  # (the golden angle)
        phase = 1.0 + 2.1 * k + 1.3 * seed * (k % 7)
        total = total + np.cos(2.0 * math.pi * (radius * math.cos(angle) * x + radius * math.sin(angle) * y) + phase)
    return np.clip(127.5 + 6.0 * total, 0.0, 255.0)


def affine_scene(hw):
    """(I1, I2, backward, forward): I1 the texture, I2 its exact warp under temporal_ref.affine_flows' map
    (boxes=False), so that I1(p) = I2(p + backward(p)) and I2(q) = I1(q + forward(q)) wherever the clip is idle."""
    from tests import temporal_ref
    H, W = hw
    back, fwd = temporal_ref.affine_flows(hw, boxes=False)
    y, x = np.mgrid[:H, :W].astype(np.float64)
    return (np.float32(texture(x, y)), np.float32(texture(x + np.float64(fwd[0]), y + np.float64(fwd[1]))),
            back, fwd)


BOX_ROWS, BOX_COLS, BOX_STEP = (30, 66), (40, 80), 6


def box_scene(hw=(96, 128)):
    """(earlier, current, disoccluded, box): a textured box that moves BOX_STEP px to the right over a static
    textured background.  ``disoccluded`` [H, W] bool: the pixels of the current frame that the box hid in the
    earlier one (a strip of BOX_STEP columns); ``box``: where the box is in the current frame."""
    H, W = hw
    y, x = np.mgrid[:H, :W].astype(np.float64)
    ground = texture(x, y)
    rows = (y >= BOX_ROWS[0]) & (y < BOX_ROWS[1])
    was = rows & (x >= BOX_COLS[0]) & (x < BOX_COLS[1])
    now = rows & (x >= BOX_COLS[0] + BOX_STEP) & (x < BOX_COLS[1] + BOX_STEP)
    earlier = np.where(was, texture(x + 300.0, y + 200.0, seed=1), ground)
    current = np.where(now, texture(x + 300.0 - BOX_STEP, y + 200.0, seed=1), ground)
    return np.float32(earlier), np.float32(current), was & ~now, now
