"""The temporal-consistency term (Ruder, Dosovitskiy, Brox, "Artistic Style Transfer for Videos", 2016) in
float64 numpy: the statement that include/stx.h makes of stx_image_flow_warp and stx_image_temporal, the
composite over several earlier frames, the per-scale preparation of terms.TemporalTerm, and the analytic flows
the GPU tests use.  There is no reference implementation of this term.

Every operation is written in the order the header gives, so that a device that rounds each float64 operation
once takes the same decisions; ``warp`` also says where a decision is too close to call (``unclear``)."""

import numpy as np
from PIL import Image

from style_transfer_amd.resample import resample_host

UNKNOWN = np.float32(1e10)
CLOSE = 1e-9


def known(flow):
    """[H, W] bool: both components finite and at most 1e9 in magnitude (as float32, before any scaling)."""
    flow = np.asarray(flow, np.float32)
    with np.errstate(invalid='ignore'):
        return (np.abs(flow[0]) <= np.float32(1e9)) & (np.abs(flow[1]) <= np.float32(1e9))


def _mix(p, y0, x0, fx, fy):
    top = p[y0, x0] + fx * (p[y0, x0 + 1] - p[y0, x0])
    bottom = p[y0 + 1, x0] + fx * (p[y0 + 1, x0 + 1] - p[y0 + 1, x0])
    return top + fy * (bottom - top)


def warp(prev, flow_b, flow_f, su=1.0, sv=1.0):
    """One earlier frame against one flow pair: dict of ``value`` [3,H,W] float64 (the bilinear samples, 0 where
    the pixel is unknown or outside), ``c`` [H,W] bool (reliable), ``unclear`` [H,W] bool (a threshold's two sides
    differ by at most 1e-9 (1 + right side), or q is within 1e-9 of the frame's edge), ``tapmax`` [3,H,W] (max
    |tap| of the sample) and the separate tests ``known``, ``inside``, ``consistent``, ``boundary``."""
    prev = np.float64(prev)
    _, H, W = prev.shape
    ok = known(flow_b)
    fb = np.where(ok[None], np.float64(np.asarray(flow_b, np.float32)), 0.0)
    u, v = su * fb[0], sv * fb[1]
    y, x = np.mgrid[:H, :W]
    qx, qy = x + u, y + v
    inside = (qx >= 0) & (qx <= W - 1) & (qy >= 0) & (qy <= H - 1)
    near = ((np.abs(qx) <= CLOSE) | (np.abs(qx - (W - 1)) <= CLOSE) | (np.abs(qy) <= CLOSE) |
            (np.abs(qy - (H - 1)) <= CLOSE))
    live = ok & inside
    qxs, qys = np.where(live, qx, 0.0), np.where(live, qy, 0.0)
    x0 = np.minimum(np.floor(qxs), W - 2).astype(np.int64)
    y0 = np.minimum(np.floor(qys), H - 2).astype(np.int64)
    fx, fy = qxs - x0, qys - y0
    value = np.stack([_mix(prev[c], y0, x0, fx, fy) for c in range(3)]) * live[None]
    taps = np.stack([np.abs(prev[:, y0 + dy, x0 + dx]) for dy in (0, 1) for dx in (0, 1)])
    # ---- forward-backward consistency
    consistent = np.ones((H, W), bool)
    if flow_f is not None:
        okf = known(flow_f)
        ff = np.where(okf[None], np.float64(np.asarray(flow_f, np.float32)), 0.0)
        taps_known = okf[y0, x0] & okf[y0, x0 + 1] & okf[y0 + 1, x0] & okf[y0 + 1, x0 + 1]
        fu, fv = su * _mix(ff[0], y0, x0, fx, fy), sv * _mix(ff[1], y0, x0, fx, fy)
        du, dv = u + fu, v + fv
        left = du * du + dv * dv
        right = 0.01 * (((u * u + v * v) + fu * fu) + fv * fv) + 0.5
        consistent = taps_known & (left <= right)
        near |= taps_known & (np.abs(left - right) <= CLOSE * (1 + right))
    # ---- motion boundaries: central differences over a replicated border
    xm, xp = np.maximum(x - 1, 0), np.minimum(x + 1, W - 1)
    ym, yp = np.maximum(y - 1, 0), np.minimum(y + 1, H - 1)
    ux, uy = (u[y, xp] - u[y, xm]) / 2.0, (u[yp, x] - u[ym, x]) / 2.0
    vx, vy = (v[y, xp] - v[y, xm]) / 2.0, (v[yp, x] - v[ym, x]) / 2.0
    left = ((ux * ux + uy * uy) + vx * vx) + vy * vy
    right = 0.01 * (u * u + v * v) + 0.002
    around = ok[y, xp] & ok[y, xm] & ok[yp, x] & ok[ym, x]
    boundary = ~around | (left > right)
    near |= around & (np.abs(left - right) <= CLOSE * (1 + right))
    c = ok & inside & consistent & ~boundary
    return dict(value=value, c=c, unclear=ok & near, tapmax=taps.max(axis=0) * live[None], known=ok, inside=inside,
                consistent=consistent, boundary=boundary)


def composite(frames, su=1.0, sv=1.0, start=None):
    """The composite of ``frames`` = [(prev, flow_b, flow_f or None), ...], closest first: (target [3,H,W] float64,
    weight [H,W] float64, unclear [H,W] bool, tapmax [3,H,W] of the frame that won each pixel).  ``start``:
    (target, weight) accumulators to go on from (no frame counts as the first)."""
    _, H, W = np.shape(frames[0][0])
    if start is None:
        target, weight = np.zeros((3, H, W)), np.zeros((H, W))
    else:
        target, weight = np.float64(start[0]).copy(), np.float64(start[1]).copy()
    unclear, tapmax = np.zeros((H, W), bool), np.zeros((3, H, W))
    for prev, flow_b, flow_f in frames:
        one = warp(prev, flow_b, flow_f, su, sv)
        take = (weight == 0) & one['c']
        # (a pixel that an unclear decision of a closer frame may have settled is unclear for the later ones)
        unclear |= one['unclear'] & ((weight == 0) | unclear)
        target = np.where(take[None], np.float64(np.float32(one['value'])), target)
        tapmax = np.where(take[None], one['tapmax'], tapmax)
        weight = np.where(take, 1.0, weight)
    return target, weight, unclear, tapmax


def clip_weight(weight):
    w = np.float64(weight)
    return np.where(np.isnan(w), 0.0, np.clip(w, 0.0, 1.0))


def temporal_loss(img, target, weight, scale=1.0):
    """(loss, gradient [3,H,W]) in float64: loss = scale * 63.75 * sum w' d^2 with d = (img - target) / 127.5 and
    w' the weight clipped to [0, 1] (NaN as 0); gradient = scale * w' * d.  Pixels with w' = 0 do not count,
    whatever they hold."""
    w = clip_weight(weight)[None]
    d = np.where(w > 0, (np.float64(img) - np.float64(target)) / 127.5, 0.0)
    return scale * 63.75 * float((w * d * d).sum()), scale * w * d


def prepare_scale(pictures, flows_b, flows_f, hw, to_image):
    """What TemporalTerm makes for a scale of h x w: every earlier PIL picture Lanczos-resized and converted with
    ``to_image`` (StyleTransfer.pil_to_image), every flow [2,H0,W0] resampled with resample.py's tables, the
    components scaled by (w / W0, h / H0).  Returns ``composite``'s tuple."""
    h, w = hw
    _, H0, W0 = np.shape(flows_b[0])
    flows_f = flows_f or [None] * len(flows_b)
    with np.errstate(all='ignore'):
        frames = [(to_image(picture.resize((w, h), Image.LANCZOS)), resample_host(fb, (h, w)),
                   resample_host(ff, (h, w)) if ff is not None else None)
                  for picture, fb, ff in zip(pictures, flows_b, flows_f)]
    return composite(frames, w / W0, h / H0)


# ------------------------------------------------------------------------------------- analytic flows
def affine_flows(hw, shift=(2.3, -1.7), angle=0.03, zoom=1.02, boxes=True):
    """(backward, forward) float32 flows [2,H,W].  The backward flow is the displacement under p -> c + zoom R (p -
    c) + shift about the picture's centre c; the forward flow the displacement under the exact inverse map, so the
    pair is consistent.  With ``boxes`` a box of the backward flow gets an extra step of (2.5, -1.5), which makes
    motion boundaries around it, and a second box of the forward flow gets +3 px, which fails the consistency
    test."""
    H, W = hw
    y, x = np.mgrid[:H, :W].astype(np.float64)
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    co, si = np.cos(angle), np.sin(angle)
    dx, dy = x - cx, y - cy
    back = np.stack([cx + zoom * (co * dx - si * dy) + shift[0] - x, cy + zoom * (si * dx + co * dy) + shift[1] - y])
    ex, ey = dx - shift[0], dy - shift[1]
    fwd = np.stack([cx + (co * ex + si * ey) / zoom - x, cy + (-si * ex + co * ey) / zoom - y])
    if boxes:
        back[0, H // 5:H // 5 + H // 4, W // 6:W // 6 + W // 4] += 2.5
        back[1, H // 5:H // 5 + H // 4, W // 6:W // 6 + W // 4] -= 1.5
        fwd[0, H // 2:H // 2 + H // 4, W // 2:W // 2 + W // 3] += 3.0
    return np.float32(back), np.float32(fwd)


def noise_picture(hw, seed):
    return np.random.RandomState(seed).uniform(-120, 130, (3,) + tuple(hw)).astype(np.float32)
