"""The Laplacian loss in float64 numpy, as include/stx.h states it: the reference of the tests.

    u(x)  = (x_B + x_G + x_R) / 382.5
    P_p u = block means over p x p blocks from the origin, edge blocks over the pixels that exist
    D v   = sum over the 4-neighbours inside the grid of (v - v_n)
    T_p   = D P_p u(content),  e_p = D P_p u(img) - T_p
    loss  = scale * sum_p w_p * sum e_p^2
    grad  = scale * sum_p w_p * 2 (D e_p)[y // p][x // p] / (n_cell * 382.5), the same on all channels
"""

import numpy as np

UNIT = 382.5


def cell_counts(h, w, p):
    """[hp, wp] pixels that exist in every cell."""
    rows = np.minimum(p, h - np.arange(0, h, p))
    cols = np.minimum(p, w - np.arange(0, w, p))
    return np.outer(rows, cols).astype(np.float64)


def pool(plane, p):
    """Block means of an [H, W] plane (np.add.reduceat over both axes)."""
    h, w = plane.shape
    sums = np.add.reduceat(np.add.reduceat(np.asarray(plane, np.float64), np.arange(0, h, p), axis=0),
                           np.arange(0, w, p), axis=1)
    return sums / cell_counts(h, w, p)


def lap(v):
    """D v: the graph Laplacian of the grid ([0 -1 0; -1 4 -1; 0 -1 0], border replicated)."""
    padded = np.pad(np.asarray(v, np.float64), 1, mode='edge')
    v = padded[1:-1, 1:-1]
    return (v - padded[:-2, 1:-1]) + (v - padded[2:, 1:-1]) + (v - padded[1:-1, :-2]) + (v - padded[1:-1, 2:])


def abs_lap(v):
    """|D| v: the matrix of absolute values of D's entries, for error budgets."""
    h, w = v.shape
    degree = np.full((h, w), 4.0)
    degree[0] -= 1
    degree[-1] -= 1
    degree[:, 0] -= 1
    degree[:, -1] -= 1
    padded = np.pad(np.asarray(v, np.float64), 1, mode='constant')
    return (degree * v + padded[:-2, 1:-1] + padded[2:, 1:-1] + padded[1:-1, :-2] + padded[1:-1, 2:])


def channel_sum(img):
    return np.asarray(img, np.float64).sum(axis=0) / UNIT


def target(content, pools):
    """[T_p for p in pools], each [hp, wp]."""
    u = channel_sum(content)
    return [lap(pool(u, p)) for p in pools]


def spread(cells, h, w, p):
    """The cell values at every pixel of the h x w picture."""
    return np.repeat(np.repeat(cells, p, axis=0), p, axis=1)[:h, :w]


def lap_loss(img, content, pools, weights, scale=1.0):
    """(loss, grad [3, H, W], [T_p]) in float64."""
    _, h, w = np.shape(img)
    u = channel_sum(img)
    targets = target(content, pools)
    loss, g = 0.0, np.zeros((h, w))
    for p, wp, t in zip(pools, weights, targets):
        e = lap(pool(u, p)) - t
        loss += scale * wp * float(np.sum(e * e))
        g += spread(scale * wp * 2 * lap(e) / (cell_counts(h, w, p) * UNIT), h, w, p)
    return loss, np.broadcast_to(g, (3, h, w)).copy(), targets


def flat(maps):
    return np.concatenate([np.ravel(m) for m in maps])
