"""Reference arithmetic of the self-similarity content term (--selfsim-weight, stx_set_selfsim_targets) for the
tests, in float64 on the same float32 inputs.  For a blob F [C, h, w] and the tile's window c [C, h, w] of the layer's
content map, sampled at the grid (a g, b g) -- g the smallest integer >= 1 with ceil(h/g) ceil(w/g) <= points, N
positions in raster order, columns f_i and c_i:

    r_i   = |f_i|,  x_i = f_i / r_i   (r_i = 0: x_i = 0, 1/r_i = 0);   y_i likewise from c_i
    DX_ij = 1 - x_i . x_j  (i != j),  DX_ii = 0;                        DC likewise from y
    sX_j  = sum_i DX_ij + N 1e-6;                                       sC likewise
    PX    = DX / sX (columns),  PC = DC / sC
    d     = PX - PC,  T = sign d,  E = sum |d| / N
    u_j   = sum_k T_kj PX_kj,  A_ij = (T_ij - u_j) / sX_j  (i != j),  A_ii = 0
    q_i   = - sum_j (A_ij + A_ji) x_j
    S_i   = (q_i - (q_i . x_i) x_i) / (2 r_i)  at the grid positions, 0 elsewhere       ( = N d(E/2)/d f_i, T held )
    loss += lw w E / 2
    diff += lw w S / (sum|S| / (C h w) + EPS)

``terms`` forms every quantity under its own signs or under signs handed in (the device's T, as swd_ref.terms takes
ranks); ``terms32`` is the same code in float32 -- numpy's order of summation -- and is the yardstick of the
tolerances: a float32 kernel is held to 4 x its error, the factor for the other order a device adds in.
``SelfsimOracleModel`` is the oracle's tile evaluation with the term added: computed in float64 from the oracle's
blobs and pushed back through the oracle's own backward pass.

The op cases of tests/test_gpu_selfsim.py and their inputs are made here, so that tests/test_selfsim_host.py can hold
the same inputs to the undecided-pairs condition on the CPU."""

import numpy as np

from oracle.num_ops import EPS, gram_lower, half_sq_norm, l1_normalize, symm_lower_times
from oracle.tile_path import OracleModel
from style_transfer_amd.config_system import selfsim_grid

# (C, h, w, points): N = 35, ragged in the 32-wide MFMA tile; g = 2, a 5 x 6 grid whose last row and column sit on the
# blob's edge; N = 130, which crosses a 128 block by two, two K steps; several blocks both ways; g = 2, N = 289; N = 2;
# N = 1
OP_SHAPES = [(64, 5, 7, 1024), (64, 9, 11, 30), (128, 13, 10, 4096), (256, 24, 24, 576), (64, 33, 33, 1024),
             (64, 1, 2, 2), (64, 1, 1, 2)]
EPS_COLUMN = 1e-6


def grid(h, w, points):
    """(g, N, positions [N, 2] as (y, x) in raster order)."""
    g, gh, gw = selfsim_grid(h, w, points)
    ys, xs = np.meshgrid(np.arange(gh) * g, np.arange(gw) * g, indexing='ij')
    return g, gh * gw, np.stack([ys.ravel(), xs.ravel()], axis=1)


def _unit(v):
    r = np.sqrt((v * v).sum(axis=1))
    inv = np.where(r > 0, 1 / np.where(r > 0, r, 1), 0).astype(v.dtype)
    return v * inv[:, None], inv


def _distances(x):
    D = 1 - x @ x.T
    np.fill_diagonal(D, 0)
    s = D.sum(axis=0) + x.dtype.type(len(x)) * x.dtype.type(EPS_COLUMN)
    return D, s


def _terms(F, c, points, signs, dtype):
    C, h, w = np.shape(F)
    g, N, _ = grid(h, w, points)
    x, inv = _unit(np.asarray(F, dtype)[:, ::g, ::g].reshape(C, N).T)
    y, _ = _unit(np.asarray(c, dtype)[:, ::g, ::g].reshape(C, N).T)
    (DX, sX), (DC, sC) = _distances(x), _distances(y)
    PX, PC = DX / sX[None, :], DC / sC[None, :]
    d = PX - PC
    T = np.sign(d) if signs is None else np.asarray(signs, dtype).reshape(N, N)
    E = np.abs(d).sum() / dtype(N)
    u = (T * PX).sum(axis=0)
    A = (T - u[None, :]) / sX[None, :]
    np.fill_diagonal(A, 0)
    q = -(A + A.T) @ x
    S_n = (q - (q * x).sum(axis=1)[:, None] * x) * (dtype(0.5) * inv)[:, None]
    S = np.zeros((C, h, w), dtype)
    S[:, ::g, ::g] = S_n.T.reshape(C, *S[:, ::g, ::g].shape[1:])
    return float(E), S, float(np.abs(S).sum()), np.sign(d).astype(np.int8) if signs is None else T.astype(np.int8), d


def terms(F, c, points, signs=None):
    """(E, S [like F], sum |S|, T int8 [N, N], d [N, N]) in float64, under the reference's own signs or ``signs``."""
    return _terms(F, c, points, signs, np.float64)


def terms32(F, c, points, signs=None):
    """The same code in float32: what a float32 implementation may give."""
    return _terms(F, c, points, signs, np.float32)


def energy(F, c, points):
    return terms(F, c, points)[0]


def undecided(F, c, points):
    """(tau, the pairs with |d64| <= tau, the pairs whose float32 sign differs from the float64 sign, N): tau = 4 x
    the largest |d32 - d64| of this case -- the pairs whose sign a float32 implementation cannot be held to."""
    d64, d32 = terms(F, c, points)[4], terms32(F, c, points)[4]
    tau = 4 * float(np.abs(d32 - d64).max())
    off = ~np.eye(len(d64), dtype=bool)
    return tau, (np.abs(d64) <= tau) & off, (np.sign(d32) != np.sign(d64)) & off, len(d64)


def undecided_cap(N):
    return max(2, N * N / 1e5)


def normalized(S):
    """The reference's normalize (num_utils.py:85-87) in float64."""
    return S / (np.abs(S).sum() / S.size + float(EPS))


def blob(c, h, w, seed):
    """Seeded rectified noise; where the blob is large enough, a few columns all zero."""
    rng = np.random.RandomState(seed)
    feat = np.maximum(rng.standard_normal((c, h * w)) * 2 + 0.5, 0).astype(np.float32)
    n = h * w
    if n >= 8:
        feat[:, rng.permutation(n)[:max(2, n // 16)]] = 0
    return feat.reshape(c, h, w)


# (c, h, w, points) -> seed: the first seed from 0 on that meets the two conditions of tests/test_selfsim_host.py on the
# CPU -- the undecided-pairs cap, and a float32 restatement whose E and sum |S| are off by at least 2^-24 of their
# value (4 x less than that would ask a float32 result for more than its own rounding)
SEEDS = {(64, 5, 7, 1024): 4, (64, 9, 11, 30): 1, (128, 13, 10, 4096): 11, (64, 33, 33, 1024): 12}      # (others: 0)


def case_inputs(c, h, w, points, seed=None):
    """(F, c) of one op case, post-ReLU.  F is rectified noise.  The content's columns are rectified noise around
    three cluster centres: a column of distances is then near 0 inside a cluster and large outside, while F's are
    all alike, so that few d_ij lie near 0 -- what the undecided-pairs cap asks for at N = 576.  A few all-zero
    columns in F and, at other places, in c."""
    seed = SEEDS.get((c, h, w, points), 0) if seed is None else seed
    rng = np.random.RandomState(5000 + 97 * seed + c + h + w)
    n = h * w
    feat = blob(c, h, w, 3000 + 97 * seed + c + h + w)
    centres = np.maximum(rng.standard_normal((c, 3)) * 2 + 0.5, 0)
    content = np.maximum(centres[:, rng.randint(3, size=n)] + 0.3 * rng.standard_normal((c, n)), 0).astype(np.float32)
    if n >= 8:
        live = np.flatnonzero(feat.reshape(c, -1).any(axis=0))
        content[:, live[rng.permutation(len(live))[:max(2, n // 16)]]] = 0
    return feat, content.reshape(c, h, w)


def case_conditions(c, h, w, points, seed=None):
    """(undecided pairs, their cap, relative float32 error of E, of sum |S|) of one op case: CPU arithmetic only."""
    F, cc = case_inputs(c, h, w, points, seed)
    _, und, _, N = undecided(F, cc, points)
    E, _, a, T, _ = terms(F, cc, points)
    E32, _, a32, _, _ = terms32(F, cc, points, signs=T)
    return int(und.sum()), undecided_cap(N), abs(E32 - E) / E if E else np.inf, abs(a32 - a) / a if a else np.inf


class SelfsimOracleModel(OracleModel):
    """``OracleModel`` with self-similarity targets: ``selfsim_points`` = {layer: points}, ``selfsim_weights`` =
    {layer: w}.  A layer with a target is part of every evaluation; its term follows the layer's style terms and
    reads the window of the layer's first content map."""

    def __init__(self, layers, params=None):
        super().__init__(layers, params)
        self.selfsim_points, self.selfsim_weights = {}, {}

    def selfsim_window(self, b, feat, start):
        fy, fx = np.asarray(start) // self.scale[b]
        fh, fw = feat.shape[-2:]
        return self.contents[0][b][:, fy:fy + fh, fx:fx + fw]

    def selfsim_loss64(self, acts, layer_weights, start):
        return sum(layer_weights.get(b, 1.0) * self.selfsim_weights.get(b, 1.0) * 0.5 *
                   terms(acts[b], self.selfsim_window(b, acts[b], start), self.selfsim_points[b])[0]
                   for b in self.selfsim_points)

    def sc_grad_tile(self, tile, start, content_layers, style_layers, layer_weights,
                     content_weight, style_weight, activations=None, dd_layers=(), dd_weight=None):
        # A copy of oracle.tile_path.OracleModel.sc_grad_tile with two additions, marked `selfsim_points`: the
        # layers that join the order and the term of such a layer.  Whoever changes that method changes this.
        net = self.net
        order = self.deep_to_shallow(list(content_layers) + list(style_layers) + list(dd_layers) +
                                     list(self.selfsim_points))
        net.blobs['data'].reshape(1, 3, *tile.shape[-2:])
        net.blobs['data'].data[0] = tile
        net._reshape()
        for b in order:
            net.blobs[b].diff[...] = 0
        net.forward(end=order[0])
        np.maximum(net.blobs[order[0]].data, 0, out=net.blobs[order[0]].data)
        if activations is not None:
            net.load_activations(activations)
        start = np.asarray(start)
        loss = 0.0
        for i, b in enumerate(order):
            lw = layer_weights.get(b, 1.0)
            feat = net.blobs[b].data[0]
            diff = net.blobs[b].diff[0]
            fy, fx = start // self.scale[b]
            fh, fw = feat.shape[-2:]
            if b in content_layers:
                for content in self.contents:
                    resid = feat - content[b][:, fy:fy + fh, fx:fx + fw]
                    loss += lw * content_weight[b] * half_sq_norm(resid)
                    diff += np.float32(lw * content_weight[b]) * l1_normalize(resid)
            if b in style_layers:
                for style in self.styles:
                    gdiff = gram_lower(feat) - style[b]
                    sgrad = symm_lower_times(gdiff, feat.reshape(feat.shape[0], -1))
                    loss += lw * style_weight[b] * half_sq_norm(gdiff) / len(self.styles)
                    diff += np.float32(lw * style_weight[b] / len(self.styles)) * \
                        l1_normalize(sgrad).reshape(feat.shape)
            if b in self.selfsim_points:
                w = lw * self.selfsim_weights.get(b, 1.0)
                E, S, _, _, _ = terms(feat, self.selfsim_window(b, feat, start), self.selfsim_points[b])
                loss += w * 0.5 * E
                diff += np.float32(w * normalized(S))
            if b in dd_layers:
                loss -= lw * dd_weight[b] * half_sq_norm(feat)
                diff -= np.float32(lw * dd_weight[b]) * l1_normalize(feat.copy())
            if i + 1 == len(order):
                net.backward(start=b)
            else:
                net.backward(start=b, end=order[i + 1])
        return loss, net.blobs['data'].diff[0].copy()
