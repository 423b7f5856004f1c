"""Reference arithmetic of the contextual style term (--cx-weight, stx_set_cx_targets) for the tests, in float64 on
the same float32 inputs.  For a blob F [C, h, w] sampled at the grid (a g, b g) -- g the smallest integer >= 1 with
ceil(h/g) ceil(w/g) <= points, N positions in raster order, columns f_i -- against a bank of M centred unit rows b_k
with the mean mu of the raw rows they came from (``bank``), eps = 1e-5, eta the bandwidth:

    z_i  = f_i - mu,  r_i = |z_i|,  x_i = z_i / r_i           (r_i = 0: x_i = 0, 1/r_i = 0)
    s_ik = x_i . b_k
    k*_i = argmax_k s_ik (lowest k),  a_i = 1 - s_ik*,  tau_i = eta (a_i + eps)
    e_ik = exp((s_ik - s_ik*) / tau_i),  Z_i = sum_k e_ik,  p_ik = e_ik / Z_i,  u_i = sum_k p_ik s_ik
    i*_k = argmax_i p_ik (lowest i),  m_k = p_{i*_k k},  CX = (1/M) sum_k m_k,  E = -log CX
    P_i  = sum_{k: i*_k = i} p_ik,  Q_i = sum_{k: i*_k = i} p_ik s_ik
    g_ik = -(1/(M CX)) [ p_ik (1[i*_k = i] - P_i) / tau_i + 1[k = k*_i] eta (Q_i - P_i u_i) / tau_i^2 ]
    q_i  = sum_k g_ik b_k,  S_i = (q_i - (q_i . x_i) x_i) / r_i  at the grid positions, 0 elsewhere
    loss += lw w E
    diff += lw w S / (sum|S| / (C h w) + EPS)

``terms`` forms every quantity under its own decisions (k*, i*) or under decisions handed in (the device's, as
selfsim_ref.terms takes signs); ``terms32`` is the same code in float32 -- numpy's order of summation -- and is the
yardstick of the tolerances: a float32 kernel is held to 4 x its error, the factor for the other order a device adds
in.  ``CxOracleModel`` is the oracle's tile evaluation with the term added: computed in float64 from the oracle's
blobs and pushed back through the oracle's own backward pass.

The op cases of tests/test_gpu_cx.py and their inputs are made here, so that tests/test_cx_host.py can hold the same
inputs to the undecided-decisions condition on the CPU."""

from types import SimpleNamespace

import numpy as np

from oracle.num_ops import EPS, gram_lower, half_sq_norm, l1_normalize, symm_lower_times
from oracle.tile_path import OracleModel
from style_transfer_amd.config_system import selfsim_grid

# (C, h, w, points, M): N = 35, ragged in the 32-wide MFMA tile both ways; N = 30 with g = 2 and M one past two
# column blocks; N = 130 and M = 1000, several blocks both ways, two K steps; N = 576, M = 513, four K steps;
# g = 2, N = 289; M = 2115: the gradient's K split, 17 slices of 128 rows with a last one of 67; N = 2; N = M = 1
OP_SHAPES = [(64, 5, 7, 1024, 31), (64, 9, 11, 30, 129), (128, 13, 10, 4096, 1000), (256, 24, 24, 576, 513),
             (64, 33, 33, 1024, 70), (64, 9, 11, 30, 2115), (64, 1, 2, 2, 3), (64, 1, 1, 2, 1)]
ETA_DEFAULT = 0.5
# (shape, eta) of every op case: eta = 0.5 on all of them and 0.1 on two
OP_CASES = [(shape, ETA_DEFAULT) for shape in OP_SHAPES] + [((64, 9, 11, 30, 129), 0.1), ((256, 24, 24, 576, 513), 0.1)]
EPS_TAU = 1e-5


def grid(h, w, points):
    """(g, N, positions [N, 2] as (y, x) in raster order)."""
    g, gh, gw = selfsim_grid(h, w, points)
    ys, xs = np.meshgrid(np.arange(gh) * g, np.arange(gw) * g, indexing='ij')
    return g, gh * gw, np.stack([ys.ravel(), xs.ravel()], axis=1)


def _unit(v):
    r = np.sqrt((v * v).sum(axis=1))
    inv = np.where(r > 0, 1 / np.where(r > 0, r, 1), 0).astype(v.dtype)
    return v * inv[:, None], inv


def bank(raw):
    """(mu [C], B [M, C]) in float64 of raw rows [M, C]: the mean over the bank's own rows and the centred unit rows
    (zero where the norm is 0)."""
    y = np.asarray(raw, np.float64)
    mu = y.mean(axis=0)
    return mu, _unit(y - mu[None, :])[0]


def _terms(F, B, mu, points, eta, decisions, dtype):
    C, h, w = np.shape(F)
    g, N, _ = grid(h, w, points)
    b, eta = np.asarray(B, dtype), dtype(eta)
    M, rows, cols = len(b), np.arange(N), np.arange(len(b))
    x, inv = _unit(np.asarray(F, dtype)[:, ::g, ::g].reshape(C, N).T - np.asarray(mu, dtype)[None, :])
    s = x @ b.T
    kstar = s.argmax(axis=1) if decisions is None else np.asarray(decisions[0]).astype(np.int64)
    best = s[rows, kstar]
    tau = eta * ((1 - best) + dtype(EPS_TAU))
    e = np.exp((s - best[:, None]) / tau[:, None])
    p = e / e.sum(axis=1)[:, None]
    u = (p * s).sum(axis=1)
    winner = p.argmax(axis=0) if decisions is None else np.asarray(decisions[1]).astype(np.int64)
    CX = p[winner, cols].sum() / dtype(M)
    E = -np.log(CX) + dtype(0)
    own = np.zeros((N, M), dtype)
    own[winner, cols] = 1
    P, Q = (own * p).sum(axis=1), (own * p * s).sum(axis=1)
    gm = p * (own - P[:, None]) / tau[:, None]
    gm[rows, kstar] += eta * (Q - P * u) / (tau * tau)
    gm *= -1 / (dtype(M) * CX)
    q = gm @ b
    S_n = (q - (q * x).sum(axis=1)[:, None] * x) * inv[:, None]
    S = np.zeros((C, h, w), dtype)
    S[:, ::g, ::g] = S_n.T.reshape(C, *S[:, ::g, ::g].shape[1:])
    assert S.dtype == dtype and s.dtype == dtype and p.dtype == dtype
    return SimpleNamespace(E=float(E), S=S, abs_sum=float(np.abs(S).sum()), kstar=kstar.astype(np.int32),
                           winner=winner.astype(np.int32), s=s, p=p, N=N, M=M)


def terms(F, B, mu, points, eta, decisions=None):
    """E, S [like F], abs_sum = sum |S|, kstar int32 [N], winner int32 [M], s and p [N, M] in float64, under the
    reference's own decisions or ``decisions`` = (kstar, winner).  B and mu are taken as they are (float32 inputs)."""
    return _terms(F, B, mu, points, eta, decisions, np.float64)


def terms32(F, B, mu, points, eta, decisions=None):
    """The same code in float32: what a float32 implementation may give."""
    return _terms(F, B, mu, points, eta, decisions, np.float32)


def energy(F, B, mu, points, eta):
    return terms(F, B, mu, points, eta).E


def _close_pairs(values, axis, tol):
    """Along ``axis``: is the gap between the two largest values at most tol?  (One value: no.)"""
    if values.shape[axis] < 2:
        return np.zeros(values.shape[1 - axis], bool)
    top = np.sort(values, axis=axis)
    top = top[:, -2:] if axis == 1 else top[-2:, :].T
    return top[:, 1] - top[:, 0] <= tol


def undecided(F, B, mu, points, eta):
    """(rows [N] bool, columns [M] bool): the decisions a float32 implementation cannot be held to -- a row whose two
    best scores lie closer than 4 x max |s32 - s64|, a column whose two best p lie closer than 4 x max |p32 - p64|."""
    t64, t32 = terms(F, B, mu, points, eta), terms32(F, B, mu, points, eta)
    tol_s, tol_p = 4 * float(np.abs(t32.s - t64.s).max()), 4 * float(np.abs(t32.p - t64.p).max())
    return _close_pairs(t64.s, 1, tol_s), _close_pairs(t64.p, 0, tol_p)


def undecided_cap(N, M):
    return max(2, (N + M) / 256)


def normalized(S):
    """The reference's normalize (num_utils.py:85-87) in float64."""
    return S / (np.abs(S).sum() / S.size + float(EPS))


def noise(shape, seed):
    """Seeded rectified noise (no all-zero columns are planted: identical columns tie exactly in i*)."""
    return np.maximum(np.random.RandomState(seed).standard_normal(shape) * 2 + 0.5, 0).astype(np.float32)


# (C, h, w, points, M) -> seed: the first seed from 0 on that meets the two conditions of tests/test_cx_host.py on the
# CPU at every eta of the case -- the undecided-decisions cap, and a float32 restatement whose E and sum |S| are off by
# at least 2^-24 of their value (4 x less than that would ask a float32 result for more than its own rounding)
SEEDS = {(64, 5, 7, 1024, 31): 20, (64, 9, 11, 30, 129): 140, (128, 13, 10, 4096, 1000): 3630, (256, 24, 24, 576, 513): 1327,
         (64, 33, 33, 1024, 70): 43, (64, 9, 11, 30, 2115): 765, (64, 1, 2, 2, 3): 4}      # (others: 0)


def case_inputs(c, h, w, points, M, seed=None):
    """(F [C, h, w], B [M, C], mu [C]) of one op case: F and the raw rows are rectified noise without duplicate
    columns; B and mu are ``bank`` of the raw rows, rounded to float32 -- the arrays the device is handed."""
    seed = SEEDS.get((c, h, w, points, M), 0) if seed is None else seed
    feat = noise((c, h, w), 3000 + 97 * seed + c + h + w)
    raw = noise((M, c), 7000 + 97 * seed + c + M)
    cols = feat.reshape(c, -1).T
    assert len(np.unique(cols, axis=0)) == len(cols) and len(np.unique(raw, axis=0)) == M
    mu, B = bank(raw)
    return feat, B.astype(np.float32), mu.astype(np.float32)


def case_conditions(shape, eta, seed=None):
    """(undecided decisions, their cap, relative float32 error of E, of sum |S|) of one op case: CPU arithmetic only."""
    points = shape[3]
    F, B, mu = case_inputs(*shape, seed=seed)
    und_rows, und_cols = undecided(F, B, mu, points, eta)
    t = terms(F, B, mu, points, eta)
    t32 = terms32(F, B, mu, points, eta, decisions=(t.kstar, t.winner))
    return (int(und_rows.sum() + und_cols.sum()), undecided_cap(t.N, t.M),
            abs(t32.E - t.E) / t.E if t.E else np.inf, abs(t32.abs_sum - t.abs_sum) / t.abs_sum if t.abs_sum else np.inf)


def conditions_hold(shape, seed):
    """Do both conditions hold at every eta the case runs at?"""
    for case, eta in OP_CASES:
        if case == shape:
            und, cap, err_e, err_a = case_conditions(shape, eta, seed)
            if und > cap or err_e < 2.0 ** -24 or err_a < 2.0 ** -24:
                return False
    return True


class CxOracleModel(OracleModel):
    """``OracleModel`` with contextual targets: ``cx_banks`` = {layer: raw rows [M, C]}, ``cx_weights`` = {layer: w},
    ``cx_points`` and ``cx_eta`` for all of them.  A layer with a target is part of every evaluation; its term follows
    the layer's style terms."""

    def __init__(self, layers, params=None):
        super().__init__(layers, params)
        self.cx_banks, self.cx_weights, self.cx_points, self.cx_eta = {}, {}, 1024, ETA_DEFAULT

    def cx_terms(self, b, feat):
        mu, B = bank(self.cx_banks[b])
        return terms(feat, B, mu, self.cx_points, self.cx_eta)

    def cx_loss64(self, acts, layer_weights):
        return sum(layer_weights.get(b, 1.0) * self.cx_weights.get(b, 1.0) * self.cx_terms(b, acts[b]).E
                   for b in self.cx_banks)

    def sc_grad_tile(self, tile, start, content_layers, style_layers, layer_weights,
                     content_weight, style_weight, activations=None, dd_layers=(), dd_weight=None,
                     extra_term=None):
        # A copy of oracle.tile_path.OracleModel.sc_grad_tile with two additions, marked `cx_banks`: the layers that
        # join the order and the term of such a layer (and `extra_term(b, feat)` -> (loss, diff) or None: another
        # optional term of the blob, which comes before this one).  Whoever changes that method changes this.
        net = self.net
        order = self.deep_to_shallow(list(content_layers) + list(style_layers) + list(dd_layers) +
                                     list(self.cx_banks))
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
            other = extra_term(b, feat) if extra_term is not None else None
            if other is not None:
                loss += lw * other[0]
                diff += np.float32(lw * other[1])
            if b in self.cx_banks:
                w = lw * self.cx_weights.get(b, 1.0)
                t = self.cx_terms(b, feat)
                loss += w * t.E
                diff += np.float32(w * normalized(t.S))
            if b in dd_layers:
                loss -= lw * dd_weight[b] * half_sq_norm(feat)
                diff -= np.float32(lw * dd_weight[b]) * l1_normalize(feat.copy())
            if i + 1 == len(order):
                net.backward(start=b)
            else:
                net.backward(start=b, end=order[i + 1])
        return loss, net.blobs['data'].diff[0].copy()
