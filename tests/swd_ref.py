"""Reference arithmetic of the sliced Wasserstein style term (--swd-weight, stx_set_swd_targets) for the tests,
in float64 on the same float32 inputs.  For a blob F [C, h, w], n = h w, unit directions V [D, C] and quantile
targets Tq [D, Q]:

    p[d][i] = v_d . f_i
    r_d(i)  = rank of i when p[d] is ordered ascending, equal values by ascending i
    t[d][r] = resample(Tq[d], Q -> n)[r]
    g[d][i] = p[d][i] - t[d][r_d(i)]
    E       = sum g^2 / (D n)
    S[c][i] = (1/D) sum_d g[d][i] V[d][c]                                  ( = n d(E/2)/dF with the ranks held )
    loss   += lw w E / 2
    diff   += lw w S / (sum|S| / (C n) + EPS)

``resample`` is the library's rule (include/stx.h) in exact integers; its weight a is the float32 the rule names and
the interpolation itself runs in float64.  Every quantity can be formed with the ranks found here or with ranks
handed in.  ``SwdOracleModel`` is the oracle's tile evaluation with this term added: computed in float64 from the
oracle's blobs and pushed back through the oracle's own backward pass.

The op cases of tests/test_gpu_swd.py and their inputs are made here, so that tests/test_swd_host.py can hold the
same inputs to the rank-quality condition on the CPU."""

import numpy as np

from oracle.num_ops import EPS, gram_lower, half_sq_norm, l1_normalize, symm_lower_times
from oracle.tile_path import OracleModel
from style_transfer_amd.config_system import swd_directions

# (C, h, w, D, Q): one element; below a wave with Q = n; odd D and n = 1023; a power of two with n = Q; n just above
# an 8192-record block; n above 65536 (several global merge levels, single and paired steps)
OP_SHAPES = [(4, 1, 1, 1, 2), (64, 5, 7, 64, 35), (8, 33, 31, 5, 64), (128, 64, 64, 128, 4096), (64, 91, 91, 16, 4096),
             (16, 257, 263, 3, 1000)]


def project(F, V):
    """p [D, n] in float64."""
    return np.asarray(V, np.float64) @ np.asarray(F, np.float64).reshape(np.shape(F)[0], -1)


def project32(F, V):
    """A float32 projection (numpy's summation order): what a float32 kernel may sort by."""
    return np.asarray(V, np.float32) @ np.asarray(F, np.float32).reshape(np.shape(F)[0], -1)


def tau(F, V):
    """tau [D, n] = C 2^-24 sum_c |V[d][c]| |F[c][i]|: the worst error of any float32 summation order."""
    C = np.shape(F)[0]
    return C * 2.0 ** -24 * (np.abs(np.asarray(V, np.float64)) @ np.abs(np.asarray(F, np.float64)).reshape(C, -1))


def ranks_of(p):
    """r [D, n]: the rank of every element under (value, index); -0 and +0 are equal values."""
    order = np.argsort(p, axis=1, kind='stable')
    ranks = np.empty_like(order)
    np.put_along_axis(ranks, order, np.broadcast_to(np.arange(p.shape[1]), p.shape), axis=1)
    return ranks


def resample(s, K):
    """resample(s[..., 0 .. M-1], M -> K) along the last axis, float64 (exact integers; a as the rule's float32)."""
    s = np.asarray(s, np.float64)
    M = s.shape[-1]
    k = np.arange(K, dtype=np.int64)
    num = (2 * k + 1) * M - K
    j = np.clip(num // (2 * K), 0, max(M - 2, 0))
    a = (np.float32(num % (2 * K)) / np.float32(2 * K)).astype(np.float64)
    nxt = np.minimum(j + 1, M - 1)
    out = s[..., j] + a * (s[..., nxt] - s[..., j])
    out = np.where(num <= 0, s[..., :1], out)
    return np.where(num // (2 * K) >= M - 1, s[..., -1:], out)


def target(F, V, Q):
    """Tq [D, Q]: the sorted projections resampled n -> Q, float64."""
    return resample(np.sort(project(F, V), axis=1), Q)


def terms(F, V, Tq, ranks=None):
    """(E / 2, S [like F], sum |S|, ranks [D, n]) in float64, under the reference's own ranks or under ``ranks``."""
    p = project(F, V)
    D, n = p.shape
    if ranks is None:
        ranks = ranks_of(p)
    g = p - np.take_along_axis(resample(Tq, n), np.asarray(ranks, np.int64), axis=1)
    S = (np.asarray(V, np.float64).T @ g) / D
    return 0.5 * float((g ** 2).sum()) / (D * n), S.reshape(np.shape(F)), float(np.abs(S).sum()), ranks


def half_e(F, V, Tq, ranks=None):
    return terms(F, V, Tq, ranks)[0]


def normalized(S):
    """The reference's normalize (num_utils.py:85-87) in float64."""
    return S / (np.abs(S).sum() / S.size + float(EPS))


def blob(c, h, w, seed):
    """Seeded rectified noise; a quarter of the columns all zero (exact ties in every direction) and two
    duplicated columns, where the blob is large enough to hold them."""
    rng = np.random.RandomState(seed)
    feat = np.maximum(rng.standard_normal((c, h * w)) * 2 + 0.5, 0).astype(np.float32)
    n = h * w
    if n >= 8:
        feat[:, rng.permutation(n)[:n // 4]] = 0
        live = np.flatnonzero(feat.any(axis=0))
        feat[:, live[1]] = feat[:, live[0]]
        feat[:, live[-1]] = feat[:, live[len(live) // 2]]
    return feat.reshape(c, h, w)


def case_inputs(c, h, w, d, q):
    """(F, V, the other blob whose quantiles are the targets) of one op case.  The other blob has another scale
    and offset, so g is not a cancelled difference."""
    feat = blob(c, h, w, 1000 + c + h + w + d)
    other = (blob(c, h, w, 2000 + c + h + w + d) * np.float32(1.5) + np.float32(0.25)).astype(np.float32)
    return feat, swd_directions(7, 'case %d %d' % (c, d), c, d), other


def rank_quality(F, V, Tq, ranks):
    """(E under the true ranks, E under ``ranks``): the rearrangement inequality makes the first the minimum."""
    return 2 * half_e(F, V, Tq), 2 * half_e(F, V, Tq, ranks)


class SwdOracleModel(OracleModel):
    """``OracleModel`` with sliced Wasserstein targets: ``swd_targets`` = {layer: (V, Tq)}, ``swd_weights`` =
    {layer: w}.  A layer with a target is part of every evaluation; its term follows the layer's style terms."""

    def __init__(self, layers, params=None):
        super().__init__(layers, params)
        self.swd_targets, self.swd_weights = {}, {}

    def swd_loss64(self, acts, layer_weights):
        return sum(layer_weights.get(b, 1.0) * self.swd_weights.get(b, 1.0) *
                   terms(acts[b], *self.swd_targets[b])[0] for b in self.swd_targets)

    def sc_grad_tile(self, tile, start, content_layers, style_layers, layer_weights,
                     content_weight, style_weight, activations=None, dd_layers=(), dd_weight=None):
        # A copy of oracle.tile_path.OracleModel.sc_grad_tile with two additions, marked `swd_targets`: the
        # layers that join the order and the term of such a layer.  Whoever changes that method changes this.
        net = self.net
        order = self.deep_to_shallow(list(content_layers) + list(style_layers) + list(dd_layers) +
                                     list(self.swd_targets))
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
            if b in self.swd_targets:
                w = lw * self.swd_weights.get(b, 1.0)
                half, S, _, _ = terms(feat, *self.swd_targets[b])
                loss += w * half
                diff += np.float32(w * normalized(S))
            if b in dd_layers:
                loss -= lw * dd_weight[b] * half_sq_norm(feat)
                diff -= np.float32(lw * dd_weight[b]) * l1_normalize(feat.copy())
            if i + 1 == len(order):
                net.backward(start=b)
            else:
                net.backward(start=b, end=order[i + 1])
        return loss, net.blobs['data'].diff[0].copy()
