"""Reference arithmetic of the mean / std style term (--stat-weight, stx_set_stat_targets) for the tests,
in float64.  For a blob F [C, h, w], n = h w, and per-channel targets MU, SD:

    mu_c  = mean F_c,   var_c = mean (F_c - mu_c)^2,   sd_c = sqrt(var_c + 1e-5)
    E     = sum_c (mu_c - MU_c)^2 + (sd_c - SD_c)^2
    S_c   = (mu_c - MU_c) + (sd_c - SD_c) (F_c - mu_c) / sd_c           ( = n d(E/2)/dF_c )
    loss += lw w E / 2
    diff += lw w S / (sum|S| / (C n) + EPS)

``StatOracleModel`` is the oracle's tile evaluation with this term added: the term itself is computed in
float64 from the oracle's blobs and pushed back through the oracle's own backward pass."""

import numpy as np

from oracle.num_ops import EPS, gram_lower, half_sq_norm, l1_normalize, symm_lower_times
from oracle.tile_path import OracleModel

SD_EPS = 1e-5


def feature_stats(F):
    """(mu [C], sd [C]) of F [C, ...] in float64."""
    f = np.asarray(F, np.float64).reshape(F.shape[0], -1)
    mu = f.mean(axis=1)
    var = ((f - mu[:, None]) ** 2).mean(axis=1)
    return mu, np.sqrt(var + SD_EPS)


def half_e(F, MU, SD):
    mu, sd = feature_stats(F)
    return 0.5 * float(((mu - MU) ** 2 + (sd - SD) ** 2).sum())


def stat_terms(F, MU, SD):
    """(E / 2, S [like F], sum |S|, b [C]) in float64."""
    f = np.asarray(F, np.float64).reshape(F.shape[0], -1)
    MU, SD = np.asarray(MU, np.float64), np.asarray(SD, np.float64)
    mu, sd = feature_stats(F)
    a, b = mu - MU, (sd - SD) / sd
    S = a[:, None] + b[:, None] * (f - mu[:, None])
    return 0.5 * float((a ** 2 + (sd - SD) ** 2).sum()), S.reshape(np.shape(F)), float(np.abs(S).sum()), b


def normalized(S):
    """The reference's normalize (num_utils.py:85-87) in float64."""
    return S / (np.abs(S).sum() / S.size + float(EPS))


def finite_difference(F, MU, SD, index, h):
    """Central difference of E / 2 along element ``index`` of F."""
    plus, minus = np.array(F, np.float64), np.array(F, np.float64)
    plus[index] += h
    minus[index] -= h
    return (half_e(plus, MU, SD) - half_e(minus, MU, SD)) / (2 * h)


class StatOracleModel(OracleModel):
    """``OracleModel`` with statistics targets: ``stat_targets`` = {layer: (MU, SD)}, ``stat_weights`` =
    {layer: w}.  A layer with a target is part of every evaluation; its term follows the layer's style terms."""

    def __init__(self, layers, params=None):
        super().__init__(layers, params)
        self.stat_targets, self.stat_weights = {}, {}

    def stat_loss64(self, acts, layer_weights):
        return sum(layer_weights.get(b, 1.0) * self.stat_weights.get(b, 1.0) *
                   stat_terms(acts[b], *self.stat_targets[b])[0] for b in self.stat_targets)

    def sc_grad_tile(self, tile, start, content_layers, style_layers, layer_weights,
                     content_weight, style_weight, activations=None, dd_layers=(), dd_weight=None):
        # A copy of oracle.tile_path.OracleModel.sc_grad_tile with two additions, marked `stat_targets`: the
        # layers that join the order and the term of such a layer.  Whoever changes that method changes this.
        net = self.net
        order = self.deep_to_shallow(list(content_layers) + list(style_layers) + list(dd_layers) +
                                     list(self.stat_targets))
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
            if b in self.stat_targets:
                w = lw * self.stat_weights.get(b, 1.0)
                half, S, _, _ = stat_terms(feat, *self.stat_targets[b])
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
