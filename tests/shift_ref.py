"""Reference arithmetic of the shifted-Gram style term (--shift-weight, stx_set_shift_targets) for the tests, in
float64.  For a blob F [C, h, w], n = h w, offsets delta = (dy, dx) along one axis each and targets T [|Delta|, C, C];
per offset P = {p : p and p + delta in the map}, n_d = (h - dy)(w - dx):

    X_d[a][b] = (1 / (C n_d)) sum_{p in P} F_a(p) F_b(p + delta)
    D_d       = X_d - T_d,        E = (1 / |Delta|) sum_d sum_ab D_d[a][b]^2
    S_a(p)    = (1 / |Delta|) sum_d (n / n_d) [ sum_b D_d[a][b] F_b(p + delta) + sum_b D_d[b][a] F_b(p - delta) ]
                                                                   ( = C n d(E/2)/dF_a(p); terms off the map are 0 )
    loss += lw w E / 2
    diff += lw w S / (sum|S| / (C n) + EPS)

``ShiftOracleModel`` is the oracle's tile evaluation with this term added: the term itself is computed in float64
from the oracle's blobs and pushed back through the oracle's own backward pass."""

import numpy as np

from oracle.num_ops import EPS, gram_lower, half_sq_norm, l1_normalize, symm_lower_times
from oracle.tile_path import OracleModel


def _windows(f, dy, dx):
    """(F at p, F at p + delta) over P, as [C, n_d] arrays."""
    c, h, w = f.shape
    return f[:, :h - dy, :w - dx].reshape(c, -1), f[:, dy:, dx:].reshape(c, -1)


def shift_gram(F, offsets):
    """X [|Delta|, C, C] of F [C, h, w] in float64."""
    f = np.asarray(F, np.float64)
    c, h, w = f.shape
    out = np.empty((len(offsets), c, c))
    for i, (dy, dx) in enumerate(offsets):
        if h - dy < 1 or w - dx < 1:
            raise ValueError('offset (%d, %d) leaves a %d x %d map without a pair' % (dy, dx, h, w))
        a, b = _windows(f, dy, dx)
        out[i] = a @ b.T / (c * a.shape[1])
    return out


def half_e(F, offsets, T):
    d = shift_gram(F, offsets) - np.asarray(T, np.float64)
    return 0.5 * float((d ** 2).sum()) / len(offsets)


def shift_terms(F, offsets, T):
    """(E / 2, S [like F], sum |S|) in float64."""
    f = np.asarray(F, np.float64)
    c, h, w = f.shape
    D = shift_gram(f, offsets) - np.asarray(T, np.float64)
    S = np.zeros_like(f)
    for (dy, dx), d in zip(offsets, D):
        n_d = (h - dy) * (w - dx)
        a, b = _windows(f, dy, dx)
        scale = h * w / (n_d * len(offsets))
        S[:, :h - dy, :w - dx] += scale * (d @ b).reshape(c, h - dy, w - dx)
        S[:, dy:, dx:] += scale * (d.T @ a).reshape(c, h - dy, w - dx)
    return 0.5 * float((D ** 2).sum()) / len(offsets), S, float(np.abs(S).sum())


def normalized(S):
    """The reference's normalize (num_utils.py:85-87) in float64."""
    return S / (np.abs(S).sum() / S.size + float(EPS))


def finite_difference(F, offsets, T, index, h):
    """Central difference of E / 2 along element ``index`` of F."""
    plus, minus = np.array(F, np.float64), np.array(F, np.float64)
    plus[index] += h
    minus[index] -= h
    return (half_e(plus, offsets, T) - half_e(minus, offsets, T)) / (2 * h)


class ShiftOracleModel(OracleModel):
    """``OracleModel`` with shifted-Gram targets: ``shift_targets`` = {layer: (offsets, T)}, ``shift_weights`` =
    {layer: w}.  A layer with a target is part of every evaluation; its term follows the layer's style terms.
    ``extra_term(b, feat, lw)`` (or None) -> (loss, diff) of one more term of blob ``b``, added in front of the
    shifted-Gram term: the hook of the tests that put another optional term on the same blob."""

    def __init__(self, layers, params=None):
        super().__init__(layers, params)
        self.shift_targets, self.shift_weights = {}, {}
        self.extra_layers, self.extra_term = (), None

    def shift_loss64(self, acts, layer_weights):
        return sum(layer_weights.get(b, 1.0) * self.shift_weights.get(b, 1.0) *
                   shift_terms(acts[b], *self.shift_targets[b])[0] for b in self.shift_targets)

    def sc_grad_tile(self, tile, start, content_layers, style_layers, layer_weights,
                     content_weight, style_weight, activations=None, dd_layers=(), dd_weight=None):
        # A copy of oracle.tile_path.OracleModel.sc_grad_tile with two additions, marked `shift_targets` (and
        # `extra_term`): the layers that join the order and the terms of such a layer.  Whoever changes that method
        # changes this.
        net = self.net
        order = self.deep_to_shallow(list(content_layers) + list(style_layers) + list(dd_layers) +
                                     list(self.extra_layers) + list(self.shift_targets))
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
            if b in self.extra_layers:
                more_loss, more_diff = self.extra_term(b, feat, lw)
                loss += more_loss
                diff += np.float32(more_diff)
            if b in self.shift_targets:
                w = lw * self.shift_weights.get(b, 1.0)
                half, S, _ = shift_terms(feat, *self.shift_targets[b])
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
