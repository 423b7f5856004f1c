"""Reference arithmetic of the nearest-neighbour feature matching term (--nnfm-weight, stx_set_nnfm_targets)
for the tests, in float64.  For a blob F [C, h, w] with columns f_i (n = h w) and a bank B [M, C] of unit or
zero rows b_j:

    r_i = |f_i|,  x_i = f_i / r_i                  (r_i = 0: x_i = 0, c_i = 0, j_i = 0, S_i = 0)
    j_i = argmax_j x_i . b_j                       (the lowest j among equal scores)
    c_i = x_i . b_{j_i}
    E   = (2/n) sum_i (1 - c_i)
    S_i = -(b_{j_i} - c_i x_i) / r_i               ( = n d(E/2)/d f_i with j_i held fixed )
    loss += lw w E / 2
    diff += lw w S / (sum|S| / (C n) + EPS)

``emulated_scores`` restates the arithmetic of the GPU's search (fp16 hi / lo pieces of x 2^13 and b 2^13, three
exact products per 16-channel step, float32 accumulation), in the style of tools/f16x2_numerics.py.
``NnfmOracleModel`` is the oracle's tile evaluation with this term added."""

import numpy as np

from oracle.num_ops import EPS, gram_lower, half_sq_norm, l1_normalize, symm_lower_times
from oracle.tile_path import OracleModel

SCALE = 8192.0      # 2^13


def unit_columns(F):
    """(x [n, C], r [n]) of F [C, ...] in float64; a zero column gives a zero row."""
    f = np.asarray(F, np.float64).reshape(np.shape(F)[0], -1).T
    r = np.sqrt((f * f).sum(axis=1))
    x = np.divide(f, r[:, None], out=np.zeros_like(f), where=r[:, None] > 0)
    return x, r


def bank_rows(h, w, stride=1):
    return -(-h // stride) * -(-w // stride)


def bank_of(F, stride=1):
    """The bank of one feature map [C, h, w]: its unit columns at y % stride == 0 and x % stride == 0, in
    raster order, [rows, C]."""
    F = np.asarray(F, np.float64)
    return unit_columns(F[:, ::stride, ::stride])[0]


def concat_banks(banks):
    """Banks of several pictures or ladder sizes: a union, in the order given."""
    return np.concatenate([np.asarray(b, np.float64) for b in banks], axis=0)


def scores64(F, B):
    return unit_columns(F)[0] @ np.asarray(B, np.float64).T


def nearest(F, B):
    """j [n]: the float64 argmax, lowest index among equals (numpy's argmax takes the first)."""
    return np.argmax(scores64(F, B), axis=1).astype(np.int64)


def terms_at(F, B, j):
    """(E, S [like F], sum |S|, c [n]) with the rows j [n] given."""
    x, r = unit_columns(F)
    b = np.asarray(B, np.float64)[np.asarray(j, np.int64)]
    c = (x * b).sum(axis=1)
    inv = np.divide(1.0, r, out=np.zeros_like(r), where=r > 0)
    c = np.where(r > 0, c, 0.0)
    S = -(b - c[:, None] * x) * inv[:, None]
    E = 2.0 * float((1.0 - c).sum()) / len(r)
    return E, S.T.reshape(np.shape(F)), float(np.abs(S).sum()), c


def terms(F, B):
    """(E, S, sum |S|, c, j) at the reference's own rows."""
    j = nearest(F, B)
    return terms_at(F, B, j) + (j,)


def normalized(S):
    """The reference's normalize (num_utils.py:85-87) in float64."""
    return S / (np.abs(S).sum() / S.size + float(EPS))


def half_e_unit(F, B):
    """E / 2 as (1 / 2n) sum_i |x_i - b_{j_i}|^2: the same number for unit rows, without the cancelled 1 - c_i
    (for differences of E between two nearby blobs)."""
    x, _ = unit_columns(F)
    b = np.asarray(B, np.float64)[nearest(F, B)]
    return float(((x - b) ** 2).sum()) / (2 * x.shape[0])


def finite_difference(F, B, index, h):
    """Central difference of E / 2 along element ``index`` of F (unit bank rows; the rows are searched anew on
    both sides)."""
    plus, minus = np.array(F, np.float64), np.array(F, np.float64)
    plus[index] += h
    minus[index] -= h
    return (half_e_unit(plus, B) - half_e_unit(minus, B)) / (2 * h)


def _split(v32):
    """float32 values (already scaled) -> fp16 hi, lo as float64: hi = fp16(v), lo = fp16(v - hi)."""
    hi = v32.astype(np.float16)
    lo = (v32 - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float64), lo.astype(np.float64)


def emulated_scores(F, B):
    """The search's scores [n, M] as the GPU forms them, over 2^26: float32 inputs, 1 / r rounded to float32,
    the pieces of f (1/r 2^13) and of b 2^13, per 16-channel step lo hi + hi lo + hi hi (each an exact sum of
    exact products here; the matrix core's own order inside a step is not modelled) added to a float32
    accumulator."""
    f = np.asarray(F, np.float32).reshape(np.shape(F)[0], -1).T
    r = np.sqrt((f.astype(np.float64) ** 2).sum(axis=1))
    inv = np.divide(1.0, r, out=np.zeros_like(r), where=r > 0).astype(np.float32)
    xs = f * (inv * np.float32(SCALE))[:, None]
    xh, xl = _split(xs.astype(np.float32))
    bh, bl = _split(np.asarray(B, np.float32) * np.float32(SCALE))
    acc = np.zeros((f.shape[0], bh.shape[0]), np.float32)
    for k in range(0, f.shape[1], 16):
        s = slice(k, k + 16)
        for a, b in ((bl, xh), (bh, xl), (bh, xh)):
            acc = (acc.astype(np.float64) + b[:, s] @ a[:, s].T).astype(np.float32)
    return acc.astype(np.float64) / SCALE ** 2


def search_error(F, B):
    """The emulation's worst |score - float64 score| over all pairs."""
    return float(np.abs(emulated_scores(F, B) - scores64(F, B)).max())


class NnfmOracleModel(OracleModel):
    """``OracleModel`` with NNFM banks: ``nnfm_banks`` = {layer: B [M, C]}, ``nnfm_weights`` = {layer: w}.  A layer
    with a bank is part of every evaluation; its term follows the layer's style terms."""

    def __init__(self, layers, params=None):
        super().__init__(layers, params)
        self.nnfm_banks, self.nnfm_weights = {}, {}

    def nnfm_loss64(self, acts, layer_weights):
        return sum(layer_weights.get(b, 1.0) * self.nnfm_weights.get(b, 1.0) * terms(acts[b], self.nnfm_banks[b])[0] / 2
                   for b in self.nnfm_banks)

    def sc_grad_tile(self, tile, start, content_layers, style_layers, layer_weights,
                     content_weight, style_weight, activations=None, dd_layers=(), dd_weight=None):
        # A copy of oracle.tile_path.OracleModel.sc_grad_tile with two additions, marked `nnfm_banks`: the
        # layers that join the order and the term of such a layer.  Whoever changes that method changes this.
        net = self.net
        order = self.deep_to_shallow(list(content_layers) + list(style_layers) + list(dd_layers) +
                                     list(self.nnfm_banks))
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
            if b in self.nnfm_banks:
                w = lw * self.nnfm_weights.get(b, 1.0)
                E, S, _, _, _ = terms(feat, self.nnfm_banks[b])
                loss += w * E / 2
                diff += np.float32(w * normalized(S))
            if b in dd_layers:
                loss -= lw * dd_weight[b] * half_sq_norm(feat)
                diff -= np.float32(lw * dd_weight[b]) * l1_normalize(feat.copy())
            if i + 1 == len(order):
                net.backward(start=b)
            else:
                net.backward(start=b, end=order[i + 1])
        return loss, net.blobs['data'].diff[0].copy()
