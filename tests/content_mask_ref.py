"""Reference arithmetic of the masked content term (--content-mask, stx_set_content_mask) for the tests.

For a blob F [C, fh, fw], the window c [C, fh, fw] of a content map and the window m [fh, fw] of the mask map:

    d     = F - c
    a     = sum m / (fh fw)
    E     = 1/2 sum m d^2                      loss += lw * cw * E
    S0    = m * d
    S     = a * S0
    diff += lw * cw * S / (sum|S0| / S0.size + EPS)

``masked_content_terms`` and ``masked_content_gradient`` work in float64; ``MaskedContentOracleModel`` is the
oracle's tile evaluation with this term in the oracle's own float32 operations, arranged so that an all-ones
mask reproduces ``OracleModel.sc_grad_tile`` bit for bit.  The mask maps are those of tests/masked_style_ref.py
(``mask_map``: block means)."""

import numpy as np

from oracle.num_ops import EPS, gram_lower, half_sq_norm, l1_normalize, roll_xy, symm_lower_times
from oracle.tile_path import OracleModel
from tests.masked_style_ref import mask_map


def masked_content_terms(F, c, m):
    """(E = 1/2 sum m d^2, S = a m d, sum |m d|, a) in float64; F, c [C, h, w], m [h, w]."""
    d = np.asarray(F, np.float64) - np.asarray(c, np.float64)
    mm = np.asarray(m, np.float64)
    a = float(mm.sum() / mm.size)
    s0 = mm * d
    return 0.5 * float((s0 * d).sum()), a * s0, float(np.abs(s0).sum()), a


def masked_content_gradient(F, c, m):
    """What the term adds to the blob's gradient at weight 1: a S0 / (sum|S0| / S0.size + EPS), float64."""
    _, s, asum, _ = masked_content_terms(F, c, m)
    return s / (asum / s.size + float(EPS))


def masked_content_term32(resid, m):
    """(E, a S0 / (sum|S0| / S0.size + EPS)) of one masked content term in the oracle's own float32 operations, from
    the residual F - c and the mask window m: what ``MaskedContentOracleModel`` adds at weight 1."""
    a = np.float32(float(m.astype(np.float64).sum()) / m.size)
    s0 = resid * m
    half = float(np.dot(s0.ravel(), resid.ravel())) / 2
    return half, a * l1_normalize(s0)


class MaskedContentOracleModel(OracleModel):
    """``OracleModel`` whose content term acts through ``cmask`` = {layer: mask map [ceil(H/s), ceil(W/s)]}
    (None: the plain term).  The maps are rolled with the content maps (``roll_contents``)."""

    def __init__(self, layers, params=None):
        super().__init__(layers, params)
        self.cmask = None

    def set_content_mask(self, M, content_layers):
        """M: an [H, W] array in [0, 1] in the content picture's frame, or None."""
        self.cmask = None if M is None else {b: mask_map(M, self.scale[b]).astype(np.float32)
                                             for b in content_layers}

    def roll_contents(self, xy_pixels):
        super().roll_contents(xy_pixels)
        for b, m in (self.cmask or {}).items():
            roll_xy(m, np.asarray(xy_pixels) // self.scale[b])

    def sc_grad_tile(self, tile, start, content_layers, style_layers, layer_weights,
                     content_weight, style_weight, activations=None, dd_layers=(), dd_weight=None):
        net = self.net
        order = self.deep_to_shallow(list(content_layers) + list(style_layers) + list(dd_layers))
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
                    if self.cmask is None:
                        loss += lw * content_weight[b] * half_sq_norm(resid)
                        diff += np.float32(lw * content_weight[b]) * l1_normalize(resid)
                        continue
                    m = self.cmask[b][fy:fy + fh, fx:fx + fw]
                    assert m.shape == (fh, fw), 'mask window outside the map'
                    half, s = masked_content_term32(resid, m)
                    loss += lw * content_weight[b] * half
                    diff += np.float32(lw * content_weight[b]) * s
            if b in style_layers:
                for style in self.styles:
                    gdiff = gram_lower(feat) - style[b]
                    sgrad = symm_lower_times(gdiff, feat.reshape(feat.shape[0], -1))
                    loss += lw * style_weight[b] * half_sq_norm(gdiff) / len(self.styles)
                    diff += np.float32(lw * style_weight[b] / len(self.styles)) * \
                        l1_normalize(sgrad).reshape(feat.shape)
            if b in dd_layers:
                loss -= lw * dd_weight[b] * half_sq_norm(feat)
                diff -= np.float32(lw * dd_weight[b]) * l1_normalize(feat.copy())
            if i + 1 == len(order):
                net.backward(start=b)
            else:
                net.backward(start=b, end=order[i + 1])
        return loss, net.blobs['data'].diff[0].copy()

    def masked_loss64(self, acts, start, cl, sl, lw, cw, sw):
        """The loss from given activations with every reduction in float64 (the maps as they are rolled now)."""
        start = np.asarray(start)
        total = 0.0
        for b in self.deep_to_shallow(list(cl) + list(sl)):
            w = lw.get(b, 1.0)
            feat = np.asarray(acts[b], np.float64)
            fy, fx = start // self.scale[b]
            fh, fw = feat.shape[-2:]
            if b in cl:
                m = np.ones((fh, fw)) if self.cmask is None else self.cmask[b][fy:fy + fh, fx:fx + fw]
                for content in self.contents:
                    half, _, _, _ = masked_content_terms(feat, content[b][:, fy:fy + fh, fx:fx + fw], m)
                    total += w * cw[b] * half
            if b in sl:
                f = feat.reshape(feat.shape[0], -1)
                for style in self.styles:
                    D = np.tril(f @ f.T / f.size) - np.tril(np.asarray(style[b], np.float64))
                    total += w * sw[b] * 0.5 * float((D * D).sum()) / len(self.styles)
        return total
