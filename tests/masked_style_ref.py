"""Reference arithmetic of the masked style term (--style-masks, stx_set_style_masks) for the tests.

For a blob F [C, fh, fw], the window m [fh, fw] of a style's mask map and its Gram target Gs:

    a    = sum m^2 / HW
    Fm   = F * m
    D    = gram_lower(Fm) - a * Gs
    loss += lw * sw * 1/2 |D|^2 / n_styles
    S    = m * (sym(D) Fm)
    diff += lw * sw / n_styles * a * S / (sum|S| / S.size + EPS)

``mask_map`` and ``masked_style_terms`` work in float64; ``MaskedOracleModel`` is the oracle's tile
evaluation with this term in the oracle's own float32 operations, arranged so that an all-ones mask
reproduces ``OracleModel.sc_grad_tile`` bit for bit."""

import numpy as np

from oracle.num_ops import gram_lower, half_sq_norm, l1_normalize, roll_xy, symm_lower_times
from oracle.tile_path import OracleModel


def mask_map(M, s):
    """Block means of an [H, W] mask at scale s: [ceil(H/s), ceil(W/s)], edge blocks over what exists."""
    M = np.asarray(M, np.float64)
    H, W = M.shape
    out = np.empty((-(-H // s), -(-W // s)))
    for y in range(out.shape[0]):
        for x in range(out.shape[1]):
            out[y, x] = M[y * s:min((y + 1) * s, H), x * s:min((x + 1) * s, W)].mean()
    return out


def masked_style_terms(F, m, Gs):
    """(1/2 |D|^2, a * S, sum |S|, a) in float64; F [C, h, w], m [h, w], Gs [C, C] (lower triangle read)."""
    c = F.shape[0]
    f = np.asarray(F, np.float64).reshape(c, -1)
    mm = np.asarray(m, np.float64).ravel()
    a = float((mm * mm).sum() / mm.size)
    fm = f * mm
    D = np.tril(fm @ fm.T / fm.size) - a * np.tril(np.asarray(Gs, np.float64))
    S = mm * ((D + np.tril(D, -1).T) @ fm)
    return 0.5 * float((D * D).sum()), (a * S).reshape(F.shape), float(np.abs(S).sum()), a


def window(full, fy, fx, fh, fw):
    return full[..., fy:fy + fh, fx:fx + fw]


def masked_style_term32(feat, m, Gs):
    """(1/2 |D|^2, a S / (sum|S| / S.size + EPS) [like feat]) of one masked style term in the oracle's own float32
    operations: what ``MaskedOracleModel`` adds at weight 1."""
    a = np.float32(float((m.astype(np.float64) ** 2).sum()) / m.size)
    fm = feat * m
    gdiff = gram_lower(fm) - a * Gs
    sgrad = symm_lower_times(gdiff, fm.reshape(fm.shape[0], -1)) * m.ravel()
    return half_sq_norm(gdiff), (a * l1_normalize(sgrad)).reshape(feat.shape)


class MaskedOracleModel(OracleModel):
    """``OracleModel`` whose style i acts through ``masks[i]`` = {layer: mask map [ceil(H/s), ceil(W/s)]}
    (None: everywhere, the plain term).  The maps are rolled with the content maps (``roll_contents``)."""

    def __init__(self, layers, params=None):
        super().__init__(layers, params)
        self.masks = []

    def set_masks(self, image_masks, style_layers):
        """image_masks: per style an [H, W] array in [0, 1] or None."""
        self.masks = [None if M is None else
                      {b: mask_map(M, self.scale[b]).astype(np.float32) for b in style_layers}
                      for M in image_masks]

    def roll_contents(self, xy_pixels):
        super().roll_contents(xy_pixels)
        for maps in self.masks:
            for b, m in (maps or {}).items():
                roll_xy(m, np.asarray(xy_pixels) // self.scale[b])

    def _mask_of(self, i, b):
        return self.masks[i].get(b) if i < len(self.masks) and self.masks[i] is not None else None

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
                    loss += lw * content_weight[b] * half_sq_norm(resid)
                    diff += np.float32(lw * content_weight[b]) * l1_normalize(resid)
            if b in style_layers:
                for si, style in enumerate(self.styles):
                    coef = lw * style_weight[b] / len(self.styles)
                    full = self._mask_of(si, b)
                    if full is None:
                        gdiff = gram_lower(feat) - style[b]
                        sgrad = symm_lower_times(gdiff, feat.reshape(feat.shape[0], -1))
                        loss += lw * style_weight[b] * half_sq_norm(gdiff) / len(self.styles)
                        diff += np.float32(coef) * l1_normalize(sgrad).reshape(feat.shape)
                        continue
                    m = window(full, fy, fx, fh, fw)
                    assert m.shape == (fh, fw), 'mask window outside the map'
                    half, s = masked_style_term32(feat, m, style[b])
                    loss += lw * style_weight[b] * half / len(self.styles)
                    diff += np.float32(coef) * s
            if b in dd_layers:
                loss -= lw * dd_weight[b] * half_sq_norm(feat)
                diff -= np.float32(lw * dd_weight[b]) * l1_normalize(feat.copy())
            if i + 1 == len(order):
                net.backward(start=b)
            else:
                net.backward(start=b, end=order[i + 1])
        return loss, net.blobs['data'].diff[0].copy()

    def masked_loss64(self, acts, start, cl, sl, lw, cw, sw):
        """The loss from given activations with every reduction in float64 (the masks as they are rolled now)."""
        start = np.asarray(start)
        total = 0.0
        for b in self.deep_to_shallow(list(cl) + list(sl)):
            w = lw.get(b, 1.0)
            feat = np.asarray(acts[b], np.float64)
            fy, fx = start // self.scale[b]
            fh, fw = feat.shape[-2:]
            if b in cl:
                for content in self.contents:
                    d = (feat - content[b][:, fy:fy + fh, fx:fx + fw].astype(np.float64)).ravel()
                    total += w * cw[b] * float(np.dot(d, d)) / 2
            if b in sl:
                for si, style in enumerate(self.styles):
                    full = self._mask_of(si, b)
                    m = np.ones((fh, fw)) if full is None else window(full, fy, fx, fh, fw)
                    half, _, _, _ = masked_style_terms(feat, m, style[b])
                    total += w * sw[b] * half / len(self.styles)
        return total
