"""One reference of the tile evaluation with every kind of loss term at once (tests/test_gpu_terms_meet.py).

Each per-feature reference file holds an ``OracleModel`` subclass that is a copy of ``sc_grad_tile`` with its own term
added, and the copies do not compose.  ``MeetOracleModel`` has one ``sc_grad_tile``: per tapped blob it walks ONE list
of terms in the library's order -- contents (masked or not), styles (masked or not), statistics, NNFM, SWD,
self-similarity, shifted Gram, contextual, Deep-Dream -- and adds each one the same way:

    loss += sign lw w half / share
    diff += sign float32(lw w / share) S          S float32: the oracle's own operations (content, style, dream, masked)
    diff += sign float32((lw w / share) S)        S float64: a term of a tests/*_ref.py file

with (half, S) = the term's callable on the blob's float32 features, ``start`` and the blob's window (fy, fx, fh, fw)
in a map of the content picture's frame; S is L1-normalised by the callable.  ``half`` is half the term's energy for
every family but the contextual one, whose loss is lw w E: its callable returns the whole E.  ``share`` is the number
of style sets for a style term and 1 otherwise; ``sign`` is -1 for Deep-Dream.  A layer that only an extra term names
joins the order; its layer weight is ``layer_weights.get(layer, 1.0)`` like every other layer's.

No term's arithmetic is stated here: the callables are adapters over oracle.num_ops and the tests/*_ref.py files.
With exactly one optional kind armed the evaluation equals that kind's own ``*OracleModel`` bit for bit
(tests/test_terms_meet_host.py), which is what makes the composite trustworthy where no other reference exists."""

import numpy as np

from oracle.num_ops import gram_lower, half_sq_norm, l1_normalize, roll_xy, symm_lower_times
from oracle.tile_path import OracleModel
from tests import (content_mask_ref, cx_ref, masked_style_ref, nnfm_cover_ref, nnfm_guided_ref, nnfm_knn_ref,
                   nnfm_patch_ref, nnfm_ref, selfsim_ref, shift_ref, stat_ref, swd_ref)
from tests.masked_style_ref import mask_map

FAMILIES = ['content', 'style', 'statistics', 'nnfm', 'swd', 'selfsim', 'shift', 'cx', 'dream']
EXTRA_ORDER = ['statistics', 'nnfm', 'swd', 'selfsim', 'shift', 'cx']       # the library's order behind the styles


class Term:
    """One term of one layer: ``fn(feat, start, window) -> (half, S normalised)`` as the oracle evaluates it and
    ``fn64(feat, start, window) -> half`` with every reduction in float64.  ``half`` is what the loss takes lw w
    times: E / 2 for every family but 'cx', whose loss is lw w E -- for that family the field is the whole E."""

    def __init__(self, name, family, weight, fn, fn64, share=1, sign=1):
        self.name, self.family, self.weight, self.fn, self.fn64 = name, family, float(weight), fn, fn64
        self.share, self.sign = share, sign


# ------------------------------------------------------------------------------------ adapters: the extra terms
def stat_term(mu, sd):
    def fn(feat, start, window):
        half, S, _, _ = stat_ref.stat_terms(feat, mu, sd)
        return half, stat_ref.normalized(S)
    return fn


def nnfm_term(bank, k=1, patch=1, cover=0.0):
    """The plain, the 3 x 3 patch, the k best and the cover form, each through its own reference file."""
    def fn(feat, start, window):
        if cover:
            J = nnfm_knn_ref.topk(feat, bank, k, patch)
            E, S, _, _ = nnfm_cover_ref.terms_at(feat, bank, J, nnfm_cover_ref.winners(feat, bank), cover, patch)
        elif k > 1:
            E, S = nnfm_knn_ref.terms(feat, bank, k, patch)[:2]
        elif patch != 1:
            E, S = nnfm_patch_ref.terms(feat, bank, patch)[:2]
        else:
            E, S = nnfm_ref.terms(feat, bank)[:2]
        return E / 2, nnfm_ref.normalized(S)
    return fn


def nnfm_guided_term(bank, seg_rows, maps, k):
    """maps [S, mh, mw]: the segments' mask maps at the layer's scale, rolled in place by ``roll_contents``."""
    def fn(feat, start, window):
        fy, fx, fh, fw = window
        m = nnfm_guided_ref.windows(maps, fy, fx, fh, fw)
        J = nnfm_guided_ref.topk(feat, bank, seg_rows, m, k)
        E, S, _, a = nnfm_guided_ref.terms_at(feat, bank, seg_rows, m, J)
        return E / 2, a * nnfm_ref.normalized(S)
    return fn


def swd_term(V, Tq):
    def fn(feat, start, window):
        half, S, _, _ = swd_ref.terms(feat, V, Tq)
        return half, swd_ref.normalized(S)
    return fn


def selfsim_term(om, layer, points):
    """Reads the window of the layer's first content map, as it lies when the term is evaluated."""
    def fn(feat, start, window):
        fy, fx, fh, fw = window
        E, S = selfsim_ref.terms(feat, om.contents[0][layer][:, fy:fy + fh, fx:fx + fw], points)[:2]
        return 0.5 * E, selfsim_ref.normalized(S)
    return fn


def shift_term(offsets, T):
    def fn(feat, start, window):
        half, S, _ = shift_ref.shift_terms(feat, offsets, T)
        return half, shift_ref.normalized(S)
    return fn


def cx_term(raw_rows, points, eta):
    """The whole E, not half of it: this term's loss is lw w E (``Term``)."""
    mu, B = cx_ref.bank(raw_rows)

    def fn(feat, start, window):
        t = cx_ref.terms(feat, B, mu, points, eta)
        return t.E, cx_ref.normalized(t.S)
    return fn


class MeetOracleModel(OracleModel):
    """``OracleModel`` with
      ``cmask``        {layer: mask map} or None -- every content term acts through it (content_mask_ref),
      ``style_masks``  per style set {layer: mask map} or None (masked_style_ref),
      ``extras``       {layer: [(family, weight, callable)]} -- statistics, nnfm, swd, selfsim, shift, cx terms,
      ``guided_maps``  {layer: [S, mh, mw]} -- the NNFM mask maps that ``nnfm_guided_term`` reads.
    ``roll_contents`` rolls every map of the content picture's frame: content maps, content mask, style masks and
    NNFM masks."""

    def __init__(self, layers, params=None):
        super().__init__(layers, params)
        self.cmask, self.style_masks, self.extras, self.guided_maps = None, [], {}, {}

    # ---- arming
    def set_content_mask(self, M, content_layers):
        self.cmask = None if M is None else {b: mask_map(M, self.scale[b]).astype(np.float32) for b in content_layers}

    def set_style_masks(self, image_masks, style_layers):
        self.style_masks = [None if M is None else {b: mask_map(M, self.scale[b]).astype(np.float32)
                                                    for b in style_layers} for M in image_masks]

    def add_extra(self, layer, family, weight, fn):
        assert family in EXTRA_ORDER
        self.extras.setdefault(layer, []).append((family, float(weight), fn))

    def add_guided(self, layer, weight, bank, seg_rows, masks, k):
        """masks: one [H, W] picture per segment, in the content picture's frame."""
        self.guided_maps[layer] = np.stack([mask_map(np.asarray(m, np.float32), self.scale[layer]) for m in masks])
        self.add_extra(layer, 'nnfm', weight, nnfm_guided_term(bank, seg_rows, self.guided_maps[layer], k))

    def roll_contents(self, xy_pixels):
        super().roll_contents(xy_pixels)
        for b, m in (self.cmask or {}).items():
            roll_xy(m, np.asarray(xy_pixels) // self.scale[b])
        for maps in self.style_masks:
            for b, m in (maps or {}).items():
                roll_xy(m, np.asarray(xy_pixels) // self.scale[b])
        for b, maps in self.guided_maps.items():
            roll_xy(maps, np.asarray(xy_pixels) // self.scale[b])

    # ---- the list of a call's terms
    def _style_mask_of(self, si, b):
        return self.style_masks[si].get(b) if si < len(self.style_masks) and self.style_masks[si] is not None else None

    def terms_of(self, b, content_layers, style_layers, content_weight, style_weight, dd_layers, dd_weight):
        """The terms of layer b in the library's order."""
        out = []
        ones = lambda window: np.ones(window[2:])
        cut = lambda full, window: full[..., window[0]:window[0] + window[2], window[1]:window[1] + window[3]]
        if b in content_layers:
            for ci, content in enumerate(self.contents):
                def fn(feat, start, window, content=content):
                    resid = feat - cut(content[b], window)
                    if self.cmask is None:
                        return half_sq_norm(resid), l1_normalize(resid)
                    m = cut(self.cmask[b], window)
                    assert m.shape == tuple(window[2:]), 'mask window outside the map'
                    return content_mask_ref.masked_content_term32(resid, m)

                def fn64(feat, start, window, content=content):
                    m = ones(window) if self.cmask is None else cut(self.cmask[b], window)
                    return content_mask_ref.masked_content_terms(feat, cut(content[b], window), m)[0]
                out.append(Term('content%d:%s' % (ci, b), 'content', content_weight[b], fn, fn64))
        if b in style_layers:
            for si, style in enumerate(self.styles):
                def fn(feat, start, window, si=si, style=style):
                    full = self._style_mask_of(si, b)
                    if full is None:
                        gdiff = gram_lower(feat) - style[b]
                        sgrad = symm_lower_times(gdiff, feat.reshape(feat.shape[0], -1))
                        return half_sq_norm(gdiff), l1_normalize(sgrad).reshape(feat.shape)
                    m = cut(full, window)
                    assert m.shape == tuple(window[2:]), 'mask window outside the map'
                    return masked_style_ref.masked_style_term32(feat, m, style[b])

                def fn64(feat, start, window, si=si, style=style):
                    full = self._style_mask_of(si, b)
                    m = ones(window) if full is None else cut(full, window)
                    return masked_style_ref.masked_style_terms(feat, m, style[b])[0]
                out.append(Term('style%d:%s' % (si, b), 'style', style_weight[b], fn, fn64, share=len(self.styles)))
        extras = sorted(self.extras.get(b, []), key=lambda t: EXTRA_ORDER.index(t[0]))
        for family, weight, call in extras:
            out.append(Term('%s:%s' % (family, b), family, weight, call,
                            lambda feat, start, window, call=call: call(np.asarray(feat, np.float32), start, window)[0]))
        if b in dd_layers:
            out.append(Term('dream:' + b, 'dream', dd_weight[b],
                            lambda feat, start, window: (half_sq_norm(feat), l1_normalize(feat.copy())),
                            lambda feat, start, window: content_mask_ref.masked_content_terms(
                                feat, np.zeros_like(feat), ones(window))[0], sign=-1))
        return out

    def order_of(self, content_layers, style_layers, dd_layers=()):
        return self.deep_to_shallow(list(content_layers) + list(style_layers) + list(dd_layers) + list(self.extras))

    def _window(self, b, feat, start):
        fy, fx = np.asarray(start) // self.scale[b]
        return int(fy), int(fx), feat.shape[-2], feat.shape[-1]

    def sc_grad_tile(self, tile, start, content_layers, style_layers, layer_weights,
                     content_weight, style_weight, activations=None, dd_layers=(), dd_weight=None, only=None):
        """``oracle.tile_path.OracleModel.sc_grad_tile`` over the one list of terms.  ``only``: the name of the single
        term whose gradient is injected (the loss is then that term's too)."""
        net = self.net
        order = self.order_of(content_layers, style_layers, dd_layers)
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
            window = self._window(b, feat, start)
            for t in self.terms_of(b, content_layers, style_layers, content_weight, style_weight, dd_layers, dd_weight):
                if only is not None and t.name != only:
                    continue
                half, S = t.fn(feat, start, window)
                coef = lw * t.weight / t.share
                value = lw * t.weight * half / t.share
                add = np.float32(coef) * S if S.dtype == np.float32 else np.float32(coef * S)
                if t.sign > 0:
                    loss += value
                    diff += add
                else:
                    loss -= value
                    diff -= add
            if i + 1 == len(order):
                net.backward(start=b)
            else:
                net.backward(start=b, end=order[i + 1])
        return loss, net.blobs['data'].diff[0].copy()

    # ---- the two helpers of the GPU tests
    def term_names(self, content_layers, style_layers, dd_layers=()):
        """[(name, family)] of a call's terms, deepest layer first."""
        zero = {b: 0.0 for b in self.blob_names}
        return [(t.name, t.family) for b in self.order_of(content_layers, style_layers, dd_layers)
                for t in self.terms_of(b, content_layers, style_layers, zero, zero, dd_layers, zero)]

    def loss64(self, acts, start, content_layers, style_layers, layer_weights, content_weight, style_weight,
               dd_layers=(), dd_weight=None):
        """(total, {family: value}, {term: value}): the loss from given activations with every reduction in float64
        (the maps as they are rolled now)."""
        total, families, terms = 0.0, {}, {}
        for b in self.order_of(content_layers, style_layers, dd_layers):
            lw = layer_weights.get(b, 1.0)
            window = self._window(b, acts[b], start)
            for t in self.terms_of(b, content_layers, style_layers, content_weight, style_weight, dd_layers, dd_weight):
                v = t.sign * lw * t.weight * t.fn64(np.asarray(acts[b], np.float64), start, window) / t.share
                terms[t.name] = v
                families[t.family] = families.get(t.family, 0.0) + v
                total += v
        return total, families, terms

    def term_gradients(self, tile, start, content_layers, style_layers, layer_weights, content_weight, style_weight,
                       activations, dd_layers=(), dd_weight=None):
        """{term: its image gradient}.  With the forward pass fixed (``activations``) the backward pass is linear in
        the injected diffs: one oracle backward per term."""
        return {name: self.sc_grad_tile(tile, start, content_layers, style_layers, layer_weights, content_weight,
                                        style_weight, activations=activations, dd_layers=dd_layers,
                                        dd_weight=dd_weight, only=name)[1]
                for name, _ in self.term_names(content_layers, style_layers, dd_layers)}
