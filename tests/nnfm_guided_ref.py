"""Reference arithmetic of the region-guided nearest-neighbour term (--nnfm-masks, stx_set_nnfm_guided_targets) for
the tests, in float64 on float32 inputs.  Blob, unit vectors x_i and lengths r_i are those of tests/nnfm_ref.py.  The
bank B holds S segments, segment s the rows [off_s, off_s + rows_s); m [S, n] are the weights of the columns, the
tile's windows of the segments' mask maps.  For every segment s and column i, with k rows per query:

    J_{i,s} = the k best rows of segment s for x_i       (tests/nnfm_knn_ref.topk on the segment alone: local indices)
    t_{i,s} = (1/k) sum_r b_{J_{i,s,r}},   c_{i,s} = x_i . t_{i,s}
    E   = (2/n) sum_i sum_s m_s(i) (1 - c_{i,s})
    S_i = sum_s m_s(i) ( -(t_{i,s} - c_{i,s} x_i) / r_i )
    a   = sum_i sum_s m_s(i) / n

An index array is J [S, k, n]; where a pair (segment, 128-column block) was not searched it holds -1 and every weight
there is 0, so such entries are never followed.  ``GuidedOracleModel`` is the oracle's tile evaluation with this term
where ``NnfmOracleModel`` has the plain one: loss += lw w E / 2, diff += lw w a S / (sum|S| / (C n) + EPS)."""

import numpy as np

from tests import nnfm_knn_ref, nnfm_ref
from tests.masked_style_ref import mask_map

BLOCK = 128     # columns of a query block


def offsets(seg_rows):
    return np.concatenate([[0], np.cumsum(seg_rows)[:-1]]).astype(np.int64)


def searched(m):
    """[S, blocks]: the pairs (segment, query block) in which some column has m_s > 0."""
    S, n = m.shape
    blocks = -(-n // BLOCK)
    padded = np.zeros((S, blocks * BLOCK))
    padded[:, :n] = m
    return (padded.reshape(S, blocks, BLOCK) > 0).any(axis=2)


def topk(F, B, seg_rows, m, k):
    """J [S, k, n]: per searched pair the lists of the segment alone, -1 elsewhere."""
    S, n = np.shape(m)
    J = np.full((S, k, n), -1, np.int64)
    on = searched(np.asarray(m))
    for s, (off, rows) in enumerate(zip(offsets(seg_rows), seg_rows)):
        own = nnfm_knn_ref.topk(F, np.asarray(B)[off:off + rows], k)
        cols = np.repeat(on[s], BLOCK)[:n]
        J[s][:, cols] = own[:, cols]
    return J


def terms_at(feat, bank, seg_rows, m, J):
    """(E, S [like feat], sum |S|, a) with the lists J [S, k, n] given; m [S, n]."""
    x, r = nnfm_ref.unit_columns(feat)
    b = np.asarray(bank, np.float64)
    m = np.asarray(m, np.float64)
    J = np.asarray(J, np.int64)
    n, k = len(r), J.shape[1]
    inv = np.divide(1.0, r, out=np.zeros_like(r), where=r > 0)
    G = np.zeros_like(x)
    E = 0.0
    for s, (off, rows) in enumerate(zip(offsets(seg_rows), seg_rows)):
        cols = np.flatnonzero(m[s] > 0)
        if not len(cols):
            continue
        lists = J[s][:, cols]
        assert lists.min() >= 0 and lists.max() < rows, 'a weighted column without a valid list in segment %d' % s
        t = b[off + lists[0]]
        for rank in range(1, k):
            t = t + b[off + lists[rank]]
        t = t / k
        c = np.where(r[cols] > 0, (x[cols] * t).sum(axis=1), 0.0)
        E += float((m[s, cols] * (1.0 - c)).sum())
        G[cols] += m[s, cols, None] * (-(t - c[:, None] * x[cols]) * inv[cols, None])
    S = G.T.reshape(np.shape(feat))
    return 2.0 * E / n, S, float(np.abs(S).sum()), float(m.sum()) / n


def half_e(feat, bank, seg_rows, m, J):
    """E / 2 with the lists held (float64: the differences of it between nearby blobs are what the central
    differences of the host test take)."""
    return terms_at(feat, bank, seg_rows, m, J)[0] / 2


def windows(maps, oy, ox, h, w, roll_xy=(0, 0)):
    """m [S, h w]: the windows at (oy, ox) of the maps [S, mh, mw] rolled by roll_xy = (x, y), in the maps' pixels."""
    rolled = np.roll(np.asarray(maps), (int(roll_xy[1]), int(roll_xy[0])), axis=(1, 2))
    return rolled[:, oy:oy + h, ox:ox + w].reshape(len(rolled), h * w)


class GuidedOracleModel(nnfm_ref.NnfmOracleModel):
    """``NnfmOracleModel`` with segments and masks: ``nnfm_segments`` = {layer: seg_rows}, ``nnfm_masks`` = the [H, W]
    pictures (one per segment, in the frame of the targets), ``nnfm_roll`` = (x, y) the shift of the frame,
    ``nnfm_k``, and ``nnfm_index`` = {layer: J [S, k, n]} (the GPU's own lists in the tile tests; searched here
    without).  The parent's evaluation runs with this module's terms and normalisation in place of its own."""

    def __init__(self, layers, params=None):
        super().__init__(layers, params)
        self.nnfm_segments, self.nnfm_masks, self.nnfm_roll, self.nnfm_k, self.nnfm_index = {}, [], (0, 0), 1, {}
        self._start, self._a = (0, 0), 1.0

    def weights_of(self, layer, feat_hw, start):
        scale = self.scale[layer]
        maps = np.stack([mask_map(np.asarray(mask, np.float32), scale) for mask in self.nnfm_masks])
        fy, fx = np.asarray(start) // scale
        roll = (self.nnfm_roll[0] // scale, self.nnfm_roll[1] // scale)
        return windows(maps, int(fy), int(fx), feat_hw[0], feat_hw[1], roll)

    def _terms(self, feat, bank):
        layer = next(b for b in self.nnfm_banks if self.nnfm_banks[b] is bank)
        seg_rows = self.nnfm_segments[layer]
        m = self.weights_of(layer, feat.shape[-2:], self._start)
        J = self.nnfm_index.get(layer)
        if J is None:
            J = topk(feat, bank, seg_rows, m, self.nnfm_k)
        E, S, asum, a = terms_at(feat, bank, seg_rows, m, J)
        self._a = a
        return E, S, asum, None, J

    def nnfm_loss64(self, acts, layer_weights, start=(0, 0)):
        self._start = start
        return sum(layer_weights.get(b, 1.0) * self.nnfm_weights.get(b, 1.0) * self._terms(acts[b], self.nnfm_banks[b])[0] / 2
                   for b in self.nnfm_banks)

    def sc_grad_tile(self, tile, start, *args, **kwargs):
        plain, plain_norm = nnfm_ref.terms, nnfm_ref.normalized
        self._start = start
        nnfm_ref.terms = self._terms
        nnfm_ref.normalized = lambda S: self._a * plain_norm(S)
        try:
            return super().sc_grad_tile(tile, start, *args, **kwargs)
        finally:
            nnfm_ref.terms, nnfm_ref.normalized = plain, plain_norm
