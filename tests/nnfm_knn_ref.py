"""Reference arithmetic of the k-nearest form of the nearest-neighbour term (--nnfm-k, stx_set_nnfm_knn_targets)
for the tests, in float64.  Blob, bank, unit vectors x_i and lengths r_i are those of tests/nnfm_ref.py (patch 1)
or tests/nnfm_patch_ref.py (patch 3: X_p, R_p, rows of 9 C).  With K' = min(k, M):

    J_i = (j_i1 ... j_iK')                  the K' rows with the best scores x_i . b_j, by (score descending, index
                                            ascending): among equal scores the lower index first
    t_i = (1/K') sum_r b_{j_ir}
    c_i = x_i . t_i
    E   = (2/n) sum_i (1 - c_i)             ( = the mean over i and r of |x_i - b_{j_ir}|^2 for unit rows )
    S_i = -(t_i - c_i x_i) / r_i            ( = n d(E/2)/d f_i with J_i held fixed; patch 3: folded like G_p )

An index set is an array J [k, n], rank-major, with -1 at the ranks from K' on.  k = 1 is the arithmetic of the two
older references, operation for operation.  ``KnnOracleModel`` is the oracle's tile evaluation with this term where
``NnfmOracleModel`` has its own, at index sets that the caller may give."""

import numpy as np

from tests import nnfm_patch_ref, nnfm_ref


def topk(F, B, k, patch=1):
    """J [k, n]: per query the min(k, M) best rows in rank order, -1 below.  A stable sort of the negated scores
    keeps the lower index first among equal scores."""
    scores = nnfm_patch_ref.scores64(F, B, patch)
    n, m = scores.shape
    order = np.argsort(-scores, axis=1, kind='stable')[:, :k]
    J = np.full((k, n), -1, np.int64)
    J[:min(k, m)] = order.T
    return J


def _rows_of(J):
    """(the ranks that exist [K', n], K')"""
    J = np.asarray(J, np.int64)
    kk = int((J[:, 0] >= 0).sum())
    assert kk >= 1 and np.all(J[:kk] >= 0) and np.all(J[kk:] == -1), 'ranks from K\' on hold -1, for every query'
    return J[:kk], kk


def terms_at(F, B, J, patch=1):
    """(E, S [like F], sum |S|, c [n]) with the index sets J [k, n] given."""
    rows, kk = _rows_of(J)
    x, r = nnfm_patch_ref.unit_patches(F, patch) if patch != 1 else nnfm_ref.unit_columns(F)
    bank = np.asarray(B, np.float64)
    t = bank[rows[0]]
    for rank in range(1, kk):
        t = t + bank[rows[rank]]
    t = t / kk if kk > 1 else t
    c = np.where(r > 0, (x * t).sum(axis=1), 0.0)
    inv = np.divide(1.0, r, out=np.zeros_like(r), where=r > 0)
    G = -(t - c[:, None] * x) * inv[:, None]
    S = nnfm_patch_ref.fold(G, np.shape(F)) if patch != 1 else G.T.reshape(np.shape(F))
    return 2.0 * float((1.0 - c).sum()) / len(r), S, float(np.abs(S).sum()), c


def terms(F, B, k, patch=1):
    """(E, S, sum |S|, c, J) at the reference's own index sets."""
    J = topk(F, B, k, patch)
    return terms_at(F, B, J, patch) + (J,)


def half_e_unit(F, B, k, patch=1, J=None):
    """E / 2 as (1 / 2 n K') sum_i sum_r |x_i - b_{j_ir}|^2: the same number for unit rows, without the cancelled
    1 - c_i.  J: the index sets to hold; None: searched here."""
    rows, kk = _rows_of(topk(F, B, k, patch) if J is None else J)
    x, _ = nnfm_patch_ref.unit_patches(F, patch) if patch != 1 else nnfm_ref.unit_columns(F)
    bank = np.asarray(B, np.float64)
    return sum(float(((x - bank[rows[rank]]) ** 2).sum()) for rank in range(kk)) / (2 * x.shape[0] * kk)


def finite_difference(F, B, index, h, k, patch=1, J=None):
    """Central difference of E / 2 along element ``index`` of F.  J: held fixed on both sides; None: searched anew
    on both sides, as the older references do."""
    plus, minus = np.array(F, np.float64), np.array(F, np.float64)
    plus[index] += h
    minus[index] -= h
    return (half_e_unit(plus, B, k, patch, J) - half_e_unit(minus, B, k, patch, J)) / (2 * h)


class KnnOracleModel(nnfm_ref.NnfmOracleModel):
    """``NnfmOracleModel`` whose term matches ``nnfm_k`` rows of banks of ``nnfm_patch`` x ``nnfm_patch`` patches.
    ``nnfm_index`` = {layer: J [k, n]} holds the index sets of a layer (the GPU's own, in the tile tests); a layer
    without one is searched here.  The term stands where the parent's stands -- the parent's evaluation runs with
    this module's terms in place of its own."""

    def __init__(self, layers, params=None):
        super().__init__(layers, params)
        self.nnfm_k, self.nnfm_patch, self.nnfm_index = 1, 1, {}

    def _terms(self, feat, bank):
        layer = next(b for b in self.nnfm_banks if self.nnfm_banks[b] is bank)
        J = self.nnfm_index.get(layer)
        if J is None:
            J = topk(feat, bank, self.nnfm_k, self.nnfm_patch)
        return terms_at(feat, bank, J, self.nnfm_patch) + (J,)

    def nnfm_loss64(self, acts, layer_weights):
        return sum(layer_weights.get(b, 1.0) * self.nnfm_weights.get(b, 1.0) * self._terms(acts[b], self.nnfm_banks[b])[0] / 2
                   for b in self.nnfm_banks)

    def sc_grad_tile(self, *args, **kwargs):
        plain = nnfm_ref.terms
        nnfm_ref.terms = self._terms
        try:
            return super().sc_grad_tile(*args, **kwargs)
        finally:
            nnfm_ref.terms = plain
