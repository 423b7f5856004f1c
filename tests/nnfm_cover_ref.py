"""Reference arithmetic of the coverage part of the nearest-neighbour term (--nnfm-cover,
stx_set_nnfm_cover_targets) for the tests, in float64.  Blob, bank, unit columns x_i and lengths r_i are those of
tests/nnfm_ref.py; the forward part E_fwd, S_fwd is tests/nnfm_knn_ref.py's at index sets J [k, n].  With M bank
rows, n columns and lambda = cover:

    i*_j    = argmax_i x_i . b_j                     (the LOWEST i among equal scores; a zero column scores 0)
    c'_j    = x_{i*_j} . b_j
    E_cov   = (2/M) sum_j (1 - c'_j)
    S_cov,i = -(n/M) sum_{j : i*_j = i} (b_j - c'_j x_i) / r_i        (0 for r_i = 0)
    E = E_fwd + lambda E_cov,   S = S_fwd + lambda S_cov

``CoverOracleModel`` is the oracle's tile evaluation with this term where ``KnnOracleModel`` has its own, at index
sets and winners that the caller may give."""

import numpy as np

from tests import nnfm_knn_ref, nnfm_ref


def winners(feat, bank):
    """i* [M]: per bank row the float64 argmax over the columns, the lowest i among equal scores (numpy's argmax
    takes the first)."""
    return np.argmax(nnfm_ref.scores64(feat, bank), axis=0).astype(np.int64)


def lists_of(winner, n):
    """The inverted index: per column the rows that it won, ascending."""
    winner = np.asarray(winner, np.int64)
    return [np.flatnonzero(winner == i) for i in range(n)]


def cover_at(feat, bank, winner):
    """(E_cov, S_cov [like feat], c' [M]) with the winners given."""
    x, r = nnfm_ref.unit_columns(feat)
    b = np.asarray(bank, np.float64)
    winner = np.asarray(winner, np.int64)
    n, m = len(r), len(b)
    xw = x[winner]
    c = (xw * b).sum(axis=1)
    G = np.zeros_like(x)
    np.add.at(G, winner, b - c[:, None] * xw)
    inv = np.divide(1.0, r, out=np.zeros_like(r), where=r > 0)
    S = -(n / m) * G * inv[:, None]
    return 2.0 * float((1.0 - c).sum()) / m, S.T.reshape(np.shape(feat)), c


def terms_at(feat, bank, J, winner, cover, patch=1):
    """(E, S [like feat], sum |S|, E_cov) of the whole term with the index sets J [k, n] and the winners [M] given."""
    assert patch == 1 or cover == 0, 'the coverage part has no patch form'
    e_fwd, s_fwd, _, _ = nnfm_knn_ref.terms_at(feat, bank, J, patch)
    if cover == 0:
        return e_fwd, s_fwd, float(np.abs(s_fwd).sum()), 0.0
    e_cov, s_cov, _ = cover_at(feat, bank, winner)
    S = s_fwd + cover * s_cov
    return e_fwd + cover * e_cov, S, float(np.abs(S).sum()), e_cov


def half_e_cov_unit(feat, bank, winner):
    """E_cov / 2 as (1 / 2M) sum_j |x_{i*_j} - b_j|^2: the same number for unit rows on live columns, without the
    cancelled 1 - c'_j (for differences between two nearby blobs, the winners held)."""
    x, _ = nnfm_ref.unit_columns(feat)
    b = np.asarray(bank, np.float64)
    return float(((x[np.asarray(winner, np.int64)] - b) ** 2).sum()) / (2 * len(b))


class CoverOracleModel(nnfm_knn_ref.KnnOracleModel):
    """``KnnOracleModel`` with the coverage part at factor ``nnfm_cover``; ``nnfm_winner`` = {layer: i* [M]} holds
    the winners of a layer (the GPU's own, in the tile tests); a layer without them is searched here."""

    def __init__(self, layers, params=None):
        super().__init__(layers, params)
        self.nnfm_cover, self.nnfm_winner = 0.0, {}

    def _terms(self, feat, bank):
        layer = next(b for b in self.nnfm_banks if self.nnfm_banks[b] is bank)
        J = self.nnfm_index.get(layer)
        if J is None:
            J = nnfm_knn_ref.topk(feat, bank, self.nnfm_k, self.nnfm_patch)
        winner = self.nnfm_winner.get(layer)
        if winner is None and self.nnfm_cover:
            winner = winners(feat, bank)
        return terms_at(feat, bank, J, winner, self.nnfm_cover, self.nnfm_patch) + (J,)
