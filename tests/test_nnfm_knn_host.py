"""Host-side checks of the k-nearest form of the nearest-neighbour term (--nnfm-k): the float64 statement of its
definition (tests/nnfm_knn_ref.py), the option, the refusals and the C ABI.  No GPU.

The finite-difference bound.  E / 2 is taken as the mean of |x_i - b_{j_ir}|^2 / 2, a sum of n K' C squares of
numbers near 1 with nothing cancelled: below 2, so its rounding stays under 1e-14.  The step is 1e-7 |f_i| (patch
3: 1e-7 R_p of the pixel's own patch, the length that r_i becomes there), so the quotient carries at most 1e-14 /
(2e-7 |f_i|) = 5e-8 / |f_i|, while the slope's scale is max |S_i| / n = O(1) / (n |f_i|) = 0.05 / |f_i| on the
20-pixel maps: 1e-6 of that scale.  The third-order term of a central difference
over a turn of 1e-7 rad is of the order 1e-14 and does not count.  (A column here is nowhere near its target -- the
mean of several rows is not a unit vector -- so no near-winner allowance is needed.)

Observed: 1.0e-7 .. 1.8e-7 of the column's max |S / n| at worst over the four settings."""

from argparse import Namespace
import ctypes

import numpy as np
import pytest

from style_transfer_amd import lib
from style_transfer_amd.config_system import check_nnfm_options, nnfm_k, parse_args
from style_transfer_amd.netspec import builtin_net
from tests import nnfm_knn_ref as ref
from tests import nnfm_patch_ref, nnfm_ref

BASE = ['-ci', 'c.png', '-si', 's.png']


def _inputs(patch, seed=0, c=12, h=4, w=5, m=9):
    """The shapes of tests/test_nnfm_host.py: C = 12, a 4 x 5 map, 9 unit bank rows; columns over five decades."""
    rng = np.random.RandomState(seed)
    B = rng.standard_normal((m, patch * patch * c))
    B /= np.linalg.norm(B, axis=1, keepdims=True)
    F = rng.standard_normal((c, h, w)) * 10.0 ** rng.uniform(-2, 3, (h, w))
    return F, B


@pytest.mark.parametrize('patch', [1, 3])
@pytest.mark.parametrize('k', [2, 4])
def test_gradient_is_the_finite_difference_of_half_e_with_the_sets_held(k, patch):
    F, B = _inputs(patch, seed=k + patch)
    E, S, asum, c, J = ref.terms(F, B, k, patch)
    assert J.shape == (k, 20) and J.min() >= 0
    n = 20
    g = S / n
    # the length that the step is a fraction of: |f_i|, and R_p of the pixel's own patch in the patch form
    r = (nnfm_patch_ref.unit_patches(F, patch)[1] if patch != 1 else nnfm_ref.unit_columns(F)[1]).reshape(F.shape[1:])
    worst = 0.0
    for index in np.ndindex(*F.shape):
        scale = np.abs(g[:, index[1], index[2]]).max()
        fd = ref.finite_difference(F, B, index, 1e-7 * r[index[1:]], k, patch, J)
        worst = max(worst, abs(fd - g[index]) / scale)
    print('k %d patch %d finite difference: %.2e of the column\'s max |S / n|' % (k, patch, worst))
    assert worst <= 1e-6
    # E is the mean over i and r of |x_i - b_{j_ir}|^2
    assert E / 2 == pytest.approx(ref.half_e_unit(F, B, k, patch), rel=1e-12)


@pytest.mark.parametrize('patch', [1, 3])
def test_k_1_is_the_older_references_exactly(patch):
    F, B = _inputs(patch, seed=5)
    ours, theirs = ref.terms(F, B, 1, patch), nnfm_patch_ref.terms(F, B, patch)
    if patch == 1:
        plain = nnfm_ref.terms(F, B)
        assert plain[0] == ours[0] and np.array_equal(plain[1], ours[1])
    assert ours[0] == theirs[0] and ours[2] == theirs[2]
    assert np.array_equal(ours[1], theirs[1]) and np.array_equal(ours[3], theirs[3])
    assert ours[4].shape == (1, 20) and np.array_equal(ours[4][0], theirs[4])
    assert ref.half_e_unit(F, B, 1, patch) == nnfm_patch_ref.half_e_unit(F, B, patch)
    index = (1, 2, 3)
    assert ref.finite_difference(F, B, index, 1e-6, 1, patch) == nnfm_patch_ref.finite_difference(F, B, index, 1e-6, patch)


def test_fewer_rows_than_k_uses_the_rows_there_are():
    F, B = _inputs(1, seed=6, m=3)
    J = ref.topk(F, B, 4)
    assert J.shape == (4, 20) and np.all(J[3] == -1) and np.all(J[:3] >= 0)
    assert np.array_equal(np.sort(J[:3], axis=0), np.tile(np.arange(3)[:, None], (1, 20)))
    assert np.array_equal(J[:3], ref.topk(F, B, 3))
    four, three = ref.terms_at(F, B, J), ref.terms_at(F, B, J[:3])
    assert four[0] == three[0] and np.array_equal(four[1], three[1])
    # the target is the mean of the three rows, whatever their order
    x, _ = nnfm_ref.unit_columns(F)
    assert np.allclose(four[3], x @ B.mean(axis=0), rtol=1e-13, atol=1e-15)


def test_duplicated_rows_come_lowest_index_first():
    F, B = _inputs(1, seed=7)
    B[6] = B[2]
    B[8] = B[2]
    F[:, 0, 0] = 3.0 * B[2]             # scores 1 on the rows 2, 6, 8, exactly equal
    J = ref.topk(F, B, 4)
    assert list(J[:3, 0]) == [2, 6, 8] and J[3, 0] not in (2, 6, 8)
    assert list(ref.topk(F, B, 2)[:, 0]) == [2, 6]
    scores = nnfm_ref.scores64(F, B)
    for i in range(20):                 # every query: descending scores, ascending indices among equals
        s = scores[i, J[:, i]]
        assert np.all(np.diff(s) <= 0)
        assert all(J[a, i] < J[a + 1, i] for a in range(3) if s[a] == s[a + 1])


@pytest.mark.parametrize('patch', [1, 3])
def test_a_zero_column_takes_the_first_rows(patch):
    F, B = _inputs(patch, seed=8)
    if patch == 1:
        F[:, 1, 2] = 0
    else:
        F[:, 0:3, 1:4] = 0              # the patch centred at (1, 2) is all zero
    E, S, asum, c, J = ref.terms(F, B, 3, patch)
    i = 1 * 5 + 2
    assert list(J[:, i]) == [0, 1, 2] and c[i] == 0
    assert np.all(np.isfinite(S))
    if patch == 1:
        assert not S[:, 1, 2].any()
    else:                               # S there is what the eight live patches around it add, without its own
        rows, _ = ref._rows_of(J)
        x, r = nnfm_patch_ref.unit_patches(F)
        G = -(B[rows].mean(axis=0) - c[:, None] * x) / np.where(r > 0, r, np.inf)[:, None]
        assert not G[i].any() and np.allclose(S, nnfm_patch_ref.fold(G, F.shape), rtol=1e-12, atol=1e-18)


def test_option_is_absent_unless_set():
    args = parse_args(argv=BASE, config_py=False)
    assert not any(name.startswith('nnfm') for name in vars(args.ns)) and 'nnfm_k' not in args
    assert nnfm_k(args) == 1
    args = parse_args(argv=BASE + ['--nnfm-weight', '1'], config_py=False)
    assert 'nnfm_k' not in args and nnfm_k(args) == 1
    args = parse_args(argv=BASE + ['--nnfm-weight', '1', '--nnfm-k', '3'], config_py=False)
    assert args.nnfm_k == 3 and nnfm_k(args) == 3
    # without --nnfm-weight the option has no effect and is not an error, whatever it holds
    args = parse_args(argv=BASE + ['--nnfm-k', '9'], config_py=False)
    assert check_nnfm_options(args) == []
    assert check_nnfm_options(Namespace(nnfm_weight=0.0, nnfm_k=True)) == []


def test_every_refused_k():
    layers = builtin_net('vgg19').blob_names()
    for bad in (0, 5, True, 2.0, '2', -1):
        with pytest.raises(ValueError, match='--nnfm-k'):
            check_nnfm_options(Namespace(nnfm_weight=1.0, nnfm_k=bad), layers)
        with pytest.raises(ValueError, match='--nnfm-k'):
            nnfm_k(Namespace(nnfm_k=bad))
    for good in (1, 2, 3, 4, np.int64(4)):
        assert check_nnfm_options(Namespace(nnfm_weight=1.0, nnfm_k=good), layers) == ['conv3_1', 'conv4_1']
        assert nnfm_k(Namespace(nnfm_k=good)) == int(good)
    with pytest.raises(ValueError, match='--nnfm-k'):
        parse_args(argv=BASE + ['--nnfm-weight', '1', '--nnfm-k', '5'], config_py=False)
    with pytest.raises(SystemExit):         # not an integer: the parser's own refusal
        parse_args(argv=BASE + ['--nnfm-weight', '1', '--nnfm-k', '2.0'], config_py=False)
    # --style-masks is refused first, as for the stride and the patch
    with pytest.raises(ValueError, match='--style-masks'):
        check_nnfm_options(Namespace(nnfm_weight=1.0, nnfm_k=2, style_masks=['m.png']), layers)


def test_precedence_of_config_files(tmp_path):
    """config.py < the command line < --config, like every option."""
    default = tmp_path / 'config.py'
    default.write_text('nnfm_weight = 1.0\nnnfm_k = 4\n')
    assert nnfm_k(parse_args(argv=BASE, config_py=default)) == 4
    assert nnfm_k(parse_args(argv=BASE + ['--nnfm-k', '2'], config_py=default)) == 2
    late = tmp_path / 'late.py'
    late.write_text('nnfm_k = 3\n')
    args = parse_args(argv=BASE + ['--nnfm-k', '2', '--config', str(late)], config_py=default)
    assert nnfm_k(args) == 3
    bad = tmp_path / 'bad.py'
    bad.write_text('nnfm_k = 2.0\n')
    with pytest.raises(ValueError, match='--nnfm-k'):
        parse_args(argv=BASE + ['--config', str(bad)], config_py=default)


class _Recorder:
    """What TileEngine.set_nnfm_targets needs of an engine, with the library call recorded instead of made."""

    def __init__(self, monkeypatch):
        self.calls = []
        self.handle = None
        self.primary = Namespace(extra_taps={})
        monkeypatch.setattr(lib, 'call', lambda name, handle, table, n: self.calls.append((name, type(table[0]), table[0], n)))

    def _cstr(self, text):
        return text.encode()


def test_k_1_makes_the_calls_of_today_and_k_above_1_the_new_one(monkeypatch):
    from style_transfer_amd.engine import TileEngine
    rec = _Recorder(monkeypatch)
    bank = np.ones((5, 64), np.float32)
    TileEngine.set_nnfm_targets(rec, {'conv1_1': bank}, {'conv1_1': 0.5})
    TileEngine.set_nnfm_targets(rec, {'conv1_1': bank}, {'conv1_1': 0.5}, 1, 1)
    TileEngine.set_nnfm_targets(rec, {'conv1_1': np.ones((5, 9 * 64), np.float32)}, None, 3, k=4)
    assert [c[0] for c in rec.calls] == ['stx_set_nnfm_patch_targets'] * 2 + ['stx_set_nnfm_knn_targets']
    assert rec.calls[0][1] is lib.NnfmPatchTarget and rec.calls[2][1] is lib.NnfmKnnTarget
    t = rec.calls[2][2]
    assert (t.layer, t.channels, t.patch, t.k, t.rows, t.weight) == (b'conv1_1', 64, 3, 4, 5, 1.0)
    for bad in (0, 5, True, 2.0):
        with pytest.raises(ValueError, match='k '):
            TileEngine.set_nnfm_targets(rec, {'conv1_1': bank}, None, 1, bad)
    assert len(rec.calls) == 3


def test_abi_symbols_are_present_and_bound():
    so = ctypes.CDLL(lib.LIB_PATH)
    header = open(lib.LIB_PATH.rsplit('/style_transfer_amd/', 1)[0] + '/include/stx.h').read()
    for name in ('stx_set_nnfm_knn_targets', 'stx_op_nnfm_knn_terms'):
        assert hasattr(so, name) and name in lib.SIGNATURES and 'int %s(' % name in header
    assert 'stx_nnfm_knn_target;' in header
    fields = [name for name, _ in lib.NnfmKnnTarget._fields_]
    assert fields == ['layer', 'channels', 'patch', 'k', 'rows', 'bank', 'mem', 'weight']
    assert len(lib.SIGNATURES['stx_op_nnfm_knn_terms']) == len(lib.SIGNATURES['stx_op_nnfm_patch_terms']) + 1
    # the older layouts stay
    assert [name for name, _ in lib.NnfmPatchTarget._fields_] == ['layer', 'channels', 'patch', 'rows', 'bank', 'mem', 'weight']
