"""Host-side checks of the coverage part of the nearest-neighbour term (--nnfm-cover): the float64 statement of its
definition (tests/nnfm_cover_ref.py), the option, the refusals, the host objects and the C ABI.  No GPU.

The directional-derivative bound.  E_cov / 2 is taken as (1 / 2M) sum_j |x_{i*_j} - b_j|^2, a sum of M C squares of
numbers below 2 with nothing cancelled, so its rounding stays under 1e-15.  Along a random direction dF (standard
normal; columns of length about 8 at C = 64) with the step 1e-5, a column turns by about 1e-5 rad: the third-order
term of the central difference is of the order 1e-10 of the slope, and the quotient's rounding 1e-15 / 2e-5 = 5e-11
against slopes n d(E_cov / 2) of the order 0.1 to 1.  Both lie four decades under the bound of 1e-6 (relative).

Observed: 3.2e-11 .. 2.4e-9 relative over the two bank sizes and three directions each (slopes 0.12 .. 0.89)."""

from argparse import Namespace
import ctypes

import numpy as np
import pytest

from style_transfer_amd import lib
from style_transfer_amd.config_system import check_nnfm_options, nnfm_cover, parse_args
from style_transfer_amd.netspec import builtin_net
from tests import nnfm_cover_ref as ref
from tests import nnfm_knn_ref, nnfm_ref

BASE = ['-ci', 'c.png', '-si', 's.png']
ON = BASE + ['--nnfm-weight', '1']


def _inputs(m, seed=0, c=64, h=5, w=7):
    rng = np.random.RandomState(seed)
    B = rng.standard_normal((m, c))
    B /= np.linalg.norm(B, axis=1, keepdims=True)
    F = rng.standard_normal((c, h, w))
    return F, B, rng


# ------------------------------------------------------------------------------------- the option
def test_option_is_absent_unless_set():
    args = parse_args(argv=BASE, config_py=False)
    assert not any(name.startswith('nnfm') for name in vars(args.ns)) and 'nnfm_cover' not in args
    assert nnfm_cover(args) == 0.0
    args = parse_args(argv=ON, config_py=False)
    assert 'nnfm_cover' not in args and nnfm_cover(args) == 0.0
    for text, value in (('0', 0.0), ('0.5', 0.5), ('2', 2.0), ('1/4', 0.25)):
        args = parse_args(argv=ON + ['--nnfm-cover', text], config_py=False)
        assert args.nnfm_cover == value and nnfm_cover(args) == value and isinstance(nnfm_cover(args), float)
    # without --nnfm-weight the option has no effect and is not an error, whatever it holds
    assert check_nnfm_options(Namespace(nnfm_weight=0.0, nnfm_cover=-1.0)) == []


def test_every_refused_cover():
    layers = builtin_net('vgg19').blob_names()
    for bad in (-1, -0.5, float('nan'), float('inf'), -float('inf'), True, '1', None):
        with pytest.raises(ValueError, match='--nnfm-cover'):
            check_nnfm_options(Namespace(nnfm_weight=1.0, nnfm_cover=bad), layers)
        with pytest.raises(ValueError, match='--nnfm-cover'):
            nnfm_cover(Namespace(nnfm_cover=bad))
    for good in (0, 0.5, 2, np.float32(0.25), np.int64(3)):
        assert check_nnfm_options(Namespace(nnfm_weight=1.0, nnfm_cover=good), layers) == ['conv3_1', 'conv4_1']
        assert nnfm_cover(Namespace(nnfm_cover=good)) == float(good)
    with pytest.raises(ValueError, match='--nnfm-cover'):
        parse_args(argv=ON + ['--nnfm-cover', '-1'], config_py=False)
    for text in ('nan', 'inf', 'much'):         # not a number: the parser's own refusal
        with pytest.raises(SystemExit):
            parse_args(argv=ON + ['--nnfm-cover', text], config_py=False)


def test_cover_with_patch_3_is_refused_and_names_both():
    with pytest.raises(ValueError) as err:
        parse_args(argv=ON + ['--nnfm-cover', '1', '--nnfm-patch', '3'], config_py=False)
    assert '--nnfm-cover' in str(err.value) and '--nnfm-patch' in str(err.value)
    args = parse_args(argv=ON + ['--nnfm-cover', '0', '--nnfm-patch', '3'], config_py=False)
    assert nnfm_cover(args) == 0.0 and args.nnfm_patch == 3
    args = parse_args(argv=ON + ['--nnfm-cover', '1', '--nnfm-patch', '1', '--nnfm-k', '3'], config_py=False)
    assert nnfm_cover(args) == 1.0
    # --style-masks is refused first, as for the stride, the patch and k
    with pytest.raises(ValueError, match='--style-masks'):
        check_nnfm_options(Namespace(nnfm_weight=1.0, nnfm_cover=1.0, nnfm_patch=3, style_masks=['m.png']))
    with pytest.raises(ValueError, match='--style-masks'):
        check_nnfm_options(Namespace(nnfm_weight=1.0, nnfm_cover=-1.0, style_masks=['m.png']))


# ------------------------------------------------------------------------------- the definition
@pytest.mark.parametrize('m', [31, 200])
def test_s_cov_is_the_directional_derivative_of_half_e_cov_with_the_winners_held(m):
    F, B, rng = _inputs(m, seed=m)
    n = 35
    winner = ref.winners(F, B)
    e_cov, s_cov, c = ref.cover_at(F, B, winner)
    assert e_cov / 2 == pytest.approx(ref.half_e_cov_unit(F, B, winner), rel=1e-12)
    for trial in range(3):
        dF = rng.standard_normal(F.shape)
        h = 1e-5
        fd = n * (ref.half_e_cov_unit(F + h * dF, B, winner) - ref.half_e_cov_unit(F - h * dF, B, winner)) / (2 * h)
        slope = float((s_cov * dF).sum())
        print('M %d direction %d: n d(E_cov / 2) %.6g, sum S_cov dF %.6g, relative %.2e'
              % (m, trial, fd, slope, abs(fd / slope - 1)))
        assert abs(fd - slope) <= 1e-6 * abs(slope)


def test_every_bank_row_lies_in_exactly_one_list():
    for m in (31, 200):
        F, B, _ = _inputs(m, seed=1)
        winner = ref.winners(F, B)
        lists = ref.lists_of(winner, 35)
        assert len(lists) == 35 and sorted(np.concatenate(lists)) == list(range(m))
        assert all(np.all(np.diff(rows) > 0) for rows in lists)
        assert all(np.all(winner[rows] == i) for i, rows in enumerate(lists))
    assert max(len(rows) for rows in lists) > 1         # 200 rows on 35 columns: some column owns several


def test_exact_multiples_of_columns_cost_nothing():
    F, _, rng = _inputs(3, seed=2)
    x, _ = nnfm_ref.unit_columns(F)
    B = x[rng.randint(0, 35, 50)]           # every row is a column's own direction
    winner = ref.winners(F, B)
    e_cov, s_cov, c = ref.cover_at(F, B, winner)
    assert abs(e_cov) < 1e-14 and np.abs(s_cov).max() < 1e-14 * np.abs(nnfm_knn_ref.terms(F, B, 1)[1]).max() + 1e-15
    assert np.allclose(c, 1.0, rtol=0, atol=1e-14)


def test_zero_bank_rows_add_two_over_m_each_and_nothing_to_s():
    F, B, _ = _inputs(31, seed=3)
    with_zero = np.concatenate([B[:10], np.zeros((2, 64)), B[10:], np.zeros((1, 64))])
    winner = ref.winners(F, with_zero)
    zero = [10, 11, 33]
    assert list(winner[zero]) == [0, 0, 0]          # every column scores 0: the lowest
    e_cov, s_cov, c = ref.cover_at(F, with_zero, winner)
    live = np.delete(np.arange(34), zero)
    e_live, s_live, _ = ref.cover_at(F, with_zero[live], winner[live])
    assert e_cov == pytest.approx((31 * e_live + 2 * 3) / 34, rel=1e-13)
    assert np.allclose(s_cov, s_live * 31 / 34, rtol=1e-13, atol=1e-18) and not c[zero].any()


def test_a_zero_column_that_wins_costs_one_and_has_no_gradient():
    F, B, _ = _inputs(31, seed=4)
    F = np.abs(F)                       # every live column has positive entries only ...
    F[:, 2, 3] = 0
    B[5] = -np.abs(B[5])                # ... so this row scores below 0 on all of them, and 0 on the zero column
    i = 2 * 7 + 3
    winner = ref.winners(F, B)
    assert winner[5] == i and np.count_nonzero(winner == i) == 1
    e_cov, s_cov, c = ref.cover_at(F, B, winner)
    assert c[5] == 0 and not s_cov[:, 2, 3].any() and np.all(np.isfinite(s_cov))
    others = np.delete(np.arange(31), 5)
    e_rest, s_rest, _ = ref.cover_at(F, B[others], winner[others])
    assert e_cov == pytest.approx((30 * e_rest + 2 * (1 - 0)) / 31, rel=1e-13)
    assert np.allclose(s_cov, s_rest * 30 / 31, rtol=1e-13, atol=1e-18)


def test_cover_0_is_the_knn_reference_and_the_sum_has_one_normalisation():
    F, B, _ = _inputs(31, seed=5)
    J = nnfm_knn_ref.topk(F, B, 3)
    winner = ref.winners(F, B)
    off = ref.terms_at(F, B, J, winner, 0.0)
    fwd = nnfm_knn_ref.terms_at(F, B, J)
    assert off[0] == fwd[0] and np.array_equal(off[1], fwd[1]) and off[2] == fwd[2] and off[3] == 0.0
    on = ref.terms_at(F, B, J, winner, 0.5)
    e_cov, s_cov, _ = ref.cover_at(F, B, winner)
    assert on[0] == fwd[0] + 0.5 * e_cov and on[3] == e_cov
    assert np.array_equal(on[1], fwd[1] + 0.5 * s_cov) and on[2] == np.abs(on[1]).sum()


# ---------------------------------------------------------------------------- the host objects
class _FakeFarm:
    def __init__(self):
        self.calls = []

    def set_nnfm_targets(self, *args):
        self.calls.append(args)


def _banks_term(extra, capsys=None):
    from style_transfer_amd.terms import NnfmBanks
    args = parse_args(argv=ON + ['--nnfm-layers', 'conv3_1'] + extra, config_py=False)
    farm = _FakeFarm()
    st = Namespace(args=args, farm=farm, engine=Namespace(concat_rows=lambda parts: parts[0]))
    term = NnfmBanks()
    term.read(st)
    term.begin()
    term._parts['conv3_1'].append(np.ones((12, 64), np.float32))
    term.finish(st, 1, False)
    term.send(st)
    return term, farm


def test_nnfm_banks_pass_cover_to_the_farm_and_print_it(capsys):
    term, farm = _banks_term(['--nnfm-cover', '0.5', '--nnfm-k', '2'])
    assert term.cover == 0.5 and len(farm.calls) == 1
    targets, weights, patch, k, cover = farm.calls[0]
    assert list(targets) == ['conv3_1'] and (patch, k, cover) == (1, 2, 0.5)
    assert capsys.readouterr().out == 'NNFM bank rows: conv3_1 12; k 2; cover 0.5\n'
    term, farm = _banks_term(['--nnfm-cover', '1'])
    assert farm.calls[0][2:] == (1, 1, 1.0)
    assert capsys.readouterr().out == 'NNFM bank rows: conv3_1 12; cover 1\n'
    # absent, or 0: the call and the line of before
    for extra in ([], ['--nnfm-cover', '0']):
        term, farm = _banks_term(extra)
        assert term.cover == 0.0 and len(farm.calls[0]) == 4 and farm.calls[0][2:] == (1, 1)
        assert capsys.readouterr().out == 'NNFM bank rows: conv3_1 12\n'


class _Recorder:
    """What TileEngine.set_nnfm_targets needs of an engine, with the library call recorded instead of made."""

    def __init__(self, monkeypatch):
        self.calls = []
        self.handle = None
        self.primary = Namespace(extra_taps={})
        monkeypatch.setattr(lib, 'call', lambda name, handle, table, n: self.calls.append((name, type(table[0]), table[0], n)))

    def _cstr(self, text):
        return text.encode()


def test_engine_makes_the_new_call_only_with_a_cover(monkeypatch):
    from style_transfer_amd.engine import TileEngine
    rec = _Recorder(monkeypatch)
    bank = np.ones((5, 64), np.float32)
    TileEngine.set_nnfm_targets(rec, {'conv1_1': bank}, {'conv1_1': 0.5}, 1, 1, 0.0)
    TileEngine.set_nnfm_targets(rec, {'conv1_1': bank}, {'conv1_1': 0.5}, 1, 3, cover=0)
    TileEngine.set_nnfm_targets(rec, {'conv1_1': bank}, None, 1, 3, 0.25)
    TileEngine.set_nnfm_targets(rec, {'conv1_1': bank}, None, cover=2)
    assert [c[0] for c in rec.calls] == ['stx_set_nnfm_patch_targets', 'stx_set_nnfm_knn_targets'] + \
        ['stx_set_nnfm_cover_targets'] * 2
    assert rec.calls[2][1] is lib.NnfmCoverTarget
    t = rec.calls[2][2]
    assert (t.layer, t.channels, t.patch, t.k, t.rows, t.weight, t.cover) == (b'conv1_1', 64, 1, 3, 5, 1.0, 0.25)
    t = rec.calls[3][2]
    assert (t.patch, t.k, t.cover) == (1, 1, 2.0)
    for bad in (-1, float('nan'), float('inf'), True, '1'):
        with pytest.raises(ValueError, match='cover'):
            TileEngine.set_nnfm_targets(rec, {'conv1_1': bank}, None, 1, 1, bad)
    with pytest.raises(ValueError, match='patch'):
        TileEngine.set_nnfm_targets(rec, {'conv1_1': np.ones((5, 9 * 64), np.float32)}, None, 3, 1, 1.0)
    assert len(rec.calls) == 4


def test_abi_symbols_are_present_and_bound():
    so = ctypes.CDLL(lib.LIB_PATH)
    header = open(lib.LIB_PATH.rsplit('/style_transfer_amd/', 1)[0] + '/include/stx.h').read()
    for name in ('stx_set_nnfm_cover_targets', 'stx_op_nnfm_cover_terms'):
        assert hasattr(so, name) and name in lib.SIGNATURES and 'int %s(' % name in header
    assert 'stx_nnfm_cover_target;' in header
    fields = [name for name, _ in lib.NnfmCoverTarget._fields_]
    assert fields == [name for name, _ in lib.NnfmKnnTarget._fields_] + ['cover']
    assert dict(lib.NnfmCoverTarget._fields_)['cover'] is ctypes.c_float
    # the knn call plus the factor and the winners
    assert len(lib.SIGNATURES['stx_op_nnfm_cover_terms']) == len(lib.SIGNATURES['stx_op_nnfm_knn_terms']) + 2
