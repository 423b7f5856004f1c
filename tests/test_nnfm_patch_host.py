"""Host-side checks of the 3 x 3 patch form of the nearest-neighbour term (--nnfm-patch 3): the float64
statement of its definition (tests/nnfm_patch_ref.py), the option, the refusals and the C ABI.  No GPU.

Observed: finite differences against S on a 4 x 5 map agree to 8.8e-9 of max |S| (bound 1e-6); the emulated
search's worst error on a 64-channel 5 x 7 map is 4.6e-8 in cosine units."""

from argparse import Namespace
import ctypes

import numpy as np
import pytest

from style_transfer_amd import lib
from style_transfer_amd.config_system import check_nnfm_options, nnfm_bank_rows, nnfm_patch, parse_args
from style_transfer_amd.netspec import builtin_net
from tests import nnfm_patch_ref as ref
from tests import nnfm_ref

BASE = ['-ci', 'c.png', '-si', 's.png']


def test_gradient_is_the_finite_difference_of_half_e():
    """S / n is d(E/2)/dF: C = 8, a 4 x 5 map, 49 bank rows (the patches of a 7 x 7 style map), 30 random elements,
    central differences with the rows searched anew on both sides -- to 1e-6 of max |S / n|."""
    rng = np.random.RandomState(0)
    F = rng.standard_normal((8, 4, 5))
    B = ref.patch_bank_of(rng.standard_normal((8, 7, 7)))
    assert B.shape == (49, 72)
    E, S, asum, c, j = ref.terms(F, B)
    n = 20
    worst = 0.0
    for _ in range(30):
        index = tuple(rng.randint(0, s) for s in F.shape)
        fd = ref.finite_difference(F, B, index, 1e-6)
        worst = max(worst, abs(fd - S[index] / n) / (np.abs(S).max() / n))
    print('patch finite difference: %.2e of max |S|' % worst)
    assert worst <= 1e-6


def test_patch_order_padding_and_fold():
    F = np.arange(2 * 3 * 4, dtype=np.float64).reshape(2, 3, 4) + 1
    P = ref.patches(F)
    assert P.shape == (12, 18)
    centre = 1 * 4 + 2                                   # pixel (1, 2)
    assert np.array_equal(P[centre, 0:2], F[:, 0, 1])    # tap (-1, -1) first, then the channel
    assert np.array_equal(P[centre, 2:4], F[:, 0, 2])    # dx is the inner index
    assert np.array_equal(P[centre, 8:10], F[:, 1, 2])   # the centre is tap 4
    assert np.array_equal(P[centre, 16:18], F[:, 2, 3])
    last_of_row = 0 * 4 + 3                              # pixel (0, 3): its right neighbour is padding,
    assert not P[last_of_row, 10:12].any()               # not pixel (1, 0)
    assert not P[last_of_row, 0:6].any() and np.array_equal(P[last_of_row, 6:8], F[:, 0, 2])
    # fold is the transpose of patches: <patches(F), G> = <F, fold(G)>
    G = np.random.RandomState(1).standard_normal(P.shape)
    assert np.isclose((P * G).sum(), (F * ref.fold(G, F.shape)).sum(), rtol=1e-13)


def test_patch_1_is_the_plain_reference_exactly():
    rng = np.random.RandomState(2)
    F = rng.standard_normal((6, 3, 4))
    B = nnfm_ref.bank_of(rng.standard_normal((6, 4, 4)))
    assert np.array_equal(ref.patch_bank_of(F, 2, patch=1), nnfm_ref.bank_of(F, 2))
    assert np.array_equal(ref.nearest(F, B, patch=1), nnfm_ref.nearest(F, B))
    ours, theirs = ref.terms(F, B, patch=1), nnfm_ref.terms(F, B)
    assert ours[0] == theirs[0] and ours[2] == theirs[2]
    assert all(np.array_equal(a, b) for a, b in zip((ours[1], ours[3], ours[4]), (theirs[1], theirs[3], theirs[4])))
    assert ref.finite_difference(F, B, (1, 2, 3), 1e-6, patch=1) == nnfm_ref.finite_difference(F, B, (1, 2, 3), 1e-6)
    # ... and the generic arithmetic at patch 1 is the same function, to rounding
    assert np.array_equal(ref.patches(F, 1), F.reshape(6, -1).T)


def test_a_bank_of_the_blob_itself_and_zero_patches():
    rng = np.random.RandomState(3)
    F = rng.standard_normal((4, 7, 8))
    F[:, 1:6, 1:6] = 0                                  # a 5 x 5 hole: the patches centred at (2..4, 2..4) are all zero
    B = ref.patch_bank_of(F)
    E, S, asum, c, j = ref.terms(F, B)
    hole = np.array([y * 8 + x for y in (2, 3, 4) for x in (2, 3, 4)])
    others = np.setdiff1d(np.arange(56), hole)
    assert not B[hole].any() and not j[hole].any() and not c[hole].any()
    assert np.array_equal(j[others], others)
    assert np.all(np.abs(c[others] - 1) <= 1e-15) and np.abs(S).max() <= 1e-13
    assert E == pytest.approx(2.0 * 9 / 56, rel=1e-12)  # the zero patches alone: 1 - 0 each


def test_bank_row_counts_and_stride():
    rng = np.random.RandomState(4)
    F = rng.standard_normal((4, 5, 7))
    full = ref.patch_bank_of(F, 1)
    for stride, rows in ((1, 35), (2, 12), (3, 6)):
        bank = ref.patch_bank_of(F, stride)
        assert bank.shape == (rows, 36) and rows == ref.bank_rows(5, 7, stride) == nnfm_bank_rows(4, 5, 7, stride, 3)
        # the stride thins the centres only: the rows are rows of the stride-1 bank
        picked = [y * 7 + x for y in range(0, 5, stride) for x in range(0, 7, stride)]
        assert np.array_equal(bank, full[picked])
    assert np.allclose(np.linalg.norm(full, axis=1), 1)


def test_the_emulated_search_is_fp32_class():
    rng = np.random.RandomState(5)
    F = rng.standard_normal((64, 5, 7)) * 37.0
    B = ref.patch_bank_of(rng.standard_normal((64, 6, 6)))
    scale = ref.common_scale(F)
    top = np.sqrt((F ** 2).sum(axis=0)).max() * scale
    assert 2 ** 12 < top <= 2 ** 13 and ref.common_scale(np.full((1, 1, 1), 4.0)) == 2.0 ** 11
    err = ref.search_error(F, B)
    print('emulated patch search: worst |score - float64| %.2e' % err)
    assert 0 < err < 1e-6


def test_option_is_absent_unless_set():
    args = parse_args(argv=BASE, config_py=False)
    assert not any(name.startswith('nnfm') for name in vars(args.ns)) and 'nnfm_patch' not in args
    assert nnfm_patch(args) == 1
    args = parse_args(argv=BASE + ['--nnfm-weight', '1'], config_py=False)
    assert 'nnfm_patch' not in args and nnfm_patch(args) == 1
    args = parse_args(argv=BASE + ['--nnfm-weight', '1', '--nnfm-patch', '3'], config_py=False)
    assert args.nnfm_patch == 3 and nnfm_patch(args) == 3
    # without --nnfm-weight the option has no effect and is not an error, whatever it holds
    args = parse_args(argv=BASE + ['--nnfm-patch', '2'], config_py=False)
    assert check_nnfm_options(args) == []


def test_every_refused_patch_value():
    layers = builtin_net('vgg19').blob_names()
    for bad in (0, 2, 5, 3.0, True):
        with pytest.raises(ValueError, match='--nnfm-patch'):
            check_nnfm_options(Namespace(nnfm_weight=1.0, nnfm_patch=bad), layers)
        with pytest.raises(ValueError, match='--nnfm-patch'):
            nnfm_patch(Namespace(nnfm_patch=bad))
    for good in (1, 3, np.int64(3)):
        assert check_nnfm_options(Namespace(nnfm_weight=1.0, nnfm_patch=good), layers) == ['conv3_1', 'conv4_1']
    with pytest.raises(ValueError, match='--nnfm-patch'):
        parse_args(argv=BASE + ['--nnfm-weight', '1', '--nnfm-patch', '2'], config_py=False)
    with pytest.raises(SystemExit):         # not an integer: the parser's own refusal
        parse_args(argv=BASE + ['--nnfm-weight', '1', '--nnfm-patch', '3.0'], config_py=False)


def test_precedence_of_config_files(tmp_path):
    """config.py < the command line < --config, like every option."""
    default = tmp_path / 'config.py'
    default.write_text('nnfm_weight = 1.0\nnnfm_patch = 3\n')
    assert nnfm_patch(parse_args(argv=BASE, config_py=default)) == 3
    assert nnfm_patch(parse_args(argv=BASE + ['--nnfm-patch', '1'], config_py=default)) == 1
    late = tmp_path / 'late.py'
    late.write_text('nnfm_patch = 3\n')
    args = parse_args(argv=BASE + ['--nnfm-patch', '1', '--config', str(late)], config_py=default)
    assert nnfm_patch(args) == 3
    bad = tmp_path / 'bad.py'
    bad.write_text('nnfm_patch = 3.0\n')
    with pytest.raises(ValueError, match='--nnfm-patch'):
        parse_args(argv=BASE + ['--config', str(bad)], config_py=default)


def test_the_2_31_refusal_names_the_stride():
    assert nnfm_bank_rows(256, 128, 128, 1, 3) == 16384
    with pytest.raises(ValueError, match='--nnfm-stride') as err:
        nnfm_bank_rows(256, 1024, 1024, 1, 3)           # 2^20 rows of 2304 values
    assert '1048576 rows' in str(err.value) and '2^31' in str(err.value)
    assert nnfm_bank_rows(256, 1024, 1024, 2, 3) == 262144
    with pytest.raises(ValueError, match='--nnfm-stride'):
        nnfm_bank_rows(256, 1024, 1024, 2, 3, rows_before=3 * 262144)       # the concatenation counts
    assert nnfm_bank_rows(256, 4096, 4096, 1, 1) == 4096 * 4096             # the plain bank: the library's own refusal

    class NoEngine:     # (nothing is allocated and no library call is made before the refusal)
        pass

    class DeviceTensor:     # (what _as_arg takes for a tensor on the GPU; never read)
        shape, dtype, is_cuda = (256, 1024, 1024), 'torch.float32', True
        contiguous = lambda self: self
        data_ptr = lambda self: 0
    from style_transfer_amd.engine import TileEngine
    with pytest.raises(ValueError, match='--nnfm-stride'):
        TileEngine.nnfm_bank(NoEngine(), DeviceTensor(), 1, 3)


def test_abi_symbols_are_present_and_bound():
    so = ctypes.CDLL(lib.LIB_PATH)
    header = open(lib.LIB_PATH.rsplit('/style_transfer_amd/', 1)[0] + '/include/stx.h').read()
    for name in ('stx_set_nnfm_patch_targets', 'stx_nnfm_patch_bank', 'stx_op_nnfm_patch_terms'):
        assert hasattr(so, name) and name in lib.SIGNATURES and 'int %s(' % name in header
    fields = [name for name, _ in lib.NnfmPatchTarget._fields_]
    assert fields == ['layer', 'channels', 'patch', 'rows', 'bank', 'mem', 'weight']
    plain = [name for name, _ in lib.NnfmTarget._fields_]
    assert plain == ['layer', 'channels', 'rows', 'bank', 'mem', 'weight']      # its layout stays
