"""Host-side checks of the nearest-neighbour feature matching term (--nnfm-weight): the float64 statement of
its definition (tests/nnfm_ref.py), the options, the refusals and the C ABI.  No GPU."""

from argparse import Namespace
import ctypes

import numpy as np
import pytest

from style_transfer_amd import lib
from style_transfer_amd.config_system import (NNFM_LAYERS_DEFAULT, check_nnfm_options, nnfm_layer_args, nnfm_stride,
                                              parse_args)
from style_transfer_amd.netspec import builtin_net
from tests import nnfm_ref

BASE = ['-ci', 'c.png', '-si', 's.png']


def _planted(seed=0, c=12, h=4, w=5, m=9):
    """A bank of random unit rows and a blob whose column i is a_i b_pi(i) + 1e-3 unit noise: the winner is
    separated from the runner-up."""
    rng = np.random.RandomState(seed)
    B = rng.standard_normal((m, c))
    B /= np.linalg.norm(B, axis=1, keepdims=True)
    pick = rng.randint(0, m, h * w)
    noise = rng.standard_normal((h * w, c))
    noise /= np.linalg.norm(noise, axis=1, keepdims=True)
    cols = 10.0 ** rng.uniform(-2, 3, h * w)[:, None] * B[pick] + 1e-3 * noise
    F = cols.T.reshape(c, h, w)
    scores = np.sort(nnfm_ref.scores64(F, B), axis=1)
    assert np.all(scores[:, -1] - scores[:, -2] > 1e-2)
    return F, B, pick


def test_gradient_is_the_finite_difference_of_half_e():
    """S / n is d(E/2)/dF where the winner does not change: the central difference in float64 agrees to 1e-5 of
    its column's max |S / n|, with steps of 1e-7 |f_i| (the columns' lengths span five decades).  The bound is the
    difference quotient's own error on the columns that lie 1e-6 rad from their winner: the step turns such a
    column by 1e-7 rad, a tenth of that angle, so the third-order term is 1e-2 x 1e-2 / 6 of the slope's
    variation, and the rounding of x - b (2^-53 per component) over a 2e-7 step adds about 1e-6."""
    F, B, pick = _planted()
    E, S, _, _, j = nnfm_ref.terms(F, B)
    assert np.array_equal(j, pick)
    n = F.shape[1] * F.shape[2]
    g = S / n
    r = np.sqrt((F ** 2).sum(axis=0))
    worst = 0.0
    for index in np.ndindex(*F.shape):
        scale = np.abs(g[:, index[1], index[2]]).max()
        fd = nnfm_ref.finite_difference(F, B, index, 1e-7 * r[index[1:]])
        worst = max(worst, abs(fd - g[index]) / scale)
    print('finite difference: %.2e of the column\'s max |S / n|' % worst)
    assert worst <= 1e-5


def test_a_bank_row_taken_from_the_blob_matches_exactly():
    rng = np.random.RandomState(1)
    F = rng.standard_normal((8, 3, 4))
    B = np.concatenate([nnfm_ref.bank_of(rng.standard_normal((8, 2, 2))), nnfm_ref.bank_of(F)])
    E, S, asum, c, j = nnfm_ref.terms(F, B)
    assert np.array_equal(j, 4 + np.arange(12))
    assert np.all(np.abs(c - 1) <= 1e-15) and abs(E) <= 1e-15 and np.abs(S).max() <= 1e-14


def test_scale_invariance():
    F, B, _ = _planted(2)
    E, S, _, _, j = nnfm_ref.terms(F, B)
    for alpha in (0.125, 3.0, 1e4):
        E2, S2, _, _, j2 = nnfm_ref.terms(alpha * F, B)
        assert np.array_equal(j, j2)
        assert E2 == pytest.approx(E, rel=1e-12)
        assert np.allclose(S2, S / alpha, rtol=1e-9, atol=1e-12 * np.abs(S).max() / alpha)


def test_zero_columns_zero_rows_and_ties():
    rng = np.random.RandomState(3)
    F = rng.standard_normal((6, 2, 3))
    F[:, 0, 1] = 0
    B = nnfm_ref.bank_of(rng.standard_normal((6, 2, 2)))
    B = np.concatenate([B, B[1:2], np.zeros((1, 6))])       # row 4 repeats row 1; row 5 is zero
    F[:, 1, 2] = 5 * B[1]
    E, S, asum, c, j = nnfm_ref.terms(F, B)
    assert j[1] == 0 and c[1] == 0 and not S[:, 0, 1].any()
    assert j[5] == 1                                         # the lowest of the equal scores
    assert np.all(np.isfinite(S)) and np.isfinite(E)
    E_at, S_at, _, _ = nnfm_ref.terms_at(F, B, np.where(np.arange(6) == 5, 4, j))
    assert E_at == pytest.approx(E, rel=1e-15) and np.allclose(S_at, S)     # given indices: the copy does as well


def test_bank_stride_and_concatenation_order():
    rng = np.random.RandomState(4)
    maps = [rng.standard_normal((4, 5, 7)), rng.standard_normal((4, 3, 4)), rng.standard_normal((4, 2, 2))]
    for stride in (1, 2, 3):
        parts = [nnfm_ref.bank_of(m, stride) for m in maps]
        for m, p in zip(maps, parts):
            assert p.shape == (nnfm_ref.bank_rows(m.shape[1], m.shape[2], stride), 4)
            picked = m[:, ::stride, ::stride]
            first, last = picked[:, 0, 0], picked[:, -1, -1]
            assert np.allclose(p[0], first / np.linalg.norm(first)) and np.allclose(p[-1], last / np.linalg.norm(last))
            if picked.shape[2] > 1:     # raster order: x first
                assert np.allclose(p[1], picked[:, 0, 1] / np.linalg.norm(picked[:, 0, 1]))
        bank = nnfm_ref.concat_banks(parts)
        assert bank.shape[0] == sum(p.shape[0] for p in parts)      # a union, not an average
        at = 0
        for p in parts:         # two style images and a ladder size: in the order they are processed
            assert np.array_equal(bank[at:at + p.shape[0]], p)
            at += p.shape[0]


def test_the_emulated_search_is_fp32_class():
    rng = np.random.RandomState(5)
    F = rng.standard_normal((64, 5, 7))
    B = nnfm_ref.bank_of(rng.standard_normal((64, 6, 6)))
    err = nnfm_ref.search_error(F, B)
    print('emulated search: worst |score - float64| %.2e' % err)
    assert 0 < err < 1e-6


def test_options_are_absent_unless_set():
    args = parse_args(argv=BASE, config_py=False)
    assert not any(name.startswith('nnfm') for name in vars(args.ns))        # the PNG comment is unchanged
    assert 'nnfm_weight' not in args and 'nnfm_layers' not in args and 'nnfm_stride' not in args
    assert nnfm_layer_args(args) == [] and check_nnfm_options(args) == [] and nnfm_stride(args) == 1
    args = parse_args(argv=BASE + ['--nnfm-weight', '3/2'], config_py=False)
    assert args.nnfm_weight == 1.5 and 'nnfm_layers' not in args and 'nnfm_stride' not in args
    assert nnfm_layer_args(args) == list(NNFM_LAYERS_DEFAULT) == ['conv3_1', 'conv4_1']
    args = parse_args(argv=BASE + ['--nnfm-weight', '0', '--nnfm-layers', 'conv1_1'], config_py=False)
    assert nnfm_layer_args(args) == []                                       # weight 0: off
    args = parse_args(argv=BASE + ['--nnfm-weight', '1', '--nnfm-stride', '2'], config_py=False)
    assert nnfm_stride(args) == 2


def test_layer_weights_go_through_parse_weights():
    from style_transfer_amd.transfer import parse_weights
    args = parse_args(argv=BASE + ['--nnfm-weight', '2', '--nnfm-layers', 'conv3_1:3', 'conv4_1'], config_py=False)
    names, weights = parse_weights(nnfm_layer_args(args), args.nnfm_weight)
    assert names == ['conv3_1', 'conv4_1'] and weights == {'conv3_1': 1.5, 'conv4_1': 0.5}
    assert check_nnfm_options(args, builtin_net('vgg19').blob_names()) == names


def test_every_refusal_of_check_nnfm_options():
    layers = builtin_net('vgg19').blob_names()
    with pytest.raises(ValueError, match='--nnfm-weight.*--style-masks'):
        parse_args(argv=BASE + ['--nnfm-weight', '1', '--style-masks', 'm.png'], config_py=False)
    args = parse_args(argv=BASE + ['--nnfm-weight', '1', '--nnfm-layers', 'conv9_9'], config_py=False)
    with pytest.raises(ValueError, match="--nnfm-layers.*'conv9_9'"):
        check_nnfm_options(args, layers)
    for bad in (['data'], ['conv3_1', 'conv3_1'], ['conv3_1:x'], [':2'], ['conv3_1:0', 'conv4_1:0']):
        with pytest.raises(ValueError, match='--nnfm-layers'):
            check_nnfm_options(Namespace(nnfm_weight=1.0, nnfm_layers=bad), layers)
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match='--nnfm-stride'):
            check_nnfm_options(Namespace(nnfm_weight=1.0, nnfm_stride=bad), layers)
    with pytest.raises(ValueError, match='--nnfm-stride'):
        parse_args(argv=BASE + ['--nnfm-weight', '1', '--nnfm-stride', '0'], config_py=False)
    assert check_nnfm_options(Namespace(nnfm_weight=0, nnfm_layers=['conv9_9'], nnfm_stride=0), layers) == []


def test_refused_before_any_gpu_work():
    from style_transfer_amd.transfer import StyleTransfer
    layers = builtin_net('vgg19').blob_names()
    args = parse_args(argv=BASE + ['--nnfm-weight', '1', '--nnfm-layers', 'conv9_9'], config_py=False)

    class NoFarm:       # (no engine: the refusal comes before anything touches one)
        master = None

        def layers(self):
            return layers
    with pytest.raises(ValueError, match='--nnfm-layers'):
        StyleTransfer(NoFarm(), args, Namespace())
    # ... and the command line refuses it before it wakes a GPU
    from style_transfer_amd import cli
    woken = []
    original = cli.TileFarm
    cli.TileFarm = lambda *a, **k: woken.append(a)
    try:
        with pytest.raises(ValueError, match='--nnfm-layers'):
            cli.main(BASE + ['--model', 'vgg19', '--nnfm-weight', '1', '--nnfm-layers', 'conv9_9'])
    finally:
        cli.TileFarm = original
    assert not woken


def test_dist_refuses_nnfm_weight():
    from style_transfer_amd.dist import broadcast_targets, refuse_unbroadcast_options
    refuse_unbroadcast_options(Namespace())
    refuse_unbroadcast_options(Namespace(nnfm_weight=0))
    with pytest.raises(NotImplementedError, match='--nnfm-weight'):
        refuse_unbroadcast_options(Namespace(nnfm_weight=1.0))
    with pytest.raises(NotImplementedError, match='--nnfm-weight'):
        broadcast_targets([], [], 'cpu', args=Namespace(nnfm_weight=1.0))


def test_abi_symbols_are_present_and_bound():
    so = ctypes.CDLL(lib.LIB_PATH)
    for name in ('stx_set_nnfm_targets', 'stx_nnfm_bank', 'stx_op_nnfm_terms'):
        assert hasattr(so, name) and name in lib.SIGNATURES
    fields = [name for name, _ in lib.NnfmTarget._fields_]
    assert fields == ['layer', 'channels', 'rows', 'bank', 'mem', 'weight']
