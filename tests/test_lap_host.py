"""The Laplacian loss without a GPU: the float64 reference against central differences, the
symmetry of D, the two options, and the three exported symbols."""

import ctypes

import numpy as np
import pytest

from style_transfer_amd import lib
from style_transfer_amd.config_system import check_lap_pools, parse_args
from tests import lap_ref

BASE = ['-ci', 'c', '-si', 's']


def test_reference_gradient_against_central_differences():
    rng = np.random.RandomState(0)
    img = rng.uniform(-120, 130, (3, 11, 13))
    content = rng.uniform(-120, 130, (3, 11, 13))
    pools, weights = [1, 4], [0.3, 0.7]
    loss, grad, targets = lap_ref.lap_loss(img, content, pools, weights, scale=2.5)
    assert loss > 0 and [t.shape for t in targets] == [(11, 13), (3, 4)]
    worst = 0.0
    for index in [(0, 0, 0), (1, 5, 6), (2, 10, 12), (0, 3, 12), (1, 10, 0), (2, 7, 7), (0, 4, 4), (1, 8, 3)]:
        h = 1e-3
        up, down = img.copy(), img.copy()
        up[index] += h
        down[index] -= h
        numeric = (lap_ref.lap_loss(up, content, pools, weights, 2.5)[0] -
                   lap_ref.lap_loss(down, content, pools, weights, 2.5)[0]) / (2 * h)
        worst = max(worst, abs(numeric - grad[index]) / np.abs(grad).max())
    print('central differences: worst error / max|grad| = %.3g' % worst)
    assert worst < 1e-7          # the loss is quadratic: central differences are exact up to rounding
    assert np.array_equal(grad[0], grad[1]) and np.array_equal(grad[0], grad[2])
    # the image itself as content: nothing to pull at
    loss0, grad0, _ = lap_ref.lap_loss(img, img, pools, weights)
    assert loss0 == 0.0 and not grad0.any()


@pytest.mark.parametrize('hw', [(1, 1), (1, 7), (5, 1), (6, 9)])
def test_d_is_symmetric_and_kills_constants(hw):
    rng = np.random.RandomState(hw[0] + hw[1])
    a, b = rng.normal(size=hw), rng.normal(size=hw)
    assert abs(np.sum(lap_ref.lap(a) * b) - np.sum(a * lap_ref.lap(b))) <= 1e-12 * np.abs(a).sum() * np.abs(b).max() * 8
    assert not lap_ref.lap(np.full(hw, 3.25)).any()
    assert np.all(np.abs(lap_ref.lap(a)) <= lap_ref.abs_lap(np.abs(a)) + 1e-15)


def test_pooling_is_block_means_over_the_pixels_that_exist():
    plane = np.arange(7 * 10, dtype=np.float64).reshape(7, 10)
    got = lap_ref.pool(plane, 4)
    assert got.shape == (2, 3)
    for i in range(2):
        for j in range(3):
            assert got[i, j] == plane[4 * i:4 * i + 4, 4 * j:4 * j + 4].mean()
    assert np.array_equal(lap_ref.cell_counts(7, 10, 4), [[16, 16, 8], [12, 12, 6]])
    assert np.array_equal(lap_ref.pool(plane, 1), plane)


def test_options_are_absent_unless_given():
    args = parse_args(None, BASE, config_py=False)
    assert 'lap_weight' not in args and 'lap_pools' not in args
    assert not hasattr(args, 'lap_weight') and getattr(args, 'lap_weight', 0) == 0
    assert check_lap_pools(args) == []
    args = parse_args(None, BASE + ['--lap-weight', '1/2'], config_py=False)
    assert args.lap_weight == 0.5 and 'lap_pools' not in args
    assert check_lap_pools(args) == [4]                      # the default when the weight is set
    args = parse_args(None, BASE + ['--lap-weight', '30', '--lap-pools', '4', '16:3'], config_py=False)
    assert args.lap_pools == ['4', '16:3'] and check_lap_pools(args) == [4, 16]


@pytest.mark.parametrize('pools', [['3'], ['128'], ['0'], ['-4'], ['four'], ['4:x'], ['1', '2', '4', '8', '16'],
                                   ['4', '16', '4:2']])
def test_bad_pool_sizes_are_refused_before_any_gpu_work(pools):
    with pytest.raises(ValueError) as err:
        parse_args(None, BASE + ['--lap-weight', '5', '--lap-pools'] + pools, config_py=False)
    assert '--lap-pools' in str(err.value)


def test_weights_normalise_to_lap_weight():
    from style_transfer_amd.transfer import lap_pool_weights
    pools, weights = lap_pool_weights(['4', '16:3'], 30)
    assert pools == [4, 16] and weights == [7.5, 22.5]
    pools, weights = lap_pool_weights(['8'], 0.25)
    assert pools == [8] and weights == [0.25]
    pools, weights = lap_pool_weights(['1:1/2', '64:-1.5', '2'], 6)
    assert pools == [1, 64, 2] and np.allclose(weights, [1, -3, 2]) and abs(np.abs(weights).sum() - 6) < 1e-12


def test_the_pool_sizes_of_the_target_hold_for_the_run():
    """The target's layout follows from the pool sizes it was made for; an evaluation takes its weights
    from the options of the moment, and sizes that differ by then are refused before the call."""
    from argparse import Namespace
    from style_transfer_amd.terms import LapTerm
    st = LapTerm.__new__(LapTerm)
    st.pools, st._key, st._weights = [4, 16], None, None
    assert st.weights(Namespace(lap_pools=['4', '16:3']), 30) == [7.5, 22.5]
    assert st.weights(Namespace(lap_pools=['4', '16:3']), 10) == [2.5, 7.5]       # a weight that moves
    assert st.weights(Namespace(lap_pools=['4:3', '16']), 10) == [7.5, 2.5]
    for other in (['4'], ['16', '4'], ['4', '8'], None):
        with pytest.raises(ValueError) as err:
            st.weights(Namespace(lap_pools=other), 10)
        assert '--lap-pools' in str(err.value)
    st.pools = [4]
    assert st.weights(Namespace(), 2.0) == [2.0]        # the default pools


def test_the_three_symbols_are_exported_with_their_signatures():
    so = ctypes.CDLL(lib.LIB_PATH)
    for name in ('stx_image_lap_floats', 'stx_image_lap_target', 'stx_image_lap'):
        assert hasattr(so, name), name
    i, vp, d = ctypes.c_int, ctypes.c_void_p, ctypes.c_double
    assert lib.NON_STATUS['stx_image_lap_floats'] == (ctypes.c_size_t, [i, i, i, lib.c_int_p])
    assert lib.SIGNATURES['stx_image_lap_target'] == [vp, vp, i, i, i, lib.c_int_p, vp]
    assert lib.SIGNATURES['stx_image_lap'] == [vp, vp, vp, i, i, i, lib.c_int_p, lib.c_double_p, vp, d,
                                               lib.c_double_p]
    # the size entry needs no engine and no GPU: sum over pools of ceil(H / p) * ceil(W / p)
    floats = lib.load().stx_image_lap_floats
    pools = (ctypes.c_int * 3)(1, 4, 64)
    assert floats(130, 67, 3, pools) == 130 * 67 + 33 * 17 + 3 * 2
    assert floats(37, 53, 1, (ctypes.c_int * 1)(4)) == 10 * 14
    for bad in ((3,), (128,), (4, 4), (1, 2, 4, 8, 16), ()):
        assert floats(64, 64, len(bad), (ctypes.c_int * max(len(bad), 1))(*bad)) == 0, bad
    assert floats(64, 64, 1, None) == 0
    # null arguments are refused with a status and a message that names them
    one = (ctypes.c_int * 1)(4)
    assert lib.load().stx_image_lap_target(None, None, 8, 8, 1, one, None) == -1
    assert 'null' in lib.load().stx_last_error().decode()
    assert lib.load().stx_image_lap(None, None, None, 8, 8, 1, one, None, None, 1.0, None) == -1
