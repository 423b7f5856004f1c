"""The SWT term for dbN / symN (style_transfer.py:716-720, num_utils.py:179-196): the closed form in
tests/swt_wavelet_ref.py against filters obtained here by spectral factorisation and against a
band-by-band transform with them, and the host side of the feature (wavelet names, level counts,
the C ABI entry point).  No GPU."""

import ctypes
import os
import re
from math import comb
from types import SimpleNamespace

import numpy as np
import pytest

from style_transfer_amd import image_ops, lib
from tests import swt_levels_ref as haar_ref
from tests import swt_wavelet_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _factorised_filter(order, mixed):
    """An orthonormal low-pass filter with ``order`` vanishing moments from the roots of
    P(y) = sum_k C(N-1+k, k) y^k, y = sin^2(w/2) = (2 - z - 1/z)/4: every root y gives the pair
    z, 1/z, and H takes one of each pair.  Not mixed: the one inside the unit circle throughout
    (minimum phase: dbN).  Mixed: the outside one for every other root (conjugates together, so h
    stays real) -- the freedom that symN uses; |H|^2 is the same."""
    ys = np.roots([comb(order - 1 + k, k) for k in reversed(range(order))]) if order > 1 else []
    keys = sorted({(round(y.real, 9), round(abs(y.imag), 9)) for y in ys})
    zs = []
    for y in ys:
        b = 2 - 4 * y
        z = (b - np.sqrt(b * b - 4 + 0j)) / 2
        if abs(z) > 1:
            z = 1 / z
        if mixed and keys.index((round(y.real, 9), round(abs(y.imag), 9))) % 2 == 0:
            z = 1 / z
        zs.append(z)
    h = np.poly(np.concatenate([-np.ones(order), np.array(zs, complex)]))
    assert np.abs(h.imag).max() <= 1e-9 * np.abs(h.real).max()
    h = h.real
    return h * (np.sqrt(2) / h.sum())


@pytest.mark.parametrize('mixed', [False, True])
@pytest.mark.parametrize('order', range(2, 9))
def test_closed_form_is_the_autocorrelation_of_a_factorised_filter(order, mixed):
    h = _factorised_filter(order, mixed)
    assert len(h) == 2 * order
    auto = np.correlate(h, h, 'full')
    r = ref.autocorrelation(order)
    err = np.abs(auto - r).max()
    print('order %d mixed %d: max |autocorrelation - closed form| = %.3g' % (order, mixed, err))
    # numpy.roots is backward stable; the roots of P are simple and well apart up to order 8, the
    # filter is a product of <= 15 factors of them: 1e-10 leaves four digits over what that costs
    assert err < 1e-10
    if mixed and order > 2:
        assert np.abs(h - _factorised_filter(order, False)).max() > 1e-3      # a different filter
    if order == 2 and not mixed:    # the textbook db2
        s3 = np.sqrt(3)
        db2 = np.array([1 + s3, 3 + s3, 3 - s3, 1 - s3]) / (4 * np.sqrt(2))
        assert min(np.abs(h - db2).max(), np.abs(h - db2[::-1]).max()) < 1e-12


@pytest.mark.parametrize('order', [1, 2, 3, 4, 8, 20, 38])
def test_half_band(order):
    r = ref.autocorrelation_exact(order)
    assert len(r) == 4 * order - 1
    c = 2 * order - 1
    assert r[c] == 1 and sum(r) == 2
    assert all(r[c + k] == 0 for k in range(-c, c + 1) if k % 2 == 0 and k != 0)
    assert all(r[c + k] == r[c - k] for k in range(c + 1))
    assert all(r[c + k] != 0 for k in range(-c, c + 1, 2))


def test_first_orders_in_rationals():
    assert [float(v) for v in ref.autocorrelation_exact(1)] == [0.5, 1, 0.5]
    assert [float(v) for v in ref.autocorrelation_exact(2)] == [-1 / 16, 0, 9 / 16, 1, 9 / 16, 0, -1 / 16]


def test_closed_form_is_the_lagrange_product():
    """The form the library builds its taps from: r[2k-1] is the weight of node k at the point 1/2
    among the nodes -N+1 .. N."""
    for order in (2, 3, 8, 20, 38):
        r = ref.autocorrelation(order)
        c = 2 * order - 1
        for k in range(1, order + 1):
            w = np.prod([(0.5 - m) / (k - m) for m in range(-order + 1, order + 1) if m != k])
            assert r[c + 2 * k - 1] == pytest.approx(w, rel=1e-12)


@pytest.mark.parametrize('levels', [1, 2, 3])
@pytest.mark.parametrize('order', [2, 3, 5])
@pytest.mark.parametrize('mixed', [False, True])
def test_closed_form_equals_filterbank(order, levels, mixed):
    """A picture that is not a power-of-two square: the closed form on the padded square equals the
    band-by-band transform of the same padded square, cropped."""
    from oracle import num_ops
    x = np.random.RandomState(10 * order + levels).uniform(-1, 1, (1, 13, 22))
    pw = num_ops._pad_width(x.shape, (1, 32, 32))
    assert pw[1] == (9, 10) and pw[2] == (5, 5)
    full = ref.swt_filterbank(np.pad(x, pw, 'symmetric')[0], _factorised_filter(order, mixed), levels)
    got = ref.swt_wavelet_detail(x, order, levels)[0]
    err = np.abs(got - full[9:22, 5:27]).max()
    print('order %d, %d levels, mixed %d: %.3g' % (order, levels, mixed, err))
    assert err < 1e-12


@pytest.mark.parametrize('shape,levels', [((3, 16, 16), 4), ((3, 37, 53), 3), ((2, 64, 20), 1)])
def test_order_one_is_haar(shape, levels):
    x = np.random.RandomState(1).uniform(-1, 1, shape)
    assert np.abs(ref.swt_wavelet_detail(x, 1, levels) - haar_ref.swt_haar_detail(x, levels)).max() < 1e-14
    loss, grad = ref.swt_norm_wavelet(x, 1, levels, 1.5)
    loss1, grad1 = haar_ref.swt_norm_haar(x, levels, 1.5)
    assert loss == pytest.approx(loss1, rel=1e-13) and np.abs(grad - grad1).max() < 1e-13


@pytest.mark.parametrize('order', [2, 8])
def test_constant_plane_has_no_detail(order):
    assert np.abs(ref.swt_wavelet_detail(np.full((2, 23, 32), 3.0), order, 3)).max() < 1e-12


def test_level_count_beyond_the_padded_side_is_refused_by_the_restatement():
    x = np.zeros((1, 13, 22))
    ref.swt_wavelet_detail(x, 2, 5)
    for levels in (0, 6):
        with pytest.raises(ValueError):
            ref.swt_wavelet_detail(x, 2, levels)


def test_wavelet_names():
    order = image_ops.swt_wavelet_order
    assert order('haar') == 1 and order('db1') == 1
    assert [order('db%d' % n) for n in (2, 4, 20, 38)] == [2, 4, 20, 38]
    assert [order('sym%d' % n) for n in (2, 4, 20)] == [2, 4, 20]
    for name in ('db0', 'db39', 'db100', 'sym1', 'sym21', 'sym0', 'coif1', 'coif3', 'bior2.2',
                 'rbio1.3', 'dmey', 'db', 'sym', 'db2 ', ' db2', 'db02', 'DB2', 'Haar', 'haar1',
                 'db-2', 'db2.0', 'sym4x', '', 'None'):
        with pytest.raises(NotImplementedError):
            order(name)


def test_swt_wavelet_refuses_before_it_touches_the_engine():
    img = SimpleNamespace(shape=(3, 37, 53), ptr=None)          # padded side 64: 1 to 6 levels
    for name in ('coif2', 'bior1.3', 'dmey', 'db39', 'sym1'):
        with pytest.raises(NotImplementedError):
            image_ops.swt_wavelet(None, img, img, 1.0, 2, name, levels=2)
    for name in ('haar', 'db2', 'sym8'):
        for levels in (0, -1, 7, 40):
            with pytest.raises(ValueError):
                image_ops.swt_wavelet(None, img, img, 1.0, 2, name, levels=levels)


def test_entry_point_is_declared_exported_and_bound():
    text = open(os.path.join(REPO, 'include', 'stx.h')).read()
    decl = re.search(r'int\s+stx_image_swt_daub_levels\s*\(([^;]*)\)\s*;', text)
    assert decl, 'stx_image_swt_daub_levels is not declared in include/stx.h'
    params = [' '.join(p.split()) for p in decl.group(1).split(',')]
    assert len(params) == 11 and params[5:7] == ['int order', 'int levels']
    sig = lib.SIGNATURES['stx_image_swt_daub_levels']
    assert len(sig) == 11 and sig[5] is ctypes.c_int
    # everything but the order is stx_image_swt_haar_levels'
    assert sig[:5] + sig[6:] == lib.SIGNATURES['stx_image_swt_haar_levels']
    assert hasattr(lib.load(), 'stx_image_swt_daub_levels')
