"""stx_image_swt_daub_levels / image_ops.swt_wavelet (the SWT term for dbN and symN;
style_transfer.py:716-720, num_utils.py:179-196) against the float64 restatement in
tests/swt_wavelet_ref.py, which tests/test_swt_wavelet_host.py holds to a band-by-band transform
with factorised filters.  PyWavelets is in neither tree: no reference vectors exist, parity with it
is unpinned as for Haar.  Tolerances are those of tests/test_gpu_swt_levels.py."""

import numpy as np
import pytest

from style_transfer_amd import image_ops, lib
from tests import swt_wavelet_ref as ref
from tests.gpu_helpers import gpu_engine, swt_call, swt_inputs, swt_rolled

pytestmark = pytest.mark.gpu

SCALE = 0.37
STX_ERR_ARG = -1

# (shape, order, levels, roll (x, y), power, seed).  Taps per axis: 2 (2 order - 1)(2^levels - 1) + 1,
# folded to the padded side N when longer.
#   (3, 37, 53), N = 64          every order of {2, 4, 8, 20} at every level count of {1, 2, 3, 5}: odd
#                                sizes, padding on both axes; folded from 64 taps on (order 20 at 1
#                                level has 79, at 5 levels 2419: the table wraps 37 times)
#   (3, 16, 16) at 4 levels      levels = log2 N, fewer taps than a workgroup has columns
#   (3, 182, 129), N = 256       several workgroups along y, padding on x much larger than on y
#   (3, 724, 1024), N = 1024     several workgroups along both axes; from 114 taps on the column pass
#                                walks the taps in chunks: order 8 at 3 levels (211 taps), order 4 at
#                                5 levels (435), order 20 at 3 levels (547)
#   (3, 70, 1100), N = 2048      order 20 at 5 levels: 2419 taps folded to 2048, more than the 1408
#                                the row pass stages at once: both passes walk chunks
# Power 1 has gradient sign(D): the seeds of its cases are chosen so that the float64 detail has no
# pixel within 1e-5 max|D| of zero, which the test asserts before it looks at the kernel.
CASES = [
    ((3, 37, 53), 2, 1, (8, -16), 2, 37),
    ((3, 37, 53), 2, 2, (-20, 11), 1, 37),
    ((3, 37, 53), 2, 3, (5, 3), 1.5, 37),
    ((3, 37, 53), 2, 5, (-7, -9), 2, 37),
    ((3, 37, 53), 4, 1, (-20, 11), 1.5, 38),
    ((3, 37, 53), 4, 2, (8, -16), 2, 38),
    ((3, 37, 53), 4, 3, (-7, -9), 1, 38),
    ((3, 37, 53), 4, 5, (0, 0), 1.5, 38),
    ((3, 37, 53), 8, 1, (5, 3), 1, 39),
    ((3, 37, 53), 8, 2, (-60, 40), 1.5, 39),
    ((3, 37, 53), 8, 3, (8, -16), 2, 39),
    ((3, 37, 53), 8, 5, (-20, 11), 1, 39),
    ((3, 37, 53), 20, 1, (-7, -9), 2, 40),
    ((3, 37, 53), 20, 2, (5, 3), 1, 40),
    ((3, 37, 53), 20, 3, (-20, 11), 1.5, 40),
    ((3, 37, 53), 20, 5, (8, -16), 2, 40),
    ((3, 37, 53), 20, 5, (-8, 16), 1, 41),
    ((3, 16, 16), 4, 4, (5, -3), 2, 16),
    ((3, 16, 16), 2, 2, (-7, 9), 1, 16),
    ((3, 182, 129), 2, 5, (-50, 77), 2, 182),
    ((3, 182, 129), 4, 3, (16, -8), 1.5, 182),
    ((3, 182, 129), 8, 2, (-131, 200), 2, 182),
    ((3, 182, 129), 20, 1, (3, -5), 1.5, 182),
    ((3, 182, 129), 20, 5, (-16, 24), 2, 182),
    ((3, 724, 1024), 2, 2, (40, -8), 2, 724),
    ((3, 724, 1024), 8, 3, (-200, 333), 2, 724),
    ((3, 724, 1024), 4, 5, (-33, 14), 1.5, 725),
    ((3, 724, 1024), 20, 3, (512, -700), 2, 726),
    ((3, 70, 1100), 20, 5, (-300, 9), 2, 70),
]


@pytest.mark.parametrize('shape,order,levels,roll,power,seed', CASES)
def test_swt_wavelet_against_restatement(shape, order, levels, roll, power, seed):
    eng = gpu_engine('vgg19')
    img, g0 = swt_inputs(shape, seed)
    rolled = swt_rolled(img, roll)
    if power == 1:
        d = np.abs(ref.swt_wavelet_detail(rolled, order, levels))
        assert d.min() >= 1e-5 * d.max(), 'seed %d puts a pixel on the sign change' % seed
    loss, grad = ref.swt_norm_wavelet(rolled, order, levels, power)
    want = g0 + np.float32(SCALE) * np.roll(grad, (-roll[1], -roll[0]), (1, 2))
    d_img, d_grad = eng.to_device(img), eng.to_device(g0)
    name = ('sym%d' if order % 4 == 0 else 'db%d') % order
    out = image_ops.swt_wavelet(eng, d_img, d_grad, SCALE, power, name, levels=levels, roll=roll)
    eng.sync()
    got = d_grad.get()
    print('%s, %d levels, %s: loss rel %.3g  grad %.3g of max|want|'
          % (name, levels, shape, out.value / (SCALE * loss) - 1,
             np.abs(got - want).max() / np.abs(want).max()))
    assert out.value == pytest.approx(SCALE * loss, rel=2e-5)
    assert np.abs(got - want).max() <= 2e-5 * np.abs(want).max()
    assert np.array_equal(d_img.get(), img)                 # the image is read only
    d_img.free()
    d_grad.free()


@pytest.mark.parametrize('shape,levels,roll,power', [((3, 37, 53), 1, (8, -16), 2),
                                                     ((3, 37, 53), 3, (-20, 11), 1.5),
                                                     ((3, 64, 20), 5, (-24, 40), 1),
                                                     ((3, 300, 520), 4, (16, 8), 1.5)])
def test_order_one_is_the_haar_entry_bit_for_bit(shape, levels, roll, power):
    eng = gpu_engine('vgg19')
    img, g0 = swt_inputs(shape, 3)
    d_img = eng.to_device(img)
    d_old, d_new, d_name = eng.to_device(g0), eng.to_device(g0), eng.to_device(g0)
    old = swt_call(eng, d_img, d_old, roll, SCALE, power, levels=levels)
    new = swt_call(eng, d_img, d_new, roll, SCALE, power, levels=levels, order=1)
    named = image_ops.swt_wavelet(eng, d_img, d_name, SCALE, power, 'haar', levels=levels, roll=roll)
    eng.sync()
    assert np.array_equal(d_old.get(), d_new.get()) and np.array_equal(d_old.get(), d_name.get())
    assert old.value == new.value == named.value and np.isfinite(new.value)
    assert not np.array_equal(d_new.get(), g0)
    for buf in (d_img, d_old, d_new, d_name):
        buf.free()


@pytest.mark.parametrize('shape,levels,power', [((3, 37, 53), 2, 1.5), ((3, 300, 520), 3, 2)])
def test_sym4_is_db4_bit_for_bit(shape, levels, power):
    eng = gpu_engine('vgg19')
    img, g0 = swt_inputs(shape, 4)
    d_img = eng.to_device(img)
    d_db, d_sym = eng.to_device(g0), eng.to_device(g0)
    db = image_ops.swt_wavelet(eng, d_img, d_db, SCALE, power, 'db4', levels=levels, roll=(-33, 14))
    sym = image_ops.swt_wavelet(eng, d_img, d_sym, SCALE, power, 'sym4', levels=levels, roll=(-33, 14))
    eng.sync()
    assert np.array_equal(d_db.get(), d_sym.get())
    assert db.value == sym.value and np.isfinite(db.value)
    assert not np.array_equal(d_db.get(), g0)
    for buf in (d_img, d_db, d_sym):
        buf.free()


@pytest.mark.parametrize('shape,order,levels,power', [((3, 300, 520), 4, 5, 1.5),
                                                      ((3, 724, 1024), 8, 3, 2)])
def test_two_runs_are_bit_identical(shape, order, levels, power):
    eng = gpu_engine('vgg19')
    img, g0 = swt_inputs(shape, 9)
    d_img = eng.to_device(img)
    runs = []
    for _ in range(2):
        d_grad = eng.to_device(g0)
        out = swt_call(eng, d_img, d_grad, (-33, 14), SCALE, power, levels=levels, order=order)
        eng.sync()
        runs.append((out.value, d_grad.get()))
        d_grad.free()
    d_img.free()
    assert runs[0][0] == runs[1][0] and np.isfinite(runs[0][0])
    assert np.array_equal(runs[0][1], runs[1][1])
    assert not np.array_equal(runs[0][1], g0)


def test_orders_and_level_counts_outside_the_range_are_refused():
    eng = gpu_engine('vgg19')
    img, g0 = swt_inputs((3, 37, 53), 1)                       # padded side 64: 1 to 6 levels
    d_img, d_grad = eng.to_device(img), eng.to_device(g0)
    for order in (0, 39, -1):
        with pytest.raises(lib.StxError) as err:
            swt_call(eng, d_img, d_grad, (0, 0), SCALE, 2, levels=2, order=order)
        assert err.value.code == STX_ERR_ARG and 'order = %d' % order in str(err.value)
    for order in (1, 2, 38):
        for levels in (0, 7, -2, 40):
            with pytest.raises(lib.StxError) as err:
                swt_call(eng, d_img, d_grad, (0, 0), SCALE, 2, levels=levels, order=order)
            assert err.value.code == STX_ERR_ARG
            assert 'levels = %d' % levels in str(err.value) and 'padded side 64' in str(err.value)
    with pytest.raises(ValueError):
        image_ops.swt_wavelet(eng, d_img, d_grad, SCALE, 2, 'db2', levels=7)
    with pytest.raises(NotImplementedError):
        image_ops.swt_wavelet(eng, d_img, d_grad, SCALE, 2, 'coif1', levels=2)
    eng.sync()
    assert np.array_equal(d_grad.get(), g0)                 # nothing has run
    swt_call(eng, d_img, d_grad, (0, 0), SCALE, 2, levels=6, order=38)
    eng.sync()
    assert not np.array_equal(d_grad.get(), g0)
    d_img.free()
    d_grad.free()
