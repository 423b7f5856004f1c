"""stx_image_swt_haar_levels (--swt-levels N of the Haar wavelet; style_transfer.py:716-720,
num_utils.py:179-196) against the float64 restatement in tests/swt_levels_ref.py, which
tests/test_swt_levels_host.py holds to a band-by-band transform.  PyWavelets is in neither tree:
no reference vectors exist, parity with it is unpinned as for one level."""

from argparse import Namespace

import numpy as np
import pytest
from PIL import Image

from style_transfer_amd import image_ops, lib
from style_transfer_amd.config_system import parse_args
from style_transfer_amd.farm import TileFarm
from style_transfer_amd.netspec import builtin_net
from style_transfer_amd.transfer import StyleTransfer
from style_transfer_amd.weights import synthetic_weights
from tests import swt_levels_ref as ref
from tests.gpu_helpers import gpu_engine, swt_call, swt_inputs, swt_rolled

pytestmark = pytest.mark.gpu

SCALE = 0.37

# (shape, levels, roll (x, y), power, seed).  Every mapping of the kernels is met:
#   (3, 16, 16) at 4 levels      levels = log2 N, the triangle spans the square almost twice
#   (3, 37, 53)                  odd sizes, padding on both axes, the odd amount behind
#   (3, 64, 20) at 5 levels      half-width 31 > picture width 20: several reflections and the wrap
#   (3, 50, 44)                  N = 64 from the height
#   (3, 300, 520), (3, 724, 1024)  several workgroups along both axes
#   (3, 200, 130) at 7 levels    the column pass walks its halo in chunks
#   (3, 70, 1100) at 11 levels   both passes do (levels = log2 N = 11)
# Power 1 has gradient sign(D): the seeds of its cases are chosen so that the float64 detail has no
# pixel within 1e-5 max|D| of zero, which the test asserts before it looks at the kernel.
CASES = [
    ((3, 16, 16), 4, (5, -3), 2, 16),
    ((3, 16, 16), 4, (-7, 9), 1, 16),
    ((3, 16, 16), 2, (0, 0), 1.5, 16),
    ((3, 37, 53), 2, (8, -16), 1.5, 37),
    ((3, 37, 53), 3, (-20, 11), 2, 37),
    ((3, 37, 53), 6, (8, -16), 1, 37),
    ((3, 64, 20), 5, (-24, 40), 1, 64),
    ((3, 64, 20), 5, (13, -50), 2, 64),
    ((3, 64, 20), 3, (-24, 40), 1.5, 64),
    ((3, 50, 44), 3, (16, 8), 1.5, 50),
    ((3, 50, 44), 6, (-16, -8), 2, 50),
    ((3, 50, 44), 4, (-5, 31), 1, 50),
    ((3, 300, 520), 5, (-131, 77), 1.5, 300),
    ((3, 724, 1024), 4, (-200, 333), 2, 724),
    ((3, 724, 1024), 2, (40, -8), 2, 725),
    ((3, 200, 130), 7, (16, -24), 2, 200),
    ((3, 70, 1100), 11, (-300, 9), 2, 70),
]


@pytest.mark.parametrize('shape,levels,roll,power,seed', CASES)
def test_swt_haar_levels_against_restatement(shape, levels, roll, power, seed):
    eng = gpu_engine('vgg19')
    img, g0 = swt_inputs(shape, seed)
    rolled = swt_rolled(img, roll)
    if power == 1:
        d = np.abs(ref.swt_haar_detail(rolled, levels))
        assert d.min() >= 1e-5 * d.max(), 'seed %d puts a pixel on the sign change' % seed
    loss, grad = ref.swt_norm_haar(rolled, levels, power)
    want = g0 + np.float32(SCALE) * np.roll(grad, (-roll[1], -roll[0]), (1, 2))
    d_img, d_grad = eng.to_device(img), eng.to_device(g0)
    out = image_ops.swt_haar(eng, d_img, d_grad, SCALE, power, roll=roll, levels=levels)
    eng.sync()
    got = d_grad.get()
    print('loss rel %.3g  grad %.3g of max|want|' % (out.value / (SCALE * loss) - 1,
                                                     np.abs(got - want).max() / np.abs(want).max()))
    assert out.value == pytest.approx(SCALE * loss, rel=2e-5)
    assert np.abs(got - want).max() <= 2e-5 * np.abs(want).max()
    assert np.array_equal(d_img.get(), img)                 # the image is read only
    d_img.free()
    d_grad.free()


@pytest.mark.parametrize('shape,roll,power', [((3, 37, 53), (8, -16), 2), ((3, 64, 20), (-24, 40), 1),
                                              ((3, 300, 520), (16, 8), 1.5)])
def test_one_level_through_the_new_entry_is_the_shipped_kernel(shape, roll, power):
    eng = gpu_engine('vgg19')
    img, g0 = swt_inputs(shape, 3)
    d_img = eng.to_device(img)
    d_old, d_new = eng.to_device(g0), eng.to_device(g0)
    old = image_ops.swt_haar(eng, d_img, d_old, SCALE, power, roll=roll)
    new = swt_call(eng, d_img, d_new, roll, SCALE, power, levels=1)
    eng.sync()
    assert np.array_equal(d_old.get(), d_new.get())
    assert old.value == new.value and np.isfinite(new.value)
    for buf in (d_img, d_old, d_new):
        buf.free()


@pytest.mark.parametrize('shape,levels,power', [((3, 300, 520), 5, 1.5), ((3, 724, 1024), 3, 2)])
def test_two_runs_are_bit_identical(shape, levels, power):
    eng = gpu_engine('vgg19')
    img, g0 = swt_inputs(shape, 9)
    d_img = eng.to_device(img)
    runs = []
    for _ in range(2):
        d_grad = eng.to_device(g0)
        out = image_ops.swt_haar(eng, d_img, d_grad, SCALE, power, roll=(-33, 14), levels=levels)
        eng.sync()
        runs.append((out.value, d_grad.get()))
        d_grad.free()
    d_img.free()
    assert runs[0][0] == runs[1][0] and np.isfinite(runs[0][0])
    assert np.array_equal(runs[0][1], runs[1][1])
    assert not np.array_equal(runs[0][1], g0)


def test_level_counts_outside_the_range_are_refused():
    eng = gpu_engine('vgg19')
    img, g0 = swt_inputs((3, 37, 53), 1)                       # padded side 64: 1 to 6 levels
    d_img, d_grad = eng.to_device(img), eng.to_device(g0)
    for levels in (0, 7, -2, 40):
        with pytest.raises(lib.StxError) as err:
            swt_call(eng, d_img, d_grad, (0, 0), SCALE, 2, levels=levels)
        assert err.value.code != 0
        assert 'levels = %d' % levels in str(err.value) and 'padded side 64' in str(err.value)
    with pytest.raises(lib.StxError):
        image_ops.swt_haar(eng, d_img, d_grad, SCALE, 2, levels=7)
    swt_call(eng, d_img, d_grad, (0, 0), SCALE, 2, levels=6)
    eng.sync()
    assert not np.array_equal(d_grad.get(), g0)
    d_img.free()
    d_grad.free()


def _first_losses(golden, extra, iterations=2):
    state = Namespace()
    base = str(golden['e2e_aux.argv']).split()
    args = parse_args(state, base + extra + ['-i', str(iterations)], config_py=False)
    net = builtin_net(args.model)
    farm = TileFarm(net, [0], synthetic_weights(net, 0), verbose=False)
    try:
        st = StyleTransfer(farm, args, state)
        log = []
        np.random.seed(args.seed)
        st.transfer_multiscale([Image.fromarray(golden['e2e_aux.content_u8'])],
                               [Image.fromarray(golden['e2e_aux.style_u8'])],
                               callback=lambda **kw: log.append(kw['loss']))
    finally:
        farm.close()
    return log


def test_swt_levels_on_the_command_line(golden):
    """--swt-weight 3 --swt-levels 3 runs; on the first evaluation -- same seed, so same start image
    and same shift -- its loss exceeds that of the run without the term and differs from that of the
    one-level run (the term itself is held to the restatement above)."""
    plain = _first_losses(golden, [])
    one = _first_losses(golden, ['--swt-weight', '3', '--swt-levels', '1'])
    three = _first_losses(golden, ['--swt-weight', '3', '--swt-levels', '3'])
    assert len(three) == 2 and all(np.isfinite(l) for l in plain + one + three)
    print('first losses: plain %.9g, 1 level %.9g, 3 levels %.9g' % (plain[0], one[0], three[0]))
    assert three[0] > plain[0]
    assert three[0] != one[0]


def test_too_many_levels_for_a_scale_stop_before_its_first_step(golden):
    """The picture of that run is 72 x 64, padded to 128: 8 levels are one too many."""
    with pytest.raises(ValueError, match='--swt-levels 8'):
        _first_losses(golden, ['--swt-weight', '3', '--swt-levels', '8'])
    assert len(_first_losses(golden, ['--swt-weight', '3', '--swt-levels', '7'], 1)) == 1
