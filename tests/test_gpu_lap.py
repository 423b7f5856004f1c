"""The Laplacian loss on the GPU (stx_image_lap_floats / _target / stx_image_lap) against the float64
numpy statement of tests/lap_ref.py -- there is no reference implementation of this term --, its exact
properties, the wiring through StyleTransfer and the command line.

Bounds (none of them comes from what the kernels give):
  * noise inputs: loss to 2e-5 relative, gradient to 2e-5 of max|grad_ref| -- the bounds of the SWT
    term, the same kind of computation (a linear filter in fp32 with a double finish);
  * pooled-value budget of a target: every rounding on the way to T_p = D P_p u(c) is relative to a sum
    of magnitudes that |D| P_p(|c_B| + |c_G| + |c_R|) / 382.5 bounds: two for the channel sum, two per
    doubling of the block (rows, then columns: 2 log2 p), one for the division, three for D (a
    difference and two levels of additions): (6 + 2 log2 p) * 2^-24 of that;
  * near the target: see test_near_the_target."""

import ctypes
import glob
import re

import numpy as np
import pytest
from PIL import Image

from style_transfer_amd import image_ops, lib
from tests import lap_ref
from tests.gpu_helpers import gpu_engine

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
CASES = [((37, 53), (4,)), ((70, 45), (16,)), ((130, 67), (1, 4, 64)), ((724, 724), (4, 16)),
         ((965, 966), (4, 16)), ((2048, 2048), (4, 16, 64)),
         ((67, 131), (2, 8, 32, 64))]          # (the remaining sizes, four at once)


def _pictures(content_hw, style_hw, seed):
    """A content and a style picture: smooth shapes under mild noise, clear of 0 and 255."""
    rng = np.random.RandomState(seed)

    def picture(hw, centre, spread):
        y, x = np.mgrid[:hw[0], :hw[1]]
        waves = np.stack([np.sin(x / (3.0 + c) + c) * np.cos(y / (4.0 - c)) for c in range(3)], axis=2)
        return Image.fromarray(np.uint8(np.clip(centre + spread * waves + rng.uniform(-12, 12, hw + (3,)),
                                                0, 255)))
    return picture(content_hw, 125, 60), picture(style_hw, 130, 45)


def _cli_run(tmp_path, monkeypatch, capsys, name, extra):
    """One run of the command line in its own directory (the recipe of test_gpu_preserve_color.py):
    (final RGB, its PNG comment, the --save-every pictures by file suffix, the losses of <RUN>_log.csv)."""
    import csv
    from style_transfer_amd import cli
    where = tmp_path / name
    where.mkdir()
    monkeypatch.chdir(where)
    argv = ['-ci', '../c.png', '-si', '../s.png', '-ii', '../c.png', '--size', '80', '--min-size', '57',
            '-i', '2', '2', '--tile-size', '64', '--save-every', '2', '--model', 'vgg19', '--weights',
            'synthetic:0', '--devices', '0', '-oi', 'out.png'] + extra
    assert cli.main(argv) == 0
    capsys.readouterr()
    final = Image.open(where / 'out.png')
    saved = {re.search(r'_out_(\d+)\.png$', p).group(1): np.asarray(Image.open(p).convert('RGB'))
             for p in sorted(glob.glob(str(where / '*_out_*.png')))}
    logs = glob.glob(str(where / '*_log.csv'))
    assert len(logs) == 1
    with open(logs[0], newline='') as f:
        losses = [row['loss'] for row in csv.DictReader(f)]
    return np.asarray(final.convert('RGB')), final.text['Comment'], saved, losses


def noise(hw, seed):
    rng = np.random.RandomState(seed)
    return (rng.uniform(-120, 130, (3,) + hw).astype(np.float32),
            rng.uniform(-120, 130, (3,) + hw).astype(np.float32))


def weights_for(pools):
    w = np.arange(1, len(pools) + 1, dtype=np.float64)
    return list(w / w.sum())


def target_budget(content, pools):
    """The pooled-value budget of the module docstring, flat like the target."""
    mags = np.abs(np.float64(content)).sum(axis=0) / lap_ref.UNIT
    return lap_ref.flat([(6 + 2 * np.log2(p)) * U * lap_ref.abs_lap(lap_ref.pool(mags, p)) for p in pools])


@pytest.mark.parametrize('hw,pools', CASES)
def test_lap_against_float64(hw, pools):
    eng = gpu_engine()
    img, content = noise(hw, hw[0] + hw[1])
    weights, scale = weights_for(pools), 3.5
    want_loss, want_grad, want_t = lap_ref.lap_loss(img, content, pools, weights, scale)
    d_img, d_content, d_grad = eng.to_device(img), eng.to_device(content), eng.empty(img.shape).zero()
    n = image_ops.lap_floats(hw[0], hw[1], pools)
    assert n == sum(-(-hw[0] // p) * -(-hw[1] // p) for p in pools)
    d_target = image_ops.lap_target(eng, d_content, pools)
    assert d_target.shape == (n,)
    got_t = d_target.get()
    t_err = np.abs(np.float64(got_t) - lap_ref.flat(want_t)) / target_budget(content, pools)
    loss = image_ops.lap_loss(eng, d_img, d_grad, d_target, pools, weights, scale)
    eng.sync()
    got = d_grad.get()
    loss_err = abs(loss.value - want_loss) / want_loss
    grad_err = np.abs(np.float64(got) - want_grad).max() / np.abs(want_grad).max()
    print('%s %s: loss error %.3g relative, gradient error %.3g of max|grad|, target error %.3g of its budget'
          % (hw, pools, loss_err, grad_err, t_err.max()))
    assert want_loss > 0 and np.abs(want_grad).max() > 0
    assert loss_err <= 2e-5
    assert grad_err <= 2e-5
    assert np.all(t_err <= 1)
    assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2])
    assert np.array_equal(d_img.get(), img)                  # the image is only read
    # the same data again: the same bytes
    d_grad.zero()
    again_t = image_ops.lap_target(eng, d_content, pools)
    again = image_ops.lap_loss(eng, d_img, d_grad, again_t, pools, weights, scale)
    eng.sync()
    assert again_t.get().tobytes() == got_t.tobytes()
    assert d_grad.get().tobytes() == got.tobytes()
    assert np.float64(again.value).tobytes() == np.float64(loss.value).tobytes()
    for arr in (d_img, d_content, d_grad, d_target, again_t):
        arr.free()


@pytest.mark.parametrize('hw,pools', [((37, 53), (4,)), ((130, 67), (1, 4, 64)), ((724, 724), (4, 16)),
                                      ((965, 966), (4, 16))])
def test_the_gradient_is_added_once_in_float32(hw, pools):
    eng = gpu_engine()
    img, content = noise(hw, 5)
    weights = weights_for(pools)
    rng = np.random.RandomState(6)
    g0 = rng.normal(0, 2e-4, img.shape).astype(np.float32)
    d_img, d_content = eng.to_device(img), eng.to_device(content)
    d_target = image_ops.lap_target(eng, d_content, pools)
    d_zero, d_prior = eng.empty(img.shape).zero(), eng.to_device(g0)
    image_ops.lap_loss(eng, d_img, d_zero, d_target, pools, weights, 1.0)
    image_ops.lap_loss(eng, d_img, d_prior, d_target, pools, weights, 1.0)
    eng.sync()
    g = d_zero.get()
    assert np.abs(g).max() > 0
    assert np.array_equal(d_prior.get(), g0 + g)             # float32(g0 + g), element for element
    for arr in (d_img, d_content, d_target, d_zero, d_prior):
        arr.free()


@pytest.mark.parametrize('hw,pools', [((37, 53), (4,)), ((130, 67), (1, 4, 64)), ((965, 966), (4, 16)),
                                      ((724, 724), (2, 8, 32))])
def test_the_content_picture_itself_costs_nothing(hw, pools):
    eng = gpu_engine()
    img, _ = noise(hw, 9)
    g0 = np.random.RandomState(10).normal(0, 1, img.shape).astype(np.float32)
    d_img, d_twin, d_grad = eng.to_device(img), eng.to_device(img), eng.to_device(g0)
    d_target = image_ops.lap_target(eng, d_twin, pools)
    loss = image_ops.lap_loss(eng, d_img, d_grad, d_target, pools, weights_for(pools), 7.0)
    eng.sync()
    assert loss.value == 0.0
    assert d_grad.get().tobytes() == g0.tobytes()
    for arr in (d_img, d_twin, d_grad, d_target):
        arr.free()


def test_near_the_target():
    """img = content + N(0, 1e-2) at 70 x 45 with pools {16}: e is a small difference of large pooled
    values, so the error is bounded against the magnitudes it is made from, not against the result:
        |grad - grad_ref| <= K 2^-24 * scale w 2 (|D| |D| (|P u(x)| + |P u(c)|))[y / p][x / p] / (n_cell 382.5)
    K counts the roundings between the pictures and e, each taken against the pooled magnitudes under
    |D|: two for the channel sum (b + g) + r, eight for the four doublings of the block from 1 to 16
    (rows, then columns, each one addition deep), one for the division by n_cell * 382.5 -- eleven on a
    pooled value --, three for D (the difference with a neighbour and two levels of additions) and
    one for the subtraction of the target: 15.  What follows e -- D again, the coefficient, the
    division -- rounds relative to |D e| itself, 1e3 times smaller here: one more unit covers it.
    K = 16."""
    K = 16
    hw, pools, weights, scale = (70, 45), (16,), [1.0], 2.0
    rng = np.random.RandomState(3)
    content = rng.uniform(-120, 130, (3,) + hw).astype(np.float32)
    img = (content + rng.normal(0, 1e-2, content.shape)).astype(np.float32)
    want_loss, want_grad, _ = lap_ref.lap_loss(img, content, pools, weights, scale)
    mags = (np.abs(lap_ref.pool(lap_ref.channel_sum(img), 16)) +
            np.abs(lap_ref.pool(lap_ref.channel_sum(content), 16)))
    cells = scale * weights[0] * 2 * lap_ref.abs_lap(lap_ref.abs_lap(mags)) / (lap_ref.cell_counts(*hw, 16) * lap_ref.UNIT)
    budget = K * U * lap_ref.spread(cells, hw[0], hw[1], 16)
    # (CPU only) the reference is not zero here, and is small against what it is made from
    assert np.abs(want_grad).min() > 0 and want_loss > 0
    assert np.abs(want_grad[0]).max() < 1e-2 * (budget / (K * U)).min()
    eng = gpu_engine()
    d_img, d_content, d_grad = eng.to_device(img), eng.to_device(content), eng.empty(img.shape).zero()
    d_target = image_ops.lap_target(eng, d_content, pools)
    image_ops.lap_loss(eng, d_img, d_grad, d_target, pools, weights, scale)
    eng.sync()
    err = np.abs(np.float64(d_grad.get()) - want_grad)
    print('near the target: worst error / budget %.3g (K = %d), error %.3g of max|grad_ref|'
          % ((err / budget).max(), K, err.max() / np.abs(want_grad).max()))
    assert np.all(err <= budget)
    for arr in (d_img, d_content, d_grad, d_target):
        arr.free()


@pytest.mark.parametrize('hw', [(50, 90), (90, 50), (40, 33)])
def test_grids_one_cell_wide(hw):
    """Pool size 64 on pictures that give a 1 x 2, a 2 x 1 and a 1 x 1 grid.  Two cells that are both
    means of thousands of noise pixels differ by little, so the error is held against the magnitudes,
    as in test_near_the_target but with the sums' own bound P |u| in place of |P u|:
        K 2^-24 * scale w 2 (|D| |D| (P|u(x)| + P|u(c)|))[y / p][x / p] / (n_cell 382.5)
    K = 6 + 2 log2 64 = 18 roundings up to D P u (module docstring), one for the subtraction of the
    target, one for everything behind e: 20."""
    K, pools, weights, scale = 20, (64,), [1.0], 2.0
    img, content = noise(hw, 11)
    want_loss, want_grad, want_t = lap_ref.lap_loss(img, content, pools, weights, scale)
    mags = lap_ref.pool((np.abs(np.float64(img)).sum(axis=0) + np.abs(np.float64(content)).sum(axis=0)) / lap_ref.UNIT, 64)
    cells = scale * 2 * lap_ref.abs_lap(lap_ref.abs_lap(mags)) / (lap_ref.cell_counts(*hw, 64) * lap_ref.UNIT)
    budget = K * U * lap_ref.spread(cells, hw[0], hw[1], 64)
    eng = gpu_engine()
    d_img, d_content, d_grad = eng.to_device(img), eng.to_device(content), eng.empty(img.shape).zero()
    d_target = image_ops.lap_target(eng, d_content, pools)
    assert d_target.shape == (want_t[0].size,)
    assert np.all(np.abs(np.float64(d_target.get()) - lap_ref.flat(want_t)) <= target_budget(content, pools))
    loss = image_ops.lap_loss(eng, d_img, d_grad, d_target, pools, weights, scale)
    eng.sync()
    err = np.abs(np.float64(d_grad.get()) - want_grad)
    if want_t[0].size == 1:                                  # one cell: D is zero
        assert loss.value == 0.0 and not err.any() and not want_grad.any()
    else:
        print('%s: worst error / budget %.3g' % (hw, (err / budget).max()))
        assert np.all(err <= budget) and np.abs(want_grad).max() > 0 and want_loss > 0
    for arr in (d_img, d_content, d_grad, d_target):
        arr.free()


def test_argument_errors():
    eng = gpu_engine()
    img, _ = noise((16, 16), 1)
    d_img, d_grad, d_target = eng.to_device(img), eng.empty(img.shape).zero(), eng.empty((256,)).zero()
    out = ctypes.c_double(0)
    w = (ctypes.c_double * 5)(1, 1, 1, 1, 1)

    def lap(pools, img_ptr=d_img.ptr, n=None, weights=w):
        arr = (ctypes.c_int * max(len(pools), 1))(*pools)
        return lib.load().stx_image_lap(eng.handle, img_ptr, d_grad.ptr, 16, 16, len(pools) if n is None else n,
                                        arr, weights, d_target.ptr, 1.0, ctypes.byref(out))

    def target(pools, content_ptr=d_img.ptr):
        arr = (ctypes.c_int * max(len(pools), 1))(*pools)
        return lib.load().stx_image_lap_target(eng.handle, content_ptr, 16, 16, len(pools), arr, d_target.ptr)
    message = lambda: lib.load().stx_last_error().decode()
    for call in (lap, target):
        assert call([4], None) == -1 and 'null' in message()                     # a null pointer
        assert call([]) == -1 and 'n_pools = 0' in message()                     # n_pools outside 1..4
        assert call([1, 2, 4, 8, 16]) == -1 and 'n_pools = 5' in message()
        assert call([3]) == -1 and 'pool size 3' in message()                    # not a power of two in 1..64
        assert call([4, 128]) == -1 and 'pool size 128' in message()
        assert call([4, 0]) == -1 and 'pool size 0' in message()
        assert call([4, 16, 4]) == -1 and 'pool size 4 is given twice' in message()   # a repeated size
    assert lap([4], weights=None) == -1 and 'weights' in message()
    assert lib.load().stx_image_lap_floats(16, 16, 1, (ctypes.c_int * 1)(3)) == 0
    with pytest.raises(lib.StxError) as err:
        image_ops.lap_target(eng, d_img, [4, 4])
    assert err.value.code == -1
    eng.sync()
    assert not d_grad.get().any()                            # nothing ran
    assert lap([4]) == 0 and target([4]) == 0                # (the same calls with good arguments do)
    eng.sync()
    for arr in (d_img, d_grad, d_target):
        arr.free()


# ------------------------------------------------------------------------------ composition
def test_transfer_makes_one_target_per_scale_and_one_call_per_evaluation(monkeypatch):
    """The pool weights carry --lap-weight (parse_weights(pools, lap_weight): sum |w| = 30), the scale
    is layer_weights['data']: scale * weights = layer_weights['data'] * 30 * [0.25, 0.75]."""
    from argparse import Namespace
    from style_transfer_amd.config_system import parse_args
    from style_transfer_amd.farm import TileFarm
    from style_transfer_amd.netspec import builtin_net
    from style_transfer_amd.terms import LapTerm
    from style_transfer_amd.transfer import StyleTransfer
    from style_transfer_amd.weights import load_weights
    net = builtin_net('vgg19')
    farm = TileFarm(net, [0], load_weights('synthetic:3', net), verbose=False)
    state = Namespace()
    args = parse_args(state, ['-ci', 'c', '-si', 's', '--size', '64', '--min-size', '45', '-i', '2', '2',
                              '--tile-size', '64', '--lap-weight', '30', '--lap-pools', '4', '16:3'],
                      config_py=False)
    st = StyleTransfer(farm, args, state)
    content, style = _pictures((64, 64), (50, 57), 21)
    targets, calls = [], []
    real_target, real_loss = image_ops.lap_target, image_ops.lap_loss

    def wrapped_target(engine, picture, pools):
        out = real_target(engine, picture, pools)
        targets.append(dict(picture=picture.get(), pools=list(pools), target=out.get(), array=out))
        return out

    def wrapped_loss(engine, img, grad, target, pools, weights, scale):
        calls.append(dict(shape=img.shape, target=target, pools=list(pools), weights=list(weights),
                          scale=scale, grad_is_own=grad is st.grad))
        return real_loss(engine, img, grad, target, pools, weights, scale)
    monkeypatch.setattr(image_ops, 'lap_target', wrapped_target)
    monkeypatch.setattr(image_ops, 'lap_loss', wrapped_loss)
    np.random.seed(0)
    st.transfer_multiscale([content], [style])
    assert [t['picture'].shape for t in targets] == [(3, 45, 45), (3, 64, 64)]     # one per scale
    for t, size in zip(targets, (45, 64)):
        want = st.pil_to_image(content.resize((size, size), Image.LANCZOS))
        assert np.array_equal(t['picture'], want)            # the content picture at that scale's size
        assert t['pools'] == [4, 16]
        ref = lap_ref.flat(lap_ref.target(want, [4, 16]))
        assert np.all(np.abs(np.float64(t['target']) - ref) <= target_budget(want, [4, 16]))
    lap_term, = [term for term in st.image_terms if isinstance(term, LapTerm)]
    assert targets[0]['array'].ptr is None and targets[1]['array'] is lap_term.target   # the old one is freed
    assert len(calls) == 4                                   # Adam: one evaluation per step
    for i, call in enumerate(calls):
        size = (45, 64)[i // 2]
        assert call['shape'] == (3, size, size) and call['grad_is_own']
        assert call['target'] is targets[i // 2]['array']
        assert call['pools'] == [4, 16]
        lw = st.layer_weights['data']
        assert np.allclose(np.float64(call['weights']) * call['scale'], lw * 30 * np.array([0.25, 0.75]),
                           rtol=1e-15, atol=0)
    farm.close()


# ------------------------------------------------------------------------------ command line
def test_cli_lap_weight(tmp_path, monkeypatch, capsys):
    content, style = _pictures((64, 80), (70, 60), 8)
    content.save(tmp_path / 'c.png')
    style.save(tmp_path / 's.png')
    bare = _cli_run(tmp_path, monkeypatch, capsys, 'bare', [])
    zero = _cli_run(tmp_path, monkeypatch, capsys, 'zero', ['--lap-weight', '0'])
    lap = _cli_run(tmp_path, monkeypatch, capsys, 'lap', ['--lap-weight', '50'])
    # ---- weight 0 == no flag: pictures and logged losses; the option shows in the comment alone
    assert bare[0].shape == (64, 80, 3) and np.array_equal(bare[0], zero[0])
    assert sorted(bare[2]) == sorted(zero[2]) == sorted(lap[2]) == ['0002', '0004']
    for key in bare[2]:
        assert np.array_equal(bare[2][key], zero[2][key]), key
    assert bare[3] == zero[3] and len(bare[3]) == 4
    assert 'lap_weight' not in bare[1] and 'lap_pools' not in bare[1]
    assert 'lap_weight=0.0' in zero[1]
    strip = lambda text: [re.sub(r', lap_weight=0\.0', '', line) for line in text.splitlines()
                          if not line.startswith('Command line:')]
    assert strip(zero[1]) == strip(bare[1])
    # ---- weight 50: the run starts on the content picture, where the term and its gradient are zero,
    # so the first logged loss is the bare one; every later one differs, and so does the picture
    assert 'lap_weight=50.0' in lap[1]
    assert len(lap[3]) == 4 and lap[3][0] == bare[3][0]
    assert all(a != b for a, b in zip(lap[3][1:], bare[3][1:]))
    # (the final picture; the one saved after the first scale's two steps has taken a single step that
    # saw the term, and its averaged iterate need not differ by a whole grey level)
    assert not np.array_equal(lap[0], bare[0])
