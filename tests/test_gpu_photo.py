"""The photorealism regulariser on the GPU (stx_image_photo) against the float64 numpy statement of
tests/photo_ref.py -- there is no reference implementation of this term --, its exact properties, the
wiring through StyleTransfer and the command line.

Bounds (none of them comes from what the kernel gives):
  * loss to 2e-5 relative, gradient to 2e-5 of max|grad_ref|: the bounds of the SWT and Laplacian terms.
    The colour-line picture at eps = 1e-7 is the case with teeth: float64 window algebra sits near 1e-7
    there and float32 window algebra near 1e-3 (tests/test_photo_host.py shows both without a GPU);
  * iterate == content, where the reference gradient is of the order of eps: K * spread_unit, with
    spread_unit = 2^-24 * 9 * max over windows of |v - m_k| / 255 * 2 scale and K four times the worst error,
    in those units and over four summation orders, of photo_ref.emulate (float64 window algebra, float32
    residuals, float32 nine-term sums) against the float64 reference for the very same inputs, computed
    on the CPU by the test.  The factor 4 is for summation order and the order of the window algebra.
    Emulated worst errors in spread_units (K / 4), the largest over the sizes: noise content 2e-9 (eps 1e-7)
    and 2e-6 (eps 1e-4), colour line 5e-6 (eps 1e-7) and 2.1e-4 (eps 1e-4) -- far below 1 because the
    residuals themselves are of the order of eps here, and a float32 rounding is relative to the residual, not
    to |v - m_k|.  Observed on an MI355X: at most 0.32 of the budget.

The tile of the kernel is 30 x 6 pixels and a launch has 1024 workgroups at most: the sizes put one and two
tiles on either side of both edges ((6, 30), (7, 31), (13, 61)) and more tiles than workgroups (724 x 724,
965 x 966) beside the single window, the strips one window thick and the rows unaligned to 16 bytes."""

import ctypes
import glob
import re

import numpy as np
import pytest
from PIL import Image

from style_transfer_amd import image_ops, lib
from tests import photo_ref
from tests.gpu_helpers import gpu_engine

pytestmark = pytest.mark.gpu
SIZES = [(3, 3), (3, 40), (40, 3), (5, 5), (6, 30), (7, 31), (13, 61), (37, 53), (64, 64), (65, 67), (130, 257),
         (724, 724), (965, 966)]
# (picture, eps): (a) noise, (b) the colour line at both eps, (c) flat content
PICTURES = [('noise', 1e-7), ('colour_line', 1e-7), ('colour_line', 1e-4), ('flat', 1e-7)]
SCALE = 3.5
_REFS = {}


def reference(kind, hw, eps, same=False):
    """(iterate, content, loss, gradient, budget) for scale 1, computed once per case and left alone.
    ``same``: the iterate is the content picture itself, and the budget is that of the module docstring for
    it: (K, spread_unit), with K four times the emulation's worst error in those units."""
    key = (kind, hw, eps, same)
    if key not in _REFS:
        img, content = getattr(photo_ref, kind)(hw, hw[0] + hw[1])
        if same:
            img = content.copy()
        fit = photo_ref.window_fit(img, content, eps)
        loss, grad = photo_ref.photo_loss(img, content, eps, 1.0, fit)
        budget = None
        if same:
            budget = (4 * photo_ref.emulated_k(img, content, eps, 1.0, grad, fit), photo_ref.spread_unit(img, 1.0))
        for arr in (img, content, grad):
            arr.setflags(write=False)
        _REFS[key] = (img, content, loss, grad, budget)
    return _REFS[key]


def run(eng, img, content, eps, scale, g0=None):
    """One call through image_ops: (loss, gradient)."""
    d_img, d_content = eng.to_device(img), eng.to_device(content)
    d_grad = eng.empty(img.shape).zero() if g0 is None else eng.to_device(g0)
    loss = image_ops.photo_loss(eng, d_img, d_grad, d_content, eps, scale)
    eng.sync()
    got = d_grad.get()
    assert np.array_equal(d_img.get(), img) and np.array_equal(d_content.get(), content)   # only read
    for arr in (d_img, d_content, d_grad):
        arr.free()
    return loss.value, got


@pytest.mark.parametrize('kind,eps', PICTURES)
@pytest.mark.parametrize('hw', SIZES)
def test_photo_against_float64(hw, kind, eps):
    eng = gpu_engine()
    img, content, want_loss, want_grad, _ = reference(kind, hw, eps)
    want_loss, want_grad = SCALE * want_loss, SCALE * want_grad
    loss, got = run(eng, img, content, eps, SCALE)
    loss_err = abs(loss - want_loss) / want_loss
    grad_err = np.abs(np.float64(got) - want_grad).max() / np.abs(want_grad).max()
    print('%s %s eps %g: loss error %.3g relative, gradient error %.3g of max|grad|'
          % (hw, kind, eps, loss_err, grad_err))
    assert want_loss > 0 and np.abs(want_grad).max() > 0
    assert loss_err <= 2e-5
    assert grad_err <= 2e-5
    # the same data again: the same bytes
    again_loss, again = run(eng, img, content, eps, SCALE)
    assert again.tobytes() == got.tobytes()
    assert np.float64(again_loss).tobytes() == np.float64(loss).tobytes()


# every size with the colour line at eps = 1e-7; the sizes up to 130 x 257 also at 1e-4 and with noise content
SAME = ([(hw, 'colour_line', 1e-7) for hw in SIZES] +
        [(hw, kind, eps) for hw in SIZES if hw[0] * hw[1] <= 130 * 257
         for kind, eps in (('colour_line', 1e-4), ('noise', 1e-7), ('noise', 1e-4))])


@pytest.mark.parametrize('hw,kind,eps', SAME)
def test_the_content_picture_itself(hw, kind, eps):
    """Iterate == content: only eps |a|^2 is left of the loss, and the gradient is of the order of eps."""
    eng = gpu_engine()
    img, content, want_loss, want_grad, (k, unit) = reference(kind, hw, eps, same=True)
    want_loss, want_grad = SCALE * want_loss, SCALE * want_grad
    budget = k * unit * SCALE                                # (the unit is linear in the scale)
    loss, got = run(eng, img, content, eps, SCALE)
    err = np.abs(np.float64(got) - want_grad).max()
    print('%s %s eps %g, iterate == content: K = %.3g, error %.3g of the budget, %.3g of max|grad_ref| = %.3g; '
          'loss error %.3g relative' % (hw, kind, eps, k, err / budget, err / np.abs(want_grad).max(),
                                        np.abs(want_grad).max(), abs(loss - want_loss) / want_loss))
    assert 0 < want_loss <= SCALE * 3 * eps * (hw[0] - 2) * (hw[1] - 2)
    assert abs(loss - want_loss) <= 2e-5 * want_loss
    assert err <= budget


@pytest.mark.parametrize('hw', [(5, 5), (37, 53), (65, 67), (965, 966)])
def test_the_gradient_is_added_once_in_float32(hw):
    eng = gpu_engine()
    img, content, _, _, _ = reference('colour_line', hw, 1e-7)
    g0 = np.random.RandomState(6).normal(0, 0.5, img.shape).astype(np.float32)
    _, g = run(eng, img, content, 1e-7, 1.0)
    _, total = run(eng, img, content, 1e-7, 1.0, g0)
    assert np.abs(g).max() > 0
    assert np.array_equal(total, g0 + g)                     # float32(g0 + g), element for element


@pytest.mark.parametrize('hw', [(7, 31), (65, 67)])
def test_scale_and_eps_reach_the_kernel(hw):
    eng = gpu_engine()
    img, content, want_loss, want_grad, _ = reference('colour_line', hw, 1e-7)
    loss1, g1 = run(eng, img, content, 1e-7, 1.0)
    loss2, g2 = run(eng, img, content, 1e-7, 2.0)
    assert loss2 == 2 * loss1 and np.array_equal(g2, 2 * g1)          # exactly: a power of two
    # eps = 1e-4 against 1e-7 differ as the reference says
    _, _, want_loss4, want_grad4, _ = reference('colour_line', hw, 1e-4)
    loss4, g4 = run(eng, img, content, 1e-4, 1.0)
    top = np.abs(want_grad).max()
    assert np.abs(want_grad4 - want_grad).max() > 1e-2 * top and abs(want_loss4 - want_loss) > 1e-2 * want_loss
    assert np.abs((np.float64(g4) - np.float64(g1)) - (want_grad4 - want_grad)).max() <= 2 * 2e-5 * top
    assert abs((loss4 - loss1) - (want_loss4 - want_loss)) <= 2 * 2e-5 * want_loss4


def test_flat_content_is_the_centred_plane_exactly():
    """Flat content: the covariance is zero, so a_k = 0 and r = v - m_k; the kernel's sums of nine equal values
    are exact, so nothing of the content picture's colour reaches the result."""
    eng = gpu_engine()
    img, content = photo_ref.flat((37, 53), 3)
    other = content + np.float32(64.0)
    loss, got = run(eng, img, content, 1e-7, 1.0)
    loss_o, got_o = run(eng, img, other, 1e-7, 1.0)
    assert loss == loss_o and got.tobytes() == got_o.tobytes()


def test_argument_errors():
    eng = gpu_engine()
    img, content = photo_ref.noise((16, 16), 1)
    g0 = np.random.RandomState(2).normal(0, 1, img.shape).astype(np.float32)
    d_img, d_content, d_grad = eng.to_device(img), eng.to_device(content), eng.to_device(g0)
    out = ctypes.c_double(0)

    def photo(img_ptr=d_img.ptr, content_ptr=d_content.ptr, grad_ptr=d_grad.ptr, H=16, W=16, eps=1e-7,
              loss=ctypes.byref(out), engine=eng.handle):
        return lib.load().stx_image_photo(engine, img_ptr, content_ptr, grad_ptr, H, W, eps, 1.0, loss)
    message = lambda: lib.load().stx_last_error().decode()
    for null in ('img_ptr', 'content_ptr', 'grad_ptr', 'loss', 'engine'):
        assert photo(**{null: None}) == -1 and 'null' in message()
    assert photo(H=2) == -1 and '2 x 16' in message()
    assert photo(W=2) == -1 and '16 x 2' in message()
    assert photo(H=0) == -1 and photo(W=-5) == -1
    for eps in (0.0, -1e-7, float('nan'), float('inf')):
        assert photo(eps=eps) == -1 and 'eps' in message()
    with pytest.raises(lib.StxError) as err:
        image_ops.photo_loss(eng, d_img, d_grad, d_content, 0.0, 1.0)
    assert err.value.code == -1
    with pytest.raises(ValueError):          # a content picture of another size never reaches the library
        image_ops.photo_loss(eng, d_img, d_grad, _Shape((3, 8, 16)), 1e-7, 1.0)
    eng.sync()
    assert d_grad.get().tobytes() == g0.tobytes()            # nothing ran
    assert photo() == 0                                      # (the same call with good arguments does)
    eng.sync()
    assert d_grad.get().tobytes() != g0.tobytes() and out.value > 0
    for arr in (d_img, d_content, d_grad):
        arr.free()


class _Shape:
    def __init__(self, shape):
        self.shape, self.ptr = shape, None


# ------------------------------------------------------------------------------ a functional check
def test_adam_steps_on_the_term_alone_lower_it():
    """From one noise start, 20 Adam steps with only this term: its value, as the float64 reference reports it
    on the downloaded picture, goes down."""
    from style_transfer_amd.optimizers import AdamOptimizer
    eng = gpu_engine()
    hw = (61, 75)
    _, content = photo_ref.colour_line(hw)
    start, _ = photo_ref.noise(hw, 12)
    d_img, d_content, d_grad = eng.to_device(start), eng.to_device(content), eng.empty(start.shape)
    opt = AdamOptimizer(eng, d_img, step_size=4.0)
    reported = []

    def evaluate(params):
        d_grad.zero()
        reported.append(image_ops.photo_loss(eng, params, d_grad, d_content, 1e-7, 1e4))
        return reported[-1], d_grad
    for _ in range(20):
        opt.update(evaluate)
    eng.sync()
    before = photo_ref.photo_loss(start, content, 1e-7, 1e4)[0]
    after = photo_ref.photo_loss(d_img.get(), content, 1e-7, 1e4)[0]
    print('the term alone: %.6g -> %.6g after 20 Adam steps' % (before, after))
    assert abs(reported[0].value - before) <= 2e-5 * before
    assert after < before
    for arr in (d_img, d_content, d_grad):
        arr.free()


# ------------------------------------------------------------------------------ composition
def _pictures(content_hw, style_hw, seed):
    """A content and a style picture: smooth shapes under mild noise, clear of 0 and 255."""
    rng = np.random.RandomState(seed)

    def picture(hw, centre, spread):
        y, x = np.mgrid[:hw[0], :hw[1]]
        waves = np.stack([np.sin(x / (3.0 + c) + c) * np.cos(y / (4.0 - c)) for c in range(3)], axis=2)
        return Image.fromarray(np.uint8(np.clip(centre + spread * waves + rng.uniform(-12, 12, hw + (3,)),
                                                0, 255)))
    return picture(content_hw, 125, 60), picture(style_hw, 130, 45)


def test_transfer_keeps_one_content_copy_per_scale_and_makes_one_call_per_evaluation(monkeypatch):
    from argparse import Namespace
    from style_transfer_amd.config_system import parse_args
    from style_transfer_amd.farm import TileFarm
    from style_transfer_amd.netspec import builtin_net
    from style_transfer_amd.transfer import StyleTransfer
    from style_transfer_amd.weights import load_weights
    net = builtin_net('vgg19')
    farm = TileFarm(net, [0], load_weights('synthetic:3', net), verbose=False)
    state = Namespace()
    args = parse_args(state, ['-ci', 'c', '-si', 's', '--size', '64', '--min-size', '45', '-i', '2', '2',
                              '--tile-size', '64', '--photo-weight', '1e4', '--photo-eps', '1e-5'],
                      config_py=False)
    st = StyleTransfer(farm, args, state)
    content, style = _pictures((64, 64), (50, 57), 21)
    calls = []
    real_loss = image_ops.photo_loss

    def wrapped_loss(engine, img, grad, content_dev, eps, scale):
        out = real_loss(engine, img, grad, content_dev, eps, scale)
        calls.append(dict(shape=img.shape, content=content_dev, picture=content_dev.get(), eps=eps, scale=scale,
                          grad_is_own=grad is st.grad, term=out))
        return out
    monkeypatch.setattr(image_ops, 'photo_loss', wrapped_loss)
    np.random.seed(0)
    st.transfer_multiscale([content], [style])
    assert len(calls) == 4                                   # Adam: one evaluation per step
    for i, call in enumerate(calls):
        size = (45, 64)[i // 2]
        assert call['shape'] == (3, size, size) and call['grad_is_own']
        want = st.pil_to_image(content.resize((size, size), Image.LANCZOS))
        assert np.array_equal(call['picture'], want)         # the content picture at that scale's size
        assert call['eps'] == 1e-5 and call['scale'] == st.layer_weights['data'] * 1e4
        assert call['term'].value > 0
    assert calls[0]['content'] is calls[1]['content'] and calls[2]['content'] is st.content_picture
    assert calls[0]['content'].ptr is None                   # the previous scale's copy is freed
    farm.close()


# ------------------------------------------------------------------------------ command line
def _cli_run(tmp_path, monkeypatch, capsys, name, extra):
    """One run of the command line in its own directory: (final RGB, its PNG comment, the losses of
    <RUN>_log.csv)."""
    import csv
    from style_transfer_amd import cli
    where = tmp_path / name
    where.mkdir()
    monkeypatch.chdir(where)
    argv = ['-ci', '../c.png', '-si', '../s.png', '-ii', '../c.png', '--size', '96', '-i', '3',
            '--tile-size', '64', '--model', 'vgg19', '--weights', 'synthetic:0', '--devices', '0',
            '-oi', 'out.png'] + extra
    assert cli.main(argv) == 0
    capsys.readouterr()
    final = Image.open(where / 'out.png')
    logs = glob.glob(str(where / '*_log.csv'))
    assert len(logs) == 1
    with open(logs[0], newline='') as f:
        losses = [row['loss'] for row in csv.DictReader(f)]
    return np.asarray(final.convert('RGB')), final.text['Comment'], losses


def test_cli_photo_weight(tmp_path, monkeypatch, capsys):
    content, style = _pictures((80, 96), (70, 60), 8)
    content.save(tmp_path / 'c.png')
    style.save(tmp_path / 's.png')
    bare = _cli_run(tmp_path, monkeypatch, capsys, 'bare', [])
    photo = _cli_run(tmp_path, monkeypatch, capsys, 'photo', ['--photo-weight', '1e4'])
    assert bare[0].shape == photo[0].shape == (80, 96, 3)
    assert 'photo_weight' not in bare[1] and 'photo_eps' not in bare[1]
    assert 'photo_weight=10000.0' in photo[1] and 'photo_eps' not in photo[1]
    strip = lambda text: [re.sub(r', photo_weight=10000\.0', '', line) for line in text.splitlines()
                          if not line.startswith('Command line:')]
    assert strip(photo[1]) == strip(bare[1])
    # the run starts on the content picture, where the term is of the order of eps; once the picture has
    # moved the term is there, and every later loss differs
    assert len(photo[2]) == len(bare[2]) == 3
    assert all(a != b for a, b in zip(photo[2][1:], bare[2][1:]))
