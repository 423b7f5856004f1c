"""The photorealism regulariser without a GPU: the two float64 statements of tests/photo_ref.py against each
other, the exact properties of the matting Laplacian, the emulations that price the GPU tests' bounds, the
two options, and the wiring through StyleTransfer with the library call replaced."""

import ctypes
from argparse import Namespace

import numpy as np
import pytest
from PIL import Image

from style_transfer_amd import image_ops, lib
from style_transfer_amd.config_system import PHOTO_EPS_DEFAULT, check_photo_options, parse_args
from tests import photo_ref

BASE = ['-ci', 'c', '-si', 's']


# ------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize('hw', [(7, 9), (3, 3)])
@pytest.mark.parametrize('eps', [1e-7, 1e-4])
def test_dense_against_matrix_free(hw, eps):
    img, content = photo_ref.noise(hw, 1)
    L = photo_ref.dense_l(content, eps)
    loss, grad = photo_ref.photo_loss(img, content, eps, scale=2.0)
    v = np.float64(img).reshape(3, -1) / 255.0
    for c in range(3):
        assert np.abs(L @ v[c] - photo_ref.apply_l(v[c].reshape(hw), content, eps).ravel()).max() <= 1e-12
        assert np.abs(2.0 * 2 * (L @ v[c]) / 255.0 - grad[c].ravel()).max() <= 1e-12
    # the loss, a sum of non-negatives, is the quadratic form
    quad = 2.0 * sum(v[c] @ L @ v[c] for c in range(3))
    assert loss > 0 and abs(loss - quad) <= 1e-12 * loss


def test_l_is_symmetric_and_kills_constants():
    _, content = photo_ref.colour_line((11, 12))
    rng = np.random.RandomState(2)
    u, v = rng.normal(size=(11, 12)), rng.normal(size=(11, 12))
    Lu, Lv = photo_ref.apply_l(u, content, 1e-7), photo_ref.apply_l(v, content, 1e-7)
    assert abs(np.sum(Lu * v) - np.sum(u * Lv)) <= 1e-9 * np.abs(Lu).sum() * np.abs(v).max()
    assert np.abs(photo_ref.apply_l(np.full((11, 12), 3.25), content, 1e-7)).max() <= 1e-13
    L = photo_ref.dense_l(content, 1e-7)
    assert np.abs(L - L.T).max() <= 1e-9 * np.abs(L).max() and np.abs(L.sum(axis=1)).max() <= 1e-9 * np.abs(L).max()
    # a corner pixel is in one window, an interior pixel in nine: the diagonal counts them (minus the fit)
    counts = photo_ref.gather(np.ones((9, 10, 9, 1)), 11, 12)[0]
    assert counts[0, 0] == 1 and counts[0, 1] == 2 and counts[1, 1] == 4 and counts[5, 5] == 9


def test_gradient_against_central_differences():
    img, content = photo_ref.noise((9, 8), 4)
    img = np.float64(img)
    loss, grad = photo_ref.photo_loss(img, content, 1e-5, scale=2.5)
    worst = 0.0
    for index in [(0, 0, 0), (1, 4, 4), (2, 8, 7), (0, 3, 7), (1, 8, 0), (2, 5, 2)]:
        h = 1e-2
        up, down = img.copy(), img.copy()
        up[index] += h
        down[index] -= h
        numeric = (photo_ref.photo_loss(up, content, 1e-5, 2.5)[0] -
                   photo_ref.photo_loss(down, content, 1e-5, 2.5)[0]) / (2 * h)
        worst = max(worst, abs(numeric - grad[index]) / np.abs(grad).max())
    print('central differences: worst error / max|grad| = %.3g' % worst)
    assert worst < 1e-8          # the loss is quadratic: central differences are exact up to rounding


@pytest.mark.parametrize('eps', [1e-7, 1e-4])
@pytest.mark.parametrize('kind', ['noise', 'colour_line'])
def test_the_content_picture_itself_costs_eps_only(kind, eps):
    """With iterate == content every plane is an exact affine function of I with a coefficient vector of
    length at most 1, so only eps |a|^2 is left: loss / scale <= 3 eps (H - 2)(W - 2)."""
    hw = (37, 53)
    _, content = getattr(photo_ref, kind)(hw, 5)
    loss, grad = photo_ref.photo_loss(content, content, eps, scale=3.0)
    assert 0 < loss / 3.0 <= 3 * eps * (hw[0] - 2) * (hw[1] - 2)
    assert np.abs(grad).max() <= 1e-2          # (of the order of eps, against ~1 for a noise iterate)


def test_flat_content_leaves_the_centred_plane():
    hw = (9, 13)
    img, content = photo_ref.flat(hw, 3)
    r, a = photo_ref.window_fit(img, content, 1e-7)
    assert np.abs(a).max() <= 1e-12          # (exactly 0 but for the rounding of the mean of nine equal values)
    v = photo_ref._windows(np.float64(img) / 255.0)
    assert np.abs(r - (v - v.mean(axis=2, keepdims=True))).max() <= 1e-15


def test_the_emulations_that_price_the_gpu_bounds():
    """On the colour-line picture at eps = 1e-7, window algebra in float32 misses the GPU tests' 2e-5 by more
    than an order of magnitude, while float64 window algebra with float32 residuals and sums sits near 1e-7:
    the case separates the two designs."""
    img, content = photo_ref.colour_line((96, 128))
    _, grad = photo_ref.photo_loss(img, content, 1e-7)
    top = np.abs(grad).max()
    all32 = np.abs(np.float64(photo_ref.all_float32(img, content, 1e-7, 1.0)) - grad).max() / top
    mixed = np.abs(np.float64(photo_ref.emulate(img, content, 1e-7, 1.0)) - grad).max() / top
    print('colour line, eps 1e-7: float32 algebra %.3g, float64 algebra with float32 residuals %.3g of max|grad|'
          % (all32, mixed))
    assert all32 > 10 * 2e-5 and mixed < 2e-5 / 10


# ------------------------------------------------------------------------------ options
def test_options_are_absent_unless_given():
    args = parse_args(None, BASE, config_py=False)
    assert 'photo_weight' not in args and 'photo_eps' not in args
    assert not hasattr(args, 'photo_weight') and getattr(args, 'photo_weight', 0) == 0
    assert check_photo_options(args) == PHOTO_EPS_DEFAULT == 1e-7
    args = parse_args(None, BASE + ['--photo-weight', '1e4'], config_py=False)
    assert args.photo_weight == 1e4 and 'photo_eps' not in args
    args = parse_args(None, BASE + ['--photo-weight', '1/2', '--photo-eps', '1e-5'], config_py=False)
    assert args.photo_weight == 0.5 and args.photo_eps == 1e-5 and check_photo_options(args) == 1e-5


@pytest.mark.parametrize('eps', ['0', '-1e-7', '-1/3'])
def test_a_bad_eps_is_refused_before_any_gpu_work(eps):
    with pytest.raises(ValueError) as err:
        parse_args(None, BASE + ['--photo-weight', '1', '--photo-eps=' + eps], config_py=False)
    assert '--photo-eps' in str(err.value)


@pytest.mark.parametrize('eps', ['nan', 'inf'])
def test_an_eps_that_is_not_finite_is_refused_wherever_it_comes_from(eps, tmp_path, capsys):
    """On the command line the option's type (a decimal or a fraction) has no such value; a config file can
    write one, and is refused by check_photo_options."""
    with pytest.raises(SystemExit):
        parse_args(None, BASE + ['--photo-weight', '1', '--photo-eps=' + eps], config_py=False)
    assert '--photo-eps' in capsys.readouterr().err
    config = tmp_path / 'config.py'
    config.write_text("photo_weight = 1.0\nphoto_eps = float('%s')\n" % eps)
    with pytest.raises(ValueError) as err:
        parse_args(None, BASE + ['--config', str(config)], config_py=False)
    assert '--photo-eps' in str(err.value)
    with pytest.raises(ValueError):
        check_photo_options(Namespace(photo_eps=float(eps)))


def test_the_symbol_is_exported_with_its_signature():
    so = ctypes.CDLL(lib.LIB_PATH)
    assert hasattr(so, 'stx_image_photo')
    i, vp, d = ctypes.c_int, ctypes.c_void_p, ctypes.c_double
    assert lib.SIGNATURES['stx_image_photo'] == [vp, vp, vp, vp, i, i, d, d, lib.c_double_p]
    # null arguments are refused with a status and a message that names them, without an engine or a GPU
    assert lib.load().stx_image_photo(None, None, None, None, 8, 8, 1e-7, 1.0, None) == -1
    assert 'null' in lib.load().stx_last_error().decode()


# ------------------------------------------------------------------------------ composition
class _Array:
    live = []

    def __init__(self, shape, data=None):
        self.shape, self.data, self.ptr = tuple(shape), data, object()
        _Array.live.append(self)

    def free(self):
        assert self.ptr is not None, 'freed twice'
        self.ptr = None
        _Array.live.remove(self)

    def copy_from(self, other):
        pass


class _Engine:
    def to_device(self, array):
        return _Array(array.shape, np.array(array))

    def empty(self, shape):
        return _Array(shape)


class _Feat:
    def free(self):
        pass


class _Loss:
    def __init__(self):
        self.added = []

    def add(self, term, engine):
        self.added.append(term)


class _Farm:
    def __init__(self):
        self.master = _Engine()

    def layers(self):
        return ['conv1_1', 'conv4_2']

    def layer_info(self, layer):
        return 8, 512

    def prepare_features_device(self, picture, layers, tile, passes=10, roll=None):
        return {layer: _Feat() for layer in layers}

    def gram_matrix(self, feat):
        return np.zeros((2, 2), np.float32)

    def set_contents_and_styles(self, contents, styles):
        pass

    def eval_sc_grad(self, *a, **kw):
        return _Loss()


def _fake_run(monkeypatch, options, sizes=(45, 64), evaluations=2):
    """StyleTransfer.transfer at ``sizes``, one scale after the other, on a farm and an engine that compute
    nothing; the step loop is replaced by ``evaluations`` calls of eval_loss_and_grad.  Returns (the
    StyleTransfer, the photo_loss calls, per scale the arrays alive after it)."""
    from style_transfer_amd.transfer import StyleTransfer
    _Array.live = []
    state = Namespace()
    args = parse_args(state, BASE + ['--style-layers', 'conv1_1', '--tv-weight', '0', '--p-weight', '0'] +
                      options, config_py=False)
    st = StyleTransfer(_Farm(), args, state)
    calls, losses = [], []

    def fake_photo(engine, img, grad, content, eps, scale):
        calls.append(dict(img=img, grad=grad, content=content, eps=eps, scale=scale))
        return 'photo term %d' % len(calls)

    def fake_loop(self, iterations, *rest):
        sc_args = (np.int32([0, 0]), ['conv4_2'], ['conv1_1'], [1.0], [1.0], [], [], None)
        for _ in range(evaluations):
            losses.append(self.eval_loss_and_grad(self.img, sc_args)[0])
    monkeypatch.setattr(image_ops, 'photo_loss', fake_photo)
    monkeypatch.setattr(StyleTransfer, '_step_loop', fake_loop)
    rng = np.random.RandomState(0)
    alive, contents = [], []
    for size in sizes:
        content = Image.fromarray(np.uint8(rng.uniform(0, 255, (size, size + 1, 3))))
        style = Image.fromarray(np.uint8(rng.uniform(0, 255, (40, 40, 3))))
        if st.img is not None:
            st.img.free()
        st.img = st.engine.to_device(st.pil_to_image(content))
        st.transfer(3, [content], [style])
        contents.append(st.pil_to_image(content))
        alive.append(list(_Array.live))
    return st, calls, losses, alive, contents


def test_transfer_keeps_one_content_copy_per_scale_and_makes_one_call_per_evaluation(monkeypatch, capsys):
    st, calls, losses, alive, contents = _fake_run(monkeypatch, ['--photo-weight', '1e4', '--photo-eps', '1e-5'])
    capsys.readouterr()
    assert len(calls) == 4                                   # one per evaluation
    lw = st.layer_weights['data']
    for i, call in enumerate(calls):
        want = contents[i // 2]
        assert call['content'].shape == call['img'].shape == want.shape
        assert np.array_equal(call['content'].data, want)    # the content picture at that scale's size
        assert call['img'] is st.img or i < 2
        assert call['grad'] is st.grad or i < 2
        assert call['eps'] == 1e-5 and call['scale'] == lw * 1e4
        assert losses[i].added == ['photo term %d' % (i + 1)]       # the only full-image term that is on
    assert calls[0]['content'] is calls[1]['content'] and calls[2]['content'] is calls[3]['content']
    assert calls[0]['content'].ptr is None and calls[2]['content'] is st.content_picture    # the old one is freed
    # alive after a scale: the iterate, the gradient, the previous average and one content copy
    assert [len(a) for a in alive] == [4, 4]


def test_the_options_are_read_at_every_evaluation(monkeypatch, capsys):
    """A config file may bind them to the run state: callables in the namespace see it at every read."""
    st, calls, _, _, _ = _fake_run(monkeypatch, ['--photo-weight', '2'], sizes=(45,), evaluations=0)
    st.args.photo_weight = lambda state: 10.0 * (state.step + 1)
    st.args.photo_eps = lambda state: 1e-6 if state.step else 1e-4
    sc_args = (np.int32([0, 0]), ['conv4_2'], ['conv1_1'], [1.0], [1.0], [], [], None)
    for step in (0, 1):
        st.state.step = step
        st.eval_loss_and_grad(st.img, sc_args)
    capsys.readouterr()
    assert [(c['scale'], c['eps']) for c in calls] == [(10.0, 1e-4), (20.0, 1e-6)]
    st.args.photo_eps = lambda state: -1.0
    with pytest.raises(ValueError, match='--photo-eps'):
        st.eval_loss_and_grad(st.img, sc_args)
    st.args.photo_eps = 1e-7
    st.args.photo_weight = 0                                 # off for this evaluation: no call
    st.eval_loss_and_grad(st.img, sc_args)
    assert len(calls) == 2


def test_the_copy_of_preserve_color_luma_is_shared(monkeypatch, capsys):
    st, calls, _, alive, _ = _fake_run(monkeypatch, ['--photo-weight', '1', '--preserve-color', 'luma'])
    capsys.readouterr()
    assert st.preserve_color == 'luma' and calls[-1]['content'] is st.content_picture       # the one kept picture
    assert calls[0]['content'].ptr is None                   # freed once, by the code that made it
    assert calls[0]['eps'] == 1e-7                           # the default
    assert [len(a) for a in alive] == [4, 4]


def test_without_the_option_no_call_and_no_allocation(monkeypatch, capsys):
    for options in ([], ['--photo-weight', '0'], ['--photo-eps', '1e-5']):
        st, calls, losses, alive, _ = _fake_run(monkeypatch, options)
        capsys.readouterr()
        assert calls == [] and st.content_picture is None
        assert all(loss.added == [] for loss in losses) and len(losses) == 4
        assert [len(a) for a in alive] == [3, 3]             # the iterate, the gradient, the previous average


def test_a_picture_without_a_window_is_refused_before_the_call(monkeypatch, capsys):
    from style_transfer_amd.transfer import StyleTransfer
    st, calls, _, _, _ = _fake_run(monkeypatch, ['--photo-weight', '1'], sizes=(45,), evaluations=0)
    st.img.free()
    st.img = st.engine.to_device(np.zeros((3, 2, 40), np.float32))
    content = Image.fromarray(np.zeros((2, 40, 3), np.uint8))
    with pytest.raises(ValueError, match='--photo-weight.*3 x 3 window'):
        st.transfer(1, [content], [content])
    capsys.readouterr()
    assert calls == []
