"""Spatial control of the content term (--content-mask) without a GPU: the options, the refusals, the float64
reference (tests/content_mask_ref.py) and the resize / roll helpers."""

from argparse import Namespace

import numpy as np
import pytest
from PIL import Image

from oracle.caffe_net import synthetic_weights
from oracle.num_ops import EPS
from oracle.tile_path import OracleModel
from style_transfer_amd.netspec import builtin_net
from tests.content_mask_ref import MaskedContentOracleModel, masked_content_gradient, masked_content_terms

BASE = ['-ci', 'c.png', '-si', 'a.png']


# ------------------------------------------------------------------------------------- the options
def test_option_is_absent_unless_given():
    from style_transfer_amd.cli import image_comment
    from style_transfer_amd.config_system import check_content_mask, parse_args
    bare = parse_args(Namespace(), BASE, config_py=False)
    assert 'content_mask' not in bare and 'content_mask' not in repr(vars(bare.ns))
    assert check_content_mask(bare) is None
    assert 'content_mask' not in image_comment(bare, BASE)
    given = parse_args(Namespace(), BASE + ['--content-mask', 'm.png'], config_py=False)
    assert given.content_mask == 'm.png' and check_content_mask(given) == 'm.png'
    comment = image_comment(given, BASE + ['--content-mask', 'm.png'])
    assert "content_mask='m.png'" in comment
    # nothing else of the comment moves: without the option it is what it was
    assert comment.replace(", content_mask='m.png'", '').replace(' --content-mask m.png', '') == \
        image_comment(bare, BASE)


def test_refused_without_content_layers_before_any_gpu_work():
    from style_transfer_amd.config_system import parse_args
    from style_transfer_amd.transfer import StyleTransfer
    with pytest.raises(ValueError, match='--content-mask needs a content term: --content-layers is empty'):
        parse_args(argv=BASE + ['--content-mask', 'm.png', '--content-layers'], config_py=False)

    class NoFarm:       # any use of the farm beyond its layer list would be GPU work
        master = None

        def layers(self):
            return builtin_net('vgg19').blob_names()

    args = parse_args(argv=BASE + ['--content-layers'], config_py=False)
    st = StyleTransfer(NoFarm(), args, Namespace())
    pic = Image.new('RGB', (64, 64))
    with pytest.raises(ValueError, match='--content-mask needs a content term'):
        st.transfer_multiscale([pic], [pic], content_mask=Image.new('L', (64, 64)))


def test_dist_refuses_content_mask():
    from style_transfer_amd.dist import broadcast_targets, refuse_unbroadcast_options
    refuse_unbroadcast_options(Namespace())
    with pytest.raises(NotImplementedError, match='--content-mask is not implemented for the one-process-per-GPU'):
        refuse_unbroadcast_options(Namespace(content_mask='m.png'))
    with pytest.raises(NotImplementedError, match='content-mask'):
        broadcast_targets([], [], 'cpu', args=Namespace(content_mask='m.png'))


# ----------------------------------------------------------------------------------- the reference
def _central_differences(f, x, h=1e-5):
    g = np.empty_like(x)
    for idx in np.ndindex(*x.shape):
        xp, xm = x.copy(), x.copy()
        xp[idx] += h
        xm[idx] -= h
        g[idx] = (f(xp) - f(xm)) / (2 * h)
    return g


def test_reference_gradient_is_m_times_d():
    """dE/dF of E = 1/2 sum m d^2 is m d: central differences in float64 on a 3 x 5 x 6 blob, ramp mask."""
    rng = np.random.RandomState(3)
    F, c = rng.standard_normal((3, 5, 6)), rng.standard_normal((3, 5, 6))
    m = np.outer(np.linspace(0.1, 1, 5), np.linspace(0, 1, 6))
    E, S, asum, a = masked_content_terms(F, c, m)
    assert a == pytest.approx(m.mean(), rel=1e-15)
    fd = _central_differences(lambda x: masked_content_terms(x, c, m)[0], F)
    md = m * (F - c)
    err = float(np.abs(fd - md).max() / np.abs(md).max())
    print('finite differences against m d: %.1e' % err)
    assert err <= 1e-8
    assert np.allclose(S, a * md, rtol=1e-15, atol=0) and asum == pytest.approx(np.abs(md).sum(), rel=1e-15)
    assert np.array_equal(masked_content_terms(F, c, np.zeros((5, 6)))[1], np.zeros_like(F))
    assert not masked_content_gradient(F, c, np.zeros((5, 6))).any()        # 0 / EPS


TILE, START = (40, 36), (8, 16)
CL, CW = ['conv2_2', 'conv3_2'], {'conv2_2': 0.02, 'conv3_2': 0.05}
SL, SW, LW = ['conv1_1', 'conv2_1'], {'conv1_1': 0.5, 'conv2_1': 0.5}, {'conv2_1': 1.5}


def _oracles():
    net = builtin_net('vgg19')
    weights = synthetic_weights(net.as_dicts(), 0)
    plain, masked = OracleModel(net.as_dicts(), weights), MaskedContentOracleModel(net.as_dicts(), weights)
    rng = np.random.RandomState(5)
    full = rng.uniform(-110, 120, (3, 64, 64)).astype(np.float32)
    style = rng.uniform(-110, 120, (3, 40, 44)).astype(np.float32)
    plain.styles = masked.styles = [plain.style_grams([style], SL, 512)]
    plain.contents = masked.contents = [plain.prepare_features(full, CL, 512)]
    tile = rng.uniform(-110, 120, (3,) + TILE).astype(np.float32)
    return plain, masked, tile


def test_reference_with_an_all_ones_mask_is_the_oracle_exactly():
    plain, masked, tile = _oracles()
    ref = plain.sc_grad_tile(tile, START, CL, SL, LW, CW, SW)
    masked.set_content_mask(np.ones((64, 64), np.float32), CL)
    got = masked.sc_grad_tile(tile, START, CL, SL, LW, CW, SW)
    assert got[0] == ref[0] and np.array_equal(got[1], ref[1])
    masked.set_content_mask(None, CL)
    got = masked.sc_grad_tile(tile, START, CL, SL, LW, CW, SW)
    assert got[0] == ref[0] and np.array_equal(got[1], ref[1])


def test_reference_with_a_uniform_mask_scales_the_content_term():
    """m == 0.25: the loss and the normalised gradient of the content term are 0.25 x the unmasked ones.  The
    loss exactly (up to rounding); the gradient up to the EPS of normalize: with q = mean |d|,
    a m d / (m q + EPS) = 0.25 d / (q + 4 EPS), against 0.25 d / (q + EPS) -- a relative 3 EPS / q, 4e-7 / q."""
    rng = np.random.RandomState(6)
    F, c = rng.standard_normal((3, 5, 6)), rng.standard_normal((3, 5, 6))
    ones, quarter = np.ones((5, 6)), np.full((5, 6), 0.25)
    E1, _, _, _ = masked_content_terms(F, c, ones)
    Eq, _, _, a = masked_content_terms(F, c, quarter)
    assert a == 0.25 and Eq == pytest.approx(0.25 * E1, rel=1e-12)
    g1, gq = masked_content_gradient(F, c, ones), masked_content_gradient(F, c, quarter)
    q = np.abs(F - c).mean()
    err = float(np.abs(gq - 0.25 * g1).max() / np.abs(0.25 * g1).max())
    print('uniform mask: gradient off by %.1e (3 EPS / q = %.1e)' % (err, 3 * EPS / q))
    assert err <= 1e-6 and err == pytest.approx(3 * EPS / q, rel=1e-3)
    # ... and through the oracle's float32 tile evaluation, content term alone
    plain, masked, tile = _oracles()
    ref = plain.sc_grad_tile(tile, START, CL, [], LW, CW, SW)
    masked.set_content_mask(np.full((64, 64), 0.25, np.float32), CL)
    got = masked.sc_grad_tile(tile, START, CL, [], LW, CW, SW)
    assert got[0] == pytest.approx(0.25 * ref[0], rel=1e-6)
    assert np.abs(got[1] - 0.25 * ref[1]).max() <= 1e-6 * np.abs(0.25 * ref[1]).max()


# ------------------------------------------------------------------------------------- the helpers
def test_resize_and_roll_helpers_match_numpy():
    from style_transfer_amd.transfer import mask_at_size, rolled_mask
    rng = np.random.RandomState(7)
    u8 = np.uint8(rng.uniform(0, 256, (37, 53)))
    pic = Image.fromarray(u8)
    same = mask_at_size(pic, (37, 53))
    assert same.dtype == np.float32 and np.array_equal(same, np.float32(u8) / np.float32(255))
    assert np.array_equal(mask_at_size(pic.convert('RGB'), (37, 53)),
                          np.float32(np.asarray(pic.convert('RGB').convert('L'))) / np.float32(255))
    small = mask_at_size(pic, (19, 27))
    want = np.float32(np.asarray(pic.resize((27, 19), Image.LANCZOS))) / np.float32(255)
    assert small.shape == (19, 27) and np.array_equal(small, np.clip(want, 0, 1))
    assert small.min() >= 0 and small.max() <= 1
    assert rolled_mask(same, None) is same
    for roll in ((5, -9), (-60, 40), (0, 0)):       # (x, y), as the step loop's roll
        assert np.array_equal(rolled_mask(same, roll), np.roll(np.roll(same, roll[0], axis=1), roll[1], axis=0))
