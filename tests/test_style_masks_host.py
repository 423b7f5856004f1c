"""Spatial control (--style-masks) without a GPU: the reference arithmetic the GPU tests lean on
(tests/masked_style_ref.py) and the command line."""

import numpy as np
import pytest

from oracle.caffe_net import synthetic_weights
from style_transfer_amd.netspec import builtin_net
from tests.helpers import make_oracle
from tests.masked_style_ref import MaskedOracleModel, mask_map, masked_style_terms


def test_all_ones_masks_reproduce_the_plain_oracle_exactly():
    om, net = make_oracle('vgg19')
    mom = MaskedOracleModel(net.as_dicts(), synthetic_weights(net.as_dicts(), 0))
    rng = np.random.RandomState(5)
    cl, cw = ['conv3_2'], {'conv3_2': 0.05}
    sl = ['conv1_1', 'conv2_1', 'conv3_1']
    sw = {l: 1 / 3 for l in sl}
    full = rng.uniform(-110, 120, (3, 64, 72)).astype(np.float32)
    styles = [rng.uniform(-110, 120, (3, 40, 44)).astype(np.float32) for _ in range(2)]
    om.styles = [om.style_grams([s], sl, 512) for s in styles]
    om.contents = [om.prepare_features(full, cl, 512)]
    mom.styles, mom.contents = om.styles, om.contents
    mom.set_masks([np.ones(full.shape[1:], np.float32)] * 2, sl)
    tile = np.ascontiguousarray(full[:, 8:56, 16:56])          # 48 x 40
    ref = om.sc_grad_tile(tile, (8, 16), cl, sl, {'conv2_1': 1.5}, cw, sw)
    got = mom.sc_grad_tile(tile, (8, 16), cl, sl, {'conv2_1': 1.5}, cw, sw)
    assert got[0] == ref[0]
    assert np.array_equal(got[1], ref[1])
    # ... and the masks matter: a half plane changes both
    half = np.ones(full.shape[1:], np.float32)
    half[:, 30:] = 0
    mom.set_masks([half, 1 - half], sl)
    other = mom.sc_grad_tile(tile, (8, 16), cl, sl, {'conv2_1': 1.5}, cw, sw)
    assert other[0] != ref[0] and not np.array_equal(other[1], ref[1])


def _central_differences(fn, F, eps=1e-5):
    fd = np.zeros_like(F)
    for idx in np.ndindex(*F.shape):
        d = np.zeros_like(F)
        d[idx] = eps
        fd[idx] = (fn(F + d) - fn(F - d)) / (2 * eps)
    return fd


def test_masked_gradient_is_the_finite_difference_gradient():
    """The chain rule through the mask, in float64 (C = 4, a 5 x 6 map, a random mask), to 1e-6 relative
    after fitting the one constant, against central finite differences of L(F) = 1/2 |tril(gram(F * m)) -
    a tril(Gs)|^2 with D = tril(gram(F * m)) - a tril(Gs):

      * dL/dF is proportional to m * ((D + D^T) Fm): the diagonal of D counts twice;
      * the term's S = m * (sym(D) Fm), sym(D) = D + strict_lower(D)^T as the reference's ssymm reads it
        (num_utils.py:60-66), counts the diagonal once: it is the gradient of L with the diagonal entries of D
        at half weight (1/4 |sym(D)|^2), and differs from dL/dF by m * (diag(D) Fm) / (C HW) exactly.

    The reference's own unmasked term has that property (set m = 1), and an all-ones mask must reproduce it
    bit for bit, so S cannot be dL/dF itself: measured here, the best constant leaves 2e-1 of max between
    the two.  Both statements are held to 1e-6."""
    rng = np.random.RandomState(2)
    C, h, w = 4, 5, 6
    F = rng.standard_normal((C, h, w))
    m = rng.uniform(0, 1, (h, w))
    Gs = np.tril(rng.standard_normal((C, C)))
    _, aS, _, a = masked_style_terms(F, m, Gs)
    S = aS / a
    mm = m.ravel()

    def d_of(x):
        fm = x.reshape(C, -1) * mm
        return np.tril(fm @ fm.T / fm.size) - a * Gs, fm

    def fit(fd, g):
        k = float((fd * g).sum() / (g * g).sum())
        return k, float(np.abs(fd - k * g).max() / np.abs(fd).max())

    D, fm = d_of(F)
    assert a == pytest.approx(float((mm * mm).sum() / mm.size), rel=1e-15)
    # the loss as it is: 1/2 |tril(.)|^2
    fd = _central_differences(lambda x: masked_style_terms(x, m, Gs)[0], F)
    k, err = fit(fd, (mm * ((D + D.T) @ fm)).reshape(F.shape))
    assert k == pytest.approx(1.0 / F.size, rel=1e-6) and err <= 1e-6
    # the term's S: the same with the diagonal of D at half weight
    fd_half = _central_differences(lambda x: 0.25 * float(((lambda d: d + np.tril(d, -1).T)(d_of(x)[0]) ** 2).sum()), F)
    k, err = fit(fd_half, S)
    assert k == pytest.approx(1.0 / F.size, rel=1e-6) and err <= 1e-6
    # ... and the two differ by the diagonal alone
    diag = (mm * (np.diag(np.diag(D)) @ fm)).reshape(F.shape) / F.size
    assert np.abs(fd - fd_half - diag).max() <= 1e-6 * np.abs(fd).max()
    print('best fit of S to dL/dF leaves %.1e of max' % fit(fd, S)[1])


@pytest.mark.parametrize('s', [1, 2, 4, 8, 16])
def test_mask_map_is_the_block_mean(s):
    rng = np.random.RandomState(s)
    M = rng.uniform(0, 1, (37, 53))
    out = mask_map(M, s)
    assert out.shape == (-(-37 // s), -(-53 // s))
    const = mask_map(np.full((37, 53), 0.375), s)
    assert np.all(const == 0.375)
    ys = np.minimum((np.arange(out.shape[0]) + 1) * s, 37) - np.arange(out.shape[0]) * s
    xs = np.minimum((np.arange(out.shape[1]) + 1) * s, 53) - np.arange(out.shape[1]) * s
    area = np.outer(ys, xs)
    assert area.sum() == 37 * 53
    assert (out * area).sum() / area.sum() == pytest.approx(M.mean(), abs=1e-12)


def test_cli_option_is_absent_unless_given_and_counts_are_checked(tmp_path):
    from style_transfer_amd.config_system import parse_args
    base = ['-ci', 'c.png', '-si', 'a.png', 'b.png']
    args = parse_args(argv=base, config_py=False)
    assert 'style_masks' not in args and 'style_masks' not in repr(vars(args.ns))
    args = parse_args(argv=base + ['--style-masks', 'ma.png', 'mb.png'], config_py=False)
    assert args.style_masks == ['ma.png', 'mb.png']
    with pytest.raises(ValueError, match='style-masks'):
        parse_args(argv=base + ['--style-masks', 'ma.png'], config_py=False)


def test_transfer_refuses_a_wrong_mask_count_before_any_gpu_work():
    from argparse import Namespace
    from PIL import Image
    from style_transfer_amd.config_system import parse_args
    from style_transfer_amd.transfer import StyleTransfer

    class NoFarm:       # any use of the farm beyond its layer list would be GPU work
        master = None

        def layers(self):
            return builtin_net('vgg19').blob_names()

    args = parse_args(argv=['-ci', 'c.png', '-si', 'a.png', 'b.png'], config_py=False)
    st = StyleTransfer(NoFarm(), args, Namespace())
    pic = Image.new('RGB', (64, 64))
    with pytest.raises(ValueError, match='style-masks'):
        st.transfer_multiscale([pic], [pic, pic], style_masks=[Image.new('L', (64, 64))])


def test_dist_refuses_style_masks():
    from argparse import Namespace
    from style_transfer_amd.dist import broadcast_targets, refuse_unbroadcast_options
    refuse_unbroadcast_options(Namespace())
    with pytest.raises(NotImplementedError, match='style-masks'):
        refuse_unbroadcast_options(Namespace(style_masks=['a.png']))
    with pytest.raises(NotImplementedError, match='style-masks'):
        broadcast_targets([], [], 'cpu', args=Namespace(style_masks=['a.png']))
