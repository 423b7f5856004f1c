"""Host-side checks of the mean / std style term (--stat-weight): the float64 statement of its definition
(tests/stat_ref.py), the options, the refusals and the C ABI.  No GPU."""

from argparse import Namespace
import ctypes

import numpy as np
import pytest

from style_transfer_amd import lib
from style_transfer_amd.config_system import (STYLE_LAYERS_DEFAULT, check_stat_options, parse_args,
                                              stat_layer_args)
from style_transfer_amd.netspec import builtin_net
from style_transfer_amd.terms import StatTargets
from tests import stat_ref

BASE = ['-ci', 'c.png', '-si', 's.png']


def _blob(seed=0, shape=(6, 5, 7)):
    rng = np.random.RandomState(seed)
    F = np.maximum(rng.standard_normal(shape) * 2 + 0.5, 0)
    F[1] = 0.75                          # a constant channel
    mu, sd = stat_ref.feature_stats(F)
    return F, mu * rng.uniform(0.5, 1.5, mu.shape) + 0.1, sd * rng.uniform(0.5, 1.5, sd.shape)


def test_gradient_is_the_finite_difference_of_half_e():
    """S / n is d(E/2)/dF: the central difference in float64 agrees to 1e-6 of max |S / n|."""
    F, MU, SD = _blob()
    _, S, _, _ = stat_ref.stat_terms(F, MU, SD)
    g = S / (F.shape[1] * F.shape[2])
    scale = np.abs(g).max()
    worst = 0.0
    for index in np.ndindex(*F.shape):
        worst = max(worst, abs(stat_ref.finite_difference(F, MU, SD, index, 1e-5) - g[index]) / scale)
    print('finite difference: %.2e of max |S / n|' % worst)
    assert worst <= 1e-6


def test_statistics_on_target_give_zero():
    F, _, _ = _blob(1)
    mu, sd = stat_ref.feature_stats(F)
    half, S, asum, b = stat_ref.stat_terms(F, mu, sd)
    assert half == 0 and asum == 0 and not S.any() and not b.any()
    assert not stat_ref.normalized(S).any()          # 0 / (0 + EPS)


def test_options_are_absent_unless_set_and_default_to_the_style_layers():
    args = parse_args(argv=BASE, config_py=False)
    assert 'stat_weight' not in args and 'stat_layers' not in args          # the PNG comment is unchanged
    assert not any(name.startswith('stat') for name in vars(args.ns))
    assert stat_layer_args(args) == [] and check_stat_options(args) == []
    args = parse_args(argv=BASE + ['--stat-weight', '3/2'], config_py=False)
    assert args.stat_weight == 1.5 and 'stat_layers' not in args
    assert stat_layer_args(args) == list(STYLE_LAYERS_DEFAULT)
    args = parse_args(argv=BASE + ['--stat-weight', '1', '--style-layers', 'conv1_1:3', 'conv2_2'], config_py=False)
    assert stat_layer_args(args) == ['conv1_1', 'conv2_2']                  # the names, not the Gram weights
    args = parse_args(argv=BASE + ['--stat-weight', '1', '--style-layers'], config_py=False)
    assert args.style_layers == [] and stat_layer_args(args) == list(STYLE_LAYERS_DEFAULT)
    args = parse_args(argv=BASE + ['--stat-weight', '0', '--stat-layers', 'conv1_1'], config_py=False)
    assert stat_layer_args(args) == []                                       # weight 0: off


def test_layer_weights_go_through_parse_weights():
    from style_transfer_amd.transfer import parse_weights
    args = parse_args(argv=BASE + ['--stat-weight', '2', '--stat-layers', 'conv1_1:3', 'conv3_1'], config_py=False)
    names, weights = parse_weights(stat_layer_args(args), args.stat_weight)
    assert names == ['conv1_1', 'conv3_1'] and weights == {'conv1_1': 1.5, 'conv3_1': 0.5}
    assert check_stat_options(args, builtin_net('vgg19').blob_names()) == names


def test_refused_with_style_masks():
    with pytest.raises(ValueError, match='--stat-weight.*--style-masks'):
        parse_args(argv=BASE + ['--stat-weight', '1', '--style-masks', 'm.png'], config_py=False)


def test_refused_for_an_unknown_layer_before_any_gpu_work():
    from style_transfer_amd.transfer import StyleTransfer
    layers = builtin_net('vgg19').blob_names()
    args = parse_args(argv=BASE + ['--stat-weight', '1', '--stat-layers', 'conv9_9'], config_py=False)
    with pytest.raises(ValueError, match="--stat-layers.*'conv9_9'"):
        check_stat_options(args, layers)
    for bad in (['data'], ['conv1_1', 'conv1_1'], ['conv1_1:x']):
        with pytest.raises(ValueError, match='--stat-layers'):
            check_stat_options(Namespace(stat_weight=1.0, stat_layers=bad, style_layers=[]), layers)

    class NoFarm:       # (no engine: the refusal comes before anything touches one)
        master = None

        def layers(self):
            return layers
    with pytest.raises(ValueError, match='--stat-layers'):
        StyleTransfer(NoFarm(), args, Namespace())
    # ... and the command line refuses it before it wakes a GPU
    from style_transfer_amd import cli
    woken = []
    original = cli.TileFarm
    cli.TileFarm = lambda *a, **k: woken.append(a)
    try:
        with pytest.raises(ValueError, match='--stat-layers'):
            cli.main(BASE + ['--model', 'vgg19', '--stat-weight', '1', '--stat-layers', 'conv9_9'])
    finally:
        cli.TileFarm = original
    assert not woken


def test_dist_refuses_stat_weight():
    from style_transfer_amd.dist import broadcast_targets, refuse_unbroadcast_options
    refuse_unbroadcast_options(Namespace())
    refuse_unbroadcast_options(Namespace(stat_weight=0))
    with pytest.raises(NotImplementedError, match='--stat-weight'):
        refuse_unbroadcast_options(Namespace(stat_weight=1.0))
    with pytest.raises(NotImplementedError, match='--stat-weight'):
        broadcast_targets([], [], 'cpu', args=Namespace(stat_weight=1.0))


def test_abi_symbols_are_present_and_bound():
    so = ctypes.CDLL(lib.LIB_PATH)
    for name in ('stx_set_stat_targets', 'stx_feature_stats', 'stx_op_stat_terms'):
        assert hasattr(so, name) and name in lib.SIGNATURES
    assert [f[0] for f in lib.StatTarget._fields_] == ['layer', 'channels', 'mean', 'sd', 'mem', 'weight']
    # NULL arguments are rejected with a status, never a crash
    assert lib.load().stx_set_stat_targets(None, None, 0) == -1
    assert lib.load().stx_feature_stats(None, None, 0, 1, 1, None, None, 0) == -1


def test_refused_when_every_layer_weight_is_zero():
    for layers in (['conv1_1:0'], ['conv1_1:0', 'conv2_1:0/3']):
        with pytest.raises(ValueError, match='--stat-layers.*must not be 0'):
            parse_args(argv=BASE + ['--stat-weight', '1', '--stat-layers'] + layers, config_py=False)
    args = parse_args(argv=BASE + ['--stat-weight', '1', '--stat-layers', 'conv1_1:0', 'conv2_1'], config_py=False)
    assert check_stat_options(args) == ['conv1_1', 'conv2_1']


class _Feat:
    def __init__(self, array):
        self.array, self.freed = array, False

    def free(self):
        assert not self.freed
        self.freed = True


class _FakeFarm:
    """A farm whose feature map of a picture at a layer is a fixed function of the picture: the host side of
    preprocess_images -- which layers it asks for, what it averages and over how many variants -- without a GPU."""
    master = None
    STRIDE = {'conv1_1': 1, 'conv2_2': 2, 'conv3_1': 4}

    def __init__(self):
        self.passes, self.feats, self.sent = [], [], []

    def layers(self):
        return list(self.STRIDE)

    @classmethod
    def feature(cls, picture, layer):
        s = cls.STRIDE[layer]
        return np.maximum(picture[:, ::s, ::s] * np.float32(0.01 * s) + np.float32(0.2), 0)

    def prepare_features_device(self, picture, layers, tile, passes=10, roll=None):
        self.passes.append(list(layers))
        feats = {layer: _Feat(self.feature(picture, layer)) for layer in layers}
        self.feats += feats.values()
        return feats

    def feature_stats(self, feat):
        mu, sd = stat_ref.feature_stats(feat.array)
        return mu.astype(np.float32), sd.astype(np.float32)

    def gram_matrix(self, feat):
        f = feat.array.reshape(feat.array.shape[0], -1)
        return np.float32(f @ f.T / f.size)

    def set_stat_targets(self, targets, weights=None):
        self.sent.append((targets, weights))


def _fake_transfer(*options):
    from style_transfer_amd.transfer import StyleTransfer
    args = parse_args(argv=BASE + ['--stat-weight', '1', '--stat-layers', 'conv1_1', 'conv2_2',
                                   '--style-layers', 'conv1_1', 'conv3_1'] + list(options), config_py=False)
    farm = _FakeFarm()
    return StyleTransfer(farm, args, Namespace()), farm


def test_targets_are_the_equal_weight_average_over_style_pictures_and_ladder_sizes(capsys):
    """Two style pictures at three ladder sizes each: (mean, sd) at a statistics layer is the plain average of
    the six feature maps' own (mean, sd), as the Gram is; the features are taken once per variant, at the
    union of both layer lists; a layer of one list only gets only that list's target."""
    from PIL import Image
    st, farm = _fake_transfer('--style-multiscale', '32', '64')
    rng = np.random.RandomState(3)
    pictures = [Image.fromarray(np.uint8(rng.uniform(0, 255, (n, n, 3)))) for n in (64, 50)]
    variants = [st.pil_to_image(v) for i, p in enumerate(pictures) for v in st._style_variants(i, p)]
    assert sorted(v.shape[1] for v in variants) == [32, 32, 45, 45, 50, 64]
    stat, = [term for term in st.target_terms if isinstance(term, StatTargets)]
    stat.layers = ['conv1_1', 'conv2_2']
    st.preprocess_images([], pictures, [], ['conv1_1', 'conv3_1'])
    capsys.readouterr()
    assert farm.passes == [['conv1_1', 'conv3_1', 'conv2_2']] * 6
    assert all(feat.freed for feat in farm.feats)
    assert sorted(stat.targets) == ['conv1_1', 'conv2_2'] and sorted(st.styles[0]) == ['conv1_1', 'conv3_1']
    for layer, (mean, sd) in stat.targets.items():
        each = [stat_ref.feature_stats(farm.feature(v, layer)) for v in variants]
        want_mean, want_sd = np.mean([e[0] for e in each], axis=0), np.mean([e[1] for e in each], axis=0)
        assert mean.dtype == np.float32 and mean.shape == sd.shape == (3,)
        # six float32 values summed and divided in float32: a few ulp
        assert np.allclose(mean, want_mean, rtol=1e-6, atol=0) and np.allclose(sd, want_sd, rtol=1e-6, atol=0)
        assert np.ptp([e[0][0] for e in each]) > 1e-3 * abs(want_mean[0])          # (the six do differ)
    for layer, gram in st.styles[0].items():
        want = np.mean([farm.gram_matrix(_Feat(farm.feature(v, layer))) for v in variants], axis=0)
        assert np.allclose(gram, want, rtol=1e-6, atol=0)


def test_only_the_layers_of_the_scale_are_sent_and_a_layer_without_a_target_is_refused():
    """--style-multiscale keeps the first scale's targets while the weights are read again every scale."""
    st, farm = _fake_transfer()
    one = (np.zeros(3, np.float32), np.ones(3, np.float32))
    stat, = [term for term in st.target_terms if isinstance(term, StatTargets)]
    stat.targets = {'conv1_1': one, 'conv2_2': one}
    stat.weights = None
    stat.send(st)
    assert farm.sent == []
    stat.weights = {'conv2_2': 1.0}                    # the list was re-read without conv1_1
    stat.send(st)
    assert list(farm.sent[-1][0]) == ['conv2_2'] and farm.sent[-1][1] == {'conv2_2': 1.0}
    stat.weights = {'conv2_2': 0.5, 'conv3_1': 0.5}    # ... and with a layer that has no target
    with pytest.raises(ValueError, match='--stat-layers conv3_1.*--style-multiscale'):
        stat.send(st)
    assert len(farm.sent) == 1
