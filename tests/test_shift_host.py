"""Host-side checks of the shifted-Gram style term (--shift-weight): the float64 statement of its definition
(tests/shift_ref.py), the options, the refusals and the C ABI.  No GPU."""

from argparse import Namespace
import ctypes

import numpy as np
import pytest

from style_transfer_amd import lib, terms
from style_transfer_amd.config_system import (SHIFT_LAYERS_DEFAULT, check_shift_options, check_shift_tile, parse_args,
                                              shift_layer_args, shift_offsets)
from style_transfer_amd.netspec import builtin_net
from tests import shift_ref

BASE = ['-ci', 'c.png', '-si', 's.png']


def _blob(seed, shape):
    rng = np.random.RandomState(seed)
    F = np.maximum(rng.standard_normal(shape) * 2 + 0.5, 0)
    F[1] = 0                            # an all-zero channel
    return F, rng


@pytest.mark.parametrize('shape,offsets', [((8, 5, 7), [(0, 1), (1, 0), (0, 6), (4, 0), (0, 3)]),
                                           ((4, 3, 9), [(0, 8), (2, 0), (0, 2), (1, 0)])])
def test_gradient_is_the_finite_difference_of_half_e(shape, offsets):
    """S / (C n) is d(E/2)/dF: the central difference in float64 agrees to 1e-6 of max |S / (C n)|."""
    F, rng = _blob(shape[0], shape)
    X = shift_ref.shift_gram(F, offsets)
    T = X * rng.uniform(0.5, 1.5, X.shape)
    _, S, _ = shift_ref.shift_terms(F, offsets, T)
    g = S / F.size
    scale = np.abs(g).max()
    worst = 0.0
    for index in np.ndindex(*F.shape):
        worst = max(worst, abs(shift_ref.finite_difference(F, offsets, T, index, 1e-4) - g[index]) / scale)
    print('finite difference: %.2e of max |S / (C n)|' % worst)
    assert worst <= 1e-6


def test_shift_gram_is_the_pairwise_definition():
    """The matrix form against the definition spelled out pair by pair; not symmetric; (0, 0) would be the Gram."""
    F, _ = _blob(2, (3, 4, 5))
    for dy, dx in [(0, 2), (3, 0)]:
        X = shift_ref.shift_gram(F, [(dy, dx)])[0]
        want = np.zeros((3, 3))
        for y in range(4 - dy):
            for x in range(5 - dx):
                want += np.outer(F[:, y, x], F[:, y + dy, x + dx])
        assert np.allclose(X, want / (3 * (4 - dy) * (5 - dx)), rtol=1e-13, atol=0)
    assert not np.allclose(shift_ref.shift_gram(F, [(0, 1)])[0], shift_ref.shift_gram(F, [(0, 1)])[0].T)
    with pytest.raises(ValueError):
        shift_ref.shift_gram(F, [(0, 5)])


def test_own_targets_give_exactly_zero():
    F, _ = _blob(1, (6, 5, 7))
    offsets = [(0, 1), (2, 0), (0, 6)]
    half, S, asum = shift_ref.shift_terms(F, offsets, shift_ref.shift_gram(F, offsets))
    assert half == 0 and asum == 0 and not S.any()
    assert not shift_ref.normalized(S).any()         # 0 / (0 + EPS)


def test_options_are_absent_unless_set_and_have_their_defaults():
    args = parse_args(argv=BASE, config_py=False)
    assert not any(name.startswith('shift') for name in vars(args.ns))      # the PNG comment is unchanged
    assert shift_layer_args(args) == [] and check_shift_options(args) == []
    args = parse_args(argv=BASE + ['--shift-weight', '3/2'], config_py=False)
    assert args.shift_weight == 1.5 and 'shift_layers' not in args and 'shift_offsets' not in args
    assert shift_layer_args(args) == list(SHIFT_LAYERS_DEFAULT) == ['conv1_1', 'conv2_1', 'conv3_1']
    assert shift_offsets(args) == [(0, 2), (2, 0), (0, 4), (4, 0), (0, 8), (8, 0)]
    args = parse_args(argv=BASE + ['--shift-weight', '1', '--shift-offsets', '3', '1'], config_py=False)
    assert shift_offsets(args) == [(0, 3), (3, 0), (0, 1), (1, 0)]
    args = parse_args(argv=BASE + ['--shift-weight', '0', '--shift-layers', 'conv1_1'], config_py=False)
    assert shift_layer_args(args) == []                                      # weight 0: off


def test_layer_weights_go_through_parse_weights():
    args = parse_args(argv=BASE + ['--shift-weight', '2', '--shift-layers', 'conv1_1:3', 'conv3_1'], config_py=False)
    names, weights = terms.parse_weights(shift_layer_args(args), args.shift_weight)
    assert names == ['conv1_1', 'conv3_1'] and weights == {'conv1_1': 1.5, 'conv3_1': 0.5}
    assert check_shift_options(args, builtin_net('vgg19').blob_names()) == names


def test_bad_offsets_are_refused():
    for bad in (['0'], ['-2'], ['2', '2'], [str(d) for d in range(1, 10)]):
        with pytest.raises(ValueError, match='--shift-offsets'):
            parse_args(argv=BASE + ['--shift-weight', '1', '--shift-offsets'] + bad, config_py=False)
    for bad in (True, 2.0, [1.5], [], 'x', [True]):
        with pytest.raises(ValueError, match='--shift-offsets'):
            shift_offsets(Namespace(shift_weight=1.0, shift_offsets=bad))
    assert shift_offsets(Namespace(shift_offsets=5)) == [(0, 5), (5, 0)]
    assert len(shift_offsets(Namespace(shift_offsets=list(range(1, 9))))) == 16      # the library's most


def test_refused_with_style_masks_an_unknown_layer_and_zero_weights():
    with pytest.raises(ValueError, match='--shift-weight.*--style-masks'):
        parse_args(argv=BASE + ['--shift-weight', '1', '--style-masks', 'm.png'], config_py=False)
    layers = builtin_net('vgg19').blob_names()
    args = parse_args(argv=BASE + ['--shift-weight', '1', '--shift-layers', 'conv9_9'], config_py=False)
    with pytest.raises(ValueError, match="--shift-layers.*'conv9_9'"):
        check_shift_options(args, layers)
    for bad in (['data'], ['conv1_1', 'conv1_1'], ['conv1_1:x']):
        with pytest.raises(ValueError, match='--shift-layers'):
            check_shift_options(Namespace(shift_weight=1.0, shift_layers=bad), layers)
    with pytest.raises(ValueError, match='--shift-layers.*must not be 0'):
        parse_args(argv=BASE + ['--shift-weight', '1', '--shift-layers', 'conv1_1:0'], config_py=False)
    # ... and the command line refuses it before it wakes a GPU
    from style_transfer_amd import cli
    woken = []
    original = cli.TileFarm
    cli.TileFarm = lambda *a, **k: woken.append(a)
    try:
        with pytest.raises(ValueError, match='--shift-layers'):
            cli.main(BASE + ['--model', 'vgg19', '--shift-weight', '1', '--shift-layers', 'conv9_9'])
    finally:
        cli.TileFarm = original
    assert not woken


def test_target_terms_lists_the_term_behind_selfsim_and_before_the_masks():
    every = Namespace(stat_weight=1.0, nnfm_weight=1.0, swd_weight=1.0, selfsim_weight=1.0, shift_weight=1.0,
                      style_layers=[], content_layers=['conv4_2'])
    kinds = [type(term) for term in terms.target_terms(every, None)]
    assert kinds == [terms.StatTargets, terms.NnfmBanks, terms.SwdTargets, terms.SelfsimTargets, terms.ShiftTargets,
                     terms.Masks]
    assert [type(term) for term in terms.target_terms(Namespace(shift_weight=1.0), None)] == [terms.ShiftTargets,
                                                                                            terms.Masks]
    assert [type(term) for term in terms.target_terms(Namespace(), None)] == [terms.Masks]
    with pytest.raises(ValueError, match='--shift-offsets'):
        terms.target_terms(Namespace(shift_weight=1.0, shift_offsets=[0]), None)


def test_dist_refuses_shift_weight():
    from style_transfer_amd.dist import UNBROADCAST_OPTIONS, broadcast_targets, refuse_unbroadcast_options
    assert ('shift_weight', True, 'the shifted-Gram targets are') in UNBROADCAST_OPTIONS
    refuse_unbroadcast_options(Namespace(shift_weight=0))
    with pytest.raises(NotImplementedError, match='--shift-weight'):
        refuse_unbroadcast_options(Namespace(shift_weight=1.0))
    with pytest.raises(NotImplementedError, match='--shift-weight'):
        broadcast_targets([], [], 'cpu', args=Namespace(shift_weight=1.0))


def test_abi_symbols_are_present_and_bound():
    so = ctypes.CDLL(lib.LIB_PATH)
    for name in ('stx_set_shift_targets', 'stx_shift_gram', 'stx_op_shift_terms'):
        assert hasattr(so, name) and name in lib.SIGNATURES
    assert [f[0] for f in lib.ShiftTarget._fields_] == ['layer', 'channels', 'n_offsets', 'offsets', 'grams', 'mem',
                                                        'weight']
    # NULL arguments are rejected with a status, never a crash
    assert lib.load().stx_set_shift_targets(None, None, 0) == -1
    assert lib.load().stx_shift_gram(None, None, 0, 32, 4, 4, None, 1, None) == -1
    assert lib.load().stx_op_shift_terms(None, None, 32, 4, 4, None, 1, None, None, None) == -1


# ------------------------------------------------------------------------------------- the host path
class _Feat:
    def __init__(self, array):
        self.array, self.shape = array, array.shape

    def free(self):
        pass


class _FakeFarm:
    """A farm whose feature map of a picture at a layer is a fixed function of the picture (no GPU)."""
    master = None
    STRIDE = {'conv1_1': 1, 'conv2_1': 2, 'conv3_1': 4}

    def __init__(self):
        self.passes, self.sent = [], []

    def layers(self):
        return list(self.STRIDE)

    def layer_info(self, layer):
        return self.STRIDE[layer], 32

    @classmethod
    def feature(cls, picture, layer):
        s = cls.STRIDE[layer]
        return np.maximum(picture[:, ::s, ::s] * np.float32(0.01 * s) + np.float32(0.2), 0)

    def prepare_features_device(self, picture, layers, tile, passes=10, roll=None):
        self.passes.append(list(layers))
        return {layer: _Feat(self.feature(picture, layer)) for layer in layers}

    def shift_gram(self, feat, offsets):
        return np.float32(shift_ref.shift_gram(feat.array, offsets))

    def gram_matrix(self, feat):
        f = feat.array.reshape(feat.array.shape[0], -1)
        return np.float32(f @ f.T / f.size)

    def set_shift_targets(self, targets, weights=None):
        self.sent.append((targets, weights))


def _fake_transfer(*options):
    from style_transfer_amd.transfer import StyleTransfer
    args = parse_args(argv=BASE + ['--shift-weight', '1', '--shift-layers', 'conv1_1', 'conv2_1', '--shift-offsets',
                                   '1', '3', '--style-layers', 'conv1_1', 'conv3_1', '--tile-size', '64'] +
                      list(options), config_py=False)
    farm = _FakeFarm()
    return StyleTransfer(farm, args, Namespace()), farm


def test_targets_are_the_average_over_the_variants_and_go_to_the_farm_with_their_offsets(capsys):
    from PIL import Image
    st, farm = _fake_transfer('--style-multiscale', '32', '64')
    rng = np.random.RandomState(3)
    pictures = [Image.fromarray(np.uint8(rng.uniform(0, 255, (n, n, 3)))) for n in (64, 50)]
    variants = [st.pil_to_image(v) for i, p in enumerate(pictures) for v in st._style_variants(i, p)]
    shift, = [term for term in st.target_terms if isinstance(term, terms.ShiftTargets)]
    st.img = np.zeros((3, 64, 64), np.float32)
    shift.read(st)
    offsets = [(0, 1), (1, 0), (0, 3), (3, 0)]
    assert shift.layers == ['conv1_1', 'conv2_1'] and shift.offsets == offsets
    assert shift.weights == {'conv1_1': 0.5, 'conv2_1': 0.5}
    st.preprocess_images([], pictures, [], ['conv1_1', 'conv3_1'])
    capsys.readouterr()
    assert farm.passes == [['conv1_1', 'conv3_1', 'conv2_1']] * len(variants)
    assert sorted(shift.targets) == ['conv1_1', 'conv2_1']
    for layer, (offs, T) in shift.targets.items():
        want = np.mean([shift_ref.shift_gram(farm.feature(v, layer), offsets) for v in variants], axis=0)
        assert offs == offsets and T.dtype == np.float32 and T.shape == (4, 3, 3)
        assert np.allclose(T, want, rtol=1e-6, atol=0)
    shift.send(st)
    sent, weights = farm.sent[-1]
    assert list(sent) == ['conv1_1', 'conv2_1'] and weights == shift.weights and sent['conv2_1'][0] == offsets
    shift.weights = {'conv2_1': 0.5, 'conv3_1': 0.5}        # a layer that has no target
    with pytest.raises(ValueError, match='--shift-layers conv3_1.*--style-multiscale'):
        shift.send(st)


def test_an_offset_that_leaves_a_tile_blob_without_a_pair_is_refused_per_scale():
    """A 64 x 64 tile is a 32 x 32 map at conv2_1: distance 31 still has a pair, 32 has none."""
    check_shift_tile([(0, 31), (31, 0)], 'conv2_1', 2, (64, 64))
    check_shift_tile([(0, 3)], 'conv3_1', 4, (13, 13))          # ceil(13 / 4) = 4 columns
    with pytest.raises(ValueError, match=r'--shift-offsets 32.*conv2_1.*--min-size'):
        check_shift_tile([(0, 31), (32, 0)], 'conv2_1', 2, (64, 64))
    with pytest.raises(ValueError, match=r'--shift-offsets 3.*conv3_1'):
        check_shift_tile([(0, 3)], 'conv3_1', 4, (64, 12))      # 3 columns
    st, farm = _fake_transfer('--shift-offsets', '1', '40')
    shift, = [term for term in st.target_terms if isinstance(term, terms.ShiftTargets)]
    st.img = np.zeros((3, 96, 128), np.float32)                 # tiles of 48 x 64: 24 x 32 maps at conv2_1
    with pytest.raises(ValueError, match=r'--shift-offsets 40.*conv2_1'):
        shift.read(st)
    st.img = np.zeros((3, 96, 96), np.float32)                  # ... of 48 x 48: 48 x 48 maps at conv1_1
    with pytest.raises(ValueError, match=r'--shift-offsets 40.*conv2_1'):
        shift.read(st)
    st.args.ns.shift_layers = ['conv1_1']
    shift.read(st)
