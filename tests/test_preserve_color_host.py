"""--preserve-color on the host (no GPU): the option (an extension of the reference's set, absent
from the namespace unless somebody set it), the colour-matching transform in float64, and the three
new entry points in the header and the bindings."""

import os
import re
from argparse import Namespace

import numpy as np
import pytest

from style_transfer_amd import config_system, image_ops, lib, transfer

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BARE = ['-ci', 'c.png', '-si', 's.png']
ENTRY_POINTS = ('stx_image_to_u8_luma', 'stx_image_color_stats', 'stx_image_color_affine')


class FakeFarm:
    master = None

    def layers(self):
        return []


# ------------------------------------------------------------------------------------ parsing
@pytest.mark.parametrize('value', ['none', 'luma', 'match'])
def test_preserve_color_parses(value):
    args = config_system.parse_args(None, BARE + ['--preserve-color', value], config_py=False)
    assert args.preserve_color == value
    assert 'preserve_color' in list(args) and 'preserve_color' in args
    assert transfer.StyleTransfer(FakeFarm(), args, Namespace()).preserve_color == value


def test_bad_value_is_refused_on_the_command_line(capsys):
    with pytest.raises(SystemExit) as err:
        config_system.parse_args(None, BARE + ['--preserve-color', 'chroma'], config_py=False)
    assert err.value.code == 2
    assert '--preserve-color' in capsys.readouterr().err


def test_bare_command_line_leaves_the_option_out():
    """The option namespace of a reference command line holds the reference's names only: readers
    take the default through getattr."""
    args = config_system.parse_args(None, BARE, config_py=False)
    assert 'preserve_color' not in list(args)
    assert 'preserve_color' not in args
    assert 'preserve_color' not in repr(vars(args)['ns'])
    assert getattr(args, 'preserve_color', 'none') == 'none'
    with pytest.raises(AttributeError):
        args.preserve_color                                         # pylint: disable=pointless-statement
    assert transfer.StyleTransfer(FakeFarm(), args, Namespace()).preserve_color == 'none'


def test_config_files_set_the_option(tmp_path):
    cfg = tmp_path / 'extra.py'
    cfg.write_text("preserve_color = 'luma'\n")
    args = config_system.parse_args(None, BARE + ['--config', str(cfg)], config_py=False)
    assert args.preserve_color == 'luma' and 'preserve_color' in list(args)
    default_cfg = tmp_path / 'config.py'
    default_cfg.write_text("preserve_color = 'match'\n")
    args = config_system.parse_args(None, BARE, config_py=default_cfg)
    assert args.preserve_color == 'match' and 'preserve_color' in list(args)
    # the precedence of every other option: config.py < command line < --config
    args = config_system.parse_args(None, BARE + ['--preserve-color', 'none'], config_py=default_cfg)
    assert args.preserve_color == 'none'
    args = config_system.parse_args(None, BARE + ['--preserve-color', 'none', '--config', str(cfg)],
                                    config_py=default_cfg)
    assert args.preserve_color == 'luma'


def test_unknown_value_raises_at_construction(tmp_path):
    cfg = tmp_path / 'extra.py'
    cfg.write_text("preserve_color = 'hue'\n")
    args = config_system.parse_args(None, BARE + ['--config', str(cfg)], config_py=False)
    with pytest.raises(ValueError, match='preserve-color'):
        transfer.StyleTransfer(FakeFarm(), args, Namespace())
    plain = config_system.parse_args(None, BARE, config_py=False)
    plain.preserve_color = 'Luma'
    with pytest.raises(ValueError):
        transfer.StyleTransfer(FakeFarm(), plain, Namespace())


# ------------------------------------------------------------------- the matching transform
def _spd(rng, scale):
    m = rng.standard_normal((3, 3))
    return scale * (m @ m.T + 0.05 * np.eye(3))


@pytest.mark.parametrize('seed', range(8))
def test_color_match_transform_on_random_spd_pairs(seed):
    rng = np.random.RandomState(seed)
    mean_s, mean_c = rng.uniform(-100, 100, 3), rng.uniform(-100, 100, 3)
    cov_s, cov_c = _spd(rng, 10.0 ** rng.uniform(0, 4)), _spd(rng, 10.0 ** rng.uniform(0, 4))
    A, b = image_ops.color_match_transform((mean_s, cov_s), (mean_c, cov_c))
    assert A.shape == (3, 3) and b.shape == (3,) and A.dtype == b.dtype == np.float64
    got = A @ cov_s @ A.T
    rel = np.abs(got - cov_c).max() / np.abs(cov_c).max()
    print('seed %d: |A S A^T - C| / |C| = %.3g' % (seed, rel))
    assert rel <= 1e-10
    assert np.abs(A @ mean_s + b - mean_c).max() <= 1e-10 * max(1.0, np.abs(mean_c).max())


def test_color_match_transform_identity_and_rank_deficiency():
    rng = np.random.RandomState(11)
    mean, cov = rng.uniform(-50, 50, 3), _spd(rng, 300.0)
    A, b = image_ops.color_match_transform((mean, cov), (mean, cov))
    assert np.abs(A - np.eye(3)).max() <= 1e-10 and np.abs(b).max() <= 1e-8
    # a flat-colour style picture (zero covariance) and a grey one (rank one): finite output
    grey = 400.0 * np.ones((3, 3))
    for cov_s in (np.zeros((3, 3)), grey):
        A, b = image_ops.color_match_transform((mean, cov_s), (mean + 3.0, cov))
        assert np.all(np.isfinite(A)) and np.all(np.isfinite(b))
    A, b = image_ops.color_match_transform((mean, cov), (mean, np.zeros((3, 3))))
    assert np.all(np.isfinite(A)) and np.all(np.isfinite(b))


# --------------------------------------------------------------------------------- the ABI
def test_entry_points_are_declared_and_bound():
    header = open(os.path.join(REPO, 'include', 'stx.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    for name in ENTRY_POINTS:
        assert name in lib.SIGNATURES, name
        assert re.search(r'\bint\s+%s\s*\(' % name, header), name
    assert len(lib.SIGNATURES['stx_image_to_u8_luma']) == 7
    assert len(lib.SIGNATURES['stx_image_color_stats']) == 5
    assert len(lib.SIGNATURES['stx_image_color_affine']) == 8
    so = lib.load()
    for name in ENTRY_POINTS:
        assert hasattr(so, name), name
    # NULL arguments are a status, never a crash (a null content picture among them)
    assert so.stx_image_to_u8_luma(None, None, None, 4, 4, None, None) == -1
    assert so.stx_image_color_stats(None, None, 4, 4, None) == -1
    assert so.stx_image_color_affine(None, None, None, 4, 4, None, None, None) == -1
