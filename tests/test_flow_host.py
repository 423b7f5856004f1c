"""The optical-flow estimator of --prev-contents without a GPU: that the method, as tests/flow_ref.py states it in
float64, is good enough for the temporal term it feeds; the options and their refusals; the .flo round trip of an
estimated flow; the command line of style_transfer_amd.flow up to the point where it needs an engine; the pyramid's
size rule; and the library's entry point (header, export, binding).

The caps on the method's quality are the issue's, not measurements: interior mean endpoint error <= 0.15 px,
consistent share >= 0.95, disoccluded pixels flagged >= 0.85, visible pixels reliable >= 0.85.  The committed
reference gives (printed by the tests): 0.049 / 0.044 px at 67 x 130, 0.048 / 0.044 px at 190 x 257 (backward /
forward), a consistent share above 0.999, 211 of the 216 disoccluded pixels flagged and 0.908 of the others
reliable."""

import ctypes
import functools
import os
from argparse import Namespace

import numpy as np
import pytest
from PIL import Image

from style_transfer_amd import flow as flow_mod
from style_transfer_amd import lib
from style_transfer_amd.cli import image_comment
from style_transfer_amd.config_system import (check_temporal_options, flow_value, parse_args,
                                              temporal_prev_contents)
from style_transfer_amd.flow import read_flo, write_flo
from tests import flow_ref, temporal_ref

BASE = ['-ci', 'c.png', '-si', 's.png']
ON = BASE + ['--temporal-weight', '100', '--prev-images', 'p.png']


# ------------------------------------------------------------------- the method, on the reference alone
@functools.lru_cache(maxsize=None)
def _affine_pair(hw):
    i1, i2, back, fwd = flow_ref.affine_scene(hw)
    return flow_ref.estimate(i1, i2), flow_ref.estimate(i2, i1), back, fwd


@pytest.mark.parametrize('hw', [(67, 130), (190, 257)])
def test_the_method_recovers_an_affine_motion(hw):
    est_b, est_f, back, fwd = _affine_pair(hw)
    for name, est, truth in (('backward', est_b, back), ('forward', est_f, fwd)):
        err = np.sqrt(((np.float64(est) - np.float64(truth)) ** 2).sum(axis=0))[8:-8, 8:-8]
        print('%s %s: interior mean endpoint error %.4f px (largest %.3f)' % (hw, name, err.mean(), err.max()))
        assert err.mean() <= 0.15
    one = temporal_ref.warp(np.zeros((3,) + hw), est_b, est_f)
    share = one['consistent'][one['inside']].mean()
    print('%s: %.4f of the in-frame pixels pass the forward-backward test' % (hw, share))
    assert share >= 0.95


def test_the_method_frees_what_a_moving_box_uncovers():
    earlier, current, disoccluded, _ = flow_ref.box_scene()
    assert disoccluded.sum() == 216                      # (a strip of 6 columns, known exactly)
    est_b, est_f = flow_ref.estimate(current, earlier), flow_ref.estimate(earlier, current)
    one = temporal_ref.warp(np.zeros((3,) + current.shape), est_b, est_f)
    flagged, reliable = (~one['c'])[disoccluded].mean(), one['c'][~disoccluded].mean()
    print('disoccluded: %d of %d unreliable (%.3f); visible: %.3f reliable'
          % ((~one['c'])[disoccluded].sum(), disoccluded.sum(), flagged, reliable))
    assert flagged >= 0.85
    assert reliable >= 0.85


def test_identical_frames_give_exactly_zero():
    frame = flow_ref.affine_scene((37, 53))[0]
    for params in (dict(), dict(levels=1, outer=1, sor=2)):
        assert not flow_ref.estimate(frame, frame, **params).any()


def test_the_scenes_are_what_they_claim():
    i1, i2, back, fwd = flow_ref.affine_scene((67, 130))
    assert i1.dtype == i2.dtype == np.float32 and 0 <= i1.min() and i1.max() <= 255
    assert abs(float(i1.mean()) - 127.5) < 15 and i1.std() > 20
    # I2 is I1's exact warp: the texture evaluated at q + forward(q); at whole steps of a pure shift that is a roll
    y, x = np.mgrid[:20, :30].astype(np.float64)
    assert np.array_equal(flow_ref.texture(x + 3.0, y - 2.0)[2:, :-3], flow_ref.texture(x, y)[:-2, 3:])
    # the spectrum stops at 0.12 cycles per pixel: two pixels apart the texture changes by far less than its range
    wide = flow_ref.texture(*np.mgrid[:64, :64][::-1].astype(np.float64))
    assert np.abs(np.diff(wide, axis=1)).max() < 60
    earlier, current, disoccluded, box = flow_ref.box_scene()
    assert np.array_equal(current[box], np.roll(earlier, flow_ref.BOX_STEP, axis=1)[box])
    assert np.array_equal(current[~box & ~disoccluded], earlier[~box & ~disoccluded])
    assert np.any(current[disoccluded] != earlier[disoccluded])


# --------------------------------------------------------------------------------------- the pyramid
def test_pyramid_sizes():
    for sizes in (flow_ref.pyramid_sizes, flow_mod.pyramid_sizes):
        assert sizes(16, 16) == [(16, 16)]
        assert sizes(21, 21) == [(21, 21), (16, 16)]
        assert sizes(21, 16) == [(21, 16)]                           # (the short side decides)
        assert sizes(22, 22) == [(22, 22), (17, 17)]
        assert sizes(22, 29) == [(22, 29), (17, 22)]
        big = sizes(1024, 1024)
        assert [h for h, _ in big] == [1024, 768, 576, 432, 324, 243, 182, 137, 103, 77, 58, 44, 33, 25, 19]
        assert sizes(1024, 1024, levels=3) == big[:3] and sizes(1024, 1024, levels=99) == big
        assert sizes(64, 64, eta=0.5) == [(64, 64), (32, 32), (16, 16)]
    assert flow_mod.launch_count(16, 16) == 3 + 1 + 5 * 23
    assert flow_mod.launch_count(22, 29, outer=1, inner=2, sor=3) == 3 + 3 + 2 * (1 + 1 + 2 * 8)
    weights = flow_ref.gauss_weights(0.75)
    assert len(weights) == 5 and abs(sum(weights) - 1) < 1e-15 and weights == weights[::-1]
    assert len(flow_ref.gauss_weights(0.2501)) == 15 and len(flow_ref.gauss_weights(0.9499)) == 3


# --------------------------------------------------------------------------------------- options
def test_no_new_name_unless_set():
    args = parse_args(None, BASE, config_py=False)
    for name in ('prev_contents', 'flow_alpha', 'flow_gamma'):
        assert name not in args and not hasattr(args, name)
    comment = image_comment(args, BASE)
    assert 'prev_contents' not in comment and 'flow_' not in comment
    assert temporal_prev_contents(args) == [] and check_temporal_options(args) == ([], [], [])
    # the file-based form keeps its namespace and comment
    args = parse_args(None, ON + ['--flows', 'b.flo'], config_py=False)
    assert not hasattr(args, 'prev_contents') and 'prev_contents' not in image_comment(args, ON)


def test_options_are_read():
    argv = ON + ['q.png', '--prev-contents', 'c1.png', 'c2.png', '--flow-alpha', '25', '--flow-gamma', '1/2']
    args = parse_args(None, argv, config_py=False)
    assert check_temporal_options(args) == (['p.png', 'q.png'], [], [])          # --flows is no longer required
    assert temporal_prev_contents(args) == ['c1.png', 'c2.png']
    assert flow_value(args, 'flow_alpha') == 25.0 and flow_value(args, 'flow_gamma') == 0.5
    comment = image_comment(args, argv)
    for text in ("prev_contents=['c1.png', 'c2.png']", 'flow_alpha=25.0', 'flow_gamma=0.5'):
        assert text in comment
    assert 'flows' not in comment
    args = parse_args(None, ON + ['--prev-contents', 'c1.png'], config_py=False)
    assert flow_value(args, 'flow_alpha') == 18.0 and flow_value(args, 'flow_gamma') == 6.0
    assert 'flow_alpha' not in image_comment(args, ON)
    assert parse_args(None, ON + ['--prev-contents', 'c1.png', '--flow-gamma', '0'], config_py=False).flow_gamma == 0


@pytest.mark.parametrize('extra,names', [
    (ON + ['--prev-contents', 'c1.png', '--flows', 'b.flo'], '--flows'),
    (ON + ['--prev-contents', 'c1.png', '--flows-fwd', 'f.flo'], '--flows-fwd'),
    (ON + ['--prev-contents', 'c1.png', 'c2.png'], '--prev-contents'),                      # different counts
    (ON + ['q.png', '--prev-contents', 'c1.png'], '--prev-contents'),
    (BASE + ['--prev-contents', 'c1.png'], '--prev-contents'),                              # without the term
    (BASE + ['--temporal-weight', '0', '--prev-images', 'p.png', '--prev-contents', 'c1.png'], '--prev-contents'),
    (BASE + ['--temporal-weight', '1', '--prev-contents', 'c1.png'], '--prev-images'),
    (ON + ['a', 'b', 'c', 'd', '--prev-contents', '1', '2', '3', '4', '5'], '--prev-images'),    # more than 4
    (ON + ['--prev-contents', 'c1.png', '--flow-alpha', '0'], '--flow-alpha'),
    (ON + ['--prev-contents', 'c1.png', '--flow-alpha', '-3'], '--flow-alpha'),
    (ON + ['--prev-contents', 'c1.png', '--flow-gamma', '-0.5'], '--flow-gamma'),
    (ON + ['--flows', 'b.flo', '--flow-alpha', '20'], '--flow-alpha'),                      # without --prev-contents
    (ON + ['--flows', 'b.flo', '--flow-gamma', '2'], '--flow-gamma'),
])
def test_refusals_name_the_option(extra, names):
    with pytest.raises(ValueError) as err:
        parse_args(None, extra, config_py=False)
    assert names in str(err.value)


@pytest.mark.parametrize('name,value', [('flow_alpha', float('nan')), ('flow_alpha', float('inf')),
                                        ('flow_gamma', float('nan')), ('flow_gamma', float('-inf')),
                                        ('flow_gamma', 'much')])
def test_values_that_are_not_finite_are_refused(name, value):
    args = Namespace(temporal_weight=1.0, prev_images=['p.png'], prev_contents=['c.png'], **{name: value})
    with pytest.raises(ValueError, match='--' + name.replace('_', '-')):
        check_temporal_options(args)


def test_image_terms_refuse_too():
    from style_transfer_amd.terms import image_terms
    with pytest.raises(ValueError, match='--prev-contents'):
        image_terms(Namespace(prev_contents=['c.png'], swt_weight=0))
    with pytest.raises(ValueError, match='--flows'):
        image_terms(Namespace(temporal_weight=2.0, prev_images=['p.png'], prev_contents=['c.png'], flows=['b.flo'],
                              swt_weight=0))


def test_a_frame_of_the_wrong_size_is_refused_when_read(tmp_path):
    from style_transfer_amd.terms import TemporalTerm
    Image.new('RGB', (24, 18)).save(tmp_path / 'c.png')
    Image.new('RGB', (24, 18)).save(tmp_path / 'p.png')
    Image.new('RGB', (24, 18)).save(tmp_path / 'good.png')
    Image.new('RGB', (18, 24)).save(tmp_path / 'turned.png')
    args = Namespace(content_image=str(tmp_path / 'c.png'), temporal_weight=1.0,
                     prev_images=[str(tmp_path / 'p.png')] * 2,
                     prev_contents=[str(tmp_path / 'good.png'), str(tmp_path / 'turned.png')])
    with pytest.raises(ValueError) as err:
        TemporalTerm(args)
    assert 'turned.png' in str(err.value) and '18 x 24' in str(err.value) and '24 x 18' in str(err.value)
    args.prev_contents[1] = str(tmp_path / 'good.png')
    args.flow_alpha = 30.0
    term = TemporalTerm(args)
    assert term.size0 == (24, 18) and len(term.frames) == 3 and term.flows_b == [] and term.flows_f == []
    assert term.flow_params == dict(alpha=30.0, gamma=6.0)
    # without --prev-contents nothing of the estimator is kept
    write_flo(tmp_path / 'b.flo', np.zeros((2, 18, 24), np.float32))
    term = TemporalTerm(Namespace(content_image=str(tmp_path / 'c.png'), temporal_weight=1.0,
                                  prev_images=[str(tmp_path / 'p.png')], flows=[str(tmp_path / 'b.flo')]))
    assert term.frames == [] and len(term.flows_b) == 1


# ------------------------------------------------------------------------------------------ .flo
def test_an_estimated_flow_survives_the_flo_round_trip(tmp_path):
    est_b = _affine_pair((67, 130))[0]
    assert est_b.dtype == np.float32 and est_b.shape == (2, 67, 130) and np.abs(est_b).max() > 1
    write_flo(tmp_path / 'est.flo', est_b)
    assert read_flo(tmp_path / 'est.flo').tobytes() == est_b.tobytes()
    assert temporal_ref.known(est_b).all()                      # (the estimator writes no unknown markers)


# ------------------------------------------------------------------------------- the command line
def test_grey_is_the_luma_of_the_picture_as_loaded():
    rgb = np.random.RandomState(5).randint(0, 256, (9, 11, 3)).astype(np.uint8)
    got = flow_mod.grey(Image.fromarray(rgb))
    assert got.dtype == np.float32 and got.shape == (9, 11)
    want = 0.299 * np.float64(rgb[..., 0]) + 0.587 * np.float64(rgb[..., 1]) + 0.114 * np.float64(rgb[..., 2])
    assert np.abs(got - want).max() <= 255 * 2.0 ** -22          # (three float32 products and two sums)
    assert flow_mod.grey(Image.fromarray(np.full((4, 4, 3), 255, np.uint8))).max() <= 255.0001
    assert np.array_equal(flow_mod.grey(Image.fromarray(rgb[..., 0])), flow_mod.grey(Image.fromarray(rgb[..., [0, 0, 0]])))


def test_main_checks_its_arguments_before_it_needs_an_engine(tmp_path, capsys):
    Image.new('RGB', (32, 24)).save(tmp_path / 'a.png')
    Image.new('RGB', (32, 24)).save(tmp_path / 'b.png')
    Image.new('RGB', (24, 32)).save(tmp_path / 'turned.png')
    Image.new('RGB', (32, 12)).save(tmp_path / 'small.png')
    a, b, out = str(tmp_path / 'a.png'), str(tmp_path / 'b.png'), str(tmp_path / 'o.flo')
    opts = flow_mod.parse_flow_args([a, b, out])
    assert (opts.frame_from, opts.frame_to, opts.out) == (a, b, out)
    assert (opts.flow_alpha, opts.flow_gamma, opts.device) == (18.0, 6.0, 0)
    opts = flow_mod.parse_flow_args([a, b, out, '--flow-alpha', '30', '--flow-gamma', '0', '--device', '2'])
    assert (opts.flow_alpha, opts.flow_gamma, opts.device) == (30.0, 0.0, 2)
    for argv, words in (([a, b, out, '--flow-alpha', '0'], '--flow-alpha'),
                        ([a, b, out, '--flow-alpha', 'nan'], '--flow-alpha'),
                        ([a, b, out, '--flow-gamma', '-1'], '--flow-gamma'),
                        ([a, b, out, '--flow-gamma', 'inf'], '--flow-gamma'),
                        ([a, b, out, '--device', '-1'], '--device'),
                        ([a, str(tmp_path / 'turned.png'), out], 'turned.png'),
                        ([str(tmp_path / 'small.png'), str(tmp_path / 'small.png'), out], 'small.png')):
        with pytest.raises(ValueError) as err:
            flow_mod.main(argv)
        assert words in str(err.value)
    with pytest.raises(FileNotFoundError):
        flow_mod.main([a, str(tmp_path / 'missing.png'), out])
    with pytest.raises(SystemExit):
        flow_mod.main([a, b])                                    # (OUT.flo is missing)
    capsys.readouterr()
    assert not os.path.exists(out)


# ----------------------------------------------------------------------------------- the library
def test_entry_point_is_exported_and_bound():
    so = ctypes.CDLL(lib.LIB_PATH)
    assert hasattr(so, 'stx_image_flow_estimate')
    vp, i = ctypes.c_void_p, ctypes.c_int
    assert lib.SIGNATURES['stx_image_flow_estimate'] == [vp, vp, vp, i, i, ctypes.POINTER(lib.FlowParams), vp]
    assert [name for name, _ in lib.FlowParams._fields_] == ['alpha', 'gamma', 'eta', 'omega', 'eps', 'levels', 'outer',
                                                            'inner', 'sor']
    assert ctypes.sizeof(lib.FlowParams) == 5 * 8 + 4 * 4
    header = open(os.path.join(os.path.dirname(lib.__file__), '..', 'include', 'stx.h')).read()
    assert 'typedef struct { double alpha, gamma, eta, omega, eps; int levels, outer, inner, sor; } stx_flow_params;' in header
    assert 'int stx_image_flow_estimate(stx_engine *e, const float *I1, const float *I2, int H, int W,' in header
    # the reference's defaults are the binding's
    from style_transfer_amd import image_ops
    params = image_ops.flow_params()
    for name in ('alpha', 'gamma', 'eta', 'omega', 'eps', 'outer', 'inner', 'sor'):
        assert getattr(params, name) == flow_ref.DEFAULTS[name]
    assert params.levels == lib.FLOW_LEVELS_ALL
    assert image_ops.flow_params(dict(alpha=3, levels=None, sor=2)).alpha == 3.0
    with pytest.raises(ValueError, match='beta'):
        image_ops.flow_params(dict(beta=1))
    # null pointers are refused before anything touches a GPU
    assert lib.load().stx_image_flow_estimate(None, None, None, 16, 16, None, None) == -1
