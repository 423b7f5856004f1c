"""The temporal-consistency term without a GPU: the .flo reader and writer, the options and their refusals, the
float64 statement of tests/temporal_ref.py against itself, and the library's two entry points (header, exports
and bindings)."""

import ctypes
import os
from argparse import Namespace

import numpy as np
import pytest

from style_transfer_amd import lib
from style_transfer_amd.cli import image_comment
from style_transfer_amd.config_system import check_temporal_options, parse_args
from style_transfer_amd.flow import FLO_UNKNOWN, read_flo, write_flo
from tests import temporal_ref

BASE = ['-ci', 'c.png', '-si', 's.png']
ON = BASE + ['--temporal-weight', '100']


# ------------------------------------------------------------------------------------------ .flo
def test_flo_round_trip(tmp_path):
    flow = np.random.RandomState(1).normal(0, 4, (2, 7, 11)).astype(np.float32)
    path = tmp_path / 'a.flo'
    write_flo(path, flow)
    raw = path.read_bytes()
    assert len(raw) == 12 + 8 * 7 * 11
    assert np.frombuffer(raw, '<f4', 1)[0] == np.float32(202021.25)
    assert list(np.frombuffer(raw, '<i4', 2, 4)) == [11, 7]                  # width, then height
    assert np.frombuffer(raw, '<f4', 2, 12).tolist() == [flow[0, 0, 0], flow[1, 0, 0]]   # interleaved (u, v)
    back = read_flo(path)
    assert back.dtype == np.float32 and back.shape == (2, 7, 11) and back.flags['C_CONTIGUOUS']
    assert back.tobytes() == flow.tobytes()


def test_flo_unknown_marker_survives(tmp_path):
    flow = np.zeros((2, 5, 6), np.float32)
    flow[:, 2, 3] = FLO_UNKNOWN
    flow[0, 0, 0] = np.inf
    flow[1, 4, 5] = np.nan
    write_flo(tmp_path / 'u.flo', flow)
    back = read_flo(tmp_path / 'u.flo')
    assert back.tobytes() == flow.tobytes()
    want = np.ones((5, 6), bool)
    want[2, 3] = want[0, 0] = want[4, 5] = False
    assert np.array_equal(temporal_ref.known(back), want)


@pytest.mark.parametrize('damage,words', [
    (lambda raw: np.float32(1234.5).tobytes() + raw[4:], 'magic'),
    (lambda raw: raw[:-3], 'too few'),
    (lambda raw: raw[:7], 'header'),
    (lambda raw: raw[:4] + np.array([0, 7], '<i4').tobytes() + raw[12:], '0 x 7'),
    (lambda raw: raw[:4] + np.array([11, -7], '<i4').tobytes() + raw[12:], '11 x -7'),
])
def test_flo_refusals_name_the_file(tmp_path, damage, words):
    good = tmp_path / 'good.flo'
    write_flo(good, np.zeros((2, 7, 11), np.float32))
    bad = tmp_path / 'broken.flo'
    bad.write_bytes(damage(good.read_bytes()))
    with pytest.raises(ValueError) as err:
        read_flo(bad)
    assert 'broken.flo' in str(err.value) and words in str(err.value)
    with pytest.raises(ValueError):
        write_flo(tmp_path / 'x.flo', np.zeros((3, 4, 4)))


# --------------------------------------------------------------------------------------- options
def test_no_new_name_unless_set():
    args = parse_args(None, BASE, config_py=False)
    for name in ('temporal_weight', 'prev_images', 'flows', 'flows_fwd', 'temporal_init'):
        assert name not in args and not hasattr(args, name)
    comment = image_comment(args, BASE)
    assert 'temporal' not in comment and 'flows' not in comment and 'prev_images' not in comment
    assert check_temporal_options(args) == ([], [], [])
    # weight 0 with nothing else: off, nothing asked for
    args = parse_args(None, BASE + ['--temporal-weight', '0'], config_py=False)
    assert args.temporal_weight == 0 and check_temporal_options(args) == ([], [], [])


def test_options_are_read():
    args = parse_args(None, ON + ['--prev-images', 'p1.png', 'p2.png', '--flows', 'b1.flo', 'b2.flo', '--flows-fwd',
                                  'f1.flo', 'f2.flo', '--temporal-init'], config_py=False)
    assert args.temporal_weight == 100.0 and args.temporal_init is True
    assert check_temporal_options(args) == (['p1.png', 'p2.png'], ['b1.flo', 'b2.flo'], ['f1.flo', 'f2.flo'])
    comment = image_comment(args, ON)
    for text in ('temporal_weight=100.0', "prev_images=['p1.png', 'p2.png']", "flows=['b1.flo', 'b2.flo']",
                 "flows_fwd=['f1.flo', 'f2.flo']", 'temporal_init=True'):
        assert text in comment
    args = parse_args(None, ON + ['--prev-images', 'p.png', '--flows', 'b.flo'], config_py=False)
    assert check_temporal_options(args) == (['p.png'], ['b.flo'], [])


@pytest.mark.parametrize('extra,names', [
    (ON + ['--flows', 'b.flo'], '--prev-images'),                                            # on without pictures
    (ON + ['--prev-images', 'p.png'], '--flows'),                                            # on without flows
    (ON + ['--prev-images', 'p.png', 'q.png', '--flows', 'b.flo'], '--flows'),               # different lengths
    (ON + ['--prev-images', 'p.png', '--flows', 'b.flo', 'c.flo'], '--flows'),
    (ON + ['--prev-images', 'p.png', 'q.png', '--flows', 'b.flo', 'c.flo', '--flows-fwd', 'f.flo'], '--flows-fwd'),
    (ON + ['--prev-images'] + ['p.png'] * 5 + ['--flows'] + ['b.flo'] * 5, '--prev-images'),     # more than 4
    (ON + ['--prev-images', 'p.png', '--flows', 'b.flo', '--temporal-init', '-ii', 'i.png'], '--init-image'),
    (BASE + ['--temporal-init'], '--temporal-init'),                                         # without the term
    (BASE + ['--temporal-weight', '0', '--temporal-init', '--prev-images', 'p.png', '--flows', 'b.flo'],
     '--temporal-init'),
])
def test_refusals_name_the_option(extra, names):
    with pytest.raises(ValueError) as err:
        parse_args(None, extra, config_py=False)
    assert names in str(err.value)


def test_image_terms_refuse_too():
    from style_transfer_amd.terms import image_terms
    with pytest.raises(ValueError, match='--flows'):
        image_terms(Namespace(temporal_weight=3.0, prev_images=['p.png'], swt_weight=0))
    with pytest.raises(ValueError, match='--temporal-init'):
        image_terms(Namespace(temporal_init=True, init_image=None, swt_weight=0))
    # a weight bound to the run state switches the term on, whatever it will return
    with pytest.raises(ValueError, match='--prev-images'):
        image_terms(Namespace(temporal_weight=lambda state: 0.0, swt_weight=0))
    assert image_terms(Namespace(swt_weight=0)) == []


def test_a_flow_of_the_wrong_size_is_refused_when_read(tmp_path):
    from PIL import Image
    from style_transfer_amd.terms import TemporalTerm
    Image.new('RGB', (12, 9)).save(tmp_path / 'c.png')
    Image.new('RGB', (12, 9)).save(tmp_path / 'p.png')
    write_flo(tmp_path / 'good.flo', np.zeros((2, 9, 12), np.float32))
    write_flo(tmp_path / 'turned.flo', np.zeros((2, 12, 9), np.float32))
    args = Namespace(content_image=str(tmp_path / 'c.png'), temporal_weight=1.0, prev_images=[str(tmp_path / 'p.png')],
                     flows=[str(tmp_path / 'good.flo')], flows_fwd=[str(tmp_path / 'turned.flo')])
    with pytest.raises(ValueError) as err:
        TemporalTerm(args)
    assert 'turned.flo' in str(err.value) and '9 x 12' in str(err.value) and '12 x 9' in str(err.value)
    args.flows_fwd = None
    term = TemporalTerm(args)
    assert term.size0 == (12, 9) and term.flows_f == [None] and term.flows_b[0].shape == (2, 9, 12)


# ---------------------------------------------------------------------------- the reference itself
def test_finite_differences_of_the_loss():
    hw = (9, 11)
    rng = np.random.RandomState(3)
    img, target = np.float64(temporal_ref.noise_picture(hw, 1)), np.float64(temporal_ref.noise_picture(hw, 2))
    weight = rng.uniform(-0.3, 1.3, hw)
    weight[2, 3] = np.nan
    loss, grad = temporal_ref.temporal_loss(img, target, weight, scale=2.5)
    assert loss > 0 and np.abs(grad).max() > 0
    assert not grad[:, 2, 3].any() and not grad[:, weight <= 0].any()
    h = 0.5     # (a central difference of a quadratic is exact at any step: a large one loses least to cancellation)
    for c, y, x in [(0, 0, 0), (1, 4, 5), (2, 8, 10), (0, 2, 3)] + [tuple(rng.randint(0, n) for n in (3,) + hw)
                                                                     for _ in range(12)]:
        up, down = img.copy(), img.copy()
        up[c, y, x] += h
        down[c, y, x] -= h
        numeric = (temporal_ref.temporal_loss(up, target, weight, 2.5)[0] -
                   temporal_ref.temporal_loss(down, target, weight, 2.5)[0]) / (2 * h)
        assert abs(numeric - grad[c, y, x]) <= 1e-9 * max(1.0, abs(grad[c, y, x]))       # (the loss is quadratic)
    # at equal weight the gradient is the auxiliary-image term's: scale * (img - aux) / 127.5
    assert np.array_equal(temporal_ref.temporal_loss(img, target, np.ones(hw), 2.5)[1], 2.5 * ((img - target) / 127.5))


def test_zero_flows_hold_everything():
    hw = (9, 11)
    prev, zero = temporal_ref.noise_picture(hw, 4), np.zeros((2,) + hw, np.float32)
    for flow_f in (zero, None):
        target, weight, _, _ = temporal_ref.composite([(prev, zero, flow_f)])
        assert np.array_equal(weight, np.ones(hw)) and np.array_equal(target, np.float64(prev))


def test_a_flow_that_leaves_the_frame_holds_nothing():
    hw = (9, 11)
    prev = temporal_ref.noise_picture(hw, 5)
    away = np.stack([np.full(hw, 40.0), np.full(hw, -35.0)]).astype(np.float32)
    target, weight, unclear, _ = temporal_ref.composite([(prev, away, None)])
    assert not weight.any() and not target.any() and not unclear.any()
    # a second, reliable frame fills what the first left free; what is held stays (first wins)
    zero = np.zeros((2,) + hw, np.float32)
    other = temporal_ref.noise_picture(hw, 6)
    target, weight, _, _ = temporal_ref.composite([(prev, away, None), (other, zero, zero)])
    assert weight.all() and np.array_equal(target, np.float64(other))
    target, weight, _, _ = temporal_ref.composite([(other, zero, zero), (prev, zero, zero)])
    assert weight.all() and np.array_equal(target, np.float64(other))


@pytest.mark.parametrize('hw', [(37, 53), (64, 64), (130, 67), (257, 190)])
def test_the_analytic_flows_decide_clearly(hw):
    """The construction of the GPU test: every kind of decision occurs, and none is close to its threshold."""
    back, fwd = temporal_ref.affine_flows(hw)
    one = temporal_ref.warp(temporal_ref.noise_picture(hw, 7), back, fwd)
    share = lambda mask: mask.mean()
    print('%s: reliable %.3f, inconsistent %.3f, boundary %.3f, outside %.3f, unclear %d'
          % (hw, share(one['c']), share(~one['consistent']), share(one['boundary']), share(~one['inside']),
             one['unclear'].sum()))
    assert 0.5 <= share(one['c']) <= 0.9
    assert share(~one['consistent']) >= 0.05 and share(one['boundary']) >= 0.01 and share(~one['inside']) >= 0.03
    assert share(one['unclear']) <= 1e-3
    # the pair is consistent where no box touches it
    plain_b, plain_f = temporal_ref.affine_flows(hw, boxes=False)
    plain = temporal_ref.warp(temporal_ref.noise_picture(hw, 7), plain_b, plain_f)
    assert plain['consistent'][plain['inside']].all()
    # (the map's own gradient, 0.0026, passes the boundary test only where the flow is under 0.25 px: around the
    # map's fixed point, which lies 79 px from the centre and so inside the largest picture alone)
    assert share(plain['boundary']) <= (0.005 if max(hw) > 158 else 0)


# ----------------------------------------------------------------------------------- the library
def test_entry_points_are_exported_and_bound():
    so = ctypes.CDLL(lib.LIB_PATH)
    assert hasattr(so, 'stx_image_flow_warp') and hasattr(so, 'stx_image_temporal')
    vp, i, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    assert lib.SIGNATURES['stx_image_flow_warp'] == [vp, vp, vp, vp, i, i, d, d, i, vp, vp]
    assert lib.SIGNATURES['stx_image_temporal'] == [vp, vp, vp, vp, vp, i, i, d, lib.c_double_p]
    header = open(os.path.join(os.path.dirname(lib.__file__), '..', 'include', 'stx.h')).read()
    assert 'int stx_image_flow_warp(stx_engine *e, const float *prev, const float *flow_b, const float *flow_f,' in header
    assert 'int stx_image_temporal(stx_engine *e, const float *img, float *grad, const float *target,' in header
    # null pointers are refused before anything touches a GPU
    assert lib.load().stx_image_flow_warp(None, None, None, None, 8, 8, 1.0, 1.0, 1, None, None) == -1
    assert lib.load().stx_image_temporal(None, None, None, None, None, 8, 8, 1.0, None) == -1
