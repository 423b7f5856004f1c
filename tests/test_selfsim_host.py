"""Host-side checks of the self-similarity content term (--selfsim-weight): the float64 statement of its
definition (tests/selfsim_ref.py), the sample grid, the options, the refusals, the term's place in the schedule and
the conditions that the inputs of tests/test_gpu_selfsim.py meet.  No GPU."""

from argparse import Namespace
import ctypes

import numpy as np
import pytest

from style_transfer_amd import lib
from style_transfer_amd.config_system import (SELFSIM_POINTS_DEFAULT, check_layer_list, check_selfsim_options,
                                              parse_args, selfsim_grid, selfsim_layer_args, selfsim_points)
from style_transfer_amd.netspec import builtin_net
from style_transfer_amd.terms import SelfsimTargets, parse_weights, target_terms
from tests import selfsim_ref

BASE = ['-ci', 'c.png', '-si', 's.png']


# ------------------------------------------------------------------------------------- the reference itself
@pytest.mark.parametrize('c,h,w,points', [(64, 5, 7, 1024), (64, 9, 11, 30), (128, 13, 10, 4096), (64, 24, 24, 576)])
def test_s_is_the_finite_difference_of_n_half_e(c, h, w, points):
    """S = N d(E/2)/dF with T held: central differences in float64 (the step is far below the smallest |d| of a
    decided pair, so the signs hold) agree to 1e-5 of max |S| on sampled entries -- on the grid, where S lives, and
    off it, where both are 0.  (The difference quotient's own rounding is a few times 2^-53 E N / (2 step) -- E is a
    sum of N^2 terms --, about 1e-6 of max |S| at N = 576 with the step 1e-5; the bound is ten times that.)  An
    all-zero column has r = 0: the term is not differentiable there and S is 0 by definition, so such columns are not
    sampled."""
    F, content = selfsim_ref.case_inputs(c, h, w, points, seed=0)
    F = F.astype(np.float64)
    E, S, _, _, d = selfsim_ref.terms(F, content, points)
    g, N, pos = selfsim_ref.grid(h, w, points)
    step, scale, worst = 1e-5, np.abs(S).max(), 0.0
    rng = np.random.RandomState(1)
    picks = [(rng.randint(c),) + tuple(pos[rng.randint(N)]) for _ in range(24)]
    picks += [(rng.randint(c), rng.randint(h), rng.randint(w)) for _ in range(8)]
    for index in picks:
        if not F[:, index[1], index[2]].any():
            assert not S[:, index[1], index[2]].any()
            continue
        plus, minus = F.copy(), F.copy()
        plus[index] += step
        minus[index] -= step
        fd = N * 0.5 * (selfsim_ref.energy(plus, content, points) - selfsim_ref.energy(minus, content, points)) / (2 * step)
        worst = max(worst, abs(fd - S[index]))
        if index[1] % g or index[2] % g:
            assert S[index] == 0 and fd == 0
    print('finite differences: worst %.2e of max |S| %.2e' % (worst / scale, scale))
    assert 0 < E <= 2 and scale > 0 and worst <= 1e-5 * scale


def test_degenerate_grids():
    """N = 1: E = 0, S = 0.  N = 2: both P are [[0, 1], [1, 0]] up to the epsilon."""
    F, content = selfsim_ref.case_inputs(64, 1, 1, 2)
    E, S, a, T, d = selfsim_ref.terms(F, content, 2)
    assert E == 0 and a == 0 and not S.any() and T.shape == (1, 1)
    F, content = selfsim_ref.case_inputs(64, 1, 2, 2)
    E, S, a, T, d = selfsim_ref.terms(F, content, 2)
    assert T.shape == (2, 2) and d[0, 0] == d[1, 1] == 0 and 0 < E < 1e-4
    # identical inputs: exactly nothing
    E, S, a, T, _ = selfsim_ref.terms(F, F, 2)
    assert E == 0 and a == 0 and not T.any()


# ------------------------------------------------------------------------------------------- the grid rule
@pytest.mark.parametrize('h,w,points,g,gh,gw', [(5, 7, 1024, 1, 5, 7), (9, 11, 30, 2, 5, 6), (13, 10, 4096, 1, 13, 10),
                                                (24, 24, 576, 1, 24, 24), (24, 24, 575, 2, 12, 12),
                                                (33, 33, 1024, 2, 17, 17), (128, 128, 1024, 4, 32, 32),
                                                (256, 256, 4096, 4, 64, 64), (1, 2, 2, 1, 1, 2), (1, 1, 2, 1, 1, 1),
                                                (7, 3, 2, 4, 2, 1)])
def test_the_grid_is_the_smallest_step_that_fits(h, w, points, g, gh, gw):
    assert selfsim_grid(h, w, points) == (g, gh, gw)
    assert gh * gw <= points and (g == 1 or -(-h // (g - 1)) * -(-w // (g - 1)) > points)
    step, N, pos = selfsim_ref.grid(h, w, points)
    assert (step, N) == (g, gh * gw) and pos.shape == (N, 2)
    assert pos[0].tolist() == [0, 0] and pos[-1].tolist() == [(gh - 1) * g, (gw - 1) * g]
    assert pos[-1][0] < h and pos[-1][1] < w                    # the last row and column lie inside the blob
    assert pos[:, 0].tolist() == sorted(pos[:, 0].tolist())     # raster order
    if gw > 1:
        assert pos[1].tolist() == [0, g]


def test_the_ragged_grid_of_the_gpu_case_ends_on_the_blobs_edge():
    _, _, pos = selfsim_ref.grid(9, 11, 30)
    assert pos[-1].tolist() == [8, 10]


# ---------------------------------------------------------------------------------------------- the options
def test_options_are_absent_unless_set_and_default_to_the_content_layers():
    args = parse_args(argv=BASE, config_py=False)
    assert not any(name.startswith('selfsim') for name in vars(args.ns))      # the PNG comment is unchanged
    assert selfsim_layer_args(args) == [] and check_selfsim_options(args) == []
    assert selfsim_points(args) == SELFSIM_POINTS_DEFAULT == 1024
    assert not any(isinstance(term, SelfsimTargets) for term in target_terms(args, None))
    args = parse_args(argv=BASE + ['--selfsim-weight', '3/2'], config_py=False)
    assert args.selfsim_weight == 1.5 and 'selfsim_layers' not in args and 'selfsim_points' not in args
    assert selfsim_layer_args(args) == [str(item).partition(':')[0] for item in args.content_layers] == ['conv4_2']
    kinds = [type(term).__name__ for term in target_terms(args, builtin_net('vgg19').blob_names())]
    assert kinds == ['SelfsimTargets', 'Masks']
    args = parse_args(argv=BASE + ['--selfsim-weight', '1', '--content-layers', 'conv3_2:2', 'conv4_2'], config_py=False)
    assert selfsim_layer_args(args) == ['conv3_2', 'conv4_2']                  # the names, not the content weights
    args = parse_args(argv=BASE + ['--selfsim-weight', '1', '--content-layers'], config_py=False)
    assert args.content_layers == [] and selfsim_layer_args(args) == ['conv4_2']
    args = parse_args(argv=BASE + ['--selfsim-weight', '0', '--selfsim-layers', 'conv3_2'], config_py=False)
    assert selfsim_layer_args(args) == []                                      # weight 0: off
    # behind the statistics term, the banks and the sliced Wasserstein targets
    args = parse_args(argv=BASE + ['--selfsim-weight', '1', '--swd-weight', '1', '--nnfm-weight', '1', '--stat-weight',
                                   '1'], config_py=False)
    assert [type(term).__name__ for term in target_terms(args, None)] == ['StatTargets', 'NnfmBanks', 'SwdTargets',
                                                                          'SelfsimTargets', 'Masks']


def test_layer_weights_go_through_parse_weights_and_points_are_read():
    args = parse_args(argv=BASE + ['--selfsim-weight', '2', '--selfsim-layers', 'conv3_2:3', 'conv4_2',
                                   '--selfsim-points', '256'], config_py=False)
    names, weights = parse_weights(selfsim_layer_args(args), args.selfsim_weight)
    assert names == ['conv3_2', 'conv4_2'] and weights == {'conv3_2': 1.5, 'conv4_2': 0.5}
    assert check_selfsim_options(args, builtin_net('vgg19').blob_names()) == names and selfsim_points(args) == 256


def test_a_weight_bound_to_run_state_switches_the_term_on():
    args = Namespace(selfsim_weight=lambda state: 1.0 / (1 + state.scale), content_layers=['conv4_2'])
    assert selfsim_layer_args(args) == ['conv4_2']


def test_style_masks_and_a_content_mask_leave_the_term_alone():
    """A content-side term: --style-masks does not refuse it (the style-side lists stay refused: check_layer_list's
    default), and --content-mask weights the content term only."""
    args = Namespace(selfsim_weight=1.0, content_layers=['conv4_2'], style_masks=['a.png'], content_mask='m.png')
    assert check_selfsim_options(args, builtin_net('vgg19').blob_names()) == ['conv4_2']
    with pytest.raises(ValueError, match='--style-masks'):
        check_layer_list(args, ['conv4_2'], '--x-weight', '--x-layers', 'one set')
    assert check_layer_list(args, ['conv4_2'], '--x-weight', '--x-layers', 'one set', style_side=False) == ['conv4_2']


@pytest.mark.parametrize('points', [0, 1, -3, 4097, True, 2.0, '8'])
def test_refused_for_points_outside_the_range(points):
    with pytest.raises(ValueError, match='--selfsim-points'):
        check_selfsim_options(Namespace(selfsim_weight=1.0, selfsim_points=points, content_layers=[]))
    if isinstance(points, int) and not isinstance(points, bool):
        with pytest.raises(ValueError, match='--selfsim-points'):
            parse_args(argv=BASE + ['--selfsim-weight', '1', '--selfsim-points=%d' % points], config_py=False)
    for ok in (2, 4096):
        assert check_selfsim_options(Namespace(selfsim_weight=1.0, selfsim_points=ok, content_layers=[])) == ['conv4_2']


def test_refused_for_a_bad_or_duplicate_layer_before_any_gpu_work():
    from style_transfer_amd.transfer import StyleTransfer
    layers = builtin_net('vgg19').blob_names()
    args = parse_args(argv=BASE + ['--selfsim-weight', '1', '--selfsim-layers', 'conv9_9'], config_py=False)
    with pytest.raises(ValueError, match="--selfsim-layers.*'conv9_9'"):
        check_selfsim_options(args, layers)
    for bad in (['data'], ['conv4_2', 'conv4_2'], ['conv4_2:x'], ['conv4_2:0']):
        with pytest.raises(ValueError, match='--selfsim-layers'):
            check_selfsim_options(Namespace(selfsim_weight=1.0, selfsim_layers=bad, content_layers=[]), layers)

    class NoFarm:       # (no engine: the refusal comes before anything touches one)
        master = None

        def layers(self):
            return layers
    with pytest.raises(ValueError, match='--selfsim-layers'):
        StyleTransfer(NoFarm(), args, Namespace())
    # ... and the command line refuses it before it wakes a GPU
    from style_transfer_amd import cli
    woken = []
    original = cli.TileFarm
    cli.TileFarm = lambda *a, **k: woken.append(a)
    try:
        with pytest.raises(ValueError, match='--selfsim-layers'):
            cli.main(BASE + ['--model', 'vgg19', '--selfsim-weight', '1', '--selfsim-layers', 'conv9_9'])
    finally:
        cli.TileFarm = original
    assert not woken


def test_not_broadcast_to_ranks():
    from style_transfer_amd.dist import refuse_unbroadcast_options
    refuse_unbroadcast_options(Namespace(selfsim_weight=0))
    with pytest.raises(NotImplementedError, match='--selfsim-weight'):
        refuse_unbroadcast_options(Namespace(selfsim_weight=1.0))


# -------------------------------------------------------------------------------------------- the schedule
class _StubFarm:
    """Records what the schedule asks of a farm; feature maps are their layer names."""
    master = None

    def __init__(self):
        self.calls = []

    def layers(self):
        return builtin_net('vgg19').blob_names()

    def prepare_features_device(self, picture, layers, tile, passes=10, roll=None):
        self.calls.append(('features', tuple(layers), passes, None if roll is None else tuple(roll)))
        return {layer: layer for layer in layers}

    def set_contents_and_styles(self, contents, styles):
        self.calls.append(('targets', [sorted(c) for c in contents]))

    def set_selfsim_targets(self, points, weights=None):
        self.calls.append(('selfsim', dict(points), dict(weights)))


def _transfer(argv):
    from style_transfer_amd.transfer import StyleTransfer
    args = parse_args(argv=BASE + argv, config_py=False)
    st = StyleTransfer(_StubFarm(), args, Namespace())
    st.pil_to_image = lambda image: image
    for term in st.target_terms:
        term.read(st)
    return st


def test_content_maps_are_taken_at_the_union_of_the_content_layers_and_the_terms_layers_once():
    st = _transfer(['--selfsim-weight', '2', '--selfsim-layers', 'conv3_2', 'conv4_2:3', '--selfsim-points', '64'])
    term = [t for t in st.target_terms if isinstance(t, SelfsimTargets)][0]
    assert term.content_layers == ('conv3_2', 'conv4_2') and term.layers == ()
    st.styles = [{}]                    # (the style targets exist: only the contents are made)
    st.preprocess_images(['picture'], [], ['conv4_2'], [], roll=(4, 8))
    assert st.farm.calls == [('features', ('conv4_2', 'conv3_2'), 1, (4, 8))]       # one call, no layer twice
    assert st.contents == [{'conv4_2': 'conv4_2', 'conv3_2': 'conv3_2'}]
    st._send_targets((4, 8))
    assert st.farm.calls[1:] == [('targets', [['conv3_2', 'conv4_2']]),
                                 ('selfsim', {'conv3_2': 64, 'conv4_2': 64}, {'conv3_2': 0.5, 'conv4_2': 1.5})]
    # without contents (--jitter before its first step) the term waits
    st.contents, st.farm.calls = [], []
    st._send_targets()
    assert st.farm.calls == [('targets', [])]


def test_with_the_defaults_no_extra_content_map_is_made_and_without_the_term_nothing_changes():
    st = _transfer(['--selfsim-weight', '1'])
    st.styles = [{}]
    st.preprocess_images(['picture'], [], ['conv4_2'], [])
    assert st.farm.calls == [('features', ('conv4_2',), 10, None)]
    st = _transfer([])
    st.styles = [{}]
    st.preprocess_images(['picture'], [], ['conv4_2'], [])
    st._send_targets()
    assert st.farm.calls == [('features', ('conv4_2',), 10, None), ('targets', [['conv4_2']])]
    # an empty --content-layers: the term's default layer carries the map
    st = _transfer(['--selfsim-weight', '1', '--content-layers'])
    st.styles = [{}]
    st.preprocess_images(['picture'], [], [], [])
    assert st.farm.calls == [('features', ('conv4_2',), 10, None)]


def test_the_c_abi_has_the_entry_points():
    assert lib.SIGNATURES['stx_set_selfsim_targets'][1]._type_ is lib.SelfsimTarget
    assert [name for name, _ in lib.SelfsimTarget._fields_] == ['layer', 'points', 'weight']
    assert len(lib.SIGNATURES['stx_op_selfsim_terms']) == 10
    t = lib.SelfsimTarget(b'conv4_2', 1024, 0.5)
    assert (t.layer, t.points, t.weight) == (b'conv4_2', 1024, 0.5) and ctypes.sizeof(t) == 24


# ------------------------------------------------------------------- the conditions of the GPU test's inputs
@pytest.mark.parametrize('c,h,w,points', selfsim_ref.OP_SHAPES)
def test_the_gpu_cases_meet_the_undecided_pairs_cap(c, h, w, points):
    """T_ij is undecided when |d64_ij| <= tau, tau = 4 x the largest |d32_ij - d64_ij| of the float32 restatement on
    the case's inputs (the factor: a device adds in another order than numpy).  The float64 reference alone has at
    most max(2, N^2 / 1e5) such pairs on the inputs that tests/test_gpu_selfsim.py uses: a condition on the inputs
    (the seeds of selfsim_ref.SEEDS are chosen for it), not a measurement of any kernel.  Every sign that the float32
    restatement flips lies among them.  Second condition, for the tolerances 4 x the restatement's error: its E and
    sum |S| are off by at least 2^-24 of their value -- a float32 result's own rounding -- so that the tolerance asks
    nothing of a float32 result that the format cannot hold."""
    F, content = selfsim_ref.case_inputs(c, h, w, points)
    tau, und, flips, N = selfsim_ref.undecided(F, content, points)
    count, cap, rel_e, rel_a = selfsim_ref.case_conditions(c, h, w, points)
    print('N %d: tau %.2e, undecided %d of %d (cap %.1f), float32 flips %d; float32 E off by %.2e, sum |S| by %.2e'
          % (N, tau, count, N * N, cap, int(flips.sum()), rel_e, rel_a))
    assert count == int(und.sum()) <= cap
    assert not (flips & ~und).any()
    assert N == 1 or (rel_e >= 2.0 ** -24 and rel_a >= 2.0 ** -24)
    # post-ReLU inputs with a few all-zero columns in both, at different places
    zero_f, zero_c = ~F.reshape(c, -1).any(axis=0), ~content.reshape(c, -1).any(axis=0)
    assert F.min() >= 0 and content.min() >= 0
    if h * w >= 8:
        assert zero_f.sum() >= 2 and zero_c.sum() >= 2 and not (zero_f & zero_c).any()
