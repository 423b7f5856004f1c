"""The composite reference of tests/terms_meet_ref.py, pinned on the CPU before the GPU tests trust it.

With exactly one optional kind armed, ``MeetOracleModel`` gives the loss and the gradient of that kind's own
``*OracleModel`` bit for bit -- statistics, the five NNFM forms, SWD, self-similarity, shifted Gram, contextual, masked
content, masked style -- on a 24 x 20 tile with taps up to conv3_1, under a window and a roll.  The sum of
``term_gradients`` equals the full gradient to float32 rounding, with all nine families armed.

The scenes of tests/terms_meet.py that arm a contextual target are held here, on the CPU, to the condition that makes
their GPU cases meaningful: on the oracle's blobs of every tile the decisions a float32 implementation cannot be held
to (cx_ref.undecided) stay within cx_ref.undecided_cap -- at most 1 of a cap of 2 per target as the scenes stand."""

import copy
import functools

import numpy as np
import pytest

from oracle.caffe_net import synthetic_weights
from style_transfer_amd.config_system import swd_directions
from style_transfer_amd.netspec import builtin_net
from tests import (content_mask_ref, cx_ref, masked_style_ref, nnfm_cover_ref, nnfm_guided_ref, nnfm_knn_ref,
                   nnfm_patch_ref, nnfm_ref, selfsim_ref, shift_ref, stat_ref, swd_ref, terms_meet_ref)

FRAME = (48, 40)
TH, TW, START, ROLL = 24, 20, (16, 8), (-8, 12)
SL = ['conv1_1', 'conv2_1', 'conv3_1']
CL = ['conv2_2']
LW = {'conv2_1': 1.5, 'conv1_2': 0.7}
CW = {'conv2_2': 0.05}
SW = {l: 1 / 3 for l in SL}
DL, DW = ['conv3_1'], {'conv3_1': 0.02}
EXTRA_LAYERS = ['conv1_2', 'conv2_2', 'conv3_1']
OFFSETS = [(0, 1), (1, 0), (0, 2), (2, 0)]
CX_POINTS = 40      # the 24 x 20 tile: 12 x 10 positions on conv2_2 (g = 2, N = 30), 6 x 5 on conv3_1 (g = 1, N = 30)


def _smooth_mask(hw, seed=0):
    y, x = np.mgrid[:hw[0], :hw[1]]
    return np.float32(0.5 + 0.5 * np.sin(0.19 * x + 0.15 * y + seed) * np.cos(0.14 * y - 0.12 * x))


@functools.lru_cache(maxsize=None)
def _scene():
    net = builtin_net('vgg19')
    layers, weights = net.as_dicts(), synthetic_weights(net.as_dicts(), 0)
    om = terms_meet_ref.MeetOracleModel(layers, weights)
    rng = np.random.RandomState(29)
    full = rng.uniform(-110, 120, (3,) + FRAME).astype(np.float32)
    pictures = [rng.uniform(-110, 120, (3, 20, 24)).astype(np.float32) for _ in range(2)]
    contents = [om.prepare_features(full, list(dict.fromkeys(CL + EXTRA_LAYERS)), 512)]
    feats = [om.features_tile(p, list(dict.fromkeys(SL + EXTRA_LAYERS))) for p in pictures]
    styles = [om.style_grams([p], SL, 512) for p in pictures]
    rolled = np.roll(full, (ROLL[0], ROLL[1]), axis=(-1, -2))
    tile = np.ascontiguousarray(rolled[:, START[0]:START[0] + TH, START[1]:START[1] + TW])
    return layers, weights, contents, styles, feats, tile


def _model(kind_class):
    layers, weights, contents, styles, _, _ = _scene()
    om = kind_class(layers, weights)
    om.contents, om.styles = copy.deepcopy(contents), copy.deepcopy(styles)
    return om


def _run(om, **kw):
    _, _, _, _, _, tile = _scene()
    om.roll_contents(ROLL)
    try:
        return om.sc_grad_tile(tile, START, CL, SL, LW, CW, SW, dd_layers=DL, dd_weight=DW, **kw)
    finally:
        om.roll_contents(-np.asarray(ROLL))


def _same(a, b):
    assert a[0] == b[0], (a[0], b[0])
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    assert np.all(np.isfinite(a[1])) and a[1].any()


def _pair(kind_class):
    return _model(terms_meet_ref.MeetOracleModel), _model(kind_class)


def test_no_optional_term_is_the_plain_oracle():
    from oracle.tile_path import OracleModel
    meet, own = _pair(OracleModel)
    _same(_run(meet), _run(own))


def test_statistics():
    feats = _scene()[4]
    meet, own = _pair(stat_ref.StatOracleModel)
    weights = {'conv2_1': 0.7, 'conv1_2': 1.3}
    own.stat_targets = {l: stat_ref.feature_stats(feats[0][l]) for l in weights}
    own.stat_weights = weights
    for l in weights:
        meet.add_extra(l, 'statistics', weights[l], terms_meet_ref.stat_term(*own.stat_targets[l]))
    _same(_run(meet), _run(own))


@pytest.mark.parametrize('form', ['plain', 'patch', 'knn', 'cover'])
def test_nnfm_forms(form):
    feats = _scene()[4]
    layer, weight = ('conv2_2', 1.3) if form == 'patch' else ('conv3_1', 0.8)
    k, patch, cover = {'plain': (1, 1, 0.0), 'patch': (1, 3, 0.0), 'knn': (3, 1, 0.0), 'cover': (2, 1, 0.5)}[form]
    bank = (nnfm_patch_ref.patch_bank_of(feats[0][layer], 2) if patch == 3 else
            nnfm_ref.bank_of(feats[0][layer])).astype(np.float32)
    meet, own = _pair({'plain': nnfm_ref.NnfmOracleModel, 'patch': nnfm_patch_ref.NnfmPatchOracleModel,
                       'knn': nnfm_knn_ref.KnnOracleModel, 'cover': nnfm_cover_ref.CoverOracleModel}[form])
    own.nnfm_banks, own.nnfm_weights = {layer: bank}, {layer: weight}
    if form in ('knn', 'cover'):
        own.nnfm_k = k
    if form == 'cover':
        own.nnfm_cover = cover
    meet.add_extra(layer, 'nnfm', weight, terms_meet_ref.nnfm_term(bank, k, patch, cover))
    _same(_run(meet), _run(own))


def test_nnfm_guided():
    feats = _scene()[4]
    layer, weight, k = 'conv3_1', 0.8, 2
    parts = [nnfm_ref.bank_of(f[layer]) for f in feats]
    bank, seg_rows = nnfm_ref.concat_banks(parts).astype(np.float32), [len(p) for p in parts]
    masks = [_smooth_mask(FRAME), np.float32(0.8) * (1 - _smooth_mask(FRAME))]
    meet, own = _pair(nnfm_guided_ref.GuidedOracleModel)
    own.nnfm_banks, own.nnfm_weights, own.nnfm_segments = {layer: bank}, {layer: weight}, {layer: seg_rows}
    own.nnfm_masks, own.nnfm_roll, own.nnfm_k = masks, ROLL, k
    meet.add_guided(layer, weight, bank, seg_rows, masks, k)
    _same(_run(meet), _run(own))


def test_swd():
    feats = _scene()[4]
    meet, own = _pair(swd_ref.SwdOracleModel)
    weights = {'conv2_1': 0.7, 'conv1_2': 1.3}
    for l in weights:
        V = swd_directions(3, l, feats[0][l].shape[0], 8)
        own.swd_targets[l] = (V, swd_ref.target(feats[0][l], V, 20).astype(np.float32))
        meet.add_extra(l, 'swd', weights[l], terms_meet_ref.swd_term(*own.swd_targets[l]))
    own.swd_weights = weights
    _same(_run(meet), _run(own))


def test_selfsim():
    meet, own = _pair(selfsim_ref.SelfsimOracleModel)
    own.selfsim_points, own.selfsim_weights = {'conv2_2': 16, 'conv1_2': 30}, {'conv2_2': 1.3, 'conv1_2': 0.7}
    for l, points in own.selfsim_points.items():
        meet.add_extra(l, 'selfsim', own.selfsim_weights[l], terms_meet_ref.selfsim_term(meet, l, points))
    _same(_run(meet), _run(own))


def _shift_targets(feats, layers):
    return {l: (OFFSETS, np.float32(shift_ref.shift_gram(feats[0][l], OFFSETS))) for l in layers}


def _cx_banks(feats, layers):
    """Raw rows: every position of the style pictures' maps."""
    return {l: np.ascontiguousarray(np.concatenate([f[l].reshape(f[l].shape[0], -1).T for f in feats]), np.float32)
            for l in layers}


def test_shift():
    """On a layer that is also a style tap (conv2_1) and on one that nothing else taps (conv1_2)."""
    feats = _scene()[4]
    meet, own = _pair(shift_ref.ShiftOracleModel)
    weights = {'conv2_1': 0.7, 'conv1_2': 1.3}
    assert 'conv2_1' in SL and 'conv1_2' not in SL + CL + DL
    own.shift_targets = {l: (offs, np.float64(T)) for l, (offs, T) in _shift_targets(feats, weights).items()}
    own.shift_weights = weights
    for l, (offs, T) in _shift_targets(feats, weights).items():
        meet.add_extra(l, 'shift', weights[l], terms_meet_ref.shift_term(offs, T))
    _same(_run(meet), _run(own))


@pytest.mark.parametrize('eta', [0.5, 0.1])
def test_cx(eta):
    """Beside the content term (conv2_2, where the grid step is 2) and beside a Gram tap (conv3_1, C = 256)."""
    feats, tile = _scene()[4:]
    meet, own = _pair(cx_ref.CxOracleModel)
    weights = {'conv2_2': 1.3, 'conv3_1': 0.8}
    assert 'conv2_2' in CL and 'conv3_1' in SL
    assert [cx_ref.grid(TH // s, TW // s, CX_POINTS)[0] for s in (2, 4)] == [2, 1]
    own.cx_banks, own.cx_weights, own.cx_points, own.cx_eta = _cx_banks(feats, weights), weights, CX_POINTS, eta
    assert own.cx_banks['conv3_1'].shape[1] == 256
    for l, rows in own.cx_banks.items():
        meet.add_extra(l, 'cx', weights[l], terms_meet_ref.cx_term(rows, CX_POINTS, eta))
    _same(_run(meet), _run(own))


def test_the_contextual_term_enters_the_loss_whole():
    """``cx_term`` hands back E where every other adapter hands back E / 2: with nothing else armed the loss is
    lw w E of cx_ref.terms on the pass's own blob."""
    feats = _scene()[4]
    meet = _model(terms_meet_ref.MeetOracleModel)
    rows = _cx_banks(feats, ['conv2_2'])['conv2_2']
    meet.add_extra('conv2_2', 'cx', 1.3, terms_meet_ref.cx_term(rows, CX_POINTS, 0.5))
    none = {b: 0.0 for b in meet.blob_names}
    tile = _scene()[5]
    loss, _ = meet.sc_grad_tile(tile, START, [], [], {'conv2_2': 0.9}, none, none)
    mu, B = cx_ref.bank(rows)
    E = cx_ref.terms(meet.net.blobs['conv2_2'].data[0], B, mu, CX_POINTS, 0.5).E
    assert E > 0 and loss == 0.9 * 1.3 * E


def test_masked_content():
    meet, own = _pair(content_mask_ref.MaskedContentOracleModel)
    mask = _smooth_mask(FRAME, 1)
    own.set_content_mask(mask, CL)
    meet.set_content_mask(mask, CL)
    _same(_run(meet), _run(own))


def test_masked_style():
    meet, own = _pair(masked_style_ref.MaskedOracleModel)
    masks = [_smooth_mask(FRAME), None]
    own.set_masks(masks, SL)
    meet.set_style_masks(masks, SL)
    _same(_run(meet), _run(own))


def test_term_gradients_add_up_and_loss64_is_the_loss():
    """Everything armed -- both newer kinds (shifted Gram, contextual) beside every older one: the single terms'
    gradients add up to the full gradient.  Each is a float32 array and the
    full pass adds the same diffs in float32 before the same linear backward pass: the two differ by the rounding of
    n_terms float32 sums, at most n_terms 2^-23 of the sum of the terms' maxima.  loss64 agrees with the float32 loss
    to the oracle's own sdot error (1e-5 at this size) and its family shares add up to it."""
    feats = _scene()[4]
    meet = _model(terms_meet_ref.MeetOracleModel)
    meet.set_content_mask(_smooth_mask(FRAME, 1), CL)
    meet.set_style_masks([_smooth_mask(FRAME), None], SL)
    meet.add_extra('conv2_1', 'statistics', 0.7, terms_meet_ref.stat_term(*stat_ref.feature_stats(feats[0]['conv2_1'])))
    bank = nnfm_ref.bank_of(feats[0]['conv3_1']).astype(np.float32)
    meet.add_extra('conv3_1', 'nnfm', 0.8, terms_meet_ref.nnfm_term(bank, 2, 1, 0.5))
    V = swd_directions(3, 'conv2_1', 128, 8)
    meet.add_extra('conv2_1', 'swd', 0.9, terms_meet_ref.swd_term(V, swd_ref.target(feats[0]['conv2_1'], V, 20)))
    meet.add_extra('conv2_2', 'selfsim', 1.3, terms_meet_ref.selfsim_term(meet, 'conv2_2', 16))
    # (added out of the library's order: terms_of sorts them)
    rows = _cx_banks(feats, ['conv2_1'])['conv2_1']
    meet.add_extra('conv2_1', 'cx', 0.6, terms_meet_ref.cx_term(rows, CX_POINTS, 0.5))
    meet.add_extra('conv2_1', 'shift', 1.1, terms_meet_ref.shift_term(*_shift_targets(feats, ['conv2_1'])['conv2_1']))
    meet.add_extra('conv2_2', 'shift', 0.4, terms_meet_ref.shift_term(*_shift_targets(feats, ['conv2_2'])['conv2_2']))
    tile = _scene()[5]
    args = (CL, SL, LW, CW, SW)
    meet.roll_contents(ROLL)
    try:
        loss, grad = meet.sc_grad_tile(tile, START, *args, dd_layers=DL, dd_weight=DW)
        acts = {b: meet.net.blobs[b].data[0].copy() for b in meet.blob_names[:meet.blob_names.index('conv3_1') + 1]}
        parts = meet.term_gradients(tile, START, *args, activations=acts, dd_layers=DL, dd_weight=DW)
        total, families, terms = meet.loss64(acts, START, *args, dd_layers=DL, dd_weight=DW)
    finally:
        meet.roll_contents(-np.asarray(ROLL))
    names = meet.term_names(CL, SL, DL)
    assert [n for n, _ in names] == list(parts) == list(terms)
    assert {f for _, f in names} == set(terms_meet_ref.FAMILIES)
    # the library's order on conv2_1: styles, statistics, swd, shift, cx
    on = [n for n, _ in names if n.endswith(':conv2_1')]
    assert on == ['style0:conv2_1', 'style1:conv2_1', 'statistics:conv2_1', 'swd:conv2_1', 'shift:conv2_1',
                  'cx:conv2_1']
    assert terms_meet_ref.FAMILIES[-3:] == ['shift', 'cx', 'dream'] and len(terms_meet_ref.FAMILIES) == 9
    assert terms_meet_ref.EXTRA_ORDER == ['statistics', 'nnfm', 'swd', 'selfsim', 'shift', 'cx']
    bound = len(parts) * 2.0 ** -23 * sum(float(np.abs(g).max()) for g in parts.values())
    err = float(np.abs(np.float64(grad) - sum(np.float64(g) for g in parts.values())).max())
    print('sum of %d term gradients off by %.3e (bound %.3e); loss %.9g, loss64 %.9g' % (len(parts), err, bound, loss, total))
    assert all(g.any() for g in parts.values())
    assert err <= bound
    assert total == pytest.approx(sum(families.values()), rel=1e-12) and families['dream'] < 0
    assert loss == pytest.approx(total, rel=1e-5)


# ------------------------------------------------------- the inputs of the GPU scenes with a contextual term
def _cx_cases():
    from tests import terms_meet as tm
    return [(name, graph) + tile for name, spec in tm.SPECS.items() if spec['cx'] for graph in tm.GRAPH_OF[name]
            for tile in (tm.VGG_TILES if graph == 'vgg19' else tm.ODD_TILES)]


def test_the_scenes_with_a_contextual_target():
    assert sorted({c[0] for c in _cx_cases()}) == ['full house', 'fused new pair', 'mixed cx']


@pytest.mark.parametrize('name,graph,th,tw,start,roll', _cx_cases())
def test_the_gpu_scenes_meet_the_undecided_decisions_cap(name, graph, th, tw, start, roll):
    """Per contextual target of the scene, on the oracle's blobs of the tile: the undecided k* and i* (cx_ref.undecided)
    number at most cx_ref.undecided_cap(N, M).  A cap on the inputs, from the reference alone: where it holds, a
    float32 implementation can differ from the reference in at most that many discrete decisions."""
    from tests import terms_meet as tm
    sc = tm.scene(name, graph)
    tile = tm.cut_tile(sc.full, th, tw, start, roll)
    acts = tm.reference(sc, tile, start, roll)[2]           # the blobs of the oracle's own pass
    for l in sc.spec['cx']:
        mu, B = cx_ref.bank(sc.cx[l])
        rows, cols = cx_ref.undecided(acts[l], B, mu, sc.spec['cx_points'], sc.spec['cx_eta'])
        g, N, _ = cx_ref.grid(*acts[l].shape[1:], sc.spec['cx_points'])
        print('%s %s %dx%d %s: g %d N %d M %d, undecided rows %d columns %d (cap %.1f)'
              % (name, graph, th, tw, l, g, N, len(B), rows.sum(), cols.sum(), cx_ref.undecided_cap(N, len(B))))
        assert N == len(rows) and len(B) == len(cols) and len(B) % 64
        assert rows.sum() + cols.sum() <= cx_ref.undecided_cap(N, len(B))
