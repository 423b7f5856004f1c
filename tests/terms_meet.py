"""The scenes of tests/test_gpu_terms_meet.py: every kind of loss term of the tile path on blobs that they share.

A scene is a graph, a 128 x 128 content picture, two 40 x 44 style pictures and a table of what each layer carries
(SPECS).  ``scene(name, graph, drop)`` builds the composite oracle (tests/terms_meet_ref.MeetOracleModel) and the
arrays the engine is armed with, once; ``arm`` arms an engine with them.  Every target is float32 on both sides.

The weights.  Every term's gradient is L1-normalised, so a weight IS the size of the term's gradient at its blob,
while the term's loss is the weight times a number that the data fix: 1/2 |F|^2 over the whole blob for Deep-Dream,
at most 1 for a nearest-neighbour or self-similarity term.  The GPU tests ask both for every term's image gradient
to be at least 5e-2 of the whole and for every family's loss to be at least 1e-3 of the sum, so the data must put the
terms' losses within three orders of magnitude of each other at equal gradients.  With the sibling files' pictures
(uniform in [-110, 120]) the Deep-Dream and content losses are 10^6 and more times a nearest-neighbour loss.  Hence
KNOBS: the pictures are scaled down until |F| is of the order of the biases' contribution (the distance terms do not
care, the square terms fall with the square), the content maps are those of a slightly different picture, and the
style pictures behind the Gram, statistics and sliced Wasserstein targets are brighter than the frame by a factor
each, which sets those losses.  Weights and knobs were tuned on the CPU from the oracle alone; the two conditions are
asserted by the tests, per scene and tile, never relaxed.

The shifted-Gram and the contextual term came later, and with them four scenes that leave the older ones as they are:
'full house' (all eight slot kinds on conv3_1; on conv2_1 the shift slot directly behind the statistics slot and the
cx slot behind it; conv3_2 tapped by a shift target alone), 'fused new pair' (one content layer with a shift target,
one with a contextual target, each riding in an injecting epilogue), 'ragged shift' (96 and 160 channels: C = 1.5 and
2.5 channel blocks, a blob of 49248 floats) and 'mixed cx' (contextual targets on an un-rectified blob under a pool
and beside statistics and self-similarity; shift behind a 1x1 convolution).  The shifted-Gram loss is a square term
like the Gram's: KNOBS['shift'] is the amplitude of the style picture behind its targets.  The contextual energy is
-log of a mean of probabilities, a few units whatever the data, and enters the loss whole; its bank holds raw feature
vectors of both style pictures at the frame's amplitude, evenly spaced over their positions (a few hundred rows, no
multiple of 64).  With 16 terms on 'full house' the smallest |g_t| / |g| is 0.065 and the smallest loss share 2.2e-3
(self-similarity).  tests/test_terms_meet_host.py holds every tile of the scenes with a contextual target to
cx_ref.undecided_cap on the CPU."""

import functools

import numpy as np

from oracle.caffe_net import synthetic_weights
from style_transfer_amd import lib
from style_transfer_amd.config_system import swd_directions
from style_transfer_amd.netspec import builtin_net
from tests import cx_ref, nnfm_patch_ref, nnfm_ref, odd_nets, shift_ref, stat_ref, swd_ref, terms_meet_ref as ref

FRAME = (128, 128)
STYLE_HW = (40, 44)
# per graph family: the frame's amplitude (of the sibling files' uniform(-110, 120) pictures), the share of another
# picture in the content maps' picture, and the amplitudes -- relative to the frame's -- of the style pictures behind
# the Gram, the statistics, the sliced Wasserstein and the shifted-Gram targets
KNOBS = {'vgg19': dict(frame=3e-4, content=0.15, gram=30.0, stat=3.0, swd=30.0, shift=30.0),
         'ragged': dict(frame=3e-4, content=0.15, gram=60.0, stat=6.0, swd=30.0, shift=60.0),
         'mixed': dict(frame=3e-4, content=0.15, gram=30.0, stat=3.0, swd=30.0, shift=60.0)}
DIRS, QUANTILES = 24, 50
VGG_TILES = [(64, 48, (0, 0), (0, 0)), (37, 53, (64, 32), (-24, 40))]
ODD_TILES = [(64, 80, (0, 0), (0, 0)), (37, 53, (64, 32), (-24, 40))]       # sizes of test_gpu_odd_nets.SMALL
FAMILIES = ref.FAMILIES

# layer -> what it carries.  content / style / dream: the weight; stat / swd: the weight; nnfm: (weight, k, patch,
# cover); selfsim: (weight, points); shift: (weight, offsets); cx: (weight, bank rows), with one 'cx_points' and one
# 'cx_eta' per scene as the library holds one of each per call of set_cx_targets.  'masks': (a style mask on style
# set 0?, a content mask?); 'guided': k or None.
OFFSETS = ((0, 1), (1, 0), (0, 2), (2, 0))
_NO_NEW = dict(shift={}, cx={}, cx_points=1024, cx_eta=0.5)
SPECS = {
    'crowded': dict(
        masks=(True, True), guided=None, n_styles=2, lw={'conv2_1': 1.5},
        content={'conv3_1': 4.0}, style={'conv2_1': 2.0, 'conv3_1': 5.0}, dream={'conv3_3': 0.7},
        stat={'conv2_1': 0.7, 'conv3_1': 1.0}, swd={'conv2_1': 1.5, 'conv3_1': 3.0},
        nnfm={'conv3_1': (2.0, 3, 1, 0.5), 'conv3_2': (2.0, 2, 3, 0.0)}, selfsim={'conv3_1': (3.0, 64)}, **_NO_NEW),
    'fused pair': dict(
        masks=(False, False), guided=None, n_styles=1, lw={'conv3_2': 0.8},
        content={'conv3_1': 1.0, 'conv3_2': 1.0}, style={'conv1_1': 1.0, 'conv3_3': 1.0}, dream={},
        stat={}, swd={'conv3_2': 1.0}, nnfm={}, selfsim={'conv3_1': (1.0, 64)}, **_NO_NEW),
    'ragged masked': dict(
        masks=(True, True), guided=None, n_styles=2, lw={'c3': 1.5},
        content={'c3': 1.6}, style={'c3': 1.8, 'c7': 13.0}, dream={'c7': 3.3},
        stat={'p1': 1.4, 'c3': 0.7, 'c6': 1.0}, swd={'p1': 1.8, 'c3': 1.0, 'c5': 2.0}, nnfm={}, selfsim={}, **_NO_NEW),
    'ragged fused': dict(
        masks=(True, False), guided=None, n_styles=2, lw={'c3': 1.5},
        content={'c3': 0.7, 'c5': 2.5}, style={'c3': 2.1, 'c7': 13.5}, dream={'c7': 3.4},
        stat={'p1': 1.4, 'c3': 0.5, 'c6': 1.0}, swd={'p1': 2.0, 'c3': 1.0, 'c5': 2.0}, nnfm={}, selfsim={}, **_NO_NEW),
    'mixed': dict(
        masks=(False, False), guided=None, n_styles=1, lw={'c5': 1.5},
        content={'c5': 1.0}, style={'c6': 3.0}, dream={},
        stat={'c5': 1.0}, swd={'c6': 4.0}, nnfm={'c3': (1.0, 1, 1, 0.0)}, selfsim={'c5': (1.0, 64)}, **_NO_NEW),
}
SPECS['guided'] = dict(SPECS['crowded'], guided=2, nnfm={'conv3_1': (3.0, 2, 1, 0.0), 'conv3_2': (3.0, 2, 1, 0.0)})
# the scenes with the shifted-Gram and the contextual term (the chain nnfm -> swd -> selfsim -> shift -> cx)
SPECS.update({
    'full house': dict(
        masks=(True, True), guided=None, n_styles=2, lw={'conv2_1': 1.5},
        content={'conv3_1': 6.5}, style={'conv2_1': 3.4, 'conv3_1': 6.4}, dream={'conv3_3': 1.1},
        stat={'conv2_1': 0.7, 'conv3_1': 1.2}, swd={'conv3_1': 4.2}, nnfm={'conv3_1': (3.4, 3, 1, 0.5)},
        selfsim={'conv3_1': (5.0, 64)},
        shift={'conv2_1': (1.0, OFFSETS), 'conv3_1': (1.9, OFFSETS), 'conv3_2': (1.8, OFFSETS)},
        cx={'conv2_1': (1.0, 300), 'conv3_1': (2.3, 200)}, cx_points=200, cx_eta=0.5),
    'fused new pair': dict(
        masks=(False, False), guided=None, n_styles=1, lw={'conv3_2': 0.8},
        content={'conv3_1': 1.0, 'conv3_2': 1.0}, style={'conv1_1': 1.0, 'conv3_3': 1.0}, dream={},
        stat={}, swd={}, nnfm={}, selfsim={},
        shift={'conv3_1': (1.0, OFFSETS)}, cx={'conv3_2': (1.0, 220)}, cx_points=200, cx_eta=0.5),
    'ragged shift': dict(
        masks=(True, False), guided=None, n_styles=2, lw={'c4': 1.5},
        content={'c3': 1.3}, style={'c4': 2.25, 'c7': 19.5}, dream={'c7': 5.0},
        stat={'p1': 2.1, 'c4': 0.42}, swd={'p1': 2.55, 'c6': 2.7}, nnfm={}, selfsim={},
        shift={'c4': (0.5, OFFSETS), 'c6': (1.2, OFFSETS)}, cx={}, cx_points=1024, cx_eta=0.5),
    'mixed cx': dict(
        masks=(False, False), guided=None, n_styles=1, lw={'c5': 1.5},
        content={'c5': 1.1}, style={'c6': 5.2}, dream={},
        stat={'c5': 1.0}, swd={'c6': 7.0}, nnfm={'c3': (1.0, 1, 1, 0.0)}, selfsim={'c5': (1.0, 64)},
        shift={'c4': (1.0, OFFSETS)}, cx={'c3': (1.0, 300), 'c5': (1.0, 200)}, cx_points=200, cx_eta=0.5),
})
GRAPH_OF = {'crowded': ['vgg19'], 'fused pair': ['vgg19'], 'guided': ['vgg19'],
            'ragged masked': ['ragged-max', 'ragged-ave'], 'ragged fused': ['ragged-max', 'ragged-ave'],
            'mixed': ['mixed-max'], 'full house': ['vgg19'], 'fused new pair': ['vgg19'],
            'ragged shift': ['ragged-max', 'ragged-ave'], 'mixed cx': ['mixed-max']}


def smooth_mask(hw, seed=0):
    y, x = np.mgrid[:hw[0], :hw[1]]
    return np.float32(0.5 + 0.5 * np.sin(0.09 * x + 0.05 * y + seed) * np.cos(0.04 * y - 0.02 * x))


def guided_masks():
    """Two masks of the frame: a smooth one, and its complement at 0.8 below row 44 and zero above -- a is not 1 and
    whole query blocks of segment 1 are not searched."""
    m0 = smooth_mask(FRAME, 2)
    m1 = np.float32(0.8) * (1 - m0)
    m1[:44] = 0
    return [m0, m1]


def net_and_weights(graph):
    if graph in odd_nets.GRAPHS:
        return odd_nets.net_and_weights(graph)
    net = builtin_net(graph)
    return net, synthetic_weights(net.as_dicts(), 0)


def cut_tile(full, th, tw, start, roll):
    rolled = np.roll(full, (roll[0], roll[1]), axis=(-1, -2))
    return np.ascontiguousarray(rolled[:, start[0]:start[0] + th, start[1]:start[1] + tw])


class Scene:
    """The oracle, armed, and what ``arm`` gives the engine."""


def _layers_of(spec):
    names = []
    for kind in ('content', 'style', 'dream', 'stat', 'swd', 'nnfm', 'selfsim', 'shift', 'cx'):
        names += list(spec[kind])
    return list(dict.fromkeys(names))


@functools.lru_cache(maxsize=None)
def _pictures(graph):
    """(the frame's picture, the content maps' picture, the style pictures at the frame's amplitude) -- the same for
    every scene of a graph."""
    knobs = KNOBS[odd_nets.family(graph)]
    rng = np.random.RandomState(11)
    draw = lambda hw: (knobs['frame'] * rng.uniform(-110, 120, (3,) + hw)).astype(np.float32)
    full = draw(FRAME)
    other = (full + np.float32(knobs['content']) * draw(FRAME)).astype(np.float32)
    return full, other, [draw(STYLE_HW) for _ in range(2)]


@functools.lru_cache(maxsize=None)
def scene(name, graph, drop=None):
    """``drop``: (family, layer) of one extra target that is left out -- not zero-weighted: its slot is not there."""
    spec = {k: (dict(v) if isinstance(v, dict) else v) for k, v in SPECS[name].items()}
    if drop is not None:
        del spec[{'statistics': 'stat'}.get(drop[0], drop[0])][drop[1]]
    net, weights = net_and_weights(graph)
    om = ref.MeetOracleModel(net.as_dicts(), weights)
    full, other, pictures = _pictures(graph)
    sc = Scene()
    sc.name, sc.graph, sc.spec, sc.om, sc.full, sc.net = name, graph, spec, om, full, net
    sc.cl, sc.cw = list(spec['content']), dict(spec['content'])
    sc.sl, sc.sw = list(spec['style']), dict(spec['style'])
    sc.dl, sc.dw = list(spec['dream']), dict(spec['dream'])
    sc.lw = dict(spec['lw'])
    layers = _layers_of(spec)
    # content maps: at the content layers and wherever a self-similarity target reads one
    map_layers = list(dict.fromkeys(sc.cl + list(spec['selfsim'])))
    om.contents = [om.prepare_features(other, map_layers, 512)] if map_layers else []
    knobs = KNOBS[odd_nets.family(graph)]
    feats = [om.features_tile(p, layers) for p in pictures]
    scaled = functools.lru_cache(maxsize=None)(
        lambda kind: om.features_tile(np.float32(knobs[kind]) * pictures[0], layers))
    om.styles = [om.style_grams([np.float32(knobs['gram']) * p], sc.sl, 512) for p in pictures[:spec['n_styles']]]
    sc.style_masks = ([smooth_mask(FRAME)] + [None] * (spec['n_styles'] - 1)) if spec['masks'][0] else []
    sc.content_mask = smooth_mask(FRAME, 1) if spec['masks'][1] else None
    if sc.style_masks:
        om.set_style_masks(sc.style_masks, sc.sl)
    if sc.content_mask is not None:
        om.set_content_mask(sc.content_mask, sc.cl)
    sc.stats = {}
    for l, w in spec['stat'].items():
        mu, sd = stat_ref.feature_stats(scaled('stat')[l])
        sc.stats[l] = (mu.astype(np.float32), sd.astype(np.float32))
        om.add_extra(l, 'statistics', w, ref.stat_term(*sc.stats[l]))
    sc.nnfm, sc.segments, sc.nnfm_masks = {}, {}, None
    if spec['guided']:
        sc.nnfm_masks = guided_masks()
    for l, (w, k, patch, cover) in spec['nnfm'].items():
        if spec['guided']:
            parts = [nnfm_ref.bank_of(f[l]) for f in feats[:2]]
            bank = nnfm_ref.concat_banks(parts).astype(np.float32)
            sc.segments[l] = [len(p) for p in parts]
            om.add_guided(l, w, bank, sc.segments[l], sc.nnfm_masks, k)
        else:
            bank = (nnfm_patch_ref.patch_bank_of(feats[0][l], 1, 3) if patch == 3 else
                    nnfm_ref.bank_of(feats[0][l])).astype(np.float32)
            om.add_extra(l, 'nnfm', w, ref.nnfm_term(bank, k, patch, cover))
        sc.nnfm[l] = np.ascontiguousarray(bank)
    sc.swd = {}
    for l, w in spec['swd'].items():
        V = swd_directions(3, l, feats[0][l].shape[0], DIRS)
        sc.swd[l] = (V, swd_ref.target(scaled('swd')[l], V, QUANTILES).astype(np.float32))
        om.add_extra(l, 'swd', w, ref.swd_term(*sc.swd[l]))
    for l, (w, points) in spec['selfsim'].items():
        om.add_extra(l, 'selfsim', w, ref.selfsim_term(om, l, points))
    sc.shift = {}
    for l, (w, offsets) in spec['shift'].items():
        sc.shift[l] = (list(offsets), np.float32(shift_ref.shift_gram(scaled('shift')[l], offsets)))
        om.add_extra(l, 'shift', w, ref.shift_term(*sc.shift[l]))
    sc.cx = {}
    for l, (w, rows) in spec['cx'].items():
        sc.cx[l] = cx_bank([f[l] for f in feats], rows)
        om.add_extra(l, 'cx', w, ref.cx_term(sc.cx[l], spec['cx_points'], spec['cx_eta']))
    return sc


def cx_bank(maps, rows):
    """[rows, C] float32: raw feature vectors of the style pictures' maps, evenly spaced over all their positions."""
    every = np.concatenate([f.reshape(f.shape[0], -1).T for f in maps])
    bank = np.ascontiguousarray(every[np.linspace(0, len(every) - 1, rows).astype(np.int64)], np.float32)
    assert len(np.unique(bank, axis=0)) == rows        # (identical rows tie exactly in k*)
    return bank


def cx_grids(sc, feature_shape):
    """{layer: (g, N)} of the scene's contextual targets; ``feature_shape(layer) -> (C, h, w)``."""
    return {l: cx_ref.grid(*feature_shape(l)[1:], sc.spec['cx_points'])[:2] for l in sc.spec['cx']}


# ----------------------------------------------------------------------------------------------- the engine's side
def _set_nnfm_table(eng, sc, weights):
    """stx_set_nnfm_cover_targets directly: its table carries patch, k and cover per target, where the Python
    wrapper arms one form per call."""
    n = len(sc.nnfm)
    table = (lib.NnfmCoverTarget * max(1, n))()
    for t, (layer, bank) in zip(table, sc.nnfm.items()):
        _, k, patch, cover = sc.spec['nnfm'][layer]
        t.layer, t.patch, t.k, t.rows = eng._cstr(layer), patch, k, bank.shape[0]
        t.channels, t.bank, t.mem = bank.shape[1] // (patch * patch), bank.ctypes.data, lib.HOST
        t.weight, t.cover = float(weights[layer]), float(cover)
    lib.call('stx_set_nnfm_cover_targets', eng.handle, table, n)
    eng.primary.extra_taps['nnfm'] = list(sc.nnfm)


def arm(eng, sc, only=None):
    """Every target of the scene.  ``only``: the family whose weights stay; the others' are zero, which keeps every
    tap, slot and scratch offset (the additivity runs)."""
    on = lambda family, weights: {l: (w if only in (None, family) else 0.0) for l, w in weights.items()}
    spec = sc.spec
    eng.set_contents_and_styles(sc.om.contents, sc.om.styles)
    if sc.style_masks:
        eng.set_style_masks(sc.style_masks)
    if sc.content_mask is not None:
        eng.set_content_mask(sc.content_mask)
    if sc.stats:
        eng.set_stat_targets(sc.stats, on('statistics', spec['stat']))
    nnfm_w = on('nnfm', {l: v[0] for l, v in spec['nnfm'].items()})
    if sc.nnfm and spec['guided']:
        eng.set_nnfm_targets(sc.nnfm, nnfm_w, 1, spec['guided'], segments=sc.segments, masks=sc.nnfm_masks)
    elif sc.nnfm:
        _set_nnfm_table(eng, sc, nnfm_w)
    if sc.swd:
        eng.set_swd_targets(sc.swd, on('swd', spec['swd']))
    if spec['selfsim']:
        eng.set_selfsim_targets({l: v[1] for l, v in spec['selfsim'].items()},
                                on('selfsim', {l: v[0] for l, v in spec['selfsim'].items()}))
    if sc.shift:
        eng.set_shift_targets(sc.shift, on('shift', {l: v[0] for l, v in spec['shift'].items()}))
    if sc.cx:
        eng.set_cx_targets(sc.cx, on('cx', {l: v[0] for l, v in spec['cx'].items()}), spec['cx_points'],
                           spec['cx_eta'])
    return dict(content_weight=on('content', sc.cw), style_weight=on('style', sc.sw), dd_weight=on('dream', sc.dw))


def disarm(eng):
    eng.set_contents_and_styles([], [])         # (clears every other target with them)


def evaluate(eng, sc, tile, start, roll, only=None):
    w = arm(eng, sc, only)
    return eng.sc_grad_tile(tile, start, roll, sc.cl, sc.sl, sc.lw, w['content_weight'], w['style_weight'],
                            dd_layers=sc.dl, dd_weight=w['dd_weight'])


def oracle_args(sc):
    return (sc.cl, sc.sl, sc.lw, sc.cw, sc.sw), dict(dd_layers=sc.dl, dd_weight=sc.dw)


def reference(sc, tile, start, roll, activations=None):
    """With the maps rolled: (loss, gradient, the blobs of the pass, loss64 of those blobs, term gradients on them).
    ``activations``: the forward pass is replaced by them and the term gradients are left out."""
    om = sc.om
    args, kw = oracle_args(sc)
    om.roll_contents(roll)
    try:
        loss, grad = om.sc_grad_tile(tile, start, *args, activations=activations, **kw)
        deepest = om.order_of(sc.cl, sc.sl, sc.dl)[0]
        blobs = om.blob_names[:om.blob_names.index(deepest) + 1]
        acts = {b: om.net.blobs[b].data[0].copy() for b in blobs}
        loss64 = om.loss64(acts, start, *args, **kw)
        parts = None if activations is not None else om.term_gradients(tile, start, *args, activations=acts, **kw)
    finally:
        om.roll_contents(-np.asarray(roll))
    return loss, grad, acts, loss64, parts


def slot_kinds(sc, layer):
    """The kinds of gradient slot that a layer's tap holds, from the scene's inputs: style, masked content,
    statistics, nnfm, swd, selfsim, shift, cx."""
    spec = sc.spec
    kinds = []
    if layer in spec['style']:
        kinds.append('style')
    if layer in spec['content'] and spec['masks'][1]:
        kinds.append('masked content')
    for key, kind in (('stat', 'statistics'), ('nnfm', 'nnfm'), ('swd', 'swd'), ('selfsim', 'selfsim'),
                      ('shift', 'shift'), ('cx', 'cx')):
        if layer in spec[key]:
            kinds.append(kind)
    return kinds
