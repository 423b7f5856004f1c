"""The tile path on graphs that are not VGG (tests/odd_nets.py), against the numpy oracle.

Every other GPU test of the tile path builds a VGG: channel counts that fill every channel block, 3x3
convolutions each followed by a ReLU, pooling layers behind rectified convolutions only, no 1x1 layer.  Much of
csrc/tile_path.cpp decides on exactly these properties; here each decision takes its other side:

  * partial channel blocks in every fused epilogue (pooled output, window codes, skipped stores, ReLU nibbles,
    the pooled gradient routed in the staging, the injecting epilogues, the K-slice reduce pass, recorded maxima);
  * 1x1 layers forward and backward, with and without a mask, under and over a tap;
  * pooling an un-rectified blob (pin_mask / bot.relu false), a rectified pooled blob (stand-alone kernel +
    relu_inplace), pool after pool and a pool on the image (the producer under the pool is no convolution),
    force_relu on a convolution, the first-layer kernel's shape in mid-graph and with a pool behind it,
    conv_small_launch into a blob that is not the image.

Tolerances are check_tile's own (tests/gpu_helpers.py): activations, loss and gradient to 1e-5, relative L2
against the oracle's end-to-end gradient 1e-2 (1e-3 without MAX pooling on tiles over 400 pixels).

The engine refuses one construct of these graphs by design: a style tap on the 3-channel blob of `narrow` (the
style term needs a multiple of 4 channels) -- asserted as a refusal that names the layer.

STX_ODD_NETS_STATS=<file>: the largest activation error and the decision-flip counts of every oracle case,
appended (profiles/odd_nets_parity.txt)."""

import functools
import os

import numpy as np
import pytest

from tests import amax_chain as ac
from tests import odd_nets
from tests.gpu_helpers import check_tile, max_rel, require_gpu
from tests.helpers import normalized_weights

pytestmark = pytest.mark.gpu
TIGHT = 1e-5
FLIP_L2 = 1e-2

# small planes: most layers slice K, and the reduce pass carries bias / mask / injection
SMALL = [(9, 13), (37, 53), (64, 80), (131, 77)]
# one larger size per graph, at which the fused paths run (asserted from the profile labels below):
#   ragged  256 x 384: the fp32 Winograd epilogue pools on even rows only; c2 -> p1 fuses forward, c4's backward
#           (fp16-split, unsplit on the 128 x 192 plane) takes p2's gradient pooled;
#   mixed   445 x 637: the only pooling layer that may ride forward is p2 behind c5 (p0 reads the image, p1 is
#           rectified, p3 reads a pooled blob), and c5 -- 256 -> 128 on a sixteenth of the tile -- slices K on
#           every plane under 112 x 160 (h2_plan), i.e. on every tile under 445 x 637; odd on purpose: p0 and
#           p1 cut windows at the border;
#   narrow  203 x 331: nothing fuses at any size -- the two convolutions under its pooling layers have the
#           first-layer shape (3 -> 64), which takes the direct family forward (no pooled epilogue) and
#           conv_small_launch backward (no pooled input): asserted as such.
LARGE = {'ragged': (256, 384), 'mixed': (445, 637), 'narrow': (203, 331)}
GRAPHS = sorted(odd_nets.GRAPHS)
CASES = [(g, t) for g in GRAPHS for t in sorted(odd_nets.TAP_SETS[odd_nets.family(g)])]

_ENGINES = {}


@pytest.fixture(scope='module', autouse=True)
def _close_engines():
    yield
    for eng in _ENGINES.values():
        eng.close()
    _ENGINES.clear()
    _scene.cache_clear()


def _engine(graph):
    """One TileEngine per graph for the oracle cases (the switch A/B cases build fresh ones)."""
    from style_transfer_amd.engine import TileEngine
    require_gpu()
    if graph not in _ENGINES:
        net, weights = odd_nets.net_and_weights(graph)
        _ENGINES[graph] = TileEngine(net, 0, weights)
    return _ENGINES[graph]


def _taps(graph, taps):
    cl, sl = odd_nets.TAP_SETS[odd_nets.family(graph)][taps]
    cl, cw = normalized_weights(cl, 0.05)
    sl, sw = normalized_weights(sl, 1)
    return cl, cw, sl, sw


@functools.lru_cache(maxsize=4)
def _scene(graph, taps, th, tw):
    """The scene of test_sc_grad_tile_odd_sizes_against_oracle: content and style targets from the oracle, a
    tile cut from a larger picture at (16, 8).  -> (oracle with its targets, tile)."""
    om, _ = odd_nets.make_oracle(graph)
    cl, _, sl, _ = _taps(graph, taps)
    rng = np.random.RandomState(th)
    full = rng.uniform(-110, 120, (3, th + 24, tw + 40)).astype(np.float32)
    style = rng.uniform(-110, 120, (3, 50, 60)).astype(np.float32)
    om.styles = [om.style_grams([style], sl, 1024)]
    om.contents = [om.prepare_features(full, cl, 1024)]
    return om, np.ascontiguousarray(full[:, 16:16 + th, 8:8 + tw])


def _flip_l2(graph, th, tw):
    return 1e-3 if graph in odd_nets.ALL_AVE and th * tw > 400 else FLIP_L2


def _blas_loss_tol(eng, cl, th, tw):
    """check_tile holds the loss to 1e-5 of the float64 value everywhere.  Against the oracle's own float32
    result it does so too, except where a content-tapped blob has more than 2^22 elements (c2 / c3 of `mixed`
    on its larger tile: 4.6 / 9.1 million): the reference sums 1/2 |F - Fc|^2 with a float32 sdot, which is
    itself only good to about 1e-4 there (measured on this scene: float32 6.302998e8, float64 6.303179e8) --
    the bound the full-size VGG cases pass for the same reason (check_tile's docstring)."""
    return 5e-4 if max(int(np.prod(eng.feature_shape(l, th, tw))) for l in cl) > 1 << 22 else TIGHT


def _record(case, stats):
    path = os.environ.get('STX_ODD_NETS_STATS')
    if path:
        with open(path, 'a') as f:
            f.write('%s: largest activation error %.2e of max, %d ReLU and %d pooling decisions differ, '
                    'gradient L2 %.2e%s\n' % (case, stats['act_err'], stats['relu_flips'], stats['pool_flips'],
                                             stats['l2'], ', clean pixels %.2e' % stats['clean_err']
                                             if 'clean_err' in stats else ''))


def _sizes(graph):
    return SMALL + [LARGE[odd_nets.family(graph)]]


# ------------------------------------------------------------------------------------ 1. against the oracle
@pytest.mark.parametrize('size', range(len(SMALL) + 1))
@pytest.mark.parametrize('graph,taps', CASES)
def test_tile_against_oracle(graph, taps, size, monkeypatch):
    for name in ('STX_CONV_ALGO', 'STX_CONV_SYMM'):
        monkeypatch.delenv(name, raising=False)
    th, tw = _sizes(graph)[size]
    om, tile = _scene(graph, taps, th, tw)
    cl, cw, sl, sw = _taps(graph, taps)
    eng = _engine(graph)
    eng.set_contents_and_styles(om.contents, om.styles)
    loss, grad, stats = check_tile(eng, om, tile, (16, 8), (-16, 24), cl, cw, sl, sw, {},
                                   flip_l2=_flip_l2(graph, th, tw), blas_loss_tol=_blas_loss_tol(eng, cl, th, tw))
    print(graph, taps, (th, tw), stats)
    _record('%s %s %dx%d' % (graph, taps, th, tw), stats)
    assert np.isfinite(loss) and np.isfinite(grad).all()
    again = eng.sc_grad_tile(tile, (16, 8), (-16, 24), cl, sl, {}, cw, sw)
    assert again[0] == loss and np.array_equal(again[1], grad)            # deterministic


@pytest.mark.parametrize('size', range(len(SMALL) + 1))
@pytest.mark.parametrize('graph', GRAPHS)
def test_feature_maps_of_every_blob(graph, size):
    """stx_features_tile of every blob, dead ends of the tap sets included; the net's last blob rectified."""
    th, tw = _sizes(graph)[size]
    om, _ = odd_nets.make_oracle(graph)
    tile = np.random.RandomState(tw).uniform(-110, 120, (3, th, tw)).astype(np.float32)
    feats = _engine(graph).features_tile(tile, om.blob_names)
    ref = om.features_tile(tile, om.blob_names)
    for b in om.blob_names:
        assert feats[b].shape == ref[b].shape, b
        assert max_rel(feats[b], ref[b]) < TIGHT, b
    # one blob asked for alone: the same bits (another set of observed blobs, another set of skipped stores)
    for b in om.blob_names[-3:]:
        assert np.array_equal(_engine(graph).features_tile(tile, [b])[b], feats[b]), b


def test_style_tap_on_three_channels_is_refused():
    """The one construct of these graphs the engine refuses: the style term needs a multiple of 4 channels.
    Refused in sc_grad_prepare, before the first launch, with the layer's name; the engine stays usable."""
    from style_transfer_amd.lib import StxError
    eng = _engine('narrow')
    tile = np.zeros((3, 32, 32), np.float32)
    eng.set_contents_and_styles([], [{'c4': np.zeros((3, 3), np.float32), 'c3': np.zeros((64, 64), np.float32)}])
    with pytest.raises(StxError, match='style layer c4'):
        eng.sc_grad_tile(tile, (0, 0), (0, 0), [], ['c4'], {}, {}, {'c4': 1.0})
    loss, grad = eng.sc_grad_tile(tile, (0, 0), (0, 0), [], ['c3'], {}, {}, {'c3': 1.0})
    assert np.isfinite(loss) and np.isfinite(grad).all()


# ------------------------------------------------------------------------- 2. which kernels ran, by label
def _random_targets(eng, cl, sl, th, tw):
    r = np.random.RandomState(3)
    eng.set_contents_and_styles(
        [{l: np.abs(r.standard_normal(eng.feature_shape(l, th, tw))).astype(np.float32) for l in cl}],
        [{l: np.tril(r.standard_normal((eng.layer_info(l)[1],) * 2)).astype(np.float32) for l in sl}])


def _labels(eng, tile, cl, cw, sl, sw):
    eng.profile(True)
    try:
        out = eng.sc_grad_tile(tile, (0, 0), (0, 0), cl, sl, {}, cw, sw)
        return out, [row[0] for row in eng.profile_read()]
    finally:
        eng.profile(False)


@pytest.mark.parametrize('graph', GRAPHS)
def test_fused_and_stand_alone_pooling_by_profile_label(graph, monkeypatch):
    """On the larger size: which pooling layers rode on a convolution and which kept their own kernels."""
    for name in ('STX_CONV_ALGO', 'STX_POOL_FWD_FUSE', 'STX_POOL_BWD_FUSE', 'STX_RELU_CODES'):
        monkeypatch.delenv(name, raising=False)
    fam = odd_nets.family(graph)
    th, tw = LARGE[fam]
    eng = _engine(graph)
    tile = np.random.RandomState(th).uniform(-110, 120, (3, th, tw)).astype(np.float32)
    labels = {}
    for taps in ('pin', 'all'):
        cl, cw, sl, sw = _taps(graph, taps)
        _random_targets(eng, cl, sl, th, tw)
        _, labels[taps] = _labels(eng, tile, cl, cw, sl, sw)
        print(graph, taps, labels[taps])
    pin, every = labels['pin'], labels['all']
    if fam == 'ragged':         # p1 behind c2, p2 behind c4: both behind rectified 3x3 convolutions
        assert any('fwd ' + p not in pin for p in ('p1', 'p2')), pin
        assert any('bwd ' + p not in pin for p in ('p1', 'p2')), pin
        # ... and with a tap on the blobs under them the gradient of those blobs must exist
        assert 'bwd p1' in every and 'bwd p2' in every, every
    elif fam == 'mixed':
        assert 'fwd p2' not in pin, pin                         # p2 rode on c5's epilogue
        assert any('bwd ' + p not in pin for p in ('p1', 'p2')), pin
        # the pool on the image, the rectified pooled blob, the second of two pools: their own kernels
        for label in ('fwd p0', 'fwd p1', 'fwd p3', 'bwd p0', 'bwd p3'):
            assert label in pin and label in every, label
        assert 'bwd p1' in every, every                         # (c3 is tapped there)
        for label in ('fwd c2', 'fwd c4', 'bwd c2', 'bwd c4'):  # the 1x1 layers ran both ways
            assert label in pin and label in every, label
    else:                       # narrow: see LARGE -- nothing can fuse, at any size
        for label in ('fwd p1', 'fwd p2', 'bwd p1', 'bwd p2', 'fwd c4', 'bwd c4'):
            assert label in pin and label in every, label


# --------------------------------------------------------------------------------- 3. fused against unfused
SWITCHES = ['STX_POOL_FWD_FUSE', 'STX_POOL_BWD_FUSE', 'STX_RELU_CODES']


@pytest.mark.parametrize('taps', ['pin', 'all'])
@pytest.mark.parametrize('graph', [g for g in GRAPHS if odd_nets.family(g) != 'narrow'])
def test_fused_paths_change_no_bit(graph, taps, monkeypatch):
    """Each fused path off in turn (fresh engines: the switches are read when a layer is planned): the pooled
    epilogue, the pooled gradient in the staging, the ReLU sign nibbles.  Loss, gradient and every pooled blob
    are BIT-IDENTICAL, and so is a second evaluation on the same engine."""
    from style_transfer_amd.engine import TileEngine
    require_gpu()
    for name in SWITCHES + ['STX_CONV_ALGO']:
        monkeypatch.delenv(name, raising=False)
    th, tw = LARGE[odd_nets.family(graph)]
    net, weights = odd_nets.net_and_weights(graph)
    cl, cw, sl, sw = _taps(graph, taps)
    pools = [l.top for l in net.layers if l.type == 'Pooling']
    tile = np.random.RandomState(tw).uniform(-110, 120, (3, th, tw)).astype(np.float32)
    out = {}
    for off in [None] + SWITCHES:
        if off:
            monkeypatch.setenv(off, '0')
        eng = TileEngine(net, 0, weights)
        try:
            _random_targets(eng, cl, sl, th, tw)
            (loss, grad), labels = _labels(eng, tile, cl, cw, sl, sw)
            again = eng.sc_grad_tile(tile, (0, 0), (0, 0), cl, sl, {}, cw, sw)
            assert again[0] == loss and np.array_equal(again[1], grad), off
            out[off] = (loss, grad, eng.features_tile(tile, pools), labels)
        finally:
            eng.close()
            if off:
                monkeypatch.delenv(off)
    n_fwd = lambda labels: sum(l.startswith('fwd p') for l in labels)
    n_bwd = lambda labels: sum(l.startswith('bwd p') for l in labels)
    assert n_fwd(out['STX_POOL_FWD_FUSE'][3]) == len(pools)
    assert n_bwd(out['STX_POOL_BWD_FUSE'][3]) == len(pools)
    assert n_fwd(out[None][3]) < len(pools)                            # (the A/B is one: something was fused)
    if taps == 'pin':
        assert n_bwd(out[None][3]) < len(pools)
    assert np.isfinite(out[None][0]) and np.isfinite(out[None][1]).all()
    for off in SWITCHES:
        assert out[off][0] == out[None][0], off
        assert np.array_equal(out[off][1], out[None][1]), off
        for p in pools:
            assert np.array_equal(out[off][2][p], out[None][2][p]), (off, p)


# ------------------------------------------------------------------------------------- 4. forced families
@pytest.mark.parametrize('algo', ['direct', 'wino2a', 'wino2b', 'wino2c', 'h2a', 'h2b', 'h2c'])
@pytest.mark.parametrize('size', [1, len(SMALL)])
@pytest.mark.parametrize('graph', ['ragged-max', 'ragged-ave'])
def test_forced_families_on_partial_channel_blocks(graph, size, algo, monkeypatch):
    """STX_CONV_ALGO forces a family where conv_choose lets it and the rest falls through: one graph whose
    channel blocks are all partial, every tap, the oracle's bounds as they stand."""
    monkeypatch.setenv('STX_CONV_ALGO', algo)
    th, tw = _sizes(graph)[size]
    om, tile = _scene(graph, 'all', th, tw)
    cl, cw, sl, sw = _taps(graph, 'all')
    eng = _engine(graph)
    eng.set_contents_and_styles(om.contents, om.styles)
    loss, grad, stats = check_tile(eng, om, tile, (16, 8), (-16, 24), cl, cw, sl, sw, {},
                                   flip_l2=_flip_l2(graph, th, tw))
    print(graph, algo, (th, tw), stats)
    _record('%s all %dx%d STX_CONV_ALGO=%s' % (graph, th, tw, algo), stats)


# ----------------------------------------------------------------------------------------- 5. maxima audit
@pytest.mark.parametrize('taps', ['pin', 'all'])
@pytest.mark.parametrize('size', [1, len(SMALL)])
@pytest.mark.parametrize('graph', [g for g in GRAPHS if odd_nets.family(g) != 'narrow'])
def test_recorded_maxima_bound_what_their_consumers_read(graph, size, taps, monkeypatch):
    """stx_amax_audit (tests/test_gpu_amax_chain.py, piece 1) where the channel blocks are partial and where
    layers that record nothing (the direct family: 1x1 layers, few channels) sit in the chain: recorded >=
    measured on every line -- a condition, not a tolerance -- and recorded == measured where the array's own
    writer recorded it.  Bound-only sites, from the code: the kEpiDgradInject epilogues of conv_h2.hip and
    conv_wino2.hip add the content term of channel 0 in lanes whose channel lies past M; they store nothing,
    but their value enters the recorded maximum -- so the gradient of a content-tapped blob whose channel
    count is no multiple of 64 carries an upper bound."""
    for name in SWITCHES + ['STX_CONV_ALGO', 'STX_CONV_H2', 'STX_CONV_H2_BWD']:
        monkeypatch.delenv(name, raising=False)
    th, tw = _sizes(graph)[size]
    eng = _engine(graph)
    cl, cw, sl, sw = _taps(graph, taps)
    tile = ac.spiked_tile(th, tw, th + tw)
    r = np.random.RandomState(3)
    eng.set_contents_and_styles(
        [{l: (50 * np.abs(r.standard_normal(eng.feature_shape(l, th, tw)))).astype(np.float32) for l in cl}],
        [{l: np.tril(1e3 * r.standard_normal((eng.layer_info(l)[1],) * 2)).astype(np.float32) for l in sl}])
    run = lambda: eng.sc_grad_tile(tile, (0, 0), (0, 0), cl, sl, {}, cw, sw)
    try:
        off = run()
        assert eng.amax_audit_read() == []
        eng.amax_audit(True)
        on = run()
        lines = eng.amax_audit_read()
        eng.amax_audit(False)
        again = run()
        assert eng.amax_audit_read() == []
    finally:
        eng.amax_audit(False)
    assert np.isfinite(off[0]) and np.isfinite(off[1]).all()
    assert on[0] == off[0] and np.array_equal(on[1], off[1])            # the audit changes no bit
    assert again[0] == off[0] and np.array_equal(again[1], off[1])
    kinds = [ac.line_kinds(l, eng.net) for l in lines]
    channels = {b: eng.layer_info(b)[1] for b in eng.net.blob_names()}
    for line, k in zip(lines, kinds):
        consumer, blob, kind, source, recorded, measured = line
        print(graph, (th, tw), taps, line[:4], '%08x %08x' % line[4:])
        assert recorded >= measured, (line, 'the recorded maximum is too small: the split can overflow')
        bound_only = kind == 'diff' and blob in cl and channels[blob] % 64 != 0
        if 'own' in k and not bound_only:
            assert recorded == measured, (line, 'the kernel that wrote the array recorded another maximum')
    if size == len(SMALL):       # not vacuous: the chain was read forward, backward and by the style terms
        seen = set().union(*kinds) if kinds else set()
        assert {'fwd', 'bwd', 'style'} <= seen, (seen, lines)
