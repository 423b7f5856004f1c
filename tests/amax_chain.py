"""Helpers of tests/test_gpu_amax_chain.py: the scenes of the audit cases, the kinds of hand-off an audit
line can be, and nets whose neighbouring blobs differ by a large power of two.

The fp16-split kernels (conv_h2.hip, the two-piece Gram and SYMM kernels; f16x2.h) scale their operand by a
power of two taken from 64 words of float bits that an earlier kernel left behind.  A consumer that reads the
wrong words -- a neighbour's, stale ones, a maximum that missed an edge -- computes the same numbers on data
whose blobs all have similar maxima: these helpers build data on which it does not."""

import functools

import numpy as np

from oracle.caffe_net import synthetic_weights
from oracle.tile_path import OracleModel
from style_transfer_amd.netspec import builtin_net
from tests.helpers import DEFAULT_STYLE_LAYERS

MODELS = ['vgg19', 'vgg16_avgpool']


@functools.lru_cache(maxsize=None)
def plain_weights(model):
    net = builtin_net(model)
    return net, synthetic_weights(net.as_dicts(), 0)


# --------------------------------------------------------------------------------------------- the audit
def spiked_tile(th, tw, seed):
    """Uniform in [-110, 120] with +-2000 at the four corner pixels of every channel: every blob's maximum then
    sits at the ragged last row / column (or the first), where a clipped pooling window, a partial patch or
    an out-of-bounds lane is most likely to be left out of a recorded maximum."""
    tile = np.random.RandomState(seed).uniform(-110, 120, (3, th, tw)).astype(np.float32)
    tile[:, 0, 0] = 2000
    tile[:, 0, tw - 1] = -2000
    tile[:, th - 1, 0] = -2000
    tile[:, th - 1, tw - 1] = 2000
    return tile


def smooth_mask(hw, seed=0):
    y, x = np.mgrid[:hw[0], :hw[1]]
    return np.float32(0.5 + 0.5 * np.sin(0.09 * x + 0.05 * y + seed) * np.cos(0.04 * y - 0.02 * x))


# Tap sets: (content layers and weights, style layers and weights, number of style images, layer weights,
# Deep-Dream layers and weights, masked?)
TAP_SETS = {
    # the defaults of test_sc_grad_tile_odd_sizes_against_oracle: every term rides in a backward epilogue
    'defaults': dict(cl=['conv4_2'], cw={'conv4_2': 0.05}, sl=DEFAULT_STYLE_LAYERS,
                     sw={l: 0.2 for l in DEFAULT_STYLE_LAYERS}, n_styles=1, lw={}, dl=[], dw={}, masked=False),
    # content on a pooling blob, two style images (stand-alone injection with several terms, behind a
    # pooling backward on conv1_2 / conv3_3 / conv2_2: the slot is zeroed first) and Deep-Dream layers
    'pool+2styles+dream': dict(cl=['pool3'], cw={'pool3': 0.3}, sl=['conv1_2', 'conv3_3'],
                               sw={'conv1_2': 0.25, 'conv3_3': 0.75}, n_styles=2,
                               lw={'conv1_2': 2.0, 'pool3': 0.5}, dl=['conv4_3', 'conv2_2'],
                               dw={'conv4_3': 0.01, 'conv2_2': 0.03}, masked=False),
    # one masked style: Gram and SYMM read F . m under the maximum of F
    'masked': dict(cl=['conv4_2'], cw={'conv4_2': 0.05}, sl=DEFAULT_STYLE_LAYERS,
                   sw={l: 0.2 for l in DEFAULT_STYLE_LAYERS}, n_styles=1, lw={'conv2_1': 1.5}, dl=[], dw={},
                   masked=True),
}


def arm(eng, taps, th, tw):
    """Random targets of the tile's own frame (the audit looks at maxima, not at the loss's value)."""
    r = np.random.RandomState(3)
    contents = [{l: (50 * np.abs(r.standard_normal(eng.feature_shape(l, th, tw)))).astype(np.float32)
                 for l in taps['cl']}]
    styles = [{l: np.tril(1e3 * r.standard_normal((eng.layer_info(l)[1],) * 2)).astype(np.float32)
               for l in taps['sl']} for _ in range(taps['n_styles'])]
    eng.set_contents_and_styles(contents, styles)
    if taps['masked']:
        eng.set_style_masks([smooth_mask((th, tw))])


def evaluate(eng, taps, tile):
    return eng.sc_grad_tile(tile, (0, 0), (0, 0), taps['cl'], taps['sl'], taps['lw'], taps['cw'], taps['sw'],
                            dd_layers=taps['dl'], dd_weight=taps['dw'])


def line_kinds(line, net):
    """What an audit line (consumer, blob, data | diff, source, recorded, measured) is an instance of:
      'fwd'      a forward convolution about to read its input blob
      'bwd'      a backward convolution about to read the gradient above it
      'style'    Gram / SYMM about to read a tapped blob (or its masked copy: also 'masked')
      'pin'      a backward convolution that takes the POOLED gradient of the pooling layer above it
      'own'      the slots are the blob's own: the kernel that wrote the array recorded them (or a pass over it)
      'inherited' the slots are another blob's: a pooling layer, forward or backward, passed the bound on
    'own' lines promise equality, every line promises recorded >= measured."""
    consumer, blob, kind, source = line[:4]
    pools = {l.top for l in net.layers if l.type == 'Pooling'}
    kinds = set()
    if consumer.startswith('fwd '):
        kinds.add('fwd')
    if consumer.startswith('bwd '):
        kinds.add('bwd')
        if blob in pools:
            kinds.add('pin')
    if consumer.startswith('style ') or consumer.startswith('masked style '):
        kinds.add('style')
    if consumer.startswith('masked style '):
        kinds.add('masked')
    kinds.add('own' if source == blob and 'masked' not in kinds else 'inherited')
    assert (kind == 'diff') == ('bwd' in kinds), line
    return kinds


def bits_to_float(bits):
    return float(np.array([bits], np.uint32).view(np.float32)[0])


# ----------------------------------------------------------------------------------------- rescaled nets
def blob_exponents(net, step):
    """{blob: K}: convolution l (1, 2, ...) and everything up to the next convolution carry 2^K_l with
    K_l = 0, step, 0, step, ... -- neighbouring convolution outputs differ by 2^|step|."""
    K, k = {'data': 0}, 0
    n = 0
    for lay in net.layers[1:]:
        if lay.type == 'Convolution':
            n += 1
            k = step if n % 2 == 0 else 0
        K[lay.top] = k
    return K


def rescaled_weights(model, step):
    """The synthetic weights with convolution l's filters times 2^(K_l - K_(l-1)) and its bias times 2^K_l
    (np.ldexp: exact).  ReLU and both poolings are positively homogeneous, so every blob of the rescaled net is
    the plain net's times 2^K_l exactly in float32 (no value of these nets comes near the ends of the range:
    oracle_range_check)."""
    net, plain = plain_weights(model)
    K = blob_exponents(net, step)
    out = {}
    for lay in net.layers[1:]:
        if lay.type != 'Convolution':
            continue
        w, b = plain[lay.name]
        out[lay.name] = (np.ldexp(w, K[lay.top] - K[lay.bottom]).astype(np.float32),
                         np.ldexp(b, K[lay.top]).astype(np.float32))
    return out


@functools.lru_cache(maxsize=None)
def rescaled_scene(model, step, th, tw):
    """(oracle with its targets, the full image, the tile, start, roll) of one rescaled case -- the scene of
    test_sc_grad_tile_odd_sizes_against_oracle on the rescaled net; step = 0: the plain net."""
    net, plain = plain_weights(model)
    om = OracleModel(net.as_dicts(), rescaled_weights(model, step) if step else plain)
    rng = np.random.RandomState(th)
    cl, sl = ['conv4_2'], DEFAULT_STYLE_LAYERS
    full = rng.uniform(-110, 120, (3, th + 24, tw + 40)).astype(np.float32)
    style = rng.uniform(-110, 120, (3, 50, 60)).astype(np.float32)
    om.styles = [om.style_grams([style], sl, 512)]
    om.contents = [om.prepare_features(full, cl, 512)]
    tile = np.ascontiguousarray(full[:, 16:16 + th, 8:8 + tw])
    return om, full, tile, (16, 8), (-16, 24)


def oracle_range_check(om, tile, start, cl, cw, sl, sw):
    """With the oracle alone: every activation, Gram, gradient blob and the loss of the evaluation is finite
    and no non-zero value is smaller than 2^-100 -- the scaling by powers of two is then exact in float32 and
    the rescaled net's decisions are the plain net's.  Returns the smallest and the largest magnitude seen."""
    from oracle.num_ops import gram_lower
    loss, grad = om.sc_grad_tile(tile, start, cl, sl, {}, cw, sw)
    deepest = om.deep_to_shallow(list(cl) + list(sl))[0]
    blobs = ['data'] + om.blob_names[:om.blob_names.index(deepest) + 1]
    arrays = {'loss': np.float32([loss]), 'grad': grad}
    for b in blobs:
        arrays['data ' + b] = om.net.blobs[b].data
        arrays['diff ' + b] = om.net.blobs[b].diff
    for b in sl:
        arrays['gram ' + b] = gram_lower(om.net.blobs[b].data[0])
    lo, hi = np.inf, 0.0
    for name, a in arrays.items():
        assert np.isfinite(a).all(), name
        mag = np.abs(np.asarray(a, np.float64))
        nz = mag[mag > 0]
        if nz.size:
            assert nz.min() >= 2.0 ** -100, (name, nz.min())
            lo, hi = min(lo, nz.min()), max(hi, nz.max())
    return lo, hi
