"""Three sequential graphs that are not VGG, as test data (tests/test_gpu_odd_nets.py, tests/test_odd_nets_host.py).

Every test graph of the tile path used to be a VGG: channel counts that are multiples of 64, 3x3 convolutions
each followed by a ReLU, pooling layers behind rectified convolutions only.  csrc/tile_path.cpp decides on
exactly these properties, so each decision had only ever taken one side.  Notation: a->b is a 3x3 / pad 1
convolution, 1x1 a 1x1 / pad 0 one, +R an in-place ReLU behind it.

  ragged   3->24+R, 24->40+R, P, 40->72+R, 72->96+R, P, 96->132+R, 132->160+R, 160->68+R
           every count a multiple of 4 (the style term needs that), none after the image a multiple of 64:
           every channel block of every kernel is partial.  96->132 and 160->68 take the fp16-split kernel
           (K a multiple of 32 and >= 64, M >= 64), the others the fp32 Winograd kernel.  P: MAX | AVE.
  mixed    AVE pool on data, 3->64+R, 1x1 64->64, 64->128, P, +R on the pooled blob, 1x1 128->256+R,
           256->128+R, P, P, 128->64
           1x1 layers both ways, with and without a mask, under and over a tap; an un-rectified blob into a
           pooling layer; a rectified pooled blob; pool after pool; a pool on the image; an un-rectified
           convolution as the net's last blob.  P: MAX | AVE.
  narrow   3->64+R, MAX, 64->4+R, 4->64+R, 1x1 64->3, 3->64+R, AVE, 64->64+R
           the first-layer kernel's shape with a pool directly behind it and again in mid-graph, a 4-channel
           and a 3-channel interior blob, backward into <= 4 channels that are not the image.

Convolution and pooling layers carry their top blob's name (the reference starts its backward passes at the
layer named like the tapped blob, style_transfer.py:606-610)."""

import functools

from oracle.caffe_net import synthetic_weights
from oracle.tile_path import OracleModel
from style_transfer_amd.netspec import LayerSpec, NetSpec


def _build(name, spec):
    """spec: ('conv', blob, cout, ksize, relu) | ('pool', blob, mode) | ('relu', blob) entries, in order."""
    net = NetSpec(name)
    net.layers.append(LayerSpec('input', 'Input', None, 'data', shape=(1, 3, 224, 224)))
    prev = 'data'
    for entry in spec:
        if entry[0] == 'conv':
            _, blob, cout, ks, relu = entry
            net.layers.append(LayerSpec(blob, 'Convolution', prev, blob, num_output=cout, kernel_size=ks,
                                        pad=1 if ks == 3 else 0))
            if relu:
                net.layers.append(LayerSpec('relu_' + blob, 'ReLU', blob, blob))
            prev = blob
        elif entry[0] == 'pool':
            _, blob, mode = entry
            net.layers.append(LayerSpec(blob, 'Pooling', prev, blob, kernel_size=2, stride=2, pool=mode))
            prev = blob
        else:
            net.layers.append(LayerSpec('relu_' + entry[1], 'ReLU', entry[1], entry[1]))
    return net


def ragged(pool='MAX'):
    return _build('ragged_' + pool.lower(), [
        ('conv', 'c1', 24, 3, True), ('conv', 'c2', 40, 3, True), ('pool', 'p1', pool),
        ('conv', 'c3', 72, 3, True), ('conv', 'c4', 96, 3, True), ('pool', 'p2', pool),
        ('conv', 'c5', 132, 3, True), ('conv', 'c6', 160, 3, True), ('conv', 'c7', 68, 3, True)])


def mixed(pool='MAX'):
    return _build('mixed_' + pool.lower(), [
        ('pool', 'p0', 'AVE'), ('conv', 'c1', 64, 3, True), ('conv', 'c2', 64, 1, False),
        ('conv', 'c3', 128, 3, False), ('pool', 'p1', pool), ('relu', 'p1'),
        ('conv', 'c4', 256, 1, True), ('conv', 'c5', 128, 3, True), ('pool', 'p2', pool), ('pool', 'p3', pool),
        ('conv', 'c6', 64, 3, False)])


def narrow():
    return _build('narrow', [
        ('conv', 'c1', 64, 3, True), ('pool', 'p1', 'MAX'), ('conv', 'c2', 4, 3, True),
        ('conv', 'c3', 64, 3, True), ('conv', 'c4', 3, 1, False), ('conv', 'c5', 64, 3, True),
        ('pool', 'p2', 'AVE'), ('conv', 'c6', 64, 3, True)])


GRAPHS = {'ragged-max': lambda: ragged('MAX'), 'ragged-ave': lambda: ragged('AVE'),
          'mixed-max': lambda: mixed('MAX'), 'mixed-ave': lambda: mixed('AVE'), 'narrow': narrow}
# (no MAX pooling anywhere: the gradient is a continuous function of the activations but for the ReLU masks)
ALL_AVE = {'ragged-ave', 'mixed-ave'}


@functools.lru_cache(maxsize=None)
def net_and_weights(graph, seed=0):
    net = GRAPHS[graph]()
    return net, synthetic_weights(net.as_dicts(), seed)


def make_oracle(graph, seed=0):
    net, weights = net_and_weights(graph, seed)
    return OracleModel(net.as_dicts(), weights), net


# Tap sets per graph family: name -> (content layers, style layers).  Weights: tests' normalized_weights.
#   'all'   a style tap on every convolution output (every injecting epilogue and the unfused injection run),
#           content on a pooled blob and, where the graph has one, on an un-rectified blob;
#   'pin'   none of the blobs under a pooling layer is tapped: the pooled-gradient route is allowed.
TAP_SETS = {
    'ragged': {
        'all': (['p2'], ['c1', 'c2', 'c3', 'c4', 'c5', 'c6', 'c7']),
        'pin': (['p1'], ['c1', 'c3', 'c5', 'c6', 'c7']),
    },
    'mixed': {
        # deepest tap: the net's last blob, the un-rectified 128->64; content on the second of two pools and
        # on the un-rectified blob under a pooling layer
        'all': (['p3', 'c3'], ['c1', 'c2', 'c3', 'c4', 'c5', 'c6']),
        # data, c3, c5 and p2 lie under pooling layers; content on an un-rectified 1x1 blob and a pooled one
        'pin': (['p3', 'c2'], ['c1', 'c2', 'c4', 'c6']),
        # deepest tap: the rectified pooled blob
        'pooled-deepest': (['p1'], ['c1', 'c2', 'c3']),
    },
    'narrow': {
        # (c4 has 3 channels: the style term refuses it, test_style_tap_on_three_channels_is_refused)
        # content on the 4-channel blob, a pooled blob and the un-rectified 3-channel blob
        'all': (['c2', 'p2', 'c4'], ['c1', 'c2', 'c3', 'c5', 'c6']),
        'pin': (['c2', 'p1'], ['c2', 'c3', 'c6']),
    },
}


def family(graph):
    return graph.split('-')[0]
