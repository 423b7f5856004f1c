"""The odd graphs of tests/odd_nets.py on the host: what netspec derives from them against the oracle's own
bookkeeping, and the prototxt writer / reader on layers no VGG file has (1x1 / pad 0 convolutions, a ReLU on a
pooled blob, AVE and MAX pooling in one file)."""

import numpy as np
import pytest

from oracle import caffe_net
from style_transfer_amd import netspec
from tests import odd_nets

GRAPHS = sorted(odd_nets.GRAPHS)


@pytest.mark.parametrize('graph', GRAPHS)
def test_prototxt_round_trip(graph):
    net, _ = odd_nets.net_and_weights(graph)
    text = netspec.to_prototxt(net)
    back = netspec.parse_prototxt(text)
    assert back.name == net.name
    assert back.layers == net.layers              # (dataclasses: field by field)
    assert netspec.to_prototxt(back) == text
    # the oracle's reader sees the same graph in the same text
    assert caffe_net.layers_from_prototxt(text) == [
        {k: v for k, v in lay.as_dict().items() if k in d} for lay, d in
        zip(net.layers, caffe_net.layers_from_prototxt(text))]


@pytest.mark.parametrize('graph', GRAPHS)
def test_shapes_and_layer_info_agree_with_the_oracle(graph):
    om, net = odd_nets.make_oracle(graph)
    assert net.blob_names() == om.blob_names
    for blob in om.blob_names:
        assert net.layer_info(blob) == (om.scale[blob], om.channels[blob]), blob
    # shapes() at an odd size against the oracle's forward pass (ceil-mode pooling at every stage)
    th, tw = 37, 53
    feats = om.features_tile(np.zeros((3, th, tw), np.float32), om.blob_names)
    shapes = net.shapes(th, tw)
    assert sorted(shapes) == sorted(om.blob_names)
    for blob in om.blob_names:
        assert shapes[blob] == feats[blob].shape, blob


def test_the_graphs_are_what_their_description_says():
    """The properties the GPU tests rely on, from the layer lists themselves."""
    net, _ = odd_nets.net_and_weights('ragged-max')
    convs = [l for l in net.layers if l.type == 'Convolution']
    assert [l.num_output for l in convs] == [24, 40, 72, 96, 132, 160, 68]
    assert all(l.num_output % 4 == 0 and l.num_output % 64 for l in convs)
    assert all(l.kernel_size == 3 and l.pad == 1 for l in convs)
    net, _ = odd_nets.net_and_weights('mixed-ave')
    kinds = [(l.type, l.bottom, l.top) for l in net.layers[1:]]
    assert kinds[0] == ('Pooling', 'data', 'p0')                               # a pool on the image
    assert ('ReLU', 'p1', 'p1') in kinds                                       # a rectified pooled blob
    assert ('Pooling', 'p2', 'p3') in kinds                                    # pool after pool
    assert ('ReLU', 'c3', 'c3') not in kinds and ('Pooling', 'c3', 'p1') in kinds     # un-rectified into a pool
    assert [l.kernel_size for l in net.layers if l.type == 'Convolution'] == [3, 1, 3, 1, 3, 3]
    assert net.layers[-1].type == 'Convolution'                                # un-rectified last blob
    net, _ = odd_nets.net_and_weights('narrow')
    chans = {l.top: l.num_output for l in net.layers if l.type == 'Convolution'}
    assert chans == {'c1': 64, 'c2': 4, 'c3': 64, 'c4': 3, 'c5': 64, 'c6': 64}
    # every tap set names blobs of its graph; 'pin' taps nothing under a pooling layer
    for graph in GRAPHS:
        net, _ = odd_nets.net_and_weights(graph)
        under_pool = {l.bottom for l in net.layers if l.type == 'Pooling'}
        for name, (cl, sl) in odd_nets.TAP_SETS[odd_nets.family(graph)].items():
            assert set(cl) | set(sl) <= set(net.blob_names()), (graph, name)
            if name == 'pin':
                assert not (set(cl) | set(sl)) & under_pool, (graph, name)
