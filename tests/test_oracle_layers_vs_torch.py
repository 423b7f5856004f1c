"""Cross-check of the oracle's Caffe-layer arithmetic against torch-CPU autograd
(BVLC/caffe itself is un-vendored, so this is the independent pin for conv/pool semantics)."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import layers as L


@pytest.mark.parametrize('cin,cout,h,w', [(3, 64, 33, 47), (64, 64, 32, 32), (256, 512, 9, 11)])
def test_conv_fwd_dgrad(cin, cout, h, w):
    rng = np.random.RandomState(cin + h)
    x = rng.standard_normal((cin, h, w)).astype(np.float32)
    wt = (rng.standard_normal((cout, cin, 3, 3)) * np.sqrt(2 / (9 * cin))).astype(np.float32)
    b = (0.01 * rng.standard_normal(cout)).astype(np.float32)
    dy = rng.standard_normal((cout, h, w)).astype(np.float32)
    xt = torch.tensor(x[None], requires_grad=True)
    yt = F.conv2d(xt, torch.tensor(wt), torch.tensor(b), padding=1)
    yt.backward(torch.tensor(dy[None]))
    y = L.conv_forward(x, wt, b)
    assert np.abs(y - yt[0].detach().numpy()).max() < 2e-4 * np.abs(y).max()
    dx = L.conv_backward_data(dy, wt)
    assert np.abs(dx - xt.grad[0].numpy()).max() < 2e-4 * np.abs(dx).max()


@pytest.mark.parametrize('h,w', [(8, 8), (7, 9), (1, 5), (33, 2)])
@pytest.mark.parametrize('mode', ['MAX', 'AVE'])
def test_pool_ceil_mode(h, w, mode):
    rng = np.random.RandomState(h * 31 + w)
    # post-ReLU-like input: many exact zeros, so MAX windows tie often
    x = np.maximum(rng.standard_normal((5, h, w)), 0).astype(np.float32)
    x[:, ::3] = 0
    y, aux = L.pool_forward(x, mode)
    xt = torch.tensor(x[None], requires_grad=True)
    if mode == 'MAX':
        yt = F.max_pool2d(xt, 2, 2, ceil_mode=True)
    else:
        yt = F.avg_pool2d(xt, 2, 2, ceil_mode=True, count_include_pad=False)
    assert y.shape == tuple(yt.shape[1:]) == (5, L.pooled_size(h), L.pooled_size(w))
    assert np.allclose(y, yt[0].detach().numpy(), atol=1e-6)
    dy = rng.standard_normal(y.shape).astype(np.float32)
    dx = L.pool_backward(dy, x.shape, aux, mode)
    if mode == 'AVE':
        yt.backward(torch.tensor(dy[None]))
        assert np.allclose(dx, xt.grad[0].numpy(), atol=1e-6)
    else:
        # every output's gradient lands on exactly one input of its window, the FIRST maximum
        assert np.allclose(dx.sum(), dy.sum(), rtol=1e-4)
        for c, i, j in [(0, 0, 0), (4, y.shape[1] - 1, y.shape[2] - 1), (2, 0, y.shape[2] - 1)]:
            win = x[c, 2 * i:2 * i + 2, 2 * j:2 * j + 2]
            k = int(np.argmax(win.ravel()))
            assert aux[c, i, j] == (k // win.shape[1]) * 2 + (k % win.shape[1])


@pytest.mark.parametrize('cin,cout,h,w', [(64, 64, 17, 23), (20, 36, 19, 31), (130, 66, 31, 33), (8, 33, 1, 1),
                                          (64, 3, 37, 50)])
def test_conv_1x1_fwd_dgrad(cin, cout, h, w):
    """1x1 / pad 0: the plane keeps its size, backward-to-data is W^T dy per pixel.  Against torch in float64
    at 2e-6 of max: float32 sums of at most 130 products (130 * 2^-24 = 8e-6 is the worst case of a sum of
    like-signed terms; random signs stay far below)."""
    rng = np.random.RandomState(cin + h)
    x = rng.standard_normal((cin, h, w)).astype(np.float32)
    wt = (rng.standard_normal((cout, cin, 1, 1)) * np.sqrt(2 / cin)).astype(np.float32)
    b = (0.01 * rng.standard_normal(cout)).astype(np.float32)
    dy = rng.standard_normal((cout, h, w)).astype(np.float32)
    xt = torch.tensor(x[None].astype(np.float64), requires_grad=True)
    yt = F.conv2d(xt, torch.tensor(wt.astype(np.float64)), torch.tensor(b.astype(np.float64)), padding=0)
    yt.backward(torch.tensor(dy[None].astype(np.float64)))
    y = L.conv_forward(x, wt, b, pad=0)
    assert y.shape == (cout, h, w) and y.dtype == np.float32
    assert np.abs(y - yt[0].detach().numpy()).max() < 2e-6 * np.abs(y).max()
    dx = L.conv_backward_data(dy, wt, pad=0)
    assert dx.shape == (cin, h, w)
    assert np.abs(dx - xt.grad[0].numpy()).max() < 2e-6 * np.abs(dx).max()


def _torch_forward(net, params, tile):
    """The graph in torch, float64: ({blob: [1,C,h,w]} with the in-place ReLUs applied, {blob: what its ReLU read})."""
    p = {k: (torch.tensor(w.astype(np.float64)), torch.tensor(b.astype(np.float64))) for k, (w, b) in params.items()}
    acts, pre = {'data': torch.tensor(np.asarray(tile, np.float64)[None], requires_grad=True)}, {}
    for lay in net.layers[1:]:
        x = acts[lay.bottom]
        if lay.type == 'Convolution':
            acts[lay.top] = F.conv2d(x, *p[lay.name], padding=lay.pad)
        elif lay.type == 'ReLU':
            pre[lay.top] = x
            acts[lay.top] = F.relu(x)
        elif lay.pool == 'MAX':
            acts[lay.top] = F.max_pool2d(x, 2, 2, ceil_mode=True)
        else:       # Caffe's AVE divides by the window clipped to the blob (pad 0)
            acts[lay.top] = F.avg_pool2d(x, 2, 2, ceil_mode=True, count_include_pad=False)
    return acts, pre


@pytest.mark.parametrize('th,tw', [(37, 53), (9, 13)])
@pytest.mark.parametrize('graph', ['ragged-max', 'ragged-ave', 'mixed-max', 'mixed-ave', 'narrow'])
def test_odd_graphs_forward_and_backward(graph, th, tw):
    """The graphs of tests/odd_nets.py through the oracle (float32) against torch autograd in float64: 1x1
    layers, un-rectified blobs into pooling layers, a ReLU on a pooled blob, pool after pool, a pool on the
    image, ceil-mode AVE windows cut by the border (odd planes at every stage of these tiles).  Every blob to
    5e-6 of its maximum -- half of what the GPU tests allow the GPU against this oracle; the gradient of a
    random linear functional of the last blob likewise, where no ReLU / MAX decision sits within the oracle's
    own error of a tie (else torch and the oracle may legitimately route differently: counted, not compared)."""
    from tests import odd_nets
    om, net = odd_nets.make_oracle(graph)
    rng = np.random.RandomState(th)
    tile = rng.uniform(-110, 120, (3, th, tw)).astype(np.float32)
    ref, pre = _torch_forward(net, om.net.params, tile)
    last = om.last_layer
    got = om.features_tile(tile, om.blob_names)
    for b in om.blob_names:
        want = ref[b][0].detach().numpy()
        if b == last:
            want = np.maximum(want, 0)          # (features_tile rectifies the net's last blob)
        assert got[b].shape == want.shape, b
        assert np.abs(got[b] - want).max() < 5e-6 * np.abs(want).max(), b
    # the clipped divisor really occurs: an AVE layer of this case reads an odd plane
    planes = {'data': tile.shape, **{b: got[b].shape for b in om.blob_names}}
    clipped = [l.name for l in net.layers if l.type == 'Pooling' and l.pool == 'AVE' and
               (planes[l.bottom][-2] % 2 or planes[l.bottom][-1] % 2)]
    assert clipped or graph == 'ragged-max', planes
    # backward: d <g, last blob> / d image
    g = rng.standard_normal(got[last].shape).astype(np.float32)
    (ref[last][0] * torch.tensor(g.astype(np.float64))).sum().backward()
    want = ref['data'].grad[0].numpy()
    onet = om.net
    onet.blobs['data'].reshape(1, 3, th, tw)
    onet.blobs['data'].data[0] = tile
    onet.forward(end=last)
    for blob in onet.blobs.values():
        blob.diff[...] = 0
    onet.blobs[last].diff[0] = g
    onet.backward(start=net.layers[-1].name)
    mine = onet.blobs['data'].diff[0]
    assert np.abs(want).max() > 0
    # near-ties: a value about to be rectified, or a MAX window's margin, within 1e-5 of the blob's maximum of
    # a decision (windows of exact zeros behind a ReLU tie on both sides alike and pass no gradient on)
    ties = 0
    for lay in net.layers[1:]:
        if lay.type == 'ReLU':
            a = pre[lay.top][0].detach().numpy()
            ties += int(np.count_nonzero(np.abs(a) < 1e-5 * np.abs(a).max()))
        elif lay.type == 'Pooling' and lay.pool == 'MAX':
            x = ref[lay.bottom][0].detach().numpy()
            stack, valid = L._windows(x.astype(np.float32))
            s = np.sort(np.where(valid[:, None], stack, -np.inf), axis=0)
            ties += int(np.count_nonzero((s[-1] - s[-2] < 1e-5 * np.abs(x).max()) & (s[-1] != 0)))
    if ties == 0:
        assert np.abs(mine - want).max() < 5e-6 * np.abs(want).max()
    else:
        assert np.linalg.norm(mine - want) < 1e-2 * np.linalg.norm(want), ties


def test_blob_with_two_consumers_adds_their_gradients():
    """Caffe puts a Split layer behind a blob that feeds two layers (net.cpp: InsertSplits); the
    reference's *_big prototxts have one (conv1_2 -> pool1, a dead end, and -> conv2_1:
    vgg19_big.prototxt:62).  The pycaffe-shaped shim against torch autograd on that graph: the
    gradient of a loss on conv2_1 and (second case) on conv2_1 AND pool1 reaches the image."""
    from oracle import caffe_net
    from style_transfer_amd.netspec import builtin_net
    layers = [l for l in builtin_net('vgg19_big').as_dicts()][:8]      # input .. relu2_1
    assert [l['name'] for l in layers][-4:] == ['relu1_2', 'pool1', 'conv2_1', 'relu2_1']
    net = caffe_net.Net(layers, weights=None)
    rng = np.random.RandomState(1)
    x = rng.uniform(-100, 100, (3, 13, 18)).astype(np.float32)
    net.blobs['data'].reshape(1, 3, 13, 18)
    net.blobs['data'].data[0] = x
    net.forward(end='relu2_1')
    g2 = rng.standard_normal(net.blobs['conv2_1'].data.shape).astype(np.float32)
    gp = rng.standard_normal(net.blobs['pool1'].data.shape).astype(np.float32)
    for with_pool in (False, True):
        for b in net.blobs.values():
            b.diff[...] = 0
        net._split.clear()
        net.blobs['conv2_1'].diff[...] = g2
        if with_pool:
            net.blobs['pool1'].diff[...] = gp
        net.backward(start='relu2_1')
        xt = torch.tensor(x[None], requires_grad=True)
        p = {k: (torch.tensor(w), torch.tensor(b)) for k, (w, b) in net.params.items()}
        h = F.relu(F.conv2d(xt, *p['conv1_1'], padding=1))
        h = F.relu(F.conv2d(h, *p['conv1_2'], padding=1))
        out = (F.relu(F.conv2d(h, *p['conv2_1'], padding=1)) * torch.tensor(g2)).sum()
        if with_pool:
            out = out + (F.max_pool2d(h, 2, 2, ceil_mode=True) * torch.tensor(gp)).sum()
        out.backward()
        got, ref = net.blobs['data'].diff[0], xt.grad[0].numpy()
        assert np.abs(ref).max() > 0
        assert np.abs(got - ref).max() < 2e-4 * np.abs(ref).max(), with_pool
