"""stx_sc_grad_tile on the caller's own buffers: where the tile and its gradient are device memory of the engine's
GPU, the first layer reads the tile where it is and the backward-into-image kernel writes the gradient where it
goes (csrc/tile_path.cpp: tile_io_direct, TileIoView) -- no copy into the input blob, none out of its diff.

The kernels and their arithmetic are the same whichever way a tile is passed, so every way must give the SAME BITS:
np.array_equal on the gradient, equal float.hex on the loss.  Which ends of a call worked in place is read from the
engine's counter (lib.Q_TILE_IO_DIRECT: up to two per call), so that a test cannot pass by never leaving the copy path.

Both kernels need float alignment only (dword buffer loads in conv_first.hip, dword stores in conv3x3_m4_kernel;
their 16-byte forms are chosen by the alignment of the OTHER blob), so a view that is 4-byte but not 16-byte aligned
works in place too -- and must give the bits of an aligned one."""

import numpy as np
import pytest

from tests import odd_nets
from tests.gpu_helpers import builtin_net, require_gpu, synthetic_weights
from tests.helpers import normalized_weights

pytestmark = pytest.mark.gpu

# 32 x 32, and the ragged size of tests/test_gpu_tile_path.py and tests/test_gpu_odd_nets.py
SIZES = [(32, 32), (37, 53)]
CL, SL = ['conv4_2'], ['conv1_1', 'conv2_1', 'conv3_1', 'conv4_1', 'conv5_1']
CW, SW = {'conv4_2': 0.05}, {l: 0.2 for l in SL}
START, ROLL = (8, 16), (-16, 24)

_STATE = {}


@pytest.fixture(scope='module', autouse=True)
def _close():
    yield
    for eng in _STATE.pop('engines', []):
        eng.close()
    _STATE.clear()


def _vgg():
    """One VGG-19 engine with synthetic weights and random targets that fit every tile of this file."""
    from style_transfer_amd.engine import TileEngine
    require_gpu()
    if 'vgg' not in _STATE:
        net = builtin_net('vgg19')
        weights = synthetic_weights(net.as_dicts(), 0)
        eng = TileEngine(net, 0, weights)
        r = np.random.RandomState(3)
        contents = [{l: np.abs(r.standard_normal(eng.feature_shape(l, 96, 128))).astype(np.float32) for l in CL}]
        styles = [{l: np.tril(r.standard_normal((eng.layer_info(l)[1],) * 2)).astype(np.float32) for l in SL}]
        eng.set_contents_and_styles(contents, styles)
        _STATE.update(vgg=eng, net=net, weights=weights, targets=(contents, styles))
        _STATE.setdefault('engines', []).append(eng)
    return _STATE['vgg']


def _tile(th, tw, seed=0):
    return np.random.RandomState(1000 * th + tw + seed).uniform(-110, 120, (3, th, tw)).astype(np.float32)


def _evaluate(eng, img, grad_out=None, taps=(CL, SL, CW, SW)):
    """-> (float.hex of the loss, gradient as an ndarray, how many ends of the call needed no copy)."""
    from style_transfer_amd import lib
    from style_transfer_amd.engine import DeviceArray
    cl, sl, cw, sw = taps
    before = eng.query(lib.Q_TILE_IO_DIRECT)
    pending = eng.sc_grad_tile_async(img, START, ROLL, cl, sl, {}, cw, sw, grad_out=grad_out)
    eng.sync()
    grad = pending.grad.get() if isinstance(pending.grad, DeviceArray) else np.array(pending.grad)
    return float(pending.loss).hex(), grad, int(eng.query(lib.Q_TILE_IO_DIRECT) - before)


def _unaligned(eng, shape):
    """A device array of `shape` whose address is 4-byte but not 16-byte aligned (a view; its owner rides along)."""
    from style_transfer_amd.engine import DeviceArray
    owner = eng.empty((int(np.prod(shape)) + 4,))
    assert owner.ptr % 16 == 0
    return DeviceArray.from_pointer(eng, owner.ptr + 4, shape, owner=owner)


@pytest.mark.parametrize('th,tw', SIZES)
def test_every_way_of_passing_a_tile_gives_the_same_bits(th, tw, monkeypatch):
    from style_transfer_amd import lib
    eng = _vgg()
    tile = _tile(th, tw)
    # (c) host arrays: the copy path, as ever
    loss_c, grad_c, direct = _evaluate(eng, tile)
    assert direct == 0 and np.isfinite(grad_c).all() and np.abs(grad_c).max() > 0
    # (a) the caller's own device buffers: both ends in place, and the tile is not written to
    d_img, d_grad = eng.to_device(tile), eng.empty(tile.shape).zero()
    loss_a, grad_a, direct = _evaluate(eng, d_img, d_grad)
    assert direct == 2
    assert loss_a == loss_c and np.array_equal(grad_a, grad_c)
    assert np.array_equal(d_img.get(), tile)
    # (b) the engine's own buffers, asked for behind a call that worked in place: the blob has its pointers back
    b_img, b_grad = eng.io_buffers(th, tw)
    b_img.set(tile)
    loss_b, grad_b, direct = _evaluate(eng, b_img, b_grad)
    assert direct == 0
    assert loss_b == loss_c and np.array_equal(grad_b, grad_c)
    # (d) views that are float-aligned and no more
    u_img, u_grad = _unaligned(eng, tile.shape), _unaligned(eng, tile.shape)
    assert u_img.ptr % 16 == 4 and u_grad.ptr % 16 == 4
    u_img.set(tile)
    loss_d, grad_d, direct = _evaluate(eng, u_img, u_grad)
    assert direct == 2
    assert loss_d == loss_c and np.array_equal(grad_d, grad_c)
    assert np.array_equal(u_img.get(), tile)
    # one end each: a host tile with a device gradient, and the other way round
    loss_e, grad_e, direct = _evaluate(eng, tile, d_grad.zero())
    assert direct == 1 and loss_e == loss_c and np.array_equal(grad_e, grad_c)
    loss_f, grad_f, direct = _evaluate(eng, d_img)
    assert direct == 1 and loss_f == loss_c and np.array_equal(grad_f, grad_c)
    # STX_TILE_IO_DIRECT=0 keeps the copies
    monkeypatch.setenv('STX_TILE_IO_DIRECT', '0')
    lib.reread_env()
    try:
        loss_g, grad_g, direct = _evaluate(eng, d_img, d_grad.zero())
    finally:
        monkeypatch.delenv('STX_TILE_IO_DIRECT')
        lib.reread_env()
    assert direct == 0 and loss_g == loss_c and np.array_equal(grad_g, grad_c)


@pytest.mark.parametrize('th,tw', SIZES)
def test_two_tiles_queued_back_to_back_each_get_their_own_result(th, tw):
    """Goes wrong if the blob's pointers are not restored between the calls, or are read later than at queueing."""
    eng = _vgg()
    tiles = [_tile(th, tw, 1), _tile(th, tw, 2)]
    want = [_evaluate(eng, t) for t in tiles]
    assert not np.array_equal(want[0][1], want[1][1])
    bufs = [(eng.to_device(t), eng.empty(t.shape).zero()) for t in tiles]
    pending = [eng.sc_grad_tile_async(img, START, ROLL, CL, SL, {}, CW, SW, grad_out=grad) for img, grad in bufs]
    eng.sync()
    for p, (loss, grad, _), (img, _), t in zip(pending, want, bufs, tiles):
        assert float(p.loss).hex() == loss and np.array_equal(p.grad.get(), grad)
        assert np.array_equal(img.get(), t)


def test_a_second_engine_of_the_sharing_group_agrees():
    from style_transfer_amd.engine import TileEngine
    eng = _vgg()
    th, tw = SIZES[1]
    tile = _tile(th, tw)
    loss, grad, _ = _evaluate(eng, tile)
    other = TileEngine(_STATE['net'], 0, share=eng)
    _STATE['engines'].append(other)
    d_img, d_grad = other.to_device(tile), other.empty(tile.shape).zero()
    loss_o, grad_o, direct = _evaluate(other, d_img, d_grad)
    assert direct == 2 and loss_o == loss and np.array_equal(grad_o, grad)
    # ... and buffers that the first engine allocated (the same GPU) serve the second as well
    e_img, e_grad = eng.to_device(tile), eng.empty(tile.shape).zero()
    eng.sync()
    loss_o, grad_o, direct = _evaluate(other, e_img, e_grad)
    assert direct == 2 and loss_o == loss and np.array_equal(grad_o, grad)


# which ends work in place on graphs whose first layer is not the VGG first layer alone: `ragged` starts with a
# 3 -> 24 convolution (the fp32 Winograd family reads the tile: the copy stays; conv_small_launch writes the
# gradient: in place), `mixed` with a pooling layer on the image (both copies stay), `narrow` with 3 -> 64 under a
# pooling layer that rides on its epilogue (not the first-layer kernel: the copy stays; gradient in place)
@pytest.mark.parametrize('graph,ends', [('ragged-max', 1), ('mixed-ave', 0), ('narrow', 1)])
def test_other_graphs(graph, ends):
    from style_transfer_amd.engine import TileEngine
    require_gpu()
    net, weights = odd_nets.net_and_weights(graph)
    eng = TileEngine(net, 0, weights)
    _STATE.setdefault('engines', []).append(eng)
    cl, sl = odd_nets.TAP_SETS[odd_nets.family(graph)]['all']
    cl, cw = normalized_weights(cl, 0.05)
    sl, sw = normalized_weights(sl, 1)
    th, tw = SIZES[1]
    r = np.random.RandomState(5)
    eng.set_contents_and_styles(
        [{l: np.abs(r.standard_normal(eng.feature_shape(l, 96, 128))).astype(np.float32) for l in cl}],
        [{l: np.tril(r.standard_normal((eng.layer_info(l)[1],) * 2)).astype(np.float32) for l in sl}])
    tile = _tile(th, tw)
    taps = (cl, sl, cw, sw)
    loss_c, grad_c, direct = _evaluate(eng, tile, taps=taps)
    assert direct == 0 and np.abs(grad_c).max() > 0
    d_img, d_grad = eng.to_device(tile), eng.empty(tile.shape).zero()
    loss_a, grad_a, direct = _evaluate(eng, d_img, d_grad, taps=taps)
    assert direct == ends
    assert loss_a == loss_c and np.array_equal(grad_a, grad_c)
    assert np.array_equal(d_img.get(), tile)


def test_fallbacks_keep_working():
    from style_transfer_amd.lib import StxError
    eng = _vgg()
    th, tw = SIZES[0]
    tile = _tile(th, tw)
    loss, grad, _ = _evaluate(eng, tile)
    # the gradient over the tile it came from: the copies, as ever
    both = eng.to_device(tile)
    loss_s, grad_s, direct = _evaluate(eng, both, both)
    assert direct == 0 and loss_s == loss and np.array_equal(grad_s, grad)
    # overlapping, not identical
    flat = eng.empty((2 * tile.size - 16,))
    from style_transfer_amd.engine import DeviceArray
    lo = DeviceArray.from_pointer(eng, flat.ptr, tile.shape, owner=flat)
    hi = DeviceArray.from_pointer(eng, flat.ptr + 4 * (tile.size - 16), tile.shape, owner=flat)
    lo.set(tile)
    _, _, direct = _evaluate(eng, lo, hi)
    assert direct == 0
    # a tap on the input blob is refused as before, and the engine goes on
    with pytest.raises(StxError):
        eng.sc_grad_tile(tile, START, ROLL, CL, SL + ['data'], {}, CW, dict(SW, data=0.2))
    loss_t, grad_t, direct = _evaluate(eng, eng.to_device(tile), eng.empty(tile.shape).zero())
    assert direct == 2 and loss_t == loss and np.array_equal(grad_t, grad)
