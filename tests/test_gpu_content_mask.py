"""Spatial control of the content term (--content-mask) on the GPU: the masked content term through its
operator hook, the tile path, the farm and the command line -- against tests/content_mask_ref.py.

Tolerances.  Operator hook, against float64 on the same float32 inputs:
  * a = sum m / (h w), summed in double and rounded once: 1e-6 relative (what the mask-map test holds);
  * S = a (m d): three float32 roundings of 6e-8 each (d, m d, a .) plus a's 1e-6, with a margin of about
    3: 4e-6 of max |S_ref|;
  * 1/2 sum m d^2 and sum |m d|, float32 tree sums: 2e-5 relative (the bound tests/test_gpu_style_masks.py
    holds its sums to).
An all-ones mask gives the unmasked hook's two sums and F - c bit for bit; an all-zero mask gives zeros.
The tile path and the farm are held as tests/gpu_helpers.check_tile holds the unmasked path (TIGHT = 1e-5).
Every case prints its figures before it asserts (pytest -s).

Observed worst values on an MI355X: a 4.0e-8, S 9.9e-8 of max, E 9.7e-8, sum |m d| 1.0e-7; tile path: loss
4.7e-7, gradient on the GPU's own activations 1.1e-6 of max, clean pixels 2.7e-6, no decision flips; farm: loss
6.7e-8, clean pixels 2.4e-6.  The all-ones tile gradients came out bit-identical to the unmasked ones."""

import ctypes
import functools

import numpy as np
import pytest
from PIL import Image

from oracle.caffe_net import synthetic_weights
from style_transfer_amd import lib
from style_transfer_amd.netspec import builtin_net
from tests.content_mask_ref import MaskedContentOracleModel, masked_content_terms
from tests.gpu_helpers import TIGHT, decision_taint, gpu_engine, l2_rel, max_rel, require_gpu

pytestmark = pytest.mark.gpu
FLIP_L2 = 1e-2


# --------------------------------------------------------------------- the masked content term
# (5, 7, 70): odd C, more than one 64-lane segment per row, a ragged tail; (64, 72, 70): 322 560 elements,
# more than 256 x 1024, so the grid cap engages
OP_SHAPES = [(5, 7, 70), (64, 37, 29), (512, 5, 3), (64, 72, 70)]
OP_MASKS = ['ones', 'zeros', 'half', 'ramp']
OP_RANGES = [1e-3, 1.0, 1e4]
OY, OX = 2, 5                   # the window's origin; roll_xy = (7, -(h + 2)): both axes wrap


def _window_mask(kind, h, w):
    if kind == 'ones':
        return np.ones((h, w), np.float32)
    if kind == 'zeros':
        return np.zeros((h, w), np.float32)
    if kind == 'half':              # a binary half plane with an odd edge
        m = np.zeros((h, w), np.float32)
        m[:, :(w // 2) | 1] = 1
        return m
    return np.outer(np.linspace(0.1, 1, h), np.linspace(0, 1, w)).astype(np.float32)


def _behind_a_roll(window, mh, mw, roll, rng):
    """A [..., mh, mw] array of noise whose roll by ``roll`` = (x, y) holds ``window`` at (OY, OX)."""
    h, w = window.shape[-2:]
    rolled = rng.uniform(0, 1, window.shape[:-2] + (mh, mw)).astype(np.float32)
    rolled[..., OY:OY + h, OX:OX + w] = window
    return np.ascontiguousarray(np.roll(rolled, (-roll[0], -roll[1]), axis=(-1, -2)))


@pytest.mark.parametrize('big', OP_RANGES)
@pytest.mark.parametrize('kind', OP_MASKS)
@pytest.mark.parametrize('c,h,w', OP_SHAPES)
def test_masked_content_terms_against_float64(c, h, w, kind, big):
    eng = gpu_engine()
    rng = np.random.RandomState(c + h + len(kind))
    feat = (np.maximum(rng.standard_normal((c, h, w)) * 2 + 0.5, 0) * big).astype(np.float32)
    cwin = (np.maximum(rng.standard_normal((c, h, w)) * 2 + 0.5, 0) * big).astype(np.float32)
    m = _window_mask(kind, h, w)
    mh, mw, roll = h + 6, w + 9, (7, -(h + 2))
    content, full = _behind_a_roll(cwin, mh, mw, roll, rng), _behind_a_roll(m, mh, mw, roll, rng)
    half_ref, s_ref, asum_ref, a_ref = masked_content_terms(feat, cwin, m)
    d_feat, d_content, d_map = eng.to_device(feat), eng.to_device(content), eng.to_device(full)
    s_out, out = eng.empty((c, h, w)), (ctypes.c_double * 3)()
    roll_c = (ctypes.c_int * 2)(*roll)
    lib.call('stx_op_masked_content_terms', eng.handle, d_feat.ptr, c, h, w, d_content.ptr, mh, mw, d_map.ptr,
             OY, OX, roll_c, s_out.ptr, out)
    s, (half, asum, a) = s_out.get(), list(out)
    assert np.all(np.isfinite(s)) and np.isfinite(half) and np.isfinite(asum)
    if kind == 'zeros':
        assert half == 0 and asum == 0 and a == 0 and not s.any()
    else:
        err = float(np.abs(s - s_ref).max() / np.abs(s_ref).max())
        print('C %d %dx%d %s x%g: S %.2e, E %.2e, sum|m d| %.2e, a %.2e'
              % (c, h, w, kind, big, err, abs(half / half_ref - 1), abs(asum / asum_ref - 1), abs(a / a_ref - 1)))
        assert a == pytest.approx(a_ref, rel=1e-6)
        assert err <= 4e-6
        assert half == pytest.approx(half_ref, rel=2e-5)
        assert asum == pytest.approx(asum_ref, rel=2e-5)
    if kind == 'ones':
        # the same walk over the same differences: the unmasked hook's sums and F - c, bit for bit
        sums = (ctypes.c_double * 2)()
        lib.call('stx_op_content_terms', eng.handle, d_feat.ptr, c, h, w, d_content.ptr, mh, mw, OY, OX, roll_c,
                 None, sums)
        assert a == 1.0
        assert half == 0.5 * sums[0] and asum == sums[1], (half, 0.5 * sums[0], asum, sums[1])
        assert np.array_equal(s, feat - cwin)
    for arr in (d_feat, d_content, d_map, s_out):
        arr.free()


# --------------------------------------------------------------------------------- the tile path
SL = ['conv1_1', 'conv2_1', 'conv3_1']
LW = {'conv2_1': 1.5}
FRAME = (128, 128)
# (content layers, their weights, style layers).  'apart': the masked term at the deepest tap, injected on its
# own; 'shared': conv3_1 is content and style layer, two gradient blobs, the stand-alone injection; 'under':
# a style layer lies deeper, so the masked term rides in the epilogue of the convolution backward above it
CONTENT = {'apart': (['conv3_2'], {'conv3_2': 0.05}, SL),
           'shared': (['conv3_1'], {'conv3_1': 0.05}, SL),
           'under': (['conv3_2'], {'conv3_2': 0.05}, ['conv1_1', 'conv2_1', 'conv4_1'])}


def _sw(sl):
    return {l: 1 / 3 for l in sl}


def _smooth_mask(hw, seed=0):
    y, x = np.mgrid[:hw[0], :hw[1]]
    return np.float32(0.5 + 0.5 * np.sin(0.09 * x + 0.05 * y + seed) * np.cos(0.04 * y - 0.02 * x))


@functools.lru_cache(maxsize=None)
def _scene(which):
    """Oracle with targets of a 128 x 128 frame and a smooth content mask, computed once."""
    cl, _, sl = CONTENT[which]
    net = builtin_net('vgg19')
    mom = MaskedContentOracleModel(net.as_dicts(), synthetic_weights(net.as_dicts(), 0))
    rng = np.random.RandomState(11)
    full = rng.uniform(-110, 120, (3,) + FRAME).astype(np.float32)
    style = rng.uniform(-110, 120, (3, 40, 44)).astype(np.float32)
    mom.styles = [mom.style_grams([style], sl, 512)]
    mom.contents = [mom.prepare_features(full, cl, 512)]
    mask = _smooth_mask(FRAME)
    mom.set_content_mask(mask, cl)
    return mom, full, mask


def _arm(eng, mom, mask):
    eng.set_contents_and_styles(mom.contents, mom.styles)
    eng.set_content_mask(mask)


def check_masked_tile(eng, mom, tile, start, roll, cl, cw, sl):
    """tests/gpu_helpers.check_tile with the masked oracle: the loss to TIGHT against the float64 formula,
    the gradient to TIGHT of max against the oracle's backward pass on the GPU's own activations (no pixel
    excluded), and against the oracle's end-to-end gradient on decision-clean pixels."""
    sw = _sw(sl)
    loss, grad = eng.sc_grad_tile(tile, start, roll, cl, sl, LW, cw, sw)
    deepest = mom.deep_to_shallow(cl + sl)[0]
    blobs = mom.blob_names[:mom.blob_names.index(deepest) + 1]
    acts = eng.features_tile(tile, blobs)
    mom.roll_contents(roll)
    try:
        ref_loss, oracle_grad = mom.sc_grad_tile(tile, start, cl, sl, LW, cw, sw)
        ref_acts = {b: mom.net.blobs[b].data[0].copy() for b in blobs}
        same_loss, same_grad = mom.sc_grad_tile(tile, start, cl, sl, LW, cw, sw, activations=acts)
        loss64 = mom.masked_loss64(ref_acts, start, cl, sl, LW, cw, sw)
    finally:
        mom.roll_contents(-np.asarray(roll))
    taint, n_relu, n_pool = decision_taint(mom.net.layers, acts, ref_acts, deepest, {'data': tile.shape})
    clean = ~taint
    scale = np.abs(oracle_grad).max()
    stats = dict(loss=abs(loss / loss64 - 1), same=max_rel(grad, same_grad), l2=l2_rel(grad, oracle_grad),
                 clean=float(np.abs(np.float64(grad) - oracle_grad)[:, clean].max() / scale) if clean.any() else 0.0,
                 flips=(n_relu, n_pool))
    print('masked content tile', cl, tile.shape, start, roll, stats)
    assert np.all(np.isfinite(grad))
    assert loss == pytest.approx(loss64, rel=TIGHT), (loss, loss64, ref_loss, same_loss)
    assert stats['same'] < TIGHT, stats
    assert stats['clean'] < TIGHT, stats
    assert stats['l2'] < FLIP_L2, stats
    return loss, grad


def _tile(full, th, tw, start, roll):
    rolled = np.roll(full, (roll[0], roll[1]), axis=(-1, -2))
    return np.ascontiguousarray(rolled[:, start[0]:start[0] + th, start[1]:start[1] + tw])


@pytest.mark.parametrize('which,th,tw,start,roll', [('apart', 64, 48, (0, 0), (0, 0)),
                                                    ('apart', 37, 53, (64, 32), (-24, 40)),
                                                    ('shared', 64, 48, (0, 0), (0, 0)),
                                                    ('shared', 37, 53, (64, 32), (-24, 40)),
                                                    ('under', 37, 53, (64, 32), (-24, 40))])
def test_masked_tile_against_the_oracle(which, th, tw, start, roll):
    """The three placements of the masked term (CONTENT) against the oracle."""
    mom, full, mask = _scene(which)
    eng = gpu_engine()
    _arm(eng, mom, mask)
    check_masked_tile(eng, mom, _tile(full, th, tw, start, roll), start, roll, *CONTENT[which])
    eng.set_content_mask(None)


@pytest.mark.parametrize('which', ['apart', 'shared', 'under'])
def test_all_ones_mask_at_tile_level(which):
    """The sums of an all-ones mask are the unmasked kernel's: the loss is bit-identical.  The gradient takes
    another route (a gradient blob instead of the recomputed difference): within TIGHT."""
    mom, full, _ = _scene(which)
    cl, cw, sl = CONTENT[which]
    eng = gpu_engine()
    tile = _tile(full, 37, 53, (64, 32), (-24, 40))
    run = lambda: eng.sc_grad_tile(tile, (64, 32), (-24, 40), cl, sl, LW, cw, _sw(sl))
    eng.set_contents_and_styles(mom.contents, mom.styles)
    plain = run()
    eng.set_content_mask(np.ones(FRAME, np.float32))
    ones = run()
    eng.set_content_mask(None)
    print('all-ones mask (%s): gradient off by %.2e of max, bit-identical: %s'
          % (which, max_rel(ones[1], plain[1]), np.array_equal(ones[1], plain[1])))
    assert ones[0] == plain[0]
    assert max_rel(ones[1], plain[1]) < TIGHT


@pytest.mark.parametrize('which', ['apart', 'shared', 'under'])
def test_masked_tile_is_bit_identical_across_schedules_and_runs(which, monkeypatch):
    mom, full, mask = _scene(which)
    cl, cw, sl = CONTENT[which]
    eng = gpu_engine()
    _arm(eng, mom, mask)
    tile = _tile(full, 64, 48, (0, 0), (0, 0))
    run = lambda: eng.sc_grad_tile(tile, (0, 0), (0, 0), cl, sl, LW, cw, _sw(sl))
    first, again = run(), run()
    assert first[0] == again[0] and np.array_equal(first[1], again[1])          # deterministic
    for value in ('0', '1'):
        monkeypatch.setenv('STX_SUMS_LATE', value)
        lib.reread_env()
        other = run()
        monkeypatch.delenv('STX_SUMS_LATE')
        lib.reread_env()
        assert other[0] == first[0] and np.array_equal(other[1], first[1]), value
    eng.set_content_mask(None)


def test_no_mask_changes_no_bit_and_targets_clear_the_mask():
    from style_transfer_amd.engine import TileEngine
    require_gpu()
    mom, full, mask = _scene('apart')
    cl, cw, sl = CONTENT['apart']
    net = builtin_net('vgg19')
    weights = synthetic_weights(net.as_dicts(), 0)
    never = TileEngine(net, 0, weights)          # no mask was ever set on this one
    eng = TileEngine(net, 0, weights)
    tile = _tile(full, 64, 48, (0, 0), (0, 0))
    run = lambda e: e.sc_grad_tile(tile, (0, 0), (0, 0), cl, sl, LW, cw, _sw(sl))
    never.set_contents_and_styles(mom.contents, mom.styles)
    before = run(never)
    _arm(eng, mom, mask)
    masked = run(eng)
    assert masked[0] != before[0] and not np.array_equal(masked[1], before[1])
    eng.set_content_mask(None)                                           # stx_set_content_mask(NULL) clears
    cleared = run(eng)
    assert cleared[0] == before[0] and np.array_equal(cleared[1], before[1])
    eng.set_content_mask(mask)
    eng.set_contents_and_styles(mom.contents, mom.styles)                # clears the mask
    fresh = run(eng)
    assert fresh[0] == before[0] and np.array_equal(fresh[1], before[1])
    again = run(never)
    assert again[0] == before[0] and np.array_equal(again[1], before[1])
    never.close()
    eng.close()


def test_mask_size_is_checked_when_it_is_set():
    """A 37 x 53 frame: the maps of conv1_2 / conv2_2 / conv3_2 are 37 x 53, 19 x 27 and 10 x 14."""
    from style_transfer_amd.engine import TileEngine
    require_gpu()
    net = builtin_net('vgg19')
    eng = TileEngine(net, 0, synthetic_weights(net.as_dicts(), 0))
    rng = np.random.RandomState(3)
    shapes = {'conv1_2': (64, 37, 53), 'conv2_2': (128, 19, 27), 'conv3_2': (256, 10, 14)}
    contents = [{l: rng.uniform(0, 1, s).astype(np.float32) for l, s in shapes.items()}]
    with pytest.raises(lib.StxError, match='no content targets'):
        eng.set_content_mask(np.ones((37, 53), np.float32))
    eng.set_contents_and_styles(contents, [])
    eng.set_content_mask(rng.uniform(0, 1, (37, 53)).astype(np.float32))
    with pytest.raises(lib.StxError, match="a 36x53 mask gives a .* map at layer .*the content picture's size"):
        eng.set_content_mask(np.ones((36, 53), np.float32))
    with pytest.raises(lib.StxError, match="the content picture's size"):
        eng.set_content_mask(np.ones((37, 57), np.float32))             # conv1_2 and conv3_2 (15 columns)
    with pytest.raises(ValueError, match=r'\[H, W\]'):
        eng.set_content_mask(np.ones((1, 37, 53), np.float32))
    eng.set_content_mask(None)
    eng.close()


# -------------------------------------------------------------------------------------- the farm
def test_farm_with_a_content_mask_against_the_oracle():
    """A 96 x 80 image in 2 x 2 tiles of 48 x 40 over two streams, a non-zero roll."""
    from oracle.tile_path import tile_grid
    from style_transfer_amd.farm import TileFarm
    require_gpu()
    cl, cw, sl = CONTENT['apart']
    sw = _sw(sl)
    net = builtin_net('vgg19')
    weights = synthetic_weights(net.as_dicts(), 0)
    mom = MaskedContentOracleModel(net.as_dicts(), weights)
    rng = np.random.RandomState(21)
    H, W, roll = 96, 80, (8, -16)
    img = rng.uniform(-110, 120, (3, H, W)).astype(np.float32)
    target = rng.uniform(-110, 120, (3, H, W)).astype(np.float32)
    style = rng.uniform(-110, 120, (3, 40, 44)).astype(np.float32)
    mom.styles = [mom.style_grams([style], sl, 512)]
    mom.contents = [mom.prepare_features(target, cl, 512)]
    mask = _smooth_mask((H, W), 1)
    mom.set_content_mask(mask, cl)
    farm = TileFarm(net, [0], weights, verbose=False, streams_per_device=2)
    farm.set_contents_and_styles(mom.contents, mom.styles)
    farm.set_content_mask(mask)
    d_img, d_grad = farm.master.to_device(img), farm.master.empty(img.shape)
    loss = farm.eval_sc_grad(d_img, d_grad, roll, cl, sl, LW, cw, sw, 64)
    grad = np.roll(d_grad.get(), (roll[0], roll[1]), axis=(-1, -2))           # into the rolled frame
    rolled = np.roll(img, (roll[0], roll[1]), axis=(-1, -2))
    ref_loss, ref_grad = mom.sc_grad(rolled, roll, 64, cl, sl, LW, cw, sw)
    # decision-clean pixels, tile by tile
    deepest = mom.deep_to_shallow(cl + sl)[0]
    blobs = mom.blob_names[:mom.blob_names.index(deepest) + 1]
    clean = np.zeros((H, W), bool)
    for (y0, y1, x0, x1) in tile_grid((H, W), 64):
        tile = np.ascontiguousarray(rolled[:, y0:y1, x0:x1])
        acts, ref_acts = farm.master.features_tile(tile, blobs), mom.features_tile(tile, blobs)
        taint, _, _ = decision_taint(mom.net.layers, acts, ref_acts, deepest, {'data': tile.shape})
        clean[y0:y1, x0:x1] = ~taint
    err = float(np.abs(np.float64(grad) - ref_grad)[:, clean].max() / np.abs(ref_grad).max())
    print('farm: %d engines, loss %.2e, clean %.2e (%.0f%% clean), l2 %.2e'
          % (len(farm.engines), abs(loss / ref_loss - 1), err, 100 * clean.mean(), l2_rel(grad, ref_grad)))
    assert farm.tile_evals == 4 and len(farm.engines) == 2
    assert loss == pytest.approx(ref_loss, rel=TIGHT)
    assert clean.any() and err < TIGHT
    assert l2_rel(grad, ref_grad) < FLIP_L2
    farm.close()


# ------------------------------------------------------------------------------ the command line
def _cli_run(tmp_path, monkeypatch, capsys, name, extra):
    import csv
    import glob
    from style_transfer_amd import cli
    where = tmp_path / name
    where.mkdir()
    monkeypatch.chdir(where)
    argv = ['-ci', '../c.png', '-si', '../s.png', '--size', '64', '--min-size', '64', '-i', '3', '--tile-size', '64',
            '--model', 'vgg19', '--weights', 'synthetic:0', '--devices', '0', '-oi', 'out.png'] + extra
    assert cli.main(argv) == 0
    capsys.readouterr()
    final = Image.open(where / 'out.png')
    logs = glob.glob(str(where / '*_log.csv'))
    assert len(logs) == 1
    with open(logs[0], newline='') as f:
        losses = [float(row['loss']) for row in csv.DictReader(f)]
    return np.asarray(final.convert('RGB')), final.text['Comment'], losses


def test_cli_content_mask(tmp_path, monkeypatch, capsys):
    rng = np.random.RandomState(4)
    picture = lambda hw: Image.fromarray(np.uint8(rng.uniform(0, 255, hw + (3,))))
    picture((64, 56)).save(tmp_path / 'c.png')
    picture((48, 52)).save(tmp_path / 's.png')
    Image.fromarray(np.uint8(255 * _smooth_mask((64, 56)))).save(tmp_path / 'm.png')
    Image.fromarray(np.full((64, 56), 255, np.uint8)).save(tmp_path / 'white.png')
    masked = _cli_run(tmp_path, monkeypatch, capsys, 'masked', ['--content-mask', '../m.png'])
    bare = _cli_run(tmp_path, monkeypatch, capsys, 'bare', [])
    white = _cli_run(tmp_path, monkeypatch, capsys, 'white', ['--content-mask', '../white.png'])
    assert masked[0].shape == (64, 56, 3) and len(masked[2]) == 3 and np.all(np.isfinite(masked[2]))
    assert "content_mask='../m.png'" in masked[1] and 'content_mask' not in bare[1]
    assert masked[2] != bare[2]
    print('cli: losses', masked[2], bare[2], white[2])
    assert white[2] == pytest.approx(bare[2], rel=TIGHT)
    # --jitter: the mask is rolled with the picture and sent again behind every iteration's targets
    jm = _cli_run(tmp_path, monkeypatch, capsys, 'jm', ['--jitter', '--content-mask', '../m.png'])
    jb = _cli_run(tmp_path, monkeypatch, capsys, 'jb', ['--jitter'])
    jw = _cli_run(tmp_path, monkeypatch, capsys, 'jw', ['--jitter', '--content-mask', '../white.png'])
    print('cli --jitter: losses', jm[2], jb[2], jw[2])
    assert len(jm[2]) == 3 and np.all(np.isfinite(jm[2])) and jm[2] != jb[2]
    assert jw[2] == pytest.approx(jb[2], rel=TIGHT)
