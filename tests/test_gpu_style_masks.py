"""Spatial control (--style-masks) on the GPU: the mask-map kernel, the masked style term through its
operator hook, the tile path, the farm and the command line -- against tests/masked_style_ref.py.

Tolerances.  The operator hook is held to what tests/test_gpu_kernels.py holds stx_op_style_terms to: S to
2e-5 of its maximum, 1/2 |D|^2 and sum |S| to 2e-5 relative (test_style_terms_over_channel_counts_and_ranges),
and S of the default (fp16-split) kernels to 3 x the error of the fp32-MFMA kernels on the same inputs + 1e-7
(test_style_terms_fp16_split_is_no_worse_than_the_fp32_kernels) -- for every mask, the all-ones mask
included.  a = sum m^2 / HW is a float sum of at most 1073 values in [0, 1]: 1e-6 relative.  The tile path
and the farm are held as tests/gpu_helpers.check_tile holds the unmasked path (TIGHT = 1e-5).

Observed worst values on an MI355X: none recorded yet -- this file has not been run on a GPU (DESIGN.md
section 3.10 says the same); every case prints its figures before it asserts (pytest -s)."""

import ctypes
import functools
import re

import numpy as np
import pytest
from PIL import Image

from oracle.caffe_net import synthetic_weights
from style_transfer_amd import lib
from style_transfer_amd.netspec import builtin_net
from tests.gpu_helpers import TIGHT, decision_taint, fp32_kernels, gpu_engine, l2_rel, max_rel
from tests.masked_style_ref import MaskedOracleModel, mask_map, masked_style_terms

pytestmark = pytest.mark.gpu
FLIP_L2 = 1e-2


# ------------------------------------------------------------------------------- the mask map
@pytest.mark.parametrize('s', [1, 2, 4, 8, 16])
@pytest.mark.parametrize('H,W', [(37, 53), (64, 48)])
def test_mask_map_kernel(H, W, s):
    eng = gpu_engine()
    M = np.random.RandomState(H + s).uniform(0, 1, (H, W)).astype(np.float32)
    ref = mask_map(M, s)
    d_m, out = eng.to_device(M), eng.empty(ref.shape)
    lib.call('stx_image_mask_map', eng.handle, d_m.ptr, H, W, s, out.ptr)
    got = out.get()
    err = float(np.abs(got - ref).max())
    print('mask map %dx%d s=%d: %.2e' % (H, W, s, err))
    assert err <= 1e-6
    for a in (d_m, out):
        a.free()


# ----------------------------------------------------------------------- the masked style term
OP_SHAPES = [(64, 37, 29), (128, 16, 16), (256, 10, 7), (512, 5, 3)]
OP_MASKS = ['ones', 'zeros', 'half', 'ramp']
OP_RANGES = [1e-3, 1.0, 1e4]
OY, OX, ROLL = 2, 5, (7, None)      # the window's origin; roll_xy = (7, -(h + 2)): both axes wrap


def _window_mask(kind, h, w):
    if kind == 'ones':
        return np.ones((h, w), np.float32)
    if kind == 'zeros':
        return np.zeros((h, w), np.float32)
    if kind == 'half':              # a binary half plane whose edge is no multiple of four
        m = np.zeros((h, w), np.float32)
        m[:, :(w // 2) | 1] = 1
        return m
    return np.outer(np.linspace(0.1, 1, h), np.linspace(0, 1, w)).astype(np.float32)


def _op_call(eng, d_feat, c, h, w, d_map, mh, mw, roll, d_tgt):
    s_out = eng.empty((c, h, w))
    out = (ctypes.c_double * 3)()
    lib.call('stx_op_masked_style_terms', eng.handle, d_feat.ptr, c, h, w, d_map.ptr, mh, mw, OY, OX,
             (ctypes.c_int * 2)(*roll), d_tgt.ptr, s_out.ptr, out)
    s = s_out.get()
    s_out.free()
    return s, list(out)


@pytest.mark.parametrize('big', OP_RANGES)
@pytest.mark.parametrize('kind', OP_MASKS)
@pytest.mark.parametrize('c,h,w', OP_SHAPES)
def test_masked_style_terms_against_float64(c, h, w, kind, big):
    eng = gpu_engine()
    rng = np.random.RandomState(c + h + len(kind))
    feat = (np.maximum(rng.standard_normal((c, h, w)) * 2 + 0.5, 0) * big).astype(np.float32)
    f64 = feat.reshape(c, -1).astype(np.float64)
    g = np.tril(f64 @ f64.T / f64.size)
    target = (g * np.tril(rng.uniform(0.5, 1.5, (c, c)))).astype(np.float32)
    # the window sits inside a larger map, behind a roll that wraps on both axes
    mh, mw, roll = h + 6, w + 9, (ROLL[0], -(h + 2))
    m = _window_mask(kind, h, w)
    rolled = rng.uniform(0, 1, (mh, mw)).astype(np.float32)
    rolled[OY:OY + h, OX:OX + w] = m
    full = np.roll(rolled, (-roll[0], -roll[1]), axis=(-1, -2))
    half_ref, s_ref, asum_ref, a_ref = masked_style_terms(feat, m, target)
    d_feat, d_map, d_tgt = eng.to_device(feat), eng.to_device(full), eng.to_device(target)
    s, (half, asum, a) = _op_call(eng, d_feat, c, h, w, d_map, mh, mw, roll, d_tgt)
    assert np.all(np.isfinite(s)) and np.isfinite(half) and np.isfinite(asum)
    if kind == 'zeros':
        assert half == 0 and asum == 0 and a == 0 and not s.any()
    else:
        with fp32_kernels():
            s32, _ = _op_call(eng, d_feat, c, h, w, d_map, mh, mw, roll, d_tgt)
        scale = np.abs(s_ref).max()
        err, err32 = float(np.abs(s - s_ref).max() / scale), float(np.abs(s32 - s_ref).max() / scale)
        print('C %d %dx%d %s x%g: S %.2e (fp32 kernels %.2e), loss %.2e, sum|S| %.2e, a %.2e'
              % (c, h, w, kind, big, err, err32, abs(half / half_ref - 1), abs(asum / asum_ref - 1),
                 abs(a / a_ref - 1)))
        assert err <= 2e-5
        assert err <= 3 * err32 + 1e-7, (err, err32)
        assert half == pytest.approx(half_ref, rel=2e-5)
        assert asum == pytest.approx(asum_ref, rel=2e-5)
        assert a == pytest.approx(a_ref, rel=1e-6)
    if kind == 'ones':
        # the Gram and D see identical inputs (F * 1, 1 * Gs): the unmasked hook's loss, bit for bit
        plain = ctypes.c_double()
        lib.call('stx_op_style_terms', eng.handle, d_feat.ptr, c, h, w, d_tgt.ptr, None, None,
                 ctypes.byref(plain), None)
        assert a == 1.0 and half == plain.value
    for arr in (d_feat, d_map, d_tgt):
        arr.free()


# --------------------------------------------------------------------------------- the tile path
CL, CW = ['conv3_2'], {'conv3_2': 0.05}
SL = ['conv1_1', 'conv2_1', 'conv3_1']
SW = {l: 1 / 3 for l in SL}
LW = {'conv2_1': 1.5}
FRAME = (128, 128)


def _smooth_mask(hw, seed=0):
    y, x = np.mgrid[:hw[0], :hw[1]]
    return np.float32(0.5 + 0.5 * np.sin(0.09 * x + 0.05 * y + seed) * np.cos(0.04 * y - 0.02 * x))


@functools.lru_cache(maxsize=None)
def _scene(n_styles):
    """Oracle with targets of a 128 x 128 frame, computed once: n_styles styles with complementary smooth
    masks (one style: a single smooth mask)."""
    net = builtin_net('vgg19')
    mom = MaskedOracleModel(net.as_dicts(), synthetic_weights(net.as_dicts(), 0))
    rng = np.random.RandomState(11)
    full = rng.uniform(-110, 120, (3,) + FRAME).astype(np.float32)
    styles = [rng.uniform(-110, 120, (3, 40, 44)).astype(np.float32) for _ in range(n_styles)]
    mom.styles = [mom.style_grams([s], SL, 512) for s in styles]
    mom.contents = [mom.prepare_features(full, CL, 512)]
    m0 = _smooth_mask(FRAME)
    masks = [m0, 1 - m0][:n_styles]
    mom.set_masks(masks, SL)
    return mom, full, masks


def _arm(eng, mom, masks):
    eng.set_contents_and_styles(mom.contents, mom.styles)
    eng.set_style_masks(masks)


def check_masked_tile(eng, mom, tile, start, roll):
    """tests/gpu_helpers.check_tile with the masked oracle: the loss to TIGHT against the float64 formula,
    the gradient to TIGHT of max against the oracle's backward pass on the GPU's own activations, and
    against the oracle's end-to-end gradient on decision-clean pixels."""
    loss, grad = eng.sc_grad_tile(tile, start, roll, CL, SL, LW, CW, SW)
    deepest = mom.deep_to_shallow(CL + SL)[0]
    blobs = mom.blob_names[:mom.blob_names.index(deepest) + 1]
    acts = eng.features_tile(tile, blobs)
    mom.roll_contents(roll)
    try:
        ref_loss, oracle_grad = mom.sc_grad_tile(tile, start, CL, SL, LW, CW, SW)
        ref_acts = {b: mom.net.blobs[b].data[0].copy() for b in blobs}
        same_loss, same_grad = mom.sc_grad_tile(tile, start, CL, SL, LW, CW, SW, activations=acts)
        loss64 = mom.masked_loss64(ref_acts, start, CL, SL, LW, CW, SW)
    finally:
        mom.roll_contents(-np.asarray(roll))
    taint, n_relu, n_pool = decision_taint(mom.net.layers, acts, ref_acts, deepest, {'data': tile.shape})
    clean = ~taint
    scale = np.abs(oracle_grad).max()
    stats = dict(loss=abs(loss / loss64 - 1), same=max_rel(grad, same_grad), l2=l2_rel(grad, oracle_grad),
                 clean=float(np.abs(np.float64(grad) - oracle_grad)[:, clean].max() / scale) if clean.any() else 0.0,
                 flips=(n_relu, n_pool))
    print('masked tile', tile.shape, start, roll, stats)
    assert np.all(np.isfinite(grad))
    assert loss == pytest.approx(loss64, rel=TIGHT), (loss, loss64, ref_loss, same_loss)
    assert stats['same'] < TIGHT, stats
    assert stats['clean'] < TIGHT, stats
    assert stats['l2'] < FLIP_L2, stats
    return loss, grad


def _tile(full, th, tw, start, roll):
    rolled = np.roll(full, (roll[0], roll[1]), axis=(-1, -2))
    return np.ascontiguousarray(rolled[:, start[0]:start[0] + th, start[1]:start[1] + tw])


@pytest.mark.parametrize('n_styles,th,tw,start,roll', [(2, 64, 48, (0, 0), (0, 0)),
                                                       (2, 37, 53, (64, 32), (-24, 40)),
                                                       (1, 64, 48, (0, 0), (0, 0))])
def test_masked_tile_against_the_oracle(n_styles, th, tw, start, roll):
    """Two styles: stand-alone injection; one masked style: the fused epilogue (tap_fusable)."""
    mom, full, masks = _scene(n_styles)
    eng = gpu_engine()
    _arm(eng, mom, masks)
    check_masked_tile(eng, mom, _tile(full, th, tw, start, roll), start, roll)
    eng.set_style_masks([])


@pytest.mark.parametrize('n_styles', [2, 1])
def test_masked_tile_is_bit_identical_across_schedules_and_runs(n_styles, monkeypatch):
    mom, full, masks = _scene(n_styles)
    eng = gpu_engine()
    _arm(eng, mom, masks)
    tile = _tile(full, 64, 48, (0, 0), (0, 0))
    run = lambda: eng.sc_grad_tile(tile, (0, 0), (0, 0), CL, SL, LW, CW, SW)
    first, again = run(), run()
    assert first[0] == again[0] and np.array_equal(first[1], again[1])          # deterministic
    for name, value in (('STX_SUMS_LATE', '0'), ('STX_TERMS_LATE', '1')):
        monkeypatch.setenv(name, value)
        lib.reread_env()
        other = run()
        monkeypatch.delenv(name)
        lib.reread_env()
        assert other[0] == first[0] and np.array_equal(other[1], first[1]), name
    eng.set_style_masks([])


def test_no_masks_changes_no_bit_and_targets_clear_masks():
    from style_transfer_amd.engine import TileEngine
    from tests.gpu_helpers import require_gpu
    require_gpu()
    mom, full, masks = _scene(2)
    net = builtin_net('vgg19')
    eng = TileEngine(net, 0, synthetic_weights(net.as_dicts(), 0))       # no mask was ever set on this one
    tile = _tile(full, 64, 48, (0, 0), (0, 0))
    run = lambda: eng.sc_grad_tile(tile, (0, 0), (0, 0), CL, SL, LW, CW, SW)
    eng.set_contents_and_styles(mom.contents, mom.styles)
    before = run()
    eng.set_style_masks(masks)
    masked = run()
    assert masked[0] != before[0] and not np.array_equal(masked[1], before[1])
    eng.set_style_masks([])
    cleared = run()
    assert cleared[0] == before[0] and np.array_equal(cleared[1], before[1])
    eng.set_style_masks(masks)
    eng.set_contents_and_styles(mom.contents, mom.styles)                # clears the masks
    fresh = run()
    assert fresh[0] == before[0] and np.array_equal(fresh[1], before[1])
    # a mask of another frame surfaces as the window range error
    eng.set_style_masks([masks[0][:40, :40], None])
    with pytest.raises(lib.StxError, match='mask'):
        run()
    with pytest.raises(lib.StxError):
        eng.set_style_masks([None, None, masks[0]])                      # no style 2
    eng.close()


# -------------------------------------------------------------------------------------- the farm
def test_farm_with_masks_against_the_oracle():
    """A 96 x 80 image in 2 x 2 tiles of 48 x 40, two masked styles, a non-zero roll."""
    from style_transfer_amd.farm import TileFarm
    from tests.gpu_helpers import require_gpu
    require_gpu()
    net = builtin_net('vgg19')
    weights = synthetic_weights(net.as_dicts(), 0)
    mom = MaskedOracleModel(net.as_dicts(), weights)
    rng = np.random.RandomState(21)
    H, W, roll = 96, 80, (8, -16)
    img = rng.uniform(-110, 120, (3, H, W)).astype(np.float32)
    styles = [rng.uniform(-110, 120, (3, 40, 44)).astype(np.float32) for _ in range(2)]
    mom.styles = [mom.style_grams([s], SL, 512) for s in styles]
    mom.contents = [mom.prepare_features(img, CL, 512)]
    m0 = _smooth_mask((H, W), 1)
    masks = [m0, 1 - m0]
    mom.set_masks(masks, SL)
    farm = TileFarm(net, [0], weights, verbose=False)
    farm.set_contents_and_styles(mom.contents, mom.styles)
    farm.set_style_masks(masks)
    d_img, d_grad = farm.master.to_device(img), farm.master.empty(img.shape)
    loss = farm.eval_sc_grad(d_img, d_grad, roll, CL, SL, LW, CW, SW, 64)
    grad = np.roll(d_grad.get(), (roll[0], roll[1]), axis=(-1, -2))           # into the rolled frame
    rolled = np.roll(img, (roll[0], roll[1]), axis=(-1, -2))
    ref_loss, ref_grad = mom.sc_grad(rolled, roll, 64, CL, SL, LW, CW, SW)
    # decision-clean pixels, tile by tile
    from oracle.tile_path import tile_grid
    deepest = mom.deep_to_shallow(CL + SL)[0]
    blobs = mom.blob_names[:mom.blob_names.index(deepest) + 1]
    clean = np.zeros((H, W), bool)
    for (y0, y1, x0, x1) in tile_grid((H, W), 64):
        tile = np.ascontiguousarray(rolled[:, y0:y1, x0:x1])
        acts, ref_acts = farm.master.features_tile(tile, blobs), mom.features_tile(tile, blobs)
        taint, _, _ = decision_taint(mom.net.layers, acts, ref_acts, deepest, {'data': tile.shape})
        clean[y0:y1, x0:x1] = ~taint
    err = float(np.abs(np.float64(grad) - ref_grad)[:, clean].max() / np.abs(ref_grad).max())
    print('farm: loss %.2e, clean %.2e (%.0f%% clean), l2 %.2e'
          % (abs(loss / ref_loss - 1), err, 100 * clean.mean(), l2_rel(grad, ref_grad)))
    assert farm.tile_evals == 4
    assert loss == pytest.approx(ref_loss, rel=TIGHT)
    assert clean.any() and err < TIGHT
    assert l2_rel(grad, ref_grad) < FLIP_L2
    farm.close()


# ------------------------------------------------------------------------------ the command line
def _cli_run(tmp_path, monkeypatch, capsys, name, styles, extra):
    import csv
    import glob
    from style_transfer_amd import cli
    where = tmp_path / name
    where.mkdir()
    monkeypatch.chdir(where)
    argv = ['-ci', '../c.png', '-si'] + styles + ['--size', '64', '--min-size', '64', '-i', '3', '--tile-size', '64',
                                                  '--model', 'vgg19', '--weights', 'synthetic:0', '--devices', '0',
                                                  '-oi', 'out.png'] + extra
    assert cli.main(argv) == 0
    capsys.readouterr()
    final = Image.open(where / 'out.png')
    logs = glob.glob(str(where / '*_log.csv'))
    assert len(logs) == 1
    with open(logs[0], newline='') as f:
        losses = [float(row['loss']) for row in csv.DictReader(f)]
    return np.asarray(final.convert('RGB')), final.text['Comment'], losses


def test_cli_style_masks(tmp_path, monkeypatch, capsys):
    rng = np.random.RandomState(4)
    picture = lambda hw: Image.fromarray(np.uint8(rng.uniform(0, 255, hw + (3,))))
    picture((64, 56)).save(tmp_path / 'c.png')
    picture((48, 52)).save(tmp_path / 's1.png')
    picture((50, 44)).save(tmp_path / 's2.png')
    ramp = np.uint8(255 * _smooth_mask((64, 56)))
    Image.fromarray(ramp).save(tmp_path / 'a.png')
    Image.fromarray(255 - ramp).save(tmp_path / 'b.png')
    Image.fromarray(np.full((64, 56), 255, np.uint8)).save(tmp_path / 'white.png')
    two = ['../s1.png', '../s2.png']
    ab = _cli_run(tmp_path, monkeypatch, capsys, 'ab', two, ['--style-masks', '../a.png', '../b.png'])
    ba = _cli_run(tmp_path, monkeypatch, capsys, 'ba', two, ['--style-masks', '../b.png', '../a.png'])
    assert ab[0].shape == (64, 56, 3) and len(ab[2]) == 3 and np.all(np.isfinite(ab[2]))
    assert re.search(r"style_masks=\['\.\./a\.png', '\.\./b\.png'\]", ab[1])
    assert not np.array_equal(ab[0], ba[0]) and ab[2] != ba[2]            # which style goes where matters
    # one style under an all-white mask is the run without the flag
    bare = _cli_run(tmp_path, monkeypatch, capsys, 'bare', ['../s1.png'], [])
    white = _cli_run(tmp_path, monkeypatch, capsys, 'white', ['../s1.png'], ['--style-masks', '../white.png'])
    assert 'style_masks' not in bare[1] and 'style_masks' in white[1]
    assert white[2] == pytest.approx(bare[2], rel=TIGHT)
