"""The temporal-consistency term on the GPU (stx_image_flow_warp, stx_image_temporal) against the float64 numpy
statement of tests/temporal_ref.py -- there is no reference implementation of this term --, its exact
properties, the wiring through StyleTransfer and the command line.

Bounds (none of them comes from what the kernels give):
  * warp, weight: equal to the reference on every decision-clear pixel.  A pixel is unclear when a threshold's
    two sides differ by at most 1e-9 (1 + right side) or q lies within 1e-9 of the frame's edge; at most 0.1 %
    of the pixels may be unclear, which is asserted on the reference before the GPU result is looked at;
  * warp, target: where both weights are 1, |T - T_ref| <= 2^-23 max|tap| -- one rounding to float32 of a
    float64 value (2^-24 of it) and float64 noise; elsewhere both are exactly 0;
  * term: loss to 2e-5 relative, gradient to 2e-5 of max|grad_ref| -- the bounds tests/test_gpu_lap.py states
    for this kind of kernel (fp32 per element, a double finish)."""

import ctypes
import functools

import numpy as np
import pytest
from PIL import Image

from style_transfer_amd import image_ops, lib
from style_transfer_amd.flow import FLO_UNKNOWN, write_flo
from tests import temporal_ref
from tests.gpu_helpers import gpu_engine
from tests.test_gpu_lap import _pictures, noise

pytestmark = pytest.mark.gpu
WARP_SIZES = [(37, 53), (64, 64), (130, 67), (257, 190)]
WARP_CASES = ['forward', 'backward only', 'forward scaled', 'backward only scaled', 'three frames', 'unknown block']
SHIFTS = [(2.3, -1.7), (-3.1, 2.2), (0.6, 4.4)]


@functools.lru_cache(maxsize=None)
def _warp_case(hw, case):
    """(frames [(prev, flow_b, flow_f)], su, sv, the reference's composite) of one case, made once."""
    H, W = hw
    count = 3 if case == 'three frames' else 1
    frames = []
    for k in range(count):
        back, fwd = temporal_ref.affine_flows(hw, shift=SHIFTS[k], angle=0.03 * (1 + k))
        if case == 'unknown block':
            back[:, H // 3:H // 3 + 6, W // 2:W // 2 + 9] = FLO_UNKNOWN
            back[0, 2, 3], back[1, H - 1, W - 2] = np.nan, -np.inf
            fwd[:, 2 * H // 3:2 * H // 3 + 5, W // 4:W // 4 + 7] = FLO_UNKNOWN
            fwd[1, H // 2, W // 2] = np.nan
        frames.append((temporal_ref.noise_picture(hw, 40 + k), back, None if 'backward only' in case else fwd))
    su, sv = (0.5, 0.75) if 'scaled' in case else (1.0, 1.0)
    for arrays in frames:
        for arr in arrays:
            if arr is not None:
                arr.setflags(write=False)
    return frames, su, sv, temporal_ref.composite(frames, su, sv)


def _run_warp(eng, frames, su, sv, start=None):
    """The frames through image_ops.flow_warp, closest first: (target, weight) as host arrays.  ``start``: host
    accumulators to go on from (then no call has ``first`` set)."""
    H, W = frames[0][0].shape[1:]
    if start is None:
        # (stale values: with ``first`` the accumulators count as zero whatever they hold)
        d_target, d_weight = eng.to_device(np.full((3, H, W), 7.0, np.float32)), eng.to_device(np.full((H, W), 0.5, np.float32))
    else:
        d_target, d_weight = eng.to_device(np.float32(start[0])), eng.to_device(np.float32(start[1]))
    for k, (prev, back, fwd) in enumerate(frames):
        arrays = [eng.to_device(prev), eng.to_device(back), eng.to_device(fwd) if fwd is not None else None]
        image_ops.flow_warp(eng, arrays[0], arrays[1], arrays[2], su, sv, start is None and k == 0, d_target, d_weight)
        eng.sync()
        for arr in arrays:
            if arr is not None:
                arr.free()
    out = d_target.get(), d_weight.get()
    d_target.free()
    d_weight.free()
    return out


def _check_composite(got, want, label):
    (got_t, got_w), (want_t, want_w, unclear, tapmax) = got, want
    clear = ~unclear
    print('%s: reference holds %.3f of the pixels, %d unclear; weights differ on %d pixel(s), %d of them clear'
          % (label, want_w.mean(), unclear.sum(), (got_w != want_w).sum(), ((got_w != want_w) & clear).sum()))
    assert set(np.unique(got_w)) <= {0.0, 1.0}
    assert np.array_equal(got_w[clear], want_w[clear])
    both = (got_w == 1) & (want_w == 1)
    err = np.abs(np.float64(got_t) - want_t)
    # (tapmax is 0 on pixels that prefilled accumulators held: those must be kept exactly)
    sampled = both[None] & (tapmax > 0)
    print('%s: worst target error / (2^-23 max|tap|) = %.3g'
          % (label, (err[sampled] / (2.0 ** -23 * tapmax[sampled])).max() if sampled.any() else 0.0))
    assert np.all(err[:, both] <= 2.0 ** -23 * tapmax[:, both])
    assert not got_t[:, got_w == 0].any() and not want_t[:, want_w == 0].any()


@pytest.mark.parametrize('case', WARP_CASES)
@pytest.mark.parametrize('hw', WARP_SIZES)
def test_warp_against_float64(hw, case):
    frames, su, sv, want = _warp_case(hw, case)
    # ---- the reference alone: the case decides clearly, and both outcomes occur
    assert want[2].mean() <= 1e-3
    assert 0.02 <= want[1].mean() <= 0.98
    eng = gpu_engine()
    got = _run_warp(eng, frames, su, sv)
    _check_composite(got, want, '%s %s' % (hw, case))
    again = _run_warp(eng, frames, su, sv)
    assert again[0].tobytes() == got[0].tobytes() and again[1].tobytes() == got[1].tobytes()
    for prev, back, fwd in frames:              # (the inputs are only read: the cached arrays are read-only hosts)
        assert not prev.flags.writeable


def test_three_frames_fill_what_the_first_leaves():
    """First-wins does something in the three-frame case: later frames add pixels, and never take one over."""
    hw = (130, 67)
    frames, su, sv, want = _warp_case(hw, 'three frames')
    first = temporal_ref.composite(frames[:1], su, sv)
    assert want[1].sum() > first[1].sum() + 100
    held = first[1] == 1
    assert np.array_equal(want[0][:, held], first[0][:, held])


@pytest.mark.parametrize('hw', WARP_SIZES)
def test_warp_goes_on_from_prefilled_accumulators(hw):
    """first = 0: a pixel whose weight is set keeps its target and weight, bit for bit; the others are taken
    where the frame is reliable and stay as they are where it is not."""
    frames, su, sv, _ = _warp_case(hw, 'forward')
    rng = np.random.RandomState(hw[0])
    weight0 = np.float32(rng.uniform(0, 1, hw) < 0.4)
    target0 = temporal_ref.noise_picture(hw, 77) * weight0[None]
    want = temporal_ref.composite(frames, su, sv, start=(target0, weight0))
    assert want[2].mean() <= 1e-3
    assert (want[1] > weight0).sum() > 50 and (want[1] == 0).sum() > 50
    eng = gpu_engine()
    got = _run_warp(eng, frames, su, sv, start=(target0, weight0))
    _check_composite(got, want, '%s prefilled' % (hw,))
    held = weight0 == 1
    assert got[0][:, held].tobytes() == target0[:, held].tobytes() and np.all(got[1][held] == 1)


# ------------------------------------------------------------------------------------------ the term
TERM_SIZES = [(37, 53), (130, 67), (724, 724), (2048, 2048)]       # (the last: past one grid of workgroups)
TERM_CASES = [(hw, kind) for hw in TERM_SIZES for kind in ('binary', 'uniform')] + [((37, 53), 'wild'),
                                                                                      ((724, 724), 'wild')]


def _weight(hw, kind, seed):
    rng = np.random.RandomState(seed)
    if kind == 'binary':
        return np.float32(rng.uniform(0, 1, hw) < 0.7)
    if kind == 'uniform':
        return rng.uniform(0, 1, hw).astype(np.float32)
    weight = rng.uniform(-0.5, 1.5, hw).astype(np.float32)         # below 0, above 1 ...
    weight[rng.uniform(0, 1, hw) < 0.05] = np.nan                  # ... and NaN
    weight[0, 0], weight[-1, -1], weight[1, 2] = -3.0, 2.5, np.nan
    return weight


@functools.lru_cache(maxsize=None)
def _term_case(hw, kind):
    img, target = noise(hw, hw[0] + hw[1])
    weight = _weight(hw, kind, hw[1])
    g0 = np.random.RandomState(6).standard_normal(img.shape).astype(np.float32)
    loss, grad = temporal_ref.temporal_loss(img, target, weight, 3.5)
    return img, target, weight, g0, loss, np.float64(g0) + grad, np.abs(grad).max()


def _run_term(eng, img, target, weight, g0, scale):
    arrays = [eng.to_device(a) for a in (img, g0, target, weight)]
    loss = image_ops.temporal_loss(eng, arrays[0], arrays[1], arrays[2], arrays[3], scale)
    eng.sync()
    got = arrays[1].get()
    assert np.array_equal(arrays[0].get(), img) and arrays[2].get().tobytes() == target.tobytes()
    assert arrays[3].get().tobytes() == weight.tobytes()         # the inputs are only read
    for arr in arrays:
        arr.free()
    return loss.value, got


@pytest.mark.parametrize('hw,kind', TERM_CASES)
def test_term_against_float64(hw, kind):
    img, target, weight, g0, want_loss, want_grad, top = _term_case(hw, kind)
    eng = gpu_engine()
    loss, got = _run_term(eng, img, target, weight, g0, 3.5)
    loss_err = abs(loss - want_loss) / want_loss
    grad_err = np.abs(np.float64(got) - want_grad).max() / top
    print('%s %s: loss error %.3g relative, gradient error %.3g of max|grad_ref|' % (hw, kind, loss_err, grad_err))
    assert want_loss > 0 and top > 0
    assert loss_err <= 2e-5
    assert grad_err <= 2e-5
    off = ~(temporal_ref.clip_weight(weight) > 0)
    assert off.any() == (kind != 'uniform')
    assert got[:, off].tobytes() == g0[:, off].tobytes()                    # where w' = 0 the gradient is not touched
    loss2, again = _run_term(eng, img, target, weight, g0, 3.5)
    assert again.tobytes() == got.tobytes() and np.float64(loss2).tobytes() == np.float64(loss).tobytes()


@pytest.mark.parametrize('hw', [(37, 53), (724, 724)])        # (the one-pixel and the four-pixel path)
def test_term_exact_properties(hw):
    eng = gpu_engine()
    img, other = noise(hw, 9)
    g0 = np.random.RandomState(10).standard_normal(img.shape).astype(np.float32)
    g0[:, 3, 4:9] = -0.0
    g0[1, 5, 6] = 0.0
    uniform = _weight(hw, 'uniform', 3)
    # img == target everywhere
    loss, got = _run_term(eng, img, img.copy(), uniform, g0, 7.0)
    assert loss == 0.0 and got.tobytes() == g0.tobytes()
    # img == target wherever w' > 0, anything elsewhere
    wild = _weight(hw, 'wild', 4)
    on = temporal_ref.clip_weight(wild) > 0
    target = np.where(on[None], img, other)
    assert on.any() and (~on).any() and np.any(target != img)
    loss, got = _run_term(eng, img, target, wild, g0, 7.0)
    assert loss == 0.0 and got.tobytes() == g0.tobytes()
    # a weight of all zeros
    loss, got = _run_term(eng, img, other, np.zeros(hw, np.float32), g0, 7.0)
    assert loss == 0.0 and got.tobytes() == g0.tobytes()
    # at weight 1 the gradient is the auxiliary-image term's, bit for bit (the same float32 expression)
    d_img, d_aux = eng.to_device(img), eng.to_device(other)
    d_a, d_b, d_one = eng.to_device(g0), eng.to_device(g0), eng.to_device(np.ones(hw, np.float32))
    image_ops.regularizers(eng, d_img, d_a, np.zeros(3, np.float32), 0.0, 2.0, 0.0, 6.0, aux=d_aux, aux_scale=7.0)
    image_ops.temporal_loss(eng, d_img, d_b, d_aux, d_one, 7.0)
    eng.sync()
    assert d_a.get().tobytes() == d_b.get().tobytes()
    for arr in (d_img, d_aux, d_a, d_b, d_one):
        arr.free()


def test_argument_errors():
    eng = gpu_engine()
    hw = (16, 16)
    img, other = noise(hw, 1)
    d_img, d_prev, d_grad, d_target = eng.to_device(img), eng.to_device(other), eng.empty(img.shape).zero(), eng.empty(img.shape).zero()
    d_flow, d_weight = eng.empty((2,) + hw).zero(), eng.empty(hw).zero()
    out = ctypes.c_double(0)
    message = lambda: lib.load().stx_last_error().decode()

    def warp(prev=d_prev.ptr, flow_b=d_flow.ptr, flow_f=d_flow.ptr, H=16, W=16, su=1.0, sv=1.0, target=d_target.ptr,
             weight=d_weight.ptr):
        return lib.load().stx_image_flow_warp(eng.handle, prev, flow_b, flow_f, H, W, su, sv, 1, target, weight)

    def term(img=d_img.ptr, grad=d_grad.ptr, target=d_target.ptr, weight=d_weight.ptr, H=16, W=16, loss=ctypes.byref(out)):
        return lib.load().stx_image_temporal(eng.handle, img, grad, target, weight, H, W, 1.0, loss)
    for null in ('prev', 'flow_b', 'target', 'weight'):
        assert warp(**{null: None}) == -1 and 'null' in message() and null in message()
    assert warp(H=1) == -1 and '1 x 16' in message()
    assert warp(W=1) == -1 and '16 x 1' in message()
    assert warp(H=0) == -1 and warp(W=-4) == -1
    for bad in (float('nan'), float('inf')):
        assert warp(su=bad) == -1 and 'finite' in message()
        assert warp(sv=bad) == -1 and 'finite' in message()
    for null in ('img', 'grad', 'target', 'weight', 'loss'):
        assert term(**{null: None}) == -1 and 'null' in message()
    assert term(H=0) == -1 and term(W=-1) == -1
    with pytest.raises(ValueError, match='flow_b'):
        image_ops.flow_warp(eng, d_prev, d_weight, None, 1, 1, True, d_target, d_weight)
    with pytest.raises(ValueError, match='weight'):
        image_ops.temporal_loss(eng, d_img, d_grad, d_target, d_flow, 1.0)
    eng.sync()
    assert not d_grad.get().any() and not d_target.get().any()        # nothing ran
    assert warp(flow_f=None) == 0 and warp() == 0 and term() == 0     # (the same calls with good arguments do)
    eng.sync()
    assert np.array_equal(d_target.get(), other) and d_weight.get().all()     # (a zero flow holds everything)
    for arr in (d_img, d_prev, d_grad, d_target, d_flow, d_weight):
        arr.free()


# ------------------------------------------------------------------------------------ command line
def _cli_run(tmp_path, monkeypatch, capsys, name, extra, init=True):
    """The recipe of tests/test_gpu_lap.py (--size 80, two scales, synthetic weights), with or without its
    --init-image: (final RGB, its PNG comment, the --save-every pictures by file suffix)."""
    import glob
    import re
    from style_transfer_amd import cli
    where = tmp_path / name
    where.mkdir()
    monkeypatch.chdir(where)
    argv = ['-ci', '../c.png', '-si', '../s.png'] + (['-ii', '../c.png'] if init else []) + [
        '--size', '80', '--min-size', '57', '-i', '2', '2', '--tile-size', '64', '--save-every', '2', '--model',
        'vgg19', '--weights', 'synthetic:0', '--devices', '0', '-oi', 'out.png'] + extra
    assert cli.main(argv) == 0
    capsys.readouterr()
    final = Image.open(where / 'out.png')
    saved = {re.search(r'_out_(\d+)\.png$', p).group(1): np.asarray(Image.open(p).convert('RGB'))
             for p in sorted(glob.glob(str(where / '*_out_*.png')))}
    return np.asarray(final.convert('RGB')), final.text['Comment'], saved


def test_cli_temporal_weight(tmp_path, monkeypatch, capsys):
    from style_transfer_amd.config_system import parse_args
    content, style = _pictures((64, 80), (70, 60), 8)
    earlier, _ = _pictures((64, 80), (8, 8), 31)
    content.save(tmp_path / 'c.png')
    style.save(tmp_path / 's.png')
    earlier.save(tmp_path / 'p.png')
    zero = np.zeros((2, 64, 80), np.float32)
    write_flo(tmp_path / 'zero.flo', zero)
    write_flo(tmp_path / 'turned.flo', np.zeros((2, 80, 64), np.float32))
    on = ['--temporal-weight', '1000', '--prev-images', '../p.png', '--flows', '../zero.flo']
    # ---- what every flow_warp call is handed and leaves
    warps = []
    real_warp = image_ops.flow_warp

    def wrapped_warp(engine, prev, flow_b, flow_f, su, sv, first, target, weight):
        real_warp(engine, prev, flow_b, flow_f, su, sv, first, target, weight)
        engine.sync()
        warps.append(dict(prev=prev.get(), flow_b=flow_b.get(), flow_f=flow_f, su=su, sv=sv, first=first,
                          target=target.get(), weight=weight.get()))
    monkeypatch.setattr(image_ops, 'flow_warp', wrapped_warp)
    bare = _cli_run(tmp_path, monkeypatch, capsys, 'bare', [])
    assert not warps
    held = _cli_run(tmp_path, monkeypatch, capsys, 'held', on)
    # ---- the term pulls the result to the earlier picture
    p = np.float64(np.asarray(earlier))
    far, near = np.abs(bare[0] - p).mean(), np.abs(held[0] - p).mean()
    print('mean |RGB - earlier picture|: %.3f without the term, %.3f with it' % (far, near))
    assert bare[0].shape == held[0].shape == (64, 80, 3)
    assert near < far
    assert 'temporal' not in bare[1] and 'prev_images' not in bare[1] and 'flows' not in bare[1]
    for text in ('temporal_weight=1000.0', "prev_images=['../p.png']", "flows=['../zero.flo']"):
        assert text in held[1]
    assert 'flows_fwd' not in held[1] and 'temporal_init' not in held[1]
    # ---- one composite per scale, equal to the reference's preparation
    mean = np.float32(parse_args(None, ['-ci', 'c', '-si', 's'], config_py=False).mean).reshape((3, 1, 1))
    to_image = lambda picture: np.ascontiguousarray(np.float32(picture).transpose((2, 0, 1))[::-1] - mean)
    assert [w['weight'].shape for w in warps] == [(46, 57), (64, 80)]
    for call in warps:
        h, w = call['weight'].shape
        assert call['first'] and call['flow_f'] is None and (call['su'], call['sv']) == (w / 80, h / 64)
        assert np.array_equal(call['prev'], to_image(earlier.resize((w, h), Image.LANCZOS)))
        assert call['flow_b'].shape == (2, h, w) and not call['flow_b'].any()
        want = temporal_ref.prepare_scale([earlier], [zero], None, (h, w), to_image)
        # (zero flows: q = (x, y) exactly on both sides, so no decision is open although the border pixels lie on
        # the frame's edge -- every weight is compared)
        assert np.array_equal(call['weight'], want[1]) and want[1].all()
        _check_composite((call['target'], call['weight']), (want[0], want[1], np.zeros((h, w), bool), want[3]),
                         'scale %d x %d' % (w, h))
    # ---- --temporal-init: the run starts from the composite instead of noise
    del warps[:]
    noise_start = _cli_run(tmp_path, monkeypatch, capsys, 'noise', on, init=False)
    warm_start = _cli_run(tmp_path, monkeypatch, capsys, 'warm', on + ['--temporal-init'], init=False)
    assert 'temporal_init=True' in warm_start[1] and 'temporal_init' not in noise_start[1]
    assert sorted(noise_start[2]) == sorted(warm_start[2]) == ['0002', '0004']
    assert not np.array_equal(noise_start[2]['0002'], warm_start[2]['0002'])
    first_far = np.abs(noise_start[2]['0002'] - np.float64(np.asarray(earlier.resize((57, 46), Image.LANCZOS)))).mean()
    first_near = np.abs(warm_start[2]['0002'] - np.float64(np.asarray(earlier.resize((57, 46), Image.LANCZOS)))).mean()
    print('first saved picture, mean |RGB - earlier picture|: %.3f from noise, %.3f from the composite' % (first_far, first_near))
    assert first_near < first_far
    assert [w['weight'].shape for w in warps] == [(46, 57), (64, 80)] * 2     # still one composite per scale
    # ---- a flow of the wrong size is refused with the file's name
    from style_transfer_amd import cli
    monkeypatch.chdir(tmp_path / 'bare')
    with pytest.raises(ValueError) as err:
        cli.main(['-ci', '../c.png', '-si', '../s.png', '--size', '80', '--model', 'vgg19', '--weights', 'synthetic:0',
                  '--devices', '0', '--temporal-weight', '1', '--prev-images', '../p.png', '--flows', '../turned.flo'])
    capsys.readouterr()
    assert 'turned.flo' in str(err.value)
