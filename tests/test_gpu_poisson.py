"""The screened-Poisson output stage on the GPU (stx_image_poisson, csrc/poisson.hip) against the float64 numpy
statement of tests/poisson_ref.py -- there is no reference implementation of this stage; tests/test_poisson_host.py
holds that statement to an exact direct solve --, its exact properties, every refusal, and --poisson-lambda through
the command lines.

The bound: the output is the float32 of a float64 computation that the device carries out in the order the
reference does, with every operation rounded once (double division is correctly rounded without fast-math).  So the
float64 values agree bit for bit, and the bound leaves room for nothing but the final rounding:
    |out - float32(ref)| <= 2^-23 max(1, |ref|).
It comes from the number formats, not from what the kernels give; every value is expected to EQUAL the reference,
and the count that differs is printed before anything is asserted."""

import functools
import glob
import re

import numpy as np
import pytest
from PIL import Image

from style_transfer_amd import image_ops, lib, poisson
from tests import poisson_ref as ref
from tests.gpu_helpers import gpu_engine

pytestmark = pytest.mark.gpu
MEAN = np.float32((103.939, 116.779, 123.68)).reshape(3, 1, 1)

# (H, W).  1 x 1: no neighbour at all; 2 x 2, 3 x 5: every pixel on an edge, one and two levels; 16 x 16: even sizes
# all the way down; 33 x 31, 37 x 53, 130 x 67, 257 x 190: odd sizes at some level in both directions (coarse cells of
# 1 and 2 children, colours that start differently from row to row), ragged blocks (64 x 4 pixels, 128 x 4 in a
# half-sweep) and several blocks each way.  No kernel is a grid-stride loop under a capped grid: a thread owns one
# pixel at every size, which the 724 x 733 case (1.6 million pixels, past every cap the library has) checks.
SHAPES = [(1, 1), (2, 2), (3, 5), (16, 16), (33, 31), (37, 53), (130, 67), (257, 190)]
DEFAULT = ref.POISSON_CYCLES_DEFAULT
CASES = ([(hw, lam, DEFAULT) for hw in SHAPES for lam in (0.5, 5.0, 500.0)] +
         [(hw, 0.04, DEFAULT) for hw in SHAPES] +         # one level: 20 sweeps a cycle and nothing else
         [(hw, 5.0, 1) for hw in SHAPES] +
         [((724, 733), 5.0, 2)])


@functools.lru_cache(maxsize=None)
def _pictures(hw):
    """(s, c) [3, H, W] in the frame the pipeline keeps its pictures in (BGR minus mean: both signs)."""
    s, c = ref.case(*hw, channels=3)
    s, c = s - MEAN, c - MEAN
    for arr in (s, c):
        arr.setflags(write=False)
    return s, c


@functools.lru_cache(maxsize=None)
def _reference(hw, lam, cycles):
    """The reference's output of one case, computed once and left alone."""
    out = ref.solve(*_pictures(hw), lam, cycles)
    out.setflags(write=False)
    return out


def _run(eng, s, c, lam, cycles):
    d_s, d_c = eng.to_device(s), eng.to_device(c)
    out = image_ops.poisson(eng, d_s, d_c, lam, cycles)
    eng.sync()
    got = out.get()
    assert d_s.get().tobytes() == s.tobytes() and d_c.get().tobytes() == c.tobytes()     # the inputs are only read
    for arr in (d_s, d_c, out):
        arr.free()
    return got


def _check(got, want, label):
    err = np.abs(np.float64(got) - np.float64(want))
    bound = 2.0 ** -23 * np.maximum(1.0, np.abs(np.float64(want)))
    print('%s: worst error / bound = %.3g (%.3g), %d of %d values differ'
          % (label, (err / bound).max(), err.max(), (got != want).sum(), want.size))
    assert got.dtype == np.float32 and got.shape == want.shape and np.isfinite(got).all()
    assert np.all(err <= bound)


@pytest.mark.parametrize('hw,lam,cycles', CASES, ids=lambda v: '%dx%d' % v if isinstance(v, tuple) else str(v))
def test_against_float64(hw, lam, cycles):
    s, c = _pictures(hw)
    want = _reference(hw, lam, cycles)
    if hw != (1, 1):        # (the case moves, by thousands of the bound: a kernel that leaves s fails)
        assert np.abs(np.float64(want) - s).max() > 1
    got = _run(gpu_engine(), s, c, lam, cycles)
    _check(got, want, '%s lambda %g, %d cycle(s)' % (hw, lam, cycles))


def test_a_single_pixel_is_left_alone():
    s, c = _pictures((1, 1))
    assert _run(gpu_engine(), s, c, 5.0, DEFAULT).tobytes() == s.tobytes()      # (no edge: b = 0)


@pytest.mark.parametrize('hw', [(2, 2), (37, 53), (257, 190)])
def test_equal_pictures_come_back_bit_for_bit(hw):
    s = _pictures(hw)[0]
    eng = gpu_engine()
    for lam, cycles in ((0.04, DEFAULT), (5.0, DEFAULT), (500.0, 2)):
        assert ref.solve(s, s.copy(), lam, cycles).tobytes() == s.tobytes()     # the reference does the same
        assert _run(eng, s, s.copy(), lam, cycles).tobytes() == s.tobytes()


@pytest.mark.parametrize('hw', [(33, 31), (130, 67)])
def test_two_runs_give_the_same_bits(hw):
    eng = gpu_engine()
    s, c = _pictures(hw)
    assert _run(eng, s, c, 5.0, DEFAULT).tobytes() == _run(eng, s, c, 5.0, DEFAULT).tobytes()


def test_the_wrapper_takes_the_default_cycles():
    s, c = _pictures((33, 31))
    assert _run(gpu_engine(), s, c, 5.0, None).tobytes() == _reference((33, 31), 5.0, DEFAULT).tobytes()


def test_every_refusal_leaves_the_output_alone():
    hw = (16, 16)
    s, c = _pictures(hw)
    eng = gpu_engine()
    d_s, d_c = eng.to_device(s), eng.to_device(c)
    fill = np.full((2, 3) + hw, 7, np.float32)          # (twice the size: room for an output that overlaps itself)
    d_out = eng.to_device(fill)
    n = 3 * hw[0] * hw[1] * 4
    ok = dict(img=d_s.ptr, content=d_c.ptr, out=d_out.ptr, H=hw[0], W=hw[1], lam=5.0, cycles=2)
    bad = [dict(img=None), dict(content=None), dict(out=None), dict(H=0), dict(W=0), dict(H=-3), dict(W=40000),
           dict(lam=float('nan')), dict(lam=float('inf')), dict(lam=0.0), dict(lam=-1.0), dict(lam=1000.5),
           dict(cycles=0), dict(cycles=33), dict(cycles=-1),
           dict(out=d_s.ptr), dict(out=d_c.ptr),                        # the output is an input
           dict(img=d_out.ptr + n - 4), dict(content=d_out.ptr + 4)]    # ... or overlaps one by a single value
    for change in bad:
        a = dict(ok, **change)
        with pytest.raises(lib.StxError) as err:
            lib.call('stx_image_poisson', eng.handle, a['img'], a['content'], a['out'], a['H'], a['W'], a['lam'],
                     a['cycles'])
        assert err.value.code == -1 and 'stx_image_poisson' in str(err.value), change
        eng.sync()
        assert d_out.get().tobytes() == fill.tobytes(), change
        assert d_s.get().tobytes() == s.tobytes() and d_c.get().tobytes() == c.tobytes(), change
    with pytest.raises(lib.StxError):
        lib.call('stx_image_poisson', None, d_s.ptr, d_c.ptr, d_out.ptr, hw[0], hw[1], 5.0, 2)
    with pytest.raises(ValueError):                     # the wrapper: pictures of two sizes
        image_ops.poisson(eng, d_s, d_out, 5.0)
    # and the call the refusals were variations of goes through
    lib.call('stx_image_poisson', eng.handle, d_s.ptr, d_c.ptr, d_out.ptr, hw[0], hw[1], 5.0, 2)
    eng.sync()
    assert d_out.get()[0].tobytes() == _reference(hw, 5.0, 2).tobytes() and not (d_out.get()[1] != 7).any()
    for arr in (d_s, d_c, d_out):
        arr.free()


# ------------------------------------------------------------------------------------------------ command line
def _content_and_style(content_hw, style_hw, seed):
    """A content picture with straight edges and flat regions, and a noisy style picture."""
    rng = np.random.RandomState(seed)
    h, w = content_hw
    content = np.empty((h, w, 3))
    content[...] = (60, 90, 140)
    content[h // 3:, w // 4:] = (200, 170, 80)
    content[:, 2 * w // 3:] += 30
    content += rng.uniform(-4, 4, content.shape)
    style = rng.uniform(20, 235, style_hw + (3,))
    return Image.fromarray(np.uint8(np.clip(content, 0, 255))), Image.fromarray(np.uint8(style))


def _cli_run(tmp_path, monkeypatch, capsys, name, extra):
    """One run of the command line in its own directory: (final RGB, its PNG comment, the --save-every pictures by
    file suffix, the losses of <RUN>_log.csv, the (img, content, lambda, cycles) of every call of the stage)."""
    import csv
    from style_transfer_amd import cli
    where = tmp_path / name
    where.mkdir()
    monkeypatch.chdir(where)
    calls = []
    original = image_ops.poisson

    def recording(engine, img, content, lam, cycles=None):
        calls.append((img.get(), content.get(), lam, cycles))
        return original(engine, img, content, lam, cycles)
    monkeypatch.setattr(image_ops, 'poisson', recording)
    argv = ['-ci', '../c.png', '-si', '../s.png', '-ii', '../c.png', '--size', '80', '--min-size', '57',
            '-i', '2', '2', '--tile-size', '64', '--save-every', '2', '--model', 'vgg19', '--weights',
            'synthetic:0', '--devices', '0', '-oi', 'out.png'] + extra
    assert cli.main(argv) == 0
    monkeypatch.setattr(image_ops, 'poisson', original)
    capsys.readouterr()
    final = Image.open(where / 'out.png')
    saved = {re.search(r'_out_(\d+)\.png$', p).group(1): np.asarray(Image.open(p).convert('RGB'))
             for p in sorted(glob.glob(str(where / '*_out_*.png')))}
    logs = glob.glob(str(where / '*_log.csv'))
    assert len(logs) == 1
    with open(logs[0], newline='') as f:
        losses = [row['loss'] for row in csv.DictReader(f)]
    return np.asarray(final.convert('RGB')), final.text['Comment'], saved, losses, calls


def _gradient_distance(out, content):
    """sum |grad out - grad content|^2 over both axes and the three channels of two RGB uint8 pictures."""
    g = np.float64(out) - np.float64(np.asarray(content.convert('RGB')))
    return float((np.diff(g, axis=0) ** 2).sum() + (np.diff(g, axis=1) ** 2).sum())


def _reference_u8(call, luma=False):
    """The picture that the pipeline's output kernel writes for the reference's solve of one recorded call."""
    eng = gpu_engine()
    s, c, lam, cycles = call
    d_f, d_c = eng.to_device(ref.solve(s, c, lam, cycles)), eng.to_device(c)
    out = image_ops.to_u8_luma(eng, d_f, d_c, MEAN) if luma else image_ops.to_u8(eng, d_f, MEAN)
    d_f.free()
    d_c.free()
    return out


def test_cli_poisson(tmp_path, monkeypatch, capsys):
    content, style = _content_and_style((64, 80), (70, 60), 8)
    content.save(tmp_path / 'c.png')
    style.save(tmp_path / 's.png')
    bare = _cli_run(tmp_path, monkeypatch, capsys, 'bare', [])
    stage = _cli_run(tmp_path, monkeypatch, capsys, 'stage', ['--poisson-lambda', '5'])
    both = _cli_run(tmp_path, monkeypatch, capsys, 'both', ['--poisson-lambda', '5', '--poisson-cycles', '4',
                                                            '--preserve-color', 'luma'])
    # ---- off: no call, and nothing in the comment; on: the optimisation is untouched
    assert not bare[4] and 'poisson' not in bare[1]
    assert stage[3] == bare[3] == both[3] and len(bare[3]) == 4
    assert 'poisson_lambda=5.0' in stage[1] and 'poisson_cycles' not in stage[1]
    assert 'poisson_lambda=5.0' in both[1] and 'poisson_cycles=4' in both[1]
    assert sorted(bare[2]) == sorted(stage[2]) == sorted(both[2]) == ['0002', '0004']
    # ---- every written picture went through the stage, at the size of its scale, against that scale's content
    # (step 2's picture, step 4's, and the final iterate -- which is step 4's -- whenever it is asked for again)
    for run, cycles in ((stage, DEFAULT), (both, 4)):
        calls = run[4]
        assert len(calls) >= 3
        assert [(c[0].shape, c[2], c[3]) for c in calls] == ([((3, 46, 57), 5.0, cycles)]
                                                             + (len(calls) - 1) * [((3, 64, 80), 5.0, cycles)])
        for later in calls[2:]:
            assert np.array_equal(later[0], calls[1][0]) and np.array_equal(later[1], calls[1][1])
    small = np.float32(content.resize((57, 46), Image.LANCZOS)).transpose(2, 0, 1)[::-1] - MEAN
    assert np.array_equal(stage[4][0][1], small)
    assert np.array_equal(stage[4][2][1], np.float32(content).transpose(2, 0, 1)[::-1] - MEAN)
    # ---- the written pictures are the output kernel's of the reference's solve of the iterate
    for key, call in (('0002', stage[4][0]), ('0004', stage[4][1])):
        assert np.array_equal(stage[2][key], _reference_u8(call)), key
    assert np.array_equal(stage[0], _reference_u8(stage[4][2]))
    assert np.array_equal(stage[0], stage[2]['0004'])
    assert not np.array_equal(stage[0], bare[0])
    # ---- its gradients are closer to the content picture's than those of the run without the option
    d_stage, d_bare = _gradient_distance(stage[0], content), _gradient_distance(bare[0], content)
    print('sum |grad out - grad content|^2: %.6g with the stage, %.6g without' % (d_stage, d_bare))
    assert d_stage < d_bare
    # ---- with --preserve-color luma: the stage first, then the luminance transfer
    assert np.array_equal(both[0], _reference_u8(both[4][2], luma=True))
    assert np.array_equal(both[2]['0002'], _reference_u8(both[4][0], luma=True))
    assert not np.array_equal(both[0], stage[0])
    # ---- the module's command line: the same stage from files (the content resized to the result's size)
    for result, size in ((tmp_path / 'bare' / 'out.png', (64, 80)),
                         (glob.glob(str(tmp_path / 'bare' / '*_out_0002.png'))[0], (46, 57))):
        monkeypatch.chdir(tmp_path)
        assert poisson.main([str(result), 'c.png', 'again.png', '--poisson-lambda', '5', '--poisson-cycles', '3']) == 0
        with Image.open(result) as picture:
            s = poisson.pil_to_picture(picture)
            c = poisson.pil_to_picture(content.resize(picture.size, Image.LANCZOS))
        assert s.shape == (3,) + size
        again = np.asarray(Image.open(tmp_path / 'again.png').convert('RGB'))
        assert np.array_equal(again, _reference_u8((s, c, 5.0, 3)))
        assert _gradient_distance(again, content.resize(picture.size, Image.LANCZOS)) < _gradient_distance(
            np.asarray(Image.open(result).convert('RGB')), content.resize(picture.size, Image.LANCZOS))
