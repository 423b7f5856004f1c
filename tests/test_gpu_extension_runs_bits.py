"""Whole runs with the optional terms on, pinned: what four small two-scale runs computed and which library calls
they made at the commit named in tests/golden/extension_runs_bits.json, on an MI355X.  The kernels use no atomics
and sum in fixed orders (every candidate of the direct-convolution autotuner accumulates in the same order), so
the same bits are expected of every later commit that does not mean to change a term's arithmetic or the
schedule between the command line and the engines' targets.

Every run: one TileFarm of VGG-19 with synthetic weights on GPU 0, a 64 x 64 content picture, two style pictures
of about 50 x 57, ``--size 64 --min-size 45 -i 2 2`` with Adam (scales of 45 and 64 pixels: per-scale state is
freed and made again), ``np.random.seed(0)`` first.  With ``--tile-size 32`` a scale has 2 x 2 tiles and a second
engine joins the GPU's shared group.
  * masks:  --tile-size 32, --style-masks (one per style picture), --content-mask, --lap-weight 30,
            --lap-pools 4 16:3, --photo-weight 1e4, --preserve-color luma, --swt-weight 1, --swt-levels 2
  * banks:  --tile-size 32, --stat-weight 1, --stat-layers conv1_1 conv2_2:2, --nnfm-weight 1, --nnfm-layers
            conv3_1, --nnfm-patch 3, --nnfm-stride 2, --content-mask, --preserve-color match,
            --style-multiscale 32 64
  * jitter: --tile-size 64, --jitter, --stat-weight 1, --nnfm-weight 1, --nnfm-layers conv3_1, --content-mask,
            --photo-weight 1e4
  * plain:  --tile-size 32
The callbacks of `masks` and `plain` have ``wants_image``, so those two run one iteration ahead of the GPU.

Pinned per run: float.hex of loss, update_size and tv_loss of every callback call; SHA-256 of the last averaged
iterate and of the picture written from it; and the number of lib.call invocations per function name (counted by
a wrapper around lib.call for the duration of the run, the release of the run's StyleTransfer included).  A later
tree may make no more calls of any name, and exactly as many of the setters, the tile evaluation, the image
kernels, the bank and statistics passes, the allocations and the copies (EXACT): one more upload, setter or wait
per step shows here.

The four runs share the farm's tile buffers and engines, so they always run together and in this order, once per
module.  A run without an entry in the file fails.  New figures (only for a change that means to move them):
    python -m tests.test_gpu_extension_runs_bits <commit> > tests/golden/extension_runs_bits.json
"""

from argparse import Namespace
import contextlib
import gc
import hashlib
import json
import os
import sys

import numpy as np
from PIL import Image
import pytest

from style_transfer_amd import lib

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'extension_runs_bits.json')
COMMON = ['-ci', 'c', '-si', 's0', 's1', '--size', '64', '--min-size', '45', '-i', '2', '2']
RUNS = {
    'masks': ['--tile-size', '32', '--style-masks', 'm0', 'm1', '--content-mask', 'cm', '--lap-weight', '30',
              '--lap-pools', '4', '16:3', '--photo-weight', '1e4', '--preserve-color', 'luma',
              '--swt-weight', '1', '--swt-levels', '2'],
    'banks': ['--tile-size', '32', '--stat-weight', '1', '--stat-layers', 'conv1_1', 'conv2_2:2',
              '--nnfm-weight', '1', '--nnfm-layers', 'conv3_1', '--nnfm-patch', '3', '--nnfm-stride', '2',
              '--content-mask', 'cm', '--preserve-color', 'match', '--style-multiscale', '32', '64'],
    'jitter': ['--tile-size', '64', '--jitter', '--stat-weight', '1', '--nnfm-weight', '1', '--nnfm-layers',
               'conv3_1', '--content-mask', 'cm', '--photo-weight', '1e4'],
    'plain': ['--tile-size', '32'],
}
RUN_AHEAD = ('masks', 'plain')
EXACT = ('stx_set_', 'stx_image_', 'stx_sc_grad_tile', 'stx_nnfm_patch_bank', 'stx_feature_stats', 'stx_malloc',
         'stx_memcpy_async')


def _picture(rng, hw, centre, spread):
    """Smooth shapes under mild noise, clear of 0 and 255 (as tests/test_gpu_photo.py makes its pictures)."""
    y, x = np.mgrid[:hw[0], :hw[1]]
    waves = np.stack([np.sin(x / (3.0 + c) + c) * np.cos(y / (4.0 - c)) for c in range(3)], axis=2)
    return Image.fromarray(np.uint8(np.clip(centre + spread * waves + rng.uniform(-12, 12, hw + (3,)), 0, 255)))


def _inputs():
    """(content, [style, style], [style mask, style mask], content mask): PIL pictures."""
    rng = np.random.RandomState(31)
    content = _picture(rng, (64, 64), 125, 60)
    styles = [_picture(rng, (50, 57), 130, 45), _picture(rng, (56, 49), 120, 50)]
    y, x = np.mgrid[:64, :64]
    left = np.clip((40 - x) * 16, 0, 255)
    grey = lambda a: Image.fromarray(np.uint8(a), 'L')
    return content, styles, [grey(left), grey(255 - left)], grey(np.clip(y * 5 + x, 0, 255))


class _Recorder:
    def __init__(self):
        self.steps = []

    def __call__(self, step, update_size, loss, tv_loss, transfer):
        self.steps.append([float(v).hex() for v in (loss, update_size, tv_loss)])


class _RecorderBehind(_Recorder):
    """Never looks at a step's image: the step loop runs one iteration ahead of it."""

    def wants_image(self, n):
        return False


@contextlib.contextmanager
def _counted_calls(counts):
    real = lib.call

    def counting(name, *args):
        counts[name] = counts.get(name, 0) + 1
        return real(name, *args)
    lib.call = counting
    try:
        yield
    finally:
        lib.call = real


def _run(farm, name, inputs):
    from style_transfer_amd.config_system import parse_args
    from style_transfer_amd.transfer import StyleTransfer
    content, styles, style_masks, content_mask = inputs
    state = Namespace()
    args = parse_args(state, COMMON + RUNS[name], config_py=False)
    recorder = (_RecorderBehind if name in RUN_AHEAD else _Recorder)()
    gc.collect()
    np.random.seed(0)
    counts = {}
    with _counted_calls(counts):
        st = StyleTransfer(farm, args, state)
        st.transfer_multiscale([content], styles, callback=recorder,
                               style_masks=style_masks if '--style-masks' in RUNS[name] else None,
                               content_mask=content_mask if '--content-mask' in RUNS[name] else None)
        raw = hashlib.sha256(st.current_raw.get().tobytes()).hexdigest()
        u8 = hashlib.sha256(st.output_u8().tobytes()).hexdigest()
        del st
        gc.collect()
    return {'steps': recorder.steps, 'raw': raw, 'u8': u8, 'calls': dict(sorted(counts.items()))}


def all_runs():
    from style_transfer_amd.farm import TileFarm
    from style_transfer_amd.netspec import builtin_net
    from style_transfer_amd.weights import load_weights
    net = builtin_net('vgg19')
    farm = TileFarm(net, [0], load_weights('synthetic:3', net), verbose=False)
    try:
        inputs = _inputs()
        return {name: _run(farm, name, inputs) for name in RUNS}
    finally:
        farm.close()


@pytest.fixture(scope='module')
def runs():
    from tests.gpu_helpers import require_gpu
    require_gpu()       # (a module fixture is made before the per-test guard of conftest.py runs)
    return all_runs()


def _pinned(name):
    with open(GOLDEN) as f:
        pinned = json.load(f)['runs']
    assert name in pinned, 'no pinned run %r' % name
    return pinned[name]


@pytest.mark.parametrize('name', list(RUNS))
def test_run_bits(runs, name):
    got, pinned = runs[name], _pinned(name)
    print(name, got['steps'], got['raw'], got['u8'])
    assert len(got['steps']) == 4
    assert got['steps'] == pinned['steps']
    assert got['raw'] == pinned['raw']
    assert got['u8'] == pinned['u8']


@pytest.mark.parametrize('name', list(RUNS))
def test_run_calls(runs, name):
    got, pinned = runs[name]['calls'], _pinned(name)['calls']
    print(name, got)
    for func, n in got.items():
        assert n <= pinned.get(func, 0), '%s: %d calls of %s, pinned %d' % (name, n, func, pinned.get(func, 0))
    for func in sorted(set(got) | set(pinned)):
        if func.startswith(EXACT):
            assert got.get(func, 0) == pinned.get(func, 0), \
                '%s: %d calls of %s, pinned %d' % (name, got.get(func, 0), func, pinned.get(func, 0))


if __name__ == '__main__':
    with contextlib.redirect_stdout(sys.stderr):
        if lib.device_count() < 1:
            raise SystemExit('no GPU visible')
        results = all_runs()
    json.dump({'commit': sys.argv[1], 'device': lib.device_name(0), 'runs': results}, sys.stdout, indent=1)
    print()
