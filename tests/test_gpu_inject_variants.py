"""The loss-injecting backward convolution (conv_h2.hip, EPI = kEpiDgradInject) body by body: what a launch injects
and where its ReLU mask comes from are compile-time parameters of the epilogue (h2_variant, h2_launch_variant), and
every body must compute, to the bit, what the one generic body computed at the commit named in
tests/golden/inject_variants_bits.json, on an MI355X.

The launch is reached through the tile path, the only caller that injects (the stx_op_* hooks carry no loss term): a
five-layer graph  data -> c1 (3 -> C) -> c2 -> c3 -> c4 -> c5  (3 x 3, C -> C, each rectified), the loss terms under
test on c2, a style term on c5 so that the backward walk passes c3 -- whose backward launch injects c2's terms into
the gradient it leaves.  Per case:

  tiling   STX_CONV_ALGO = h2a | h2b | h2c: 64 channels x 8 rows, 128 channels x 8 rows, 64 channels x 16 rows
  form     style term | content term (its window rolled by a non-zero shift) | both
  mask     nibbles (c2's producer leaves them) | the fp32 blob (STX_RELU_CODES=0) | none (c2 not rectified)
  input    plain | pooled: a MAX pooling layer between c3 and c4, whose backward pass rides in c3's (PIN)
  shape    16 x 32 and 17 x 33 (h2a, h2b), 32 x 32 and 33 x 35 (the two-patch tiling h2c), C = 64; and C = 96 on the
           ragged shape: two channel tiles, the second one partial, so that every lane role meets the end of the
           channels as well as the ragged edges of the plane;
           128 -> 128, every channel block of the 128-channel tiling full: 72 x 256 and 73 x 257 (h2a), 136 x 256 and
           137 x 257 (h2b, h2c).

Channel counts and planes: a launch with K >= 128 slices its reduction on a plane that leaves compute units idle
(h2_plan: two slices cost less than one round), and a sliced launch injects in the reduce pass, not in this epilogue.
64 and 96 channels have fewer than two pairs of chunks per slice and never split, on any plane; the 128-channel
planes are the smallest on which two slices would need a second round of 256 workgroups (144 / 180 workgroups for
h2a, 136 / 162 for h2b, 144 / 162 for h2c), so the launch stays whole.  That the epilogue under test ran, unsplit, is
asserted from the engine's counters (lib.Q_INJECT_SPECIALISED, lib.Q_INJECT_VARIANTS): each
case must launch the body it is meant to -- style or content alone onto a rectified blob: the specialised one; both
terms, an un-rectified blob, a content term with a pooled input: the generic one -- and a case that is not in the
file fails.

New figures (only for a change that means to move them; the module then asks no counter, so that it runs at a commit
that has none):
    python -m tests.test_gpu_inject_variants <commit> > tests/golden/inject_variants_bits.json
"""

import contextlib
import hashlib
import json
import os
import sys

import numpy as np
import pytest

from style_transfer_amd import lib
from style_transfer_amd.netspec import LayerSpec, NetSpec

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'inject_variants_bits.json')
TILINGS = ['h2a', 'h2b', 'h2c']
FORMS = ['style', 'content', 'both']
MASKS = ['nibbles', 'fp32', 'none']
SHAPES = {'h2a': [(16, 32), (17, 33)], 'h2b': [(16, 32), (17, 33)], 'h2c': [(32, 32), (33, 35)]}
SHAPES_128 = {'h2a': [(72, 256), (73, 257)], 'h2b': [(136, 256), (137, 257)], 'h2c': [(136, 256), (137, 257)]}
START, ROLL = (8, 16), (-16, 24)
SWITCHES = ('STX_CONV_ALGO', 'STX_RELU_CODES', 'STX_POOL_BWD_FUSE', 'STX_H2_INJECT_GENERIC')
# h2_variant's codes (csrc/common.h)
STYLE, CONTENT, NIBBLES, BLOB = 1, 2, 4, 8


def graph(C, rectified, pooled):
    net = NetSpec('inject_%d_%d_%d' % (C, rectified, pooled))
    net.layers.append(LayerSpec('input', 'Input', None, 'data', shape=(1, 3, 224, 224)))
    prev = 'data'
    for i in range(1, 6):
        blob = 'c%d' % i
        net.layers.append(LayerSpec(blob, 'Convolution', prev, blob, num_output=C, kernel_size=3, pad=1))
        if i != 2 or rectified:
            net.layers.append(LayerSpec('relu_' + blob, 'ReLU', blob, blob))
        prev = blob
        if pooled and i == 3:
            net.layers.append(LayerSpec('p3', 'Pooling', prev, 'p3', kernel_size=2, stride=2, pool='MAX'))
            prev = 'p3'
    return net


def expected_variant(form, mask, pooled):
    if form == 'both' or mask == 'none' or (form == 'content' and pooled):
        return 0
    return (STYLE if form == 'style' else CONTENT) | (NIBBLES if mask == 'nibbles' else BLOB)


def cases(tiling, pooled):
    """[(key, C, form, mask, (th, tw))] of one tiling and input kind."""
    out = []
    for form in FORMS:
        for mask in MASKS:
            for n, (th, tw) in enumerate(SHAPES[tiling]):
                for C in ([64, 96] if n == 1 else [64]):
                    key = '%s/%s/%s/%s/C%d/%dx%d' % (tiling, 'pooled' if pooled else 'plain', form, mask, C, th, tw)
                    out.append((key, C, form, mask, (th, tw)))
            for th, tw in SHAPES_128[tiling]:
                key = '%s/%s/%s/%s/C128/%dx%d' % (tiling, 'pooled' if pooled else 'plain', form, mask, th, tw)
                out.append((key, 128, form, mask, (th, tw)))
    return out


_MAPS = {}


def content_map(C):
    """The content target of c2: a map larger than every tile of its channel count, from START on."""
    if C not in _MAPS:
        h, w = (160, 288) if C == 128 else (64, 96)
        _MAPS[C] = np.abs(np.random.RandomState(7).standard_normal((C, h, w))).astype(np.float32)
    return _MAPS[C]


def set_switches(values):
    for name in SWITCHES:
        os.environ.pop(name, None)
    os.environ.update(values)
    lib.reread_env()


def run_group(tiling, pooled, counters):
    """Every case of (tiling, pooled) -> {key: {'loss': float.hex, 'grad': sha256, ...}}; with `counters` also what
    the engine's counters say about the launches of each case."""
    from oracle.caffe_net import synthetic_weights
    from style_transfer_amd.engine import TileEngine
    results = {}
    engines = {}
    try:
        for key, C, form, mask, (th, tw) in cases(tiling, pooled):
            set_switches(dict({'STX_CONV_ALGO': tiling}, **({'STX_RELU_CODES': '0'} if mask == 'fp32' else {})))
            ek = (C, mask)
            if ek not in engines:
                net = graph(C, mask != 'none', pooled)
                engines[ek] = TileEngine(net, 0, synthetic_weights(net.as_dicts(), C))
            eng = engines[ek]
            cl = ['c2'] if form in ('content', 'both') else []
            sl = (['c2'] if form in ('style', 'both') else []) + ['c5']
            cw, sw = {l: 0.05 for l in cl}, {l: 0.2 for l in sl}
            r = np.random.RandomState(11)
            eng.set_contents_and_styles(
                [{l: content_map(C) for l in cl}],
                [{l: np.tril(r.standard_normal((C, C))).astype(np.float32) for l in sl}])
            tile = np.random.RandomState(100 * th + tw).uniform(-110, 120, (3, th, tw)).astype(np.float32)
            eng.profile(True)
            before = (eng.query(lib.Q_INJECT_SPECIALISED), eng.query(lib.Q_INJECT_VARIANTS)) if counters else None
            loss, grad = eng.sc_grad_tile(tile, START, ROLL, cl, sl, {}, cw, sw)
            labels = [row[0] for row in eng.profile_read()]
            eng.profile(False)
            assert np.isfinite(loss) and np.isfinite(grad).all() and np.abs(grad).max() > 0, key
            # the shape of the evaluation the case is about: c3's backward launch ran, and with a pooled input the
            # pooling layer's own backward kernel did not
            assert 'bwd c3' in labels and 'bwd p3' not in labels, (key, labels)
            results[key] = {'loss': float(loss).hex(), 'grad': hashlib.sha256(grad.tobytes()).hexdigest()}
            if counters:
                results[key]['launches'] = int(eng.query(lib.Q_INJECT_SPECIALISED) - before[0])
                results[key]['variants'] = (int(before[1]), int(eng.query(lib.Q_INJECT_VARIANTS)))
    finally:
        for eng in engines.values():
            eng.close()
        set_switches({})
    return results


@pytest.fixture(scope='module')
def golden():
    with open(GOLDEN) as f:
        yield json.load(f)['cases']
    _MAPS.clear()


@pytest.mark.parametrize('pooled', [False, True], ids=['plain', 'pooled'])
@pytest.mark.parametrize('tiling', TILINGS)
def test_every_body_reproduces_the_generic_body_bit_for_bit(golden, tiling, pooled):
    from tests.gpu_helpers import require_gpu
    require_gpu()
    saved = {k: os.environ.get(k) for k in SWITCHES}
    try:
        got = run_group(tiling, pooled, counters=True)
    finally:
        set_switches({k: v for k, v in saved.items() if v is not None})
    for key, _, form, mask, _ in cases(tiling, pooled):
        assert key in golden, 'no recorded figures for ' + key
        assert got[key]['loss'] == golden[key]['loss'], key
        assert got[key]['grad'] == golden[key]['grad'], key
        # the body the case is meant to launch: once per evaluation, and no other -- the engine's set of the bodies
        # it has launched gains that body's bit or stays as it was
        want = expected_variant(form, mask, pooled)
        before, after = got[key]['variants']
        assert got[key]['launches'] == (1 if want else 0), (key, got[key])
        assert after == (before | (1 << want) if want else before), (key, got[key])


def all_cases():
    out = {}
    for tiling in TILINGS:
        for pooled in (False, True):
            out.update(run_group(tiling, pooled, counters=False))
    return out


if __name__ == '__main__':
    with contextlib.redirect_stdout(sys.stderr):
        if lib.device_count() < 1:
            raise SystemExit('no GPU visible')
        results = all_cases()
    json.dump({'commit': sys.argv[1], 'device': lib.device_name(0), 'cases': results}, sys.stdout, indent=1)
    print()
