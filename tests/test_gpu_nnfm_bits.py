"""The bits of the nearest-neighbour term, pinned: SHA-256 digests of what the plain and the 3 x 3 patch form
wrote at the commit named in tests/golden/nnfm_bits.json -- the last one with two search kernels and two of every
host path -- on an MI355X.  The kernels use no atomics and sum in fixed orders, so the same digests are expected
of every later commit that does not mean to change the term's arithmetic.

  * op cases: C in {64, 128} (2 and 4 stages per bank block, 18 and 36 in the patch form) x maps (1, 1) (padding
    all round), (3, 5) (less than a query block, ragged rows), (31, 33) (several query blocks, one spanning map
    rows) x bank rows 1, 128 (one block, one slice), 129 (two slices: the merge kernel), 300 (a ragged last
    block); each through stx_op_nnfm_terms and through stx_op_nnfm_patch_terms at patch 1 and 3: the bytes of S,
    of the index array and of the two doubles.
  * banks: stx_nnfm_bank and stx_nnfm_patch_bank (patch 1 and 3) of the (31, 33) maps at strides 1 and 2.
  * tiles: loss and gradient bytes of the `alone` tile of tests/test_gpu_nnfm_patch.py with a bank of either form,
    the plain one set through stx_set_nnfm_targets and its own struct (nothing else in the suite runs that setter).

A case without an entry in the file fails.  New digests (only for a change that means to move the bits):
    python -m tests.test_gpu_nnfm_bits <commit> > tests/golden/nnfm_bits.json
"""

import ctypes
import hashlib
import json
import os
import struct
import sys

import numpy as np
import pytest

from style_transfer_amd import lib
from tests.gpu_helpers import gpu_engine

pytestmark = pytest.mark.gpu

CHANNELS = [64, 128]
MAPS = [(1, 1), (3, 5), (31, 33)]
ROWS = [1, 128, 129, 300]
STRIDES = [1, 2]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'nnfm_bits.json')


def _sha(*parts):
    return hashlib.sha256(b''.join(parts)).hexdigest()


def _unit_rows(rng, m, width):
    b = rng.standard_normal((m, width))
    return (b / np.linalg.norm(b, axis=1, keepdims=True)).astype(np.float32)


def _feat(rng, c, h, w):
    return np.maximum(rng.standard_normal((c, h, w)), 0).astype(np.float32) + np.float32(1e-3)


def _op(eng, feat, bank, name, patch=None):
    c, h, w = feat.shape
    d_feat, d_bank = eng.to_device(feat), eng.to_device(bank)
    s_out = eng.empty((c, h, w))
    idx = eng.empty((h * w,), np.int32)
    out = (ctypes.c_double * 2)()
    try:
        args = (d_feat.ptr, c, h, w) + (() if patch is None else (patch,)) + (d_bank.ptr, bank.shape[0])
        lib.call(name, eng.handle, *args, s_out.ptr, idx.ptr, out)
        return _sha(s_out.get().tobytes(), idx.get().tobytes(), struct.pack('<2d', out[0], out[1]))
    finally:
        for arr in (d_feat, d_bank, s_out, idx):
            arr.free()


def op_digests(eng, c, h, w, m):
    rng = np.random.RandomState(c + 7 * h + 13 * w + m)
    feat, plain, patch = _feat(rng, c, h, w), _unit_rows(rng, m, c), _unit_rows(rng, m, 9 * c)
    key = 'op C%d %dx%d M%d ' % (c, h, w, m)
    return {key + 'plain': _op(eng, feat, plain, 'stx_op_nnfm_terms'),
            key + 'patch1': _op(eng, feat, plain, 'stx_op_nnfm_patch_terms', 1),
            key + 'patch3': _op(eng, feat, patch, 'stx_op_nnfm_patch_terms', 3)}


def bank_digests(eng, c, stride):
    h, w = 31, 33
    d_feat = eng.to_device(_feat(np.random.RandomState(1000 + c), c, h, w))
    rows = -(-h // stride) * -(-w // stride)
    out = {}
    for tag, patch in (('plain', None), ('patch1', 1), ('patch3', 3)):
        d_bank = eng.empty((rows, (patch or 1) ** 2 * c))
        if patch is None:
            lib.call('stx_nnfm_bank', eng.handle, d_feat.ptr, lib.DEVICE, c, h, w, stride, d_bank.ptr, lib.DEVICE)
        else:
            lib.call('stx_nnfm_patch_bank', eng.handle, d_feat.ptr, lib.DEVICE, c, h, w, patch, stride, d_bank.ptr,
                     lib.DEVICE)
        out['bank C%d stride %d %s' % (c, stride, tag)] = _sha(d_bank.get().tobytes())
        d_bank.free()
    d_feat.free()
    return out


def tile_digests(eng):
    from tests.test_gpu_nnfm_patch import LW, NNFM_W, SW, TILE_CASES, _scene
    om, full, bank = _scene()
    cl, sl = TILE_CASES['alone']
    eng.set_contents_and_styles(om.contents, om.styles)
    out = {}
    run = lambda: eng.sc_grad_tile(full, (0, 0), (0, 0), cl, sl, LW, {}, SW)
    sha = lambda loss, grad: _sha(struct.pack('<d', loss), np.ascontiguousarray(grad).tobytes())
    d_plain = eng.to_device(np.ascontiguousarray(bank.reshape(-1, 9, 256)[:, 4]))       # any [rows, 256] array
    try:
        # the plain setter itself, through its own struct: TileEngine sets both forms as patch targets
        table = (lib.NnfmTarget * 1)()
        t = table[0]
        t.layer, t.channels, t.rows, t.bank, t.mem = b'conv3_1', 256, d_plain.shape[0], d_plain.ptr, lib.DEVICE
        t.weight = NNFM_W['conv3_1']
        lib.call('stx_set_nnfm_targets', eng.handle, table, 1)
        eng.primary.extra_taps['nnfm'] = ['conv3_1']
        out['tile alone plain'] = sha(*run())
        eng.set_nnfm_targets({'conv3_1': bank}, NNFM_W, patch=3)
        out['tile alone patch3'] = sha(*run())
    finally:
        eng.set_nnfm_targets({})
        d_plain.free()
    return out


def _held(got):
    with open(GOLDEN) as f:
        pinned = json.load(f)['digests']
    for key, digest in got.items():
        assert key in pinned, 'no pinned digest for %r' % key
        assert digest == pinned[key], '%s: %s, pinned %s' % (key, digest, pinned[key])


@pytest.mark.parametrize('m', ROWS)
@pytest.mark.parametrize('h,w', MAPS)
@pytest.mark.parametrize('c', CHANNELS)
def test_op_bits(c, h, w, m):
    _held(op_digests(gpu_engine(), c, h, w, m))


@pytest.mark.parametrize('stride', STRIDES)
@pytest.mark.parametrize('c', CHANNELS)
def test_bank_bits(c, stride):
    _held(bank_digests(gpu_engine(), c, stride))


def test_tile_bits():
    _held(tile_digests(gpu_engine()))


if __name__ == '__main__':
    engine = gpu_engine()
    digests = {}
    for c_ in CHANNELS:
        for h_, w_ in MAPS:
            for m_ in ROWS:
                digests.update(op_digests(engine, c_, h_, w_, m_))
        for stride_ in STRIDES:
            digests.update(bank_digests(engine, c_, stride_))
    digests.update(tile_digests(engine))
    json.dump({'commit': sys.argv[1], 'device': lib.device_name(0), 'digests': digests}, sys.stdout, indent=1)
    print()
