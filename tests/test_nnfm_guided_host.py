"""Host-side checks of the region-guided nearest-neighbour term (--nnfm-masks): the float64 statement of its
definition (tests/nnfm_guided_ref.py), the option and its refusals, the segment bookkeeping of the banks, the masks'
way to the engines and the C ABI.  No GPU.

The finite-difference bound.  E / 2 is a weighted mean of 30 numbers 1 - c below 2, each c a 64-term dot product of
numbers below 1: its float64 rounding stays under 1e-14.  The step is 1e-6 |f_i|, so the quotient carries at most
1e-14 / (2e-6 |f_i|) = 5e-9 / |f_i|.  The slope's scale is the column's max |S / n|: an element of t - c x is of the
order 1 / sqrt(C) = 0.125, the weights of the two segments add up to about 1 and n = 15, so about 0.125 / (15 |f_i|)
= 8e-3 / |f_i| -- the quotient's error is 6e-7 of it, and the bound is 1e-6 with the lists held.  The third-order
term of a central difference over a turn of 1e-6 rad is of the order 1e-12 and does not count.  (With C = 12 and a
step of 1e-7 |f_i| tests/test_nnfm_knn_host.py holds the same 1e-6; at C = 64 the elements are smaller and that
step's rounding share would be ten times the one here.)"""

from argparse import Namespace
import ctypes

import numpy as np
import pytest
from PIL import Image

from style_transfer_amd import lib
from style_transfer_amd.config_system import check_nnfm_options, nnfm_masks, parse_args
from style_transfer_amd.netspec import builtin_net
from style_transfer_amd.terms import NnfmBanks, mask_at_size, rolled_mask
from tests import nnfm_guided_ref as ref
from tests import nnfm_knn_ref, nnfm_ref

BASE = ['-ci', 'c.png', '-si', 's1.png', 's2.png']
ON = ['--nnfm-weight', '1', '--nnfm-masks', 'a.png', 'b.png']


def _inputs(seed=0, c=64, h=3, w=5, seg_rows=(7, 9)):
    rng = np.random.RandomState(seed)
    B = rng.standard_normal((sum(seg_rows), c))
    B /= np.linalg.norm(B, axis=1, keepdims=True)
    F = rng.standard_normal((c, h, w)) * 10.0 ** rng.uniform(-2, 3, (h, w))
    m = rng.uniform(0, 1, (len(seg_rows), h * w))
    return F, B, list(seg_rows), m


def test_gradient_is_the_finite_difference_of_half_e_with_the_lists_held():
    F, B, seg_rows, m = _inputs(seed=3)
    k, n = 2, 15
    J = ref.topk(F, B, seg_rows, m, k)
    assert J.shape == (2, k, n) and J.min() >= 0
    E, S, asum, a = ref.terms_at(F, B, seg_rows, m, J)
    assert a == pytest.approx(m.sum() / n, rel=1e-15) and asum == np.abs(S).sum()
    g = S / n
    r = nnfm_ref.unit_columns(F)[1].reshape(F.shape[1:])
    worst = 0.0
    for index in np.ndindex(*F.shape):
        h = 1e-6 * r[index[1:]]
        plus, minus = F.copy(), F.copy()
        plus[index] += h
        minus[index] -= h
        fd = (ref.half_e(plus, B, seg_rows, m, J) - ref.half_e(minus, B, seg_rows, m, J)) / (2 * h)
        worst = max(worst, abs(fd - g[index]) / np.abs(g[:, index[1], index[2]]).max())
    print('guided finite difference, C 64 3x5 S 2 k 2: %.2e of the column\'s max |S / n|' % worst)
    assert worst <= 1e-6


@pytest.mark.parametrize('k', [1, 3])
def test_one_segment_of_ones_is_the_unguided_reference_exactly(k):
    F, B, _, _ = _inputs(seed=4)
    seg_rows, m = [len(B)], np.ones((1, 15))
    J = ref.topk(F, B, seg_rows, m, k)
    assert np.array_equal(J[0], nnfm_knn_ref.topk(F, B, k))
    ours, theirs = ref.terms_at(F, B, seg_rows, m, J), nnfm_knn_ref.terms_at(F, B, J[0])
    assert ours[0] == pytest.approx(theirs[0], rel=1e-14) and np.allclose(ours[1], theirs[1], rtol=1e-14, atol=0)
    assert ours[3] == 1.0
    half = ref.terms_at(F, B, seg_rows, 0.5 * m, J)
    assert np.array_equal(half[1], 0.5 * ours[1]) and half[3] == 0.5 and half[0] == pytest.approx(0.5 * ours[0], rel=1e-14)


def test_per_segment_lists_are_the_lists_of_the_segment_alone_and_unsearched_pairs_hold_minus_one():
    F, B, seg_rows, _ = _inputs(seed=5, h=3, w=100, seg_rows=(5, 11, 4))       # n = 300: three query blocks
    m = np.zeros((3, 300))
    m[0, :128] = 1
    m[1, 128:] = 1
    m[2, 200] = 0.25            # one column makes the third block of segment 2 a searched pair
    on = ref.searched(m)
    assert on.tolist() == [[True, False, False], [False, True, True], [False, True, False]]
    J = ref.topk(F, B, seg_rows, m, 2)
    off = ref.offsets(seg_rows)
    for s in range(3):
        alone = nnfm_knn_ref.topk(F, B[off[s]:off[s] + seg_rows[s]], 2)
        for b in range(3):
            cols = slice(128 * b, min(128 * (b + 1), 300))
            if on[s, b]:
                assert np.array_equal(J[s][:, cols], alone[:, cols])        # zero-weight columns of the block included
            else:
                assert np.all(J[s][:, cols] == -1)
    E, S, asum, a = ref.terms_at(F, B, seg_rows, m, J)
    assert a == pytest.approx((128 + 172 + 0.25) / 300) and np.all(np.isfinite(S))
    # all masks zero: nothing
    zero = ref.terms_at(F, B, seg_rows, 0 * m, ref.topk(F, B, seg_rows, 0 * m, 2))
    assert zero[0] == 0 and not zero[1].any() and zero[2] == 0 and zero[3] == 0


# ---------------------------------------------------------------------------------------------- the option
def test_option_is_absent_unless_set_and_the_comment_carries_it_only_then():
    from style_transfer_amd.cli import image_comment
    bare = parse_args(Namespace(), BASE + ['--nnfm-weight', '1'], config_py=False)
    assert 'nnfm_masks' not in bare and 'nnfm_masks' not in repr(vars(bare.ns)) and nnfm_masks(bare) == []
    assert 'nnfm_masks' not in image_comment(bare, BASE + ['--nnfm-weight', '1'])
    given = parse_args(Namespace(), BASE + ON, config_py=False)
    assert given.nnfm_masks == ['a.png', 'b.png'] and nnfm_masks(given) == ['a.png', 'b.png']
    assert "nnfm_masks=['a.png', 'b.png']" in image_comment(given, BASE + ON)
    assert check_nnfm_options(given, builtin_net('vgg19').blob_names()) == ['conv3_1', 'conv4_1']


def test_every_new_refusal_and_the_old_one_first():
    layers = builtin_net('vgg19').blob_names()
    two = dict(nnfm_weight=1.0, style_images=['s1.png', 's2.png'], nnfm_masks=['a.png', 'b.png'])
    assert check_nnfm_options(Namespace(**two), layers) == ['conv3_1', 'conv4_1']
    with pytest.raises(ValueError, match='--nnfm-patch 3'):
        check_nnfm_options(Namespace(nnfm_patch=3, **two), layers)
    with pytest.raises(ValueError, match='--nnfm-cover'):
        check_nnfm_options(Namespace(nnfm_cover=0.5, **two), layers)
    assert check_nnfm_options(Namespace(nnfm_cover=0.0, nnfm_patch=1, nnfm_k=4, **two), layers)
    with pytest.raises(ValueError, match='one mask per style image'):
        check_nnfm_options(Namespace(nnfm_weight=1.0, style_images=['s1.png'], nnfm_masks=['a.png', 'b.png']), layers)
    with pytest.raises(ValueError, match='one mask per style image'):
        parse_args(Namespace(), BASE + ['--nnfm-weight', '1', '--nnfm-masks', 'a.png'], config_py=False)
    nine = ['m%d.png' % i for i in range(9)]
    with pytest.raises(ValueError, match='at most 8'):
        check_nnfm_options(Namespace(nnfm_weight=1.0, style_images=nine, nnfm_masks=nine), layers)
    with pytest.raises(ValueError, match='--nnfm-weight is needed'):
        parse_args(Namespace(), BASE + ['--nnfm-masks', 'a.png', 'b.png'], config_py=False)
    # --style-masks: the existing refusal, unchanged, before any of the new ones
    for extra in (dict(), dict(nnfm_patch=3), dict(nnfm_cover=0.5), dict(nnfm_masks=['a.png'])):
        merged = dict(two, style_masks=['x.png', 'y.png'], **extra)
        with pytest.raises(ValueError, match='--nnfm-weight cannot be combined with --style-masks'):
            check_nnfm_options(Namespace(**merged), layers)
    with pytest.raises(ValueError, match='--style-masks'):
        parse_args(Namespace(), BASE + ON + ['--style-masks', 'x.png', 'y.png'], config_py=False)


def test_dist_refuses_the_masks_like_the_content_mask():
    from style_transfer_amd.dist import UNBROADCAST_OPTIONS, refuse_unbroadcast_options
    assert ('nnfm_masks', False, 'the masks are') in UNBROADCAST_OPTIONS
    with pytest.raises(NotImplementedError, match='--nnfm-masks'):
        refuse_unbroadcast_options(Namespace(nnfm_masks=['a.png']))


# ------------------------------------------------------------------------------ banks, segments and masks
class _Part:
    def __init__(self, rows):
        self.shape = (rows, 64)


class _FakeFarm:
    """What NnfmBanks needs of a farm and an engine: banks are row counts, the sent targets are recorded."""

    def __init__(self):
        self.sent = []

    def nnfm_bank(self, feat, stride, patch):
        return _Part(-(-feat.shape[1] // stride) * -(-feat.shape[2] // stride))

    def concat_rows(self, parts):
        return _Part(sum(p.shape[0] for p in parts))

    def set_nnfm_targets(self, targets, weights, patch, k, cover=0.0, segments=None, masks=None):
        self.sent.append(dict(rows={l: t.shape[0] for l, t in targets.items()}, weights=weights, patch=patch, k=k,
                              cover=cover, segments=segments, masks=masks))


def _stripes(hw, left):
    m = np.zeros(hw, np.uint8)
    m[:, :hw[1] // 2] = 255
    return Image.fromarray(m if left else 255 - m)


def test_banks_record_the_rows_of_every_picture_and_send_resized_rolled_masks(capsys):
    farm = _FakeFarm()
    st = Namespace(args=Namespace(nnfm_weight=2.0, nnfm_layers=['conv3_1', 'conv4_1:3'], nnfm_k=2), farm=farm, engine=farm,
                   img=np.zeros((3, 40, 48), np.float32), nnfm_masks=[_stripes((80, 96), True), _stripes((80, 96), False)])
    term = NnfmBanks()
    term.read(st)
    assert [m.shape for m in term.masks] == [(40, 48)] * 2 and term.masks[0].dtype == np.float32
    assert np.array_equal(term.masks[0], mask_at_size(st.nnfm_masks[0], (40, 48)))
    term.begin()
    # two pictures, two ladder sizes each (--style-multiscale): every size of a picture goes into its segment
    shapes = {0: [(10, 12), (5, 6)], 1: [(8, 8), (4, 4)]}
    for index in (0, 1):
        for h, w in shapes[index]:
            for layer, div in (('conv3_1', 1), ('conv4_1', 2)):
                term.take(st, layer, np.zeros((64, -(-h // div), -(-w // div)), np.float32))
        term.picture_done(st, index)
    term.finish(st, 4, quiet=False)
    assert term.segments == {'conv3_1': [120 + 30, 64 + 16], 'conv4_1': [30 + 9, 16 + 4]}
    printed = capsys.readouterr().out
    assert 'NNFM bank rows: conv3_1 230 (150 + 80), conv4_1 59 (39 + 20); k 2\n' in printed, printed
    term.send(st, roll=(5, -3))
    sent = farm.sent[-1]
    assert sent['segments'] == term.segments and sent['rows'] == {'conv3_1': 230, 'conv4_1': 59}
    assert sent['k'] == 2 and sent['patch'] == 1 and sent['cover'] == 0
    assert sent['weights'] == pytest.approx({'conv3_1': 0.5, 'conv4_1': 1.5})
    for got, mask in zip(sent['masks'], term.masks):
        assert np.array_equal(got, rolled_mask(mask, (5, -3))) and np.array_equal(got, np.roll(mask, (-3, 5), (0, 1)))
    term.send(st)
    assert all(np.array_equal(got, mask) for got, mask in zip(farm.sent[-1]['masks'], term.masks))
    # a mask count that is not the picture count is refused before the library is asked
    term.masks = term.masks[:1]
    with pytest.raises(ValueError, match='--nnfm-masks'):
        term.send(st)
    assert len(farm.sent) == 2


def test_without_masks_the_banks_are_sent_as_before(capsys):
    farm = _FakeFarm()
    st = Namespace(args=Namespace(nnfm_weight=1.0, nnfm_layers=['conv3_1']), farm=farm, engine=farm,
                   img=np.zeros((3, 40, 48), np.float32), nnfm_masks=None)
    term = NnfmBanks()
    term.read(st)
    term.begin()
    term.take(st, 'conv3_1', np.zeros((64, 10, 12), np.float32))
    term.picture_done(st, 0)
    term.finish(st, 1, quiet=False)
    assert 'NNFM bank rows: conv3_1 120\n' in capsys.readouterr().out
    term.send(st)
    assert farm.sent[-1]['segments'] is None and farm.sent[-1]['masks'] is None


class _Recorder:
    def __init__(self, monkeypatch):
        self.calls = []
        self.handle = None
        self.primary = Namespace(extra_taps={})
        monkeypatch.setattr(lib, 'call', lambda name, *args: self.calls.append((name,) + args))

    def _cstr(self, text):
        return text.encode()


def test_engine_builds_the_guided_call_and_refuses_what_the_library_would(monkeypatch):
    from style_transfer_amd.engine import TileEngine
    rec = _Recorder(monkeypatch)
    rec._set_nnfm_guided_targets = lambda *a: TileEngine._set_nnfm_guided_targets(rec, *a)
    bank = np.ones((12, 64), np.float32)
    masks = [np.zeros((16, 24), np.float32), np.ones((16, 24), np.float32)]
    TileEngine.set_nnfm_targets(rec, {'conv1_1': bank}, {'conv1_1': 0.5}, 1, 3, segments={'conv1_1': [5, 7]}, masks=masks)
    name, handle, table, n, ptrs, segments, H, W, mem = rec.calls[-1]
    assert name == 'stx_set_nnfm_guided_targets' and n == 1 and (segments, H, W, mem) == (2, 16, 24, lib.HOST)
    t = table[0]
    assert (t.layer, t.channels, t.k, t.segments, t.weight) == (b'conv1_1', 64, 3, 2, 0.5) and list(t.seg_rows[0:2]) == [5, 7]
    assert ptrs[0] == masks[0].ctypes.data and ptrs[1] == masks[1].ctypes.data
    assert rec.primary.extra_taps['nnfm'] == ['conv1_1']
    bad = [dict(segments={'conv1_1': [5, 6]}, masks=masks),                 # the rows do not add up
           dict(segments={'conv1_1': [2, 10]}, masks=masks),                # a segment below k
           dict(segments={'conv1_1': [12]}, masks=masks),                   # one count for two masks
           dict(segments={'conv1_1': [5, 7]}, masks=[masks[0], masks[1][:8]]),
           dict(segments={'conv1_1': [5, 7]}, masks=None),
           dict(segments={'conv1_1': [5, 7]}, masks=masks, patch=3),
           dict(segments={'conv1_1': [5, 7]}, masks=masks, cover=0.5)]
    for kwargs in bad:
        with pytest.raises(ValueError):
            TileEngine.set_nnfm_targets(rec, {'conv1_1': bank}, None, kwargs.pop('patch', 1), 3, kwargs.pop('cover', 0.0),
                                        **kwargs)
    with pytest.raises(ValueError, match='1 to 8'):
        TileEngine.set_nnfm_targets(rec, {'conv1_1': np.ones((27, 64), np.float32)}, None, 1, 3,
                                    segments={'conv1_1': [3] * 9}, masks=[masks[0]] * 9)
    assert len(rec.calls) == 1


def test_abi_symbols_are_present_and_bound():
    so = ctypes.CDLL(lib.LIB_PATH)
    header = open(lib.LIB_PATH.rsplit('/style_transfer_amd/', 1)[0] + '/include/stx.h').read()
    for name in ('stx_set_nnfm_guided_targets', 'stx_op_nnfm_guided_terms'):
        assert hasattr(so, name) and name in lib.SIGNATURES and 'int %s(' % name in header
    assert 'stx_nnfm_guided_target;' in header and '#define STX_NNFM_MAX_SEGMENTS 8' in header
    assert lib.NNFM_MAX_SEGMENTS == 8
    fields = [name for name, _ in lib.NnfmGuidedTarget._fields_]
    assert fields == ['layer', 'channels', 'k', 'segments', 'seg_rows', 'bank', 'mem', 'weight']
    assert len(lib.SIGNATURES['stx_set_nnfm_guided_targets']) == 8 and len(lib.SIGNATURES['stx_op_nnfm_guided_terms']) == 18
    # the older layouts stay
    assert [name for name, _ in lib.NnfmKnnTarget._fields_] == ['layer', 'channels', 'patch', 'k', 'rows', 'bank', 'mem', 'weight']
