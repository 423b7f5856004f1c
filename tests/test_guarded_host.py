"""tests/guarded.py would fail: numpy stand-ins for a kernel on the harness's own layout, one correct and one per
way of leaving an array, each reported with its kind and its offset (no GPU)."""

import numpy as np
import pytest

from tests import guarded

C, H, W = 3, 5, 7
N = C * H * W


def _operands(offset=0, untouched=None):
    """x [C, H, W] and y [C, H, W] under plane guards -> (bookkeeping, the flat arrays and where their bodies start)."""
    g = guarded.HostGuarded()
    x = np.random.RandomState(0).standard_normal((C, H, W)).astype(np.float32)
    xf, xs = g.input('x', x, offset=offset)
    yf, ys = g.output('y', (C, H, W), offset=offset, untouched=untouched)
    return g, xf, xs.start, yf, ys.start


def _correct(xf, x0, yf, y0):
    yf[y0:y0 + N] = 2 * xf[x0:x0 + N]


def test_the_layout():
    for offset in (0, 4, 8):
        g, xf, x0, yf, y0 = _operands(offset)
        assert x0 >= guarded.plane_guard(H, W) and (4 * x0 - offset) % 16 == 0
        assert len(xf) - x0 - N == guarded.plane_guard(H, W) == H * W + 1024
        words = xf.view(np.uint32)
        assert np.all(words[:x0] == guarded.IN_NAN) and np.all(words[x0 + N:] == guarded.IN_NAN)
        assert np.all(np.isfinite(xf[x0:x0 + N])) and np.all(np.isnan(xf[:x0]))
        assert np.all(yf.view(np.uint32) == guarded.OUT_NAN) and np.all(np.isnan(yf))
    flat = guarded.layout(np.zeros(5, np.int8), guarded.FLAT_GUARD, 'output')
    assert flat.dtype == np.int8 and len(flat) == 2 * 1024 + 5 and np.all(flat.view(np.uint8) == guarded.OUT_BYTE)
    assert guarded.default_guard((4, 9)) == guarded.default_guard((64, 3, 3, 3)) == 1024
    assert guarded.IN_NAN != guarded.OUT_NAN and guarded.IN_BYTE != guarded.OUT_BYTE


@pytest.mark.parametrize('offset', [0, 4, 8])
def test_a_correct_stand_in_passes(offset):
    g, xf, x0, yf, y0 = _operands(offset)
    _correct(xf, x0, yf, y0)
    assert g.findings() == []


def test_one_float_behind_the_body():
    g, xf, x0, yf, y0 = _operands()
    _correct(xf, x0, yf, y0)
    yf[y0 + N] = 1.0
    assert g.findings() == [guarded.Finding('a', 'y', N, 1)]


def test_one_float_in_front_of_the_body():
    g, xf, x0, yf, y0 = _operands()
    _correct(xf, x0, yf, y0)
    yf[y0 - 1] = 1.0
    assert g.findings() == [guarded.Finding('a', 'y', -1, 1)]


def test_a_whole_surplus_plane():
    g, xf, x0, yf, y0 = _operands()
    _correct(xf, x0, yf, y0)
    yf[y0 + N:y0 + N + H * W] = 0.5                 # channel C of a ragged channel tile
    assert g.findings() == [guarded.Finding('a', 'y', N, H * W)]


def test_a_surplus_patch_row_of_the_last_channel():
    g, xf, x0, yf, y0 = _operands()
    _correct(xf, x0, yf, y0)
    yf[y0 + N + W:y0 + N + 2 * W] = 0.5             # row H + 1 of the last plane
    assert g.findings() == [guarded.Finding('a', 'y', N + W, W)]


def test_one_element_unwritten():
    g, xf, x0, yf, y0 = _operands()
    _correct(xf, x0, yf, y0)
    yf.view(np.uint32)[y0 + 17] = guarded.OUT_NAN
    assert g.findings() == [guarded.Finding('b', 'y', 17, 1)]


def test_accumulating_into_the_output():
    g, xf, x0, yf, y0 = _operands()
    yf[y0:y0 + N] += 2 * xf[x0:x0 + N]              # y += ... on poison
    # NaN + finite is a NaN; hardware that hands the operand's payload on leaves the poison itself (b), any other
    # leaves another NaN (d).  Which one this machine does is asked of it, not assumed:
    probe = np.array([guarded.OUT_NAN], np.uint32).view(np.float32) + np.float32(1)
    kind = 'b' if probe.view(np.uint32)[0] == guarded.OUT_NAN else 'd'
    assert g.findings() == [guarded.Finding(kind, 'y', 0, N)]


def test_one_flipped_bit_of_an_input():
    g, xf, x0, yf, y0 = _operands()
    _correct(xf, x0, yf, y0)
    xf.view(np.uint32)[x0 + 40] ^= 1
    assert g.findings() == [guarded.Finding('c', 'x', 40, 1)]
    g, xf, x0, yf, y0 = _operands()
    _correct(xf, x0, yf, y0)
    xf[x0 - 3] = 0.0                                # an input's guard counts too
    assert g.findings() == [guarded.Finding('c', 'x', -3, 1)]


def test_a_stray_read_times_zero():
    g, xf, x0, yf, y0 = _operands()
    _correct(xf, x0, yf, y0)
    with np.errstate(invalid='ignore'):
        yf[y0] += np.float32(0) * xf[x0 - 1]        # x[-1], "multiplied by a zero weight"
    assert g.findings() == [guarded.Finding('d', 'y', 0, 1)]
    g, xf, x0, yf, y0 = _operands()
    _correct(xf, x0, yf, y0)
    with np.errstate(invalid='ignore'):
        yf[y0 + N - 1] += np.float32(0) * xf[x0 + N]        # ... and the element behind the last
    assert g.findings() == [guarded.Finding('d', 'y', N - 1, 1)]


def test_an_output_documented_as_partly_written():
    keep = np.zeros((C, H, W), bool)
    keep[:, ::2, ::2] = True
    g, xf, x0, yf, y0 = _operands(untouched=keep)
    y = yf[y0:y0 + N].reshape(C, H, W)
    y[~keep] = 1.0
    assert g.findings() == []
    y[0, 0, 2] = 1.0                                # an element of the untouched set
    assert g.findings() == [guarded.Finding('e', 'y', 2, 1)]
    g, xf, x0, yf, y0 = _operands(untouched=keep)
    y = yf[y0:y0 + N].reshape(C, H, W)
    y[~keep] = 1.0
    y.view(np.uint32)[0, 0, 1] = guarded.OUT_NAN    # an element of the written set left alone
    assert g.findings() == [guarded.Finding('b', 'y', 1, 1)]


def test_byte_and_integer_outputs():
    g = guarded.HostGuarded()
    tf, ts = g.output('signs', (4, 4), np.int8)
    jf, js = g.output('index', (9,), np.int32)
    tf[ts.start:ts.start + 16] = -1
    jf[js.start:js.start + 9] = np.arange(9)
    assert g.findings() == []
    tf[ts.start + 16] = 0
    jf[js.start + 4:js.start + 6] = jf[0]
    assert g.findings() == [guarded.Finding('a', 'signs', 16, 1), guarded.Finding('b', 'index', 4, 2)]


def test_the_conv_rows_of_the_device_table_state_the_launchers_plan():
    """tests/test_gpu_op_memory.py's clause on its own table, without a device: it is arithmetic only."""
    from tests import test_gpu_op_memory
    test_gpu_op_memory.test_the_conv_rows_state_the_launchers_plan()


def test_the_plan_arithmetic_on_worked_examples():
    """tests/conv_plan.py against figures worked by hand from the launchers' cost models."""
    from tests import conv_plan
    # wino2_uniform_plan, 64 -> 66 at 17 x 35, 16 x 16 patches: 8 chunks, 2 x 2 x 3 = 12 items, one round either way:
    # 8 x 2.05 + 6 = 22.4 unsplit against 4 x 2.05 + 6 + 3 x 0.157 / 3 + 5 = 19.36 in two slices
    f, cost = conv_plan.wino2_uniform(1, 64, 66, 17, 35)
    assert f == 2 and abs(cost - 19.357) < 1e-2
    assert conv_plan.wino2_uniform(1, 56, 66, 17, 35) == (1, 7 * 2.05 + 6.0)           # 7 chunks: no slice keeps 4
    # h2_plan, 128 -> 130 at 9 x 33, 64 x 8 x 32: 4 pairs; 2 x 4 x 2 + 8.5 = 24.5 against 2 x 2 x 2 + 8.5 + 0.154 + 5
    assert conv_plan.h2_plan(0, 128, 130, 9, 33)[0] == 2 and conv_plan.h2_plan(0, 96, 130, 9, 33) == (1, 20.5)
    # wino2_tail_plan, 128 -> 64 at 259 x 261, 16 x 16 patches: 289 = 256 + 33 items, 4 slices, 67.6 against 77.6
    items, slices, cost = conv_plan.wino2_tail(1, 128, 64, 259, 261)
    assert (items, slices) == (33, 4) and abs(cost - 67.6) < 0.1
    assert abs(conv_plan.wino2_uniform(1, 128, 64, 259, 261)[1] - 77.6) < 1e-9
    # direct_splitk_factor: 8 chunks of 8 on a small plane -> 2; 7 chunks -> 1; variant 3 never
    assert conv_plan.direct_split(5, 64, 66, 17, 35) == 2 and conv_plan.direct_split(5, 56, 66, 17, 35) == 1
    assert conv_plan.direct_split(3, 130, 20, 13, 70) == 1


def test_every_finding_is_described():
    g, xf, x0, yf, y0 = _operands()
    yf[y0 - 1] = 1.0
    xf[x0] = 3.0
    text = guarded.describe(g.findings())
    assert '(a) y' in text and '(b) y' in text and '(c) x' in text and 'offset -1' in text
