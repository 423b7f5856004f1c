"""tests/image_ops_ref.py (the references of tests/test_gpu_image_ops_large.py) at small shapes against
what already pins the operations: the oracle's regularizers and roll, the reference's own Adam vectors."""

import numpy as np
import pytest

from oracle import num_ops
from oracle.tile_path import regularizer_loss_grad
from tests import image_ops_ref as ref
from tests.gpu_helpers import max_rel

MEAN = np.float32((103.939, 116.779, 123.68)).reshape(3, 1, 1)


def test_reduction_geometry_at_the_grid_cap():
    assert [ref.reduction_blocks(n) for n in (1, 256, 257, 262144, 262145)] == [1, 1, 2, 1024, 1024]
    assert [ref.terms_per_thread(n) for n in (1, 257, 262144, 262145, 2097153, 4200003)] == [1, 1, 1, 2, 9, 17]
    # k of the bound: (terms per thread) + 1 + 6 + 3
    assert ref.sum_bound(np.ones(262145)) == pytest.approx(12 * 2.0 ** -24 * 262145, rel=1e-15)


def test_block_sums_follow_the_grid_stride_loop():
    rng = np.random.RandomState(0)
    for n in (1, 300, 262144 + 777):
        t = rng.randint(-9, 10, n).astype(np.float32)
        blocks = ref.reduction_blocks(n)
        sums = np.zeros(blocks)
        np.add.at(sums, (np.arange(n) // 256) % blocks, np.abs(t))
        assert ref.max_block_abs_sum(t) == sums.max()
    assert ref.int_sum(np.float32([3, -8, 2])) == -3
    with pytest.raises(AssertionError):
        ref.int_sum(np.float32([0.5]))


def test_step_stats_terms_are_the_tv_norm_terms():
    rng = np.random.RandomState(1)
    avg = rng.uniform(-1, 1, (3, 7, 9)).astype(np.float32)
    old = rng.uniform(-1, 1, (3, 7, 9)).astype(np.float32)
    upd, tv = ref.step_stats_terms(avg, old)
    assert np.array_equal(upd, np.abs(avg - old))
    # num_utils.tv_norm with beta = 2 sums xdiff^2 + ydiff^2 + EPS
    loss, _ = num_ops.tv_loss_grad(avg, beta=2)
    assert float(tv.sum(dtype=np.float64)) + avg.size * ref.EPS == pytest.approx(loss, rel=1e-6)


@pytest.mark.parametrize('roll', [(0, 0), (-24, 40), (8, -16)])
def test_shifted_aux_and_p_aux_gradient_against_the_oracle(roll):
    rng = np.random.RandomState(2)
    img = rng.uniform(-120, 130, (3, 13, 17)).astype(np.float32)
    aux = rng.uniform(-120, 130, (3, 13, 17)).astype(np.float32)
    g0 = rng.standard_normal(img.shape).astype(np.float32)
    met = ref.shifted_aux(aux, roll)
    assert np.array_equal(met, num_ops.roll_xy(aux.copy(), (-roll[0], -roll[1])))
    y, x = 5, 11
    assert met[1, y, x] == aux[1, (y + roll[1]) % 13, (x + roll[0]) % 17]
    want = g0.copy()
    regularizer_loss_grad(img, MEAN, want, 0.7, 0.0, 2.0, 2.0, 6.0, met, 10.0)
    got = ref.p_aux_grad32(img, MEAN, g0, 0.7 * 2.0, 6.0, aux, 0.7 * 10.0, roll)
    assert got.dtype == np.float32
    assert max_rel(got, want) < 1e-6


def test_roll_add_is_roll_xy():
    rng = np.random.RandomState(3)
    src = rng.standard_normal((4, 6, 5)).astype(np.float32)
    a = np.float32(1 / 3)
    got = ref.roll_add32(src, [((2, -1), 0.0, 3.0), ((-7, 4), 1 / 3, 0.0)])
    want = num_ops.roll_xy(src.copy(), (2, -1)) / np.float32(3) + a * num_ops.roll_xy(src.copy(), (-7, 4))
    assert got.dtype == np.float32
    assert max_rel(got, want) < 2e-7        # (the sum's terms are added the other way round)
    assert np.array_equal(ref.roll_add32(src, [((2, -1), 0.0, 3.0)]),
                          num_ops.roll_xy(src.copy(), (2, -1)) / np.float32(3))


def test_lbfgs_pieces():
    rng = np.random.RandomState(4)
    g_new, g_old, s, z = [rng.standard_normal(50).astype(np.float32) for _ in range(4)]
    y, sy, yy = ref.lbfgs_pair_ref(g_new, g_old, s)
    assert np.array_equal(y, g_new - g_old)
    assert sy.sum() == pytest.approx(float(np.dot(np.float64(s), np.float64(y))), rel=1e-12)
    assert yy.sum() == pytest.approx(float(np.dot(np.float64(y), np.float64(y))), rel=1e-12)
    assert ref.dev_coef(1.0, 6.0, 2.0) == 3 and ref.dev_coef(1.0, 6.0, 2.0, -1.0, 10.0, 2.0) == -2
    assert ref.dev_scale(4.0, 2.0, 1.0) == 2
    f, g = ref.dev_coef(1.0, 0.3, 7.0), ref.dev_scale(0.9, 1.7, 3.0)
    v, terms = ref.axpy_dot_dev_ref(f, g_new, g_old, z, g)
    assert v.dtype == np.float32
    want = (0.9 / (1.7 / 3.0)) * (0.3 / 7.0 * np.float64(g_new) + g_old)
    assert max_rel(v, want) < 3e-7
    assert terms.sum() == pytest.approx(float(np.dot(np.float64(z), np.float64(v))), rel=1e-12)


def test_adam_scalars():
    for step in (1, 2, 7):
        lr, c1, c2, cp = ref.adam_scalars(step, 15, 0.9, 0.999, 0.95, 0.05, 0.5, False)
        assert lr == pytest.approx(15 / (1 + 0.05 * (step - 1)) ** 0.5, rel=1e-12)
        assert (c1, c2, cp) == pytest.approx((1 - 0.9 ** step, 1 - 0.999 ** step, 1 - 0.95 ** step), rel=1e-12)
        assert ref.adam_scalars(step, 15, 0.9, 0.999, 0.95, 0.05, 0.5, True)[1] == 1


@pytest.mark.parametrize('biased', [0, 1])
def test_adam_restatements_follow_the_reference_trajectory(golden, biased):
    """optimizers.AdamOptimizer on the quadratic of tests/golden/make_golden.py; the rolls of that
    trajectory are no-ops on un-rolled state (every operation is elementwise)."""
    target = golden['opt.target']
    for step_fn in (ref.adam_step32, lambda *a: ref.adam_step64(*a)[0]):
        state = {'params': golden['opt.x0'].copy(), 'g1': np.zeros_like(target), 'g2': np.zeros_like(target),
                 'p1': np.zeros_like(target)}
        for i in range(len(golden['opt.rolls'])):
            lr, c1, c2, cp = ref.adam_scalars(i + 1, 15, 0.9, 0.999, 1 - 1 / 20, 0.05, 0.5, bool(biased))
            d = state['params'] - target
            assert float(np.sum(d * d, dtype=np.float64)) == pytest.approx(
                golden['opt.adam_biased%d.loss' % biased][i], rel=1e-5)
            grad = (2 * d).astype(np.float32)
            state = step_fn(state['params'], grad, state['g1'], state['g2'], state['p1'], lr, 0.9, 0.999,
                            1 - 1 / 20, c1, c2, cp)
            assert max_rel(state['avg'], golden['opt.adam_biased%d.avg' % biased][i]) < 5e-6
        assert max_rel(state['params'], golden['opt.adam_biased%d.params' % biased]) < 5e-6


def test_adam_float32_restatement_stays_within_the_worst_case_of_its_roundings():
    """The derivation in adam_step64's docstring, held on the CPU: numpy's float32 operations round
    once each, like the kernel's."""
    rng = np.random.RandomState(5)
    n = 20000
    state = [rng.uniform(-130, 130, n), rng.standard_normal(n) * 30, rng.standard_normal(n) * 10,
             rng.uniform(0.01, 900, n), rng.uniform(-130, 130, n)]
    state = [v.astype(np.float32) for v in state]
    consts = ref.adam_scalars(7, 2.0, 0.9, 0.999, 0.95, 0.05, 0.5, False)
    args = state + [consts[0], 0.9, 0.999, 0.95] + list(consts[1:])
    got = ref.adam_step32(*args)
    values, bound, worst = ref.adam_step64(*args)
    for k in values:
        assert got[k].dtype == np.float32
        # (second-order terms and the sum's own rounding: 1 %)
        assert np.all(np.abs(got[k] - values[k]) <= 1.01 * worst[k]), k
    for k in ('g1', 'g2'):
        assert np.all(worst[k] <= bound[k])
