"""The full-image kernels of image_ops.hip past their grid caps -- the second and later passes of the
grid-stride loops, the incremental (x, y, c) walk of pos3_advance, finish_partials_kernel with more
than 256 partials, tile_move4_kernel with more lanes than its grid, tile_move_kernel on a tile wider
than 2048 -- at the smallest shapes that reach them.

Sums are held exactly where that is possible: small integers held as float32 make every product,
every thread's, wave's and workgroup's sum and the double finish exact, so one element dropped, read
twice or paired with the wrong neighbour changes the result (the condition, every workgroup's sum of
|terms| below 2^24, is asserted from the reference data).  Float-valued sums are held to k * 2^-24 *
sum |term| with k from the accumulation structure (tests/image_ops_ref.py: sum_bound; the TV term of
the step statistics carries two roundings inside the term where the other sums carry one, and is
held to the same k).  Element-wise kernels, moves and maps are held bit for bit: image_ops.hip is
built with -ffp-contract=off.  Lines starting with `BOUND` report each bounded comparison's largest
error beside its bound (pytest -s).
"""

import ctypes
import functools

import numpy as np
import pytest

from oracle import num_ops
from oracle.tile_path import regularizer_loss_grad
from style_transfer_amd import image_ops, lib
from tests import image_ops_ref as ref
from tests.gpu_helpers import gpu_engine, max_rel

pytestmark = pytest.mark.gpu
MEAN = np.float32((103.939, 116.779, 123.68)).reshape(3, 1, 1)
SENTINEL = np.float32(-7777.25)
GUARD = 64                                      # floats behind every output, preset to SENTINEL
NMAX = 4200003
# wave and workgroup edges, the reductions' grid cap (1024 x 256) on both sides, ragged passes
NS_SUM = (1, 63, 64, 255, 256, 257, 262143, 262144, 262145, 2097153, 4200003)
NS_PAIR = (262145, 4200003)
# the element-wise grid cap (8192 x 256) on both sides
NS_ELEM = (1, 257, 2097152, 2097153, 4200003)
STATS_SHAPES = ((431, 613), (181, 1021), (2, 150001), (70001, 2))   # x carry, y carry, sc >= 1, long row
_DEVICE = {}


def report(what, err, bound):
    print('BOUND %s: error %.4g, bound %.4g, ratio %.3f' % (what, err, bound, err / bound if bound else 0.0))


# ------------------------------------------------------------------------------ shared vectors
@functools.lru_cache(maxsize=None)
def vectors(kind):
    """Four host vectors of NMAX floats, 'int' (integers of [-8, 8]) or 'normal'; never written."""
    rng = np.random.RandomState(21 if kind == 'int' else 22)
    out = {}
    for name in 'xyzw':
        v = ref.small_ints(rng, NMAX) if kind == 'int' else rng.standard_normal(NMAX).astype(np.float32)
        v.setflags(write=False)
        out[name] = v
    return out


@functools.lru_cache(maxsize=None)
def prefix_sums(kind):
    """Running float64 sums of x y, |x y| and |x| (exact for 'int'): [n - 1] is the sum over n."""
    v = vectors(kind)
    xy = v['x'].astype(np.float64) * v['y'].astype(np.float64)
    return {'dot': np.cumsum(xy), 'abs_dot': np.cumsum(np.abs(xy)),
            'abs': np.cumsum(np.abs(v['x'].astype(np.float64)))}


def device_vectors(eng, kind):
    """The same vectors on the GPU, uploaded once; kernels only read them."""
    if kind not in _DEVICE:
        _DEVICE[kind] = {k: eng.to_device(v) for k, v in vectors(kind).items()}
    return _DEVICE[kind]


def guarded(eng, host, n):
    """host[:n] on the GPU with GUARD sentinels behind it."""
    return eng.to_device(np.concatenate([np.ravel(host)[:n], np.full(GUARD, SENTINEL, np.float32)]))


def check_guarded(dev, want, what):
    got = dev.get()
    n = got.size - GUARD
    assert np.array_equal(got[:n], np.ravel(want)), what
    assert np.all(got[n:] == SENTINEL), what + ': wrote past its end'


def assert_exact_sum(terms):
    """The condition under which an integer-valued reduction is exact in float32."""
    assert ref.max_block_abs_sum(terms) < 2 ** 24


# --------------------------------------------------------- 1, 2: dot, |x|, mean |x|: exact / bounded
def dot_family(eng, d, n):
    """(stx_vec_dot, stx_vec_dot_async, stx_vec_abs_sum_async, stx_vec_mean_abs) over n elements."""
    sc = image_ops.DeviceScalars(eng, 2)
    out, mean = ctypes.c_double(), ctypes.c_double()
    lib.call('stx_vec_dot', eng.handle, d['x'].ptr, d['y'].ptr, n, ctypes.byref(out))
    lib.call('stx_vec_dot_async', eng.handle, d['x'].ptr, d['y'].ptr, n, sc.ptr(0))
    lib.call('stx_vec_abs_sum_async', eng.handle, d['x'].ptr, n, sc.ptr(1))
    lib.call('stx_vec_mean_abs', eng.handle, d['x'].ptr, n, ctypes.byref(mean))
    dev = sc.array.get()
    sc.free()
    return out.value, dev[0], dev[1], mean.value


@pytest.mark.parametrize('n', NS_SUM)
def test_dot_and_abs_sums_are_exact_on_small_integers(n):
    eng = gpu_engine()
    v, sums = vectors('int'), prefix_sums('int')
    assert_exact_sum(v['x'][:n] * v['y'][:n])
    want_dot, want_abs = sums['dot'][n - 1], sums['abs'][n - 1]
    assert want_dot == ref.int_sum(v['x'][:n] * v['y'][:n]) and want_abs == ref.int_sum(np.abs(v['x'][:n]))
    dot, dot_async, abs_async, mean_abs = dot_family(eng, device_vectors(eng, 'int'), n)
    assert dot == want_dot
    assert dot_async == want_dot
    assert abs_async == want_abs
    assert mean_abs == pytest.approx(want_abs / n, rel=1e-12)


@pytest.mark.parametrize('n', NS_SUM)
def test_dot_and_abs_sums_within_the_bound_of_their_accumulation(n):
    eng = gpu_engine()
    sums = prefix_sums('normal')
    k = ref.terms_per_thread(n) + 1 + 6 + 3
    dot, dot_async, abs_async, mean_abs = dot_family(eng, device_vectors(eng, 'normal'), n)
    bound_dot, bound_abs = k * ref.U * sums['abs_dot'][n - 1], k * ref.U * sums['abs'][n - 1]
    assert dot == dot_async
    report('dot n=%d' % n, abs(dot - sums['dot'][n - 1]), bound_dot)
    report('abs_sum n=%d' % n, abs(abs_async - sums['abs'][n - 1]), bound_abs)
    assert abs(dot - sums['dot'][n - 1]) <= bound_dot
    assert abs(abs_async - sums['abs'][n - 1]) <= bound_abs
    assert mean_abs == pytest.approx(abs_async / n, rel=1e-15)


# ------------------------------------------------------------------------- 1, 2: stx_vec_lbfgs_pair
@pytest.mark.parametrize('n', NS_PAIR)
@pytest.mark.parametrize('kind', ['int', 'normal'])
def test_lbfgs_pair_sums_and_arrays(kind, n):
    eng = gpu_engine()
    v, d = vectors(kind), device_vectors(eng, kind)
    y_want, sy_terms, yy_terms = ref.lbfgs_pair_ref(v['x'][:n], v['z'][:n], v['y'][:n])
    g_old, y = guarded(eng, v['z'], n), guarded(eng, v['w'], n)
    sc = image_ops.DeviceScalars(eng, 2)
    sy = ctypes.c_double()
    lib.call('stx_vec_lbfgs_pair', eng.handle, d['x'].ptr, g_old.ptr, d['y'].ptr, y.ptr, n, sc.ptr(0),
             ctypes.byref(sy))
    got = sc.array.get()
    assert sy.value == got[0]
    if kind == 'int':
        assert_exact_sum(sy_terms)
        assert_exact_sum(yy_terms)
        assert got[0] == ref.int_sum(sy_terms)
        assert got[1] == ref.int_sum(yy_terms)
    else:
        for name, value, terms in (('s.y', got[0], sy_terms), ('y.y', got[1], yy_terms)):
            report('lbfgs_pair %s n=%d' % (name, n), abs(value - terms.sum()), ref.sum_bound(terms))
            assert abs(value - terms.sum()) <= ref.sum_bound(terms)
    check_guarded(y, y_want, 'y')
    check_guarded(g_old, v['x'][:n], 'g_old')
    for a in (g_old, y, sc):
        a.free()


# ----------------------------------------------------------------------- 1, 2: stx_vec_axpy_dot_dev
@pytest.mark.parametrize('n', NS_PAIR)
@pytest.mark.parametrize('kind', ['int', 'normal'])
def test_axpy_dot_dev_variants(kind, n):
    """With and without b, src = y and src distinct, scaled and unscaled: y bit for bit, <z, y> exact
    (integers: f = 3 or -2, g = 2) or within the bound."""
    eng = gpu_engine()
    v, d = vectors(kind), device_vectors(eng, kind)
    a, da, b, db, c2, c_s, den, div = ((6.0, 2.0, 10.0, 2.0, -1.0, 4.0, 2.0, 1.0) if kind == 'int' else
                                       (0.3, 7.0, 1.9, 3.0, -1.0, 0.9, 1.7, 3.0))
    sc = image_ops.DeviceScalars(eng, 4)
    sc.array.set(np.float64([a, b, den, 0.0]))
    for with_b in (False, True):
        f = ref.dev_coef(1.0, a, da, c2, b if with_b else None, db)
        for distinct in (False, True):
            for scaled in (False, True):
                what = 'axpy_dot_dev %s n=%d b=%d src=%d scaled=%d' % (kind, n, with_b, distinct, scaled)
                src = v['w'] if distinct else v['z']
                want, terms = ref.axpy_dot_dev_ref(f, v['x'][:n], src[:n], v['y'][:n],
                                                   ref.dev_scale(c_s, den, div) if scaled else None)
                y = guarded(eng, v['z'], n)
                lib.call('stx_vec_axpy_dot_dev', eng.handle, 1.0, sc.ptr(0), da, c2,
                         sc.ptr(1) if with_b else None, db, c_s, sc.ptr(2) if scaled else None, div,
                         d['x'].ptr, d['w'].ptr if distinct else y.ptr, y.ptr, d['y'].ptr, n, sc.ptr(3))
                got = sc.array.get()[3]
                if kind == 'int':
                    assert_exact_sum(terms)
                    assert got == ref.int_sum(terms), what
                else:
                    report(what, abs(got - terms.sum()), ref.sum_bound(terms))
                    assert abs(got - terms.sum()) <= ref.sum_bound(terms), what
                check_guarded(y, want, what)
                y.free()
    sc.free()


# ------------------------------------------------------------------ 1, 2: the step statistics' walk
@pytest.mark.parametrize('hw', STATS_SHAPES)
@pytest.mark.parametrize('kind', ['int', 'normal'])
def test_step_stats_sums_through_the_incremental_walk(kind, hw):
    eng = gpu_engine()
    rng = np.random.RandomState(hw[0])
    shape = (3,) + hw
    if kind == 'int':
        avg, old = ref.small_ints(rng, shape), ref.small_ints(rng, shape)
    else:
        avg, old = [rng.standard_normal(shape).astype(np.float32) for _ in range(2)]
    n = avg.size
    upd_terms, tv_terms = ref.step_stats_terms(avg, old)
    d_avg, d_old, d_old2 = eng.to_device(avg), eng.to_device(old), eng.to_device(old)
    upd, tv = image_ops.step_stats(eng, d_avg, d_old)
    lazy = image_ops.step_stats_async(eng, d_avg, d_old2)
    eng.wait_fence(eng.fence())
    raw = lazy._raw[0], lazy._raw[1]
    if kind == 'int':
        assert_exact_sum(upd_terms)
        assert_exact_sum(tv_terms)
        assert raw == (ref.int_sum(upd_terms), ref.int_sum(tv_terms))
        assert upd == pytest.approx(ref.int_sum(upd_terms) / n, rel=1e-12)
        assert tv == pytest.approx(np.sqrt(ref.int_sum(tv_terms) / n), rel=1e-12)
    else:
        for name, value, terms in (('update', raw[0], upd_terms), ('tv', raw[1], tv_terms)):
            report('step_stats %s %dx%d' % (name, hw[0], hw[1]), abs(value - terms.sum()), ref.sum_bound(terms))
            assert abs(value - terms.sum()) <= ref.sum_bound(terms)
    assert lazy.values() == (upd, tv)
    assert np.array_equal(d_old.get(), avg)
    assert np.array_equal(d_old2.get(), avg)
    assert np.array_equal(d_avg.get(), avg)


# ----------------------------------------------------------------- 3: element-wise, bit for bit
@pytest.mark.parametrize('n', NS_ELEM)
def test_elementwise_kernels_bit_for_bit_past_their_grid(n):
    eng = gpu_engine()
    v, d = vectors('normal'), device_vectors(eng, 'normal')
    f = np.float32
    x, y0 = v['x'][:n], v['y'][:n]
    sc = image_ops.DeviceScalars(eng, 3)
    sc.array.set(np.float64([0.3, 1.9, 1.7]))

    y = guarded(eng, y0, n)
    lib.call('stx_vec_axpy', eng.handle, -0.37, d['x'].ptr, y.ptr, n)
    check_guarded(y, f(-0.37) * x + y0, 'axpy')
    lib.call('stx_vec_scale', eng.handle, 1.7, y.ptr, n)
    check_guarded(y, f(1.7) * (f(-0.37) * x + y0), 'scale')
    y.free()

    for with_b in (False, True):
        y = guarded(eng, y0, n)
        lib.call('stx_vec_axpy_dev', eng.handle, -1.0, sc.ptr(0), 7.0, 1.0, sc.ptr(1) if with_b else None, 3.0,
                 d['x'].ptr, y.ptr, n)
        check_guarded(y, ref.dev_coef(-1.0, 0.3, 7.0, 1.0, 1.9 if with_b else None, 3.0) * x + y0,
                      'axpy_dev b=%d' % with_b)
        y.free()

    y = guarded(eng, y0, n)
    lib.call('stx_vec_scale_dev', eng.handle, 0.9, sc.ptr(2), float(n), y.ptr, n)
    check_guarded(y, ref.dev_scale(0.9, 1.7, float(n)) * y0, 'scale_dev')
    y.free()

    s, p = guarded(eng, y0, n), guarded(eng, v['z'], n)
    lib.call('stx_vec_scale2_axpy', eng.handle, -1.0, 0.3, s.ptr, p.ptr, n)
    s_want = f(0.3) * (f(-1.0) * y0)
    check_guarded(s, s_want, 'scale2_axpy s')
    check_guarded(p, f(1.0) * s_want + v['z'][:n], 'scale2_axpy params')
    for a in (s, p, sc):
        a.free()


def test_vector_calls_refuse_an_empty_vector():
    """n == 0 is STX_ERR_ARG before any launch, in every stx_vec_* call and in stx_adam_step."""
    eng = gpu_engine()
    a = [guarded(eng, np.ones(4, np.float32), 4) for _ in range(6)]
    sc = image_ops.DeviceScalars(eng, 2)
    sc.array.set(np.float64([1.0, 1.0]))
    out = ctypes.c_double()
    h, p = eng.handle, [arr.ptr for arr in a]
    calls = [('stx_vec_dot', h, p[0], p[1], 0, ctypes.byref(out)),
             ('stx_vec_mean_abs', h, p[0], 0, ctypes.byref(out)),
             ('stx_vec_dot_async', h, p[0], p[1], 0, sc.ptr(0)),
             ('stx_vec_abs_sum_async', h, p[0], 0, sc.ptr(0)),
             ('stx_vec_axpy', h, 1.0, p[0], p[1], 0),
             ('stx_vec_scale', h, 2.0, p[0], 0),
             ('stx_vec_axpy_dev', h, 1.0, sc.ptr(0), 1.0, 0.0, None, 1.0, p[0], p[1], 0),
             ('stx_vec_scale_dev', h, 1.0, sc.ptr(0), 1.0, p[0], 0),
             ('stx_vec_axpy_dot_dev', h, 1.0, sc.ptr(0), 1.0, 0.0, None, 1.0, 0.0, None, 1.0, p[0], p[1], p[1],
              p[2], 0, sc.ptr(1)),
             ('stx_vec_lbfgs_pair', h, p[0], p[1], p[2], p[3], 0, sc.ptr(0), ctypes.byref(out)),
             ('stx_vec_scale2_axpy', h, 1.0, 1.0, p[0], p[1], 0),
             ('stx_adam_step', h, p[0], p[1], p[2], p[3], p[4], p[5], 0, 1.0, 0.9, 0.999, 0.0, 0.1, 0.001, 1.0)]
    assert {c[0] for c in calls} == {k for k in lib.SIGNATURES if k.startswith('stx_vec_')} | {'stx_adam_step'}
    for call in calls:
        with pytest.raises(lib.StxError) as err:
            lib.call(*call)
        assert err.value.code == -1, call[0]            # STX_ERR_ARG
    for arr in a:
        check_guarded(arr, np.ones(4, np.float32), 'untouched')
    assert np.array_equal(sc.array.get(), [1.0, 1.0])


# ------------------------------------------------------------------------------------- 3: Adam
ADAM = dict(step_size=2.0, b1=0.9, b2=0.999, bp1=0.95, decay=0.05, power=0.5)


@pytest.mark.parametrize('n', NS_ELEM[-2:])
@pytest.mark.parametrize('biased', [0, 1])
def test_adam_step_against_float64_from_the_same_state(biased, n):
    """Seven updates on the GPU; the first and the seventh are compared with float64 evaluated from
    the state the kernel itself left before them: every output within 8 * 2^-24 * S (adam_step64).

    The data keep that bound sound, which is asserted from the reference: |params| starts in
    [48, 130] and moves by at most 2 * 2 a step, so it stays away from zero; an element's gradients
    share one magnitude (times 0.5 .. 1, either sign), which keeps the moments' ratio R <= 2 and g2
    far from subnormals."""
    eng = gpu_engine()
    rng = np.random.RandomState(31 + biased)
    params0 = (rng.uniform(48, 130, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    magnitude = np.exp(rng.uniform(-1, 1, n))
    base = (magnitude * rng.uniform(0.5, 1, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    names = ('params', 'grad', 'g1', 'g2', 'p1', 'avg')
    zero = np.zeros(n, np.float32)
    dev = {k: guarded(eng, params0 if k == 'params' else zero, n) for k in names}
    for step in range(1, 8):
        grad = np.roll(base, 9973 * step) * np.float32(1 if step % 2 else -1)
        dev['grad'].free()
        dev['grad'] = guarded(eng, grad, n)
        lr, c1, c2, cp = ref.adam_scalars(step, biased_g1=bool(biased), **ADAM)
        checked = step in (1, 7)
        if checked:
            state = [dev[k].get()[:n] for k in ('params', 'grad', 'g1', 'g2', 'p1')]
            dev['avg'].free()
            dev['avg'] = guarded(eng, np.full(n, SENTINEL), n)       # written only: every element must be
        lib.call('stx_adam_step', eng.handle, *[dev[k].ptr for k in names], n, lr, ADAM['b1'], ADAM['b2'],
                 ADAM['bp1'], c1, c2, cp)
        if not checked:
            continue
        args = state + [lr, ADAM['b1'], ADAM['b2'], ADAM['bp1'], c1, c2, cp]
        values, bound, worst = ref.adam_step64(*args)
        restated = ref.adam_step32(*args)
        identical = True
        assert not np.any(dev['avg'].get()[:n] == SENTINEL), 'elements the step never reached'
        for k in values:
            got = dev[k].get()
            assert np.all(got[n:] == SENTINEL), k
            got = got[:n]
            assert np.all(worst[k] <= bound[k]), 'the data do not support the bound of ' + k
            err = np.abs(got - values[k])
            worst_at = int(np.argmax(err / bound[k]))
            report('adam %s n=%d biased=%d step=%d' % (k, n, biased, step), err[worst_at], bound[k][worst_at])
            assert np.all(err <= bound[k]), k
            identical = identical and np.array_equal(got, restated[k])
        print('adam n=%d biased=%d step=%d: bit-identical to the float32 restatement: %s'
              % (n, biased, step, identical))
        check_guarded(dev['grad'], grad, 'grad')
    for a in dev.values():
        a.free()


# ---------------------------------------------------- 4: regularizers and Haar through the walk
def _uniform_images(seed, shape, count):
    rng = np.random.RandomState(seed)
    return [rng.uniform(-120, 130, shape).astype(np.float32) for _ in range(count)] + \
        [rng.standard_normal(shape).astype(np.float32)]


@pytest.mark.parametrize('hw,tv_power,p_power,aux_roll', [((431, 613), 2.0, 6.0, (-24, 40)),
                                                          ((181, 1021), 1.5, 2.5, (8, -16)),
                                                          ((2, 150001), 2.0, 6.0, None),
                                                          ((70001, 2), 1.5, 2.5, None)])
def test_regularizers_against_oracle_past_the_grid(hw, tv_power, p_power, aux_roll):
    """(the oracle's circular differences are np.roll: it takes H = 2 and W = 2 as they are)"""
    eng = gpu_engine()
    img, aux, g0 = _uniform_images(hw[1], (3,) + hw, 2)
    met = ref.shifted_aux(aux, aux_roll) if aux_roll else None
    want = g0.copy()
    want_loss = regularizer_loss_grad(img, MEAN, want, 0.7, 5.0, tv_power, 2.0, p_power, met, 10.0)
    d_grad = eng.to_device(g0)
    res = image_ops.regularizers(eng, eng.to_device(img), d_grad, MEAN, 0.7 * 5.0, tv_power, 0.7 * 2.0, p_power,
                                 eng.to_device(aux) if aux_roll else None, 0.7 * 10.0, aux_roll)
    eng.sync()
    assert res.value == pytest.approx(want_loss, rel=1e-5)
    assert max_rel(d_grad.get(), want) < 1e-5


def test_regularizers_p_and_aux_gradient_bit_for_bit_past_the_grid():
    """Without the TV term the gradient is a few float32 operations per element (the default p = 6 by
    multiplication): every element equals numpy's, so a pixel met at the wrong (x, y, c) shows."""
    eng = gpu_engine()
    img, aux, g0 = _uniform_images(7, (3, 431, 613), 2)
    d_grad = eng.to_device(g0)
    image_ops.regularizers(eng, eng.to_device(img), d_grad, MEAN, 0.0, 2.0, 1.4, 6.0, eng.to_device(aux), 7.0,
                           (-24, 40))
    eng.sync()
    assert np.array_equal(d_grad.get(), ref.p_aux_grad32(img, MEAN, g0, 1.4, 6.0, aux, 7.0, (-24, 40)))


def test_swt_haar_term_against_oracle_past_the_grid():
    eng = gpu_engine()
    shape, roll, power, scale = (3, 431, 613), (-24, 40), 1.5, 0.37
    img, g0 = _uniform_images(8, shape, 1)
    rolled = np.roll(img, (roll[1], roll[0]), (1, 2))          # roll = (x, y)
    loss, grad = num_ops.swt_norm_haar1(rolled / np.float32(127.5), power)
    want = g0 + np.float32(scale) * np.roll(grad, (-roll[1], -roll[0]), (1, 2))
    d_grad = eng.to_device(g0)
    out = image_ops.swt_haar(eng, eng.to_device(img), d_grad, scale, power, roll=roll)
    eng.sync()
    assert out.value == pytest.approx(scale * loss, rel=2e-5)
    assert np.abs(d_grad.get() - want).max() <= 2e-5 * np.abs(want).max()


# ------------------------------------------------------------- 5: moves and maps past their grids
@pytest.mark.parametrize('shape,rect,rolls', [
    # 16-byte path: 3 * 1100 rows of 320 padded lanes = 1 056 000 against the grid's 1 048 576; the
    # second shift puts the tile's first source column at 1000, so the wrap falls inside the tile
    ((3, 1104, 1040), (0, 1100, 8, 1036), [(-52, 37), (48, -300)]),
    # dword path: a tile of 2051 columns against 8 workgroups of 256 per row
    ((3, 5, 2100), (1, 4, 3, 2054), [(7, -2)])])
def test_cut_and_put_tile_past_their_grids(shape, rect, rolls):
    eng = gpu_engine()
    rng = np.random.RandomState(shape[1])
    img = rng.standard_normal(shape).astype(np.float32)
    d_img = eng.to_device(img)
    y0, y1, x0, x1 = rect
    for roll in rolls:
        rolled = num_ops.roll_xy(img.copy(), roll)
        tile = guarded(eng, np.full((3, y1 - y0, x1 - x0), SENTINEL), 3 * (y1 - y0) * (x1 - x0))
        image_ops.cut_tile(eng, d_img, roll, rect, tile)
        check_guarded(tile, rolled[:, y0:y1, x0:x1], 'cut %s' % (roll,))
        # put: the tile goes back un-rolled, and nothing outside the rect changes
        full = eng.to_device(np.full(shape, SENTINEL))
        image_ops.put_tile(eng, full, roll, rect, tile)
        expect = np.full(shape, SENTINEL)
        expect[:, y0:y1, x0:x1] = rolled[:, y0:y1, x0:x1]
        assert np.array_equal(full.get(), num_ops.roll_xy(expect, (-roll[0], -roll[1]))), roll
        assert np.array_equal(d_img.get(), img)
        tile.free()
        full.free()


def _map_source():
    return np.random.RandomState(41).standard_normal((64, 182, 181)).astype(np.float32)   # 2 108 288 elements


def test_map_place_past_its_grid():
    eng = gpu_engine()
    src = _map_source()
    dst = eng.to_device(np.full((64, 190, 200), SENTINEL))
    eng.map_place(dst, 5, 13, eng.to_device(src))
    want = np.full((64, 190, 200), SENTINEL)
    want[:, 5:187, 13:194] = src
    assert np.array_equal(dst.get(), want)


def test_map_roll_add_past_its_grid():
    eng = gpu_engine()
    src = _map_source()
    d_src, acc = eng.to_device(src), guarded(eng, np.full(src.shape, SENTINEL), src.size)
    passes = [((11, -4), 0.0, 3.0), ((-7, 190), 1 / 3, 0.0), ((200, -1), 1 / 3, 0.0)]
    for roll, alpha, divisor in passes:
        lib.call('stx_map_roll_add', eng.handle, acc.ptr, d_src.ptr, 64, 182, 181, (ctypes.c_int * 2)(*roll),
                 alpha, divisor)
    check_guarded(acc, ref.roll_add32(src, passes), 'roll_add')
    assert np.array_equal(d_src.get(), src)


@pytest.mark.parametrize('shape,hw,method', [((3, 420, 500), (837, 840), 'lanczos'),
                                             ((3, 1000, 1400), (700, 1001), 'bilinear')])
def test_resample_is_bit_identical_to_pillow_past_its_grid(shape, hw, method):
    from PIL import Image
    from style_transfer_amd.resample import resample_device
    eng = gpu_engine()
    a = np.random.RandomState(hw[0]).uniform(-100, 100, shape).astype(np.float32)
    pil_method = Image.LANCZOS if method == 'lanczos' else Image.BILINEAR
    want = np.stack([np.asarray(Image.fromarray(a[c]).resize((hw[1], hw[0]), pil_method)) for c in range(3)])
    d_a = eng.to_device(a)
    assert np.array_equal(resample_device(eng, d_a, hw, method).get(), want)
    if method == 'lanczos':
        assert np.array_equal(resample_device(eng, d_a, hw, method, clamp_min_zero=True).get(), np.maximum(0, want))


def test_to_u8_past_its_grid():
    """A plane of 2 098 152 pixels; exact .0, 254.999, 255.0, -0.0 and sums within one ulp of an
    integer sit at the head of every plane and at its tail, which the last pass converts."""
    eng = gpu_engine()
    rng = np.random.RandomState(51)
    img = rng.uniform(-300, 400, (3, 1449, 1448)).astype(np.float32)
    flat = img.reshape(3, -1)
    for c in range(3):
        m = MEAN[c, 0, 0]
        at = np.float32([0.0, 1.0, 37.0, 128.0, 254.0, 254.999, 255.0, 256.0, -1.0]) - m     # img + mean near these
        seeds = np.concatenate([at, np.nextafter(at, np.float32(np.inf)), np.nextafter(at, np.float32(-np.inf)),
                                np.float32([-0.0, 0.0, 255.0, 254.999, -m])])
        flat[c, :seeds.size] = seeds
        flat[c, -seeds.size:] = seeds
    assert np.array_equal(image_ops.to_u8(eng, eng.to_device(img), MEAN), ref.to_u8_ref(img, MEAN))
