"""References of the full-image kernels (image_ops.hip) for tests/test_gpu_image_ops_large.py: exact
integer sums, float64 sums with a bound from the accumulation structure, float32 restatements in the
kernels' operation order, and Adam in float64 with a bound per output.

The reductions share one structure (dot_kernel, lbfgs_pair_kernel, axpy_dot_dev_kernel,
step_stats_kernel, regularizers_kernel): a grid-stride loop over ``blocks_for(n)`` workgroups of 256
threads, a float accumulator per thread, six wave shuffle steps, three adds of the four wave sums,
and a finish in double.  Element i is summed by thread i % 256 of workgroup (i // 256) % blocks.
tests/test_image_ops_ref.py holds this module to the oracle and to the reference's own vectors.
"""

import numpy as np

U = 2.0 ** -24                 # the largest relative error of one float32 rounding
K_BLOCKS = 1024                # common.h: kBlocks, the cap of a reduction's grid
EPS = float(np.finfo(np.float32).eps)


# ------------------------------------------------------------------------------- the reductions
def reduction_blocks(n):
    """common.h: blocks_for(n)."""
    return min((n + 255) // 256, K_BLOCKS)


def terms_per_thread(n):
    """Most elements one thread of the grid-stride loop adds."""
    return -(-n // (256 * reduction_blocks(n)))


def sum_bound(terms, n=None):
    """k * 2^-24 * sum |term| with k = (terms per thread) + 1 + 6 + 3: the adds of a thread, the
    rounding of the term itself, the wave shuffle steps and the adds of the wave sums.  The finish is
    in double and adds nothing."""
    terms = np.asarray(terms, np.float64)
    n = terms.size if n is None else n
    return (terms_per_thread(n) + 1 + 6 + 3) * U * float(np.abs(terms).sum())


def max_block_abs_sum(terms):
    """The largest sum of |term| any one workgroup adds.  While it is below 2^24 and every term is an
    integer, every float32 partial sum of the reduction is an integer below 2^24, hence exact."""
    t = np.abs(np.asarray(terms, np.float64)).ravel()
    blocks = reduction_blocks(t.size)
    stride = 256 * blocks
    padded = np.zeros(-(-t.size // stride) * stride)
    padded[:t.size] = t
    return float(padded.reshape(-1, blocks, 256).sum(axis=(0, 2)).max())


def small_ints(rng, shape, lo=-8, hi=8):
    """Integers of [lo, hi] held as float32."""
    return rng.randint(lo, hi + 1, size=shape).astype(np.float32)


def int_sum(terms):
    """The sum of integer-valued terms, in int64."""
    t = np.asarray(terms)
    assert np.array_equal(t, np.rint(t))
    return int(t.astype(np.int64).sum())


def step_stats_terms(avg, old):
    """(|avg - old|, xdiff^2 + ydiff^2) as float64, with circular forward differences taken in the
    arrays' own type like step_stats_kernel's (style_transfer.py:808-815): the first term is the
    kernel's own value, the second its two squares and their sum without their roundings.  The
    statistics are mean(first) and sqrt(mean(second))."""
    xd = (avg - np.roll(avg, -1, axis=-1)).astype(np.float64)
    yd = (avg - np.roll(avg, -1, axis=-2)).astype(np.float64)
    return np.abs(avg - old).astype(np.float64), xd * xd + yd * yd


def lbfgs_pair_ref(g_new, g_old, s):
    """(y, terms of <s, y>, terms of <y, y>) of lbfgs_pair_kernel: y = -1 * g_old + g_new in float32,
    the terms as float64 products of the float32 values."""
    y = np.float32(-1.0) * g_old + g_new
    y64 = y.astype(np.float64)
    return y, s.astype(np.float64) * y64, y64 * y64


def dev_coef(c1, a, da, c2=0.0, b=None, db=1.0):
    """The coefficient of axpy_dev_kernel / axpy_dot_dev_kernel: formed in double, rounded once."""
    coef = a / da * c1
    if b is not None:
        coef += b / db * c2
    return np.float32(coef)


def dev_scale(c, den, den_div=1.0):
    """The factor of scale_dev_kernel (and of axpy_dot_dev_kernel's scaling)."""
    return np.float32(c / (den / den_div))


def axpy_dot_dev_ref(f, x, src, z, g=None):
    """(y, terms of <z, y>) of axpy_dot_dev_kernel: y = [g] (f x + src) in float32."""
    y = f * x + src
    if g is not None:
        y = g * y
    return y, z.astype(np.float64) * y.astype(np.float64)


# ----------------------------------------------------------------------------------------- Adam
def adam_scalars(step, step_size, b1, b2, bp1, decay, power, biased_g1):
    """(lr, c1, c2, cp) of update number ``step`` (1-based) of AdamOptimizer (optimizers.py:26-42):
    lr = step_size / i^power with i = 1 + decay (step - 1); the corrections are 1 - beta^step, and 1
    for the uncorrected first moment."""
    i = 1.0
    for _ in range(step - 1):
        i += decay
    lr = step_size / i ** power

    def corr(beta, correct=True):
        accum = 1.0 if correct else 0.0
        for _ in range(step):
            accum *= beta
        return 1 - accum
    return lr, corr(b1, not biased_g1), corr(b2), corr(bp1)


def _adam_consts(lr, b1, b2, bp1, c1, c2, cp):
    """The scalars as adam_launch hands them to the kernel: formed in double, rounded to float32."""
    return [np.float32(v) for v in (lr, b1, b2, bp1, 1.0 - b1, 1.0 - b2, 1.0 - bp1, c1, c2, cp)]


def adam_step32(params, grad, g1, g2, p1, lr, b1, b2, bp1, c1, c2, cp):
    """adam_kernel restated in numpy float32, one rounding per operation in the kernel's order.
    Returns {'params', 'g1', 'g2', 'p1', 'avg'}; the inputs are left alone."""
    lr, b1, b2, bp1, omb1, omb2, ombp1, c1, c2, cp = _adam_consts(lr, b1, b2, bp1, c1, c2, cp)
    m1 = g1 * b1 + omb1 * grad
    m2 = g2 * b2 + omb2 * (grad * grad)
    step = (m1 / c1) / (np.sqrt(m2 / c2) + np.float32(EPS))
    p = params + (-lr) * step
    a = p1 * bp1 + ombp1 * p
    return {'params': p, 'g1': m1, 'g2': m2, 'p1': a, 'avg': a / cp}


def adam_step64(params, grad, g1, g2, p1, lr, b1, b2, bp1, c1, c2, cp):
    """The same step in float64 from the same float32 state and the same float32 scalars.  Returns
    (values, bound, worst), three dicts over {'params', 'g1', 'g2', 'p1', 'avg'}:

    bound = 8 * 2^-24 * S, S the sum of the absolute values of the terms added to form the output
    (params: |p| + lr |step|) -- what the float32 kernel is held to;
    worst = the first-order worst case of the roundings on the output's path.  With t1 = g1 b1,
    t2 = (1 - b1) g, S1 = |t1| + |t2|, den = sqrt(m2 / c2) + EPS and R = S1 / (c1 den):
        m1: 2u S1                       m2: 3u m2 (all terms positive)
        step: 2u R + 6u |step|          (m1 / c1: +u; m2 / c2, sqrt, + EPS: 4u; the division: +u)
        params: 2u lr R + 7u lr |step| + u |p'|
        p1: 2u Sa + (1 - bp1) d(params),  Sa = |p1 bp1| + |(1 - bp1) p'|;   avg: that / cp + u |avg|
    `worst <= bound` is a condition on the DATA (the first moment's cancellation R reaches params
    through the step, which S does not see): the test asserts it before it asserts the bound."""
    f64 = lambda v: np.asarray(v, np.float64)
    lr, b1, b2, bp1, omb1, omb2, ombp1, c1, c2, cp = [float(v) for v in _adam_consts(lr, b1, b2, bp1, c1, c2, cp)]
    params, grad, g1, g2, p1 = f64(params), f64(grad), f64(g1), f64(g2), f64(p1)
    t1, t2 = g1 * b1, omb1 * grad
    m1, s1 = t1 + t2, np.abs(t1) + np.abs(t2)
    m2 = g2 * b2 + omb2 * (grad * grad)
    den = np.sqrt(m2 / c2) + EPS
    step = (m1 / c1) / den
    p = params - lr * step
    t5, t6 = p1 * bp1, ombp1 * p
    a, sa = t5 + t6, np.abs(t5) + np.abs(t6)
    values = {'params': p, 'g1': m1, 'g2': m2, 'p1': a, 'avg': a / cp}
    s_p = np.abs(params) + lr * np.abs(step)
    bound = {k: 8 * U * s for k, s in (('params', s_p), ('g1', s1), ('g2', m2), ('p1', sa), ('avg', sa / cp))}
    d_p = U * (2 * lr * s1 / (c1 * den) + 7 * lr * np.abs(step) + np.abs(p))
    d_a = 2 * U * sa + ombp1 * d_p
    worst = {'params': d_p, 'g1': 2 * U * s1, 'g2': 3 * U * m2, 'p1': d_a,
             'avg': d_a / cp + U * np.abs(a / cp)}
    return values, bound, worst


# --------------------------------------------------------------------------------- regularizers
def shifted_aux(aux, roll):
    """The auxiliary image as the un-rolled picture meets it under the iteration's shift roll =
    (x, y): pixel (y, x) meets aux[(y + ry) mod H][(x + rx) mod W] (regularizers_kernel)."""
    return np.roll(aux, (-int(roll[1]), -int(roll[0])), axis=(-2, -1))


def p_aux_grad32(img, mean, g0, p_scale, p_power, aux=None, aux_scale=0.0, aux_roll=(0, 0)):
    """The gradient regularizers_kernel leaves without a TV term, for an integer p_power in 2..9, in
    numpy float32 in the kernel's order: g = p_scale * (p * sign(z) * |z|^(p-1)) + g0 with z =
    (img + mean - 127.5) / 127.5 and the power by repeated multiplication, then g = aux_scale * d + g
    with d = (img - shifted aux) / 127.5."""
    f = np.float32
    assert p_power == int(p_power) and 2 <= p_power <= 9
    z = (img + np.asarray(mean, f).reshape(3, 1, 1) - f(127.5)) / f(127.5)
    az = np.abs(z)
    ap1 = az.copy()
    for _ in range(int(p_power) - 2):
        ap1 = ap1 * az
    g = f(p_scale) * (f(p_power) * np.sign(z) * ap1) + g0
    if aux is not None:
        d = (img - shifted_aux(aux, aux_roll)) / f(127.5)
        g = f(aux_scale) * d + g
    return g


# --------------------------------------------------------------------------------- moves and maps
def roll_add32(src, passes):
    """stx_map_roll_add in numpy float32: passes = [(roll_xy, alpha, init_divisor), ...]; a pass with
    a divisor sets acc = roll2(src) / divisor, any other adds alpha * roll2(src)."""
    acc = None
    for (rx, ry), alpha, divisor in passes:
        v = np.roll(src, (int(ry), int(rx)), axis=(-2, -1))
        acc = v / np.float32(divisor) if divisor else np.float32(alpha) * v + acc
    return acc


def to_u8_ref(img, mean):
    """get_image (style_transfer.py:378-386): RGB HWC bytes of clip(img + mean, 0, 255), truncated."""
    return np.uint8(np.clip((img + mean)[::-1].transpose(1, 2, 0), 0, 255))
