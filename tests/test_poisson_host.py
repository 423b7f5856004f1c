"""The screened-Poisson output stage without a GPU: the numpy statement of tests/poisson_ref.py against an exact
direct solve -- the scheme is held to its convergence cap before any GPU result is held to the scheme --, its exact
properties, the level counts and every refusal of the options.

Convergence cap: max |e_multigrid - e_direct| <= 0.01 on pictures in 0 ... 255, a hundredth of a grey level of the
8-bit output.  The default cycle count is the smallest count that meets the cap on every case below, plus 2.
Measured (max |e - e_direct| after 5, 6, 7, 8, 9 cycles; the cap is first met at the count marked *):

    (33, 31)    lambda 0.5: 3.7e-08 6.1e-10 1.0e-11 1.2e-12 1.1e-12   (*3)     lambda 5:   2.4e-04 2.0e-05 1.8e-06 1.6e-07 1.4e-08  (*4)
                lambda 50:  1.1e-02 2.2e-03 4.2e-04 8.1e-05 1.6e-05   (*6)     lambda 500: 3.6e-02 1.0e-02 2.8e-03 7.8e-04 2.1e-04  (*7)
    (67, 130)   lambda 0.5: 4.6e-08 7.5e-10 1.3e-11 4.7e-12 4.8e-12   (*3)     lambda 5:   3.9e-04 3.6e-05 3.3e-06 3.2e-07 3.1e-08  (*4)
                lambda 50:  4.5e-03 4.7e-04 5.5e-05 6.2e-06 7.1e-07   (*5)     lambda 500: 1.6e-01 3.4e-02 7.2e-03 1.5e-03 3.3e-04  (*7)
    (190, 257)  lambda 0.5: 6.8e-08 1.1e-09 2.1e-11 1.2e-11 1.2e-11   (*3)     lambda 5:   3.6e-04 3.4e-05 3.2e-06 3.1e-07 2.9e-08  (*4)
                lambda 50:  2.6e-03 2.9e-04 3.2e-05 3.8e-06 4.2e-07   (*5)     lambda 500: 5.2e-02 9.8e-03 1.8e-03 3.5e-04 6.6e-05  (*6)

so 7 cycles meet it everywhere and the default is 9."""

import argparse
import functools
import os
import re

import numpy as np
import pytest
from PIL import Image

from style_transfer_amd import config_system, image_ops, lib, poisson, transfer
from tests import poisson_ref as ref

SHAPES = [(33, 31), (67, 130), (190, 257)]
LAMBDAS = [0.5, 5.0, 50.0, 500.0]
CAP = 0.01


@functools.lru_cache(maxsize=None)
def _errors(hw, lam):
    """max |e - e_direct| after 1 .. default cycles of one case."""
    s, c = ref.case(*hw)
    exact = ref.direct(s, c, lam)
    lv = ref.levels(hw[0], hw[1], lam)
    bs, es = [None] * len(lv), [None] * len(lv)
    bs[0] = ref.rhs(s, c, lam)
    es[0] = np.zeros_like(bs[0])
    out = []
    for _ in range(ref.POISSON_CYCLES_DEFAULT):
        ref.w_cycle(es, bs, lv, 0)
        out.append(float(np.abs(es[0] - exact).max()))
    return tuple(out)


def test_the_direct_solve_solves_the_system():
    for hw in SHAPES[:2]:
        s, c = ref.case(*hw)
        for lam in LAMBDAS:
            b = ref.rhs(s, c, lam)
            r = np.abs(ref.apply_operator(ref.direct(s, c, lam), lam) - b).max()
            print(hw, lam, 'direct: |A e - b| / |b| = %.3g' % (r / np.abs(b).max()))
            assert r <= 1e-11 * np.abs(b).max()


@pytest.mark.parametrize('lam', LAMBDAS)
@pytest.mark.parametrize('hw', SHAPES)
def test_the_default_cycles_meet_the_cap(hw, lam):
    errors = _errors(hw, lam)
    print(hw, lam, ' '.join('%.1e' % e for e in errors))
    assert errors[ref.POISSON_CYCLES_DEFAULT - 3] <= CAP        # two cycles before the default already do
    assert errors[-1] <= CAP


def test_the_default_is_the_smallest_sufficient_count_plus_two():
    first = max(next(k + 1 for k, e in enumerate(_errors(hw, lam)) if e <= CAP) for hw in SHAPES for lam in LAMBDAS)
    assert first + 2 == ref.POISSON_CYCLES_DEFAULT == config_system.POISSON_CYCLES_DEFAULT == poisson.POISSON_CYCLES_DEFAULT
    # about 0.2 of the error is left per cycle
    for hw in SHAPES:
        for lam in LAMBDAS:
            e = _errors(hw, lam)
            rates = [e[k + 1] / e[k] for k in range(1, len(e) - 1) if e[k + 1] > 1e-9]
            assert max(rates) < 0.35, (hw, lam, rates)


# ------------------------------------------------------------------------------------------- exact properties
@pytest.mark.parametrize('hw', [(1, 1), (2, 2), (3, 5), (33, 31)])
def test_equal_pictures_give_a_correction_of_exactly_plus_zero(hw):
    s, _ = ref.case(*hw, channels=3)
    s = s - np.float32(120)                 # (both signs, as the pipeline's pictures are)
    for lam in (0.04, 5.0, 500.0):
        e = ref.correction(s, s.copy(), lam)
        assert not e.any() and not np.signbit(e).any()
        assert ref.solve(s, s.copy(), lam).tobytes() == s.tobytes()


def test_a_constant_content_picture_keeps_the_mean():
    """The columns of A sum to 1 and b sums to 0, so sum e = -sum r for ANY e with residual r = b - A e: the mean is
    kept as far as the residual has gone.  That is to 1e-9 of sum |e| for the exact solve at every lambda, for the
    default cycles up to lambda 5 (where they leave |r| < 1e-6 |b|), and at lambda 500 -- where the default cycles
    stop at the convergence cap, 1.5e-5 measured here -- for the 32 cycles that converge to rounding; the identity
    itself holds at every count."""
    for hw in [(33, 31), (67, 130)]:
        s, _ = ref.case(*hw)
        c = np.full(hw, 77, np.float32)
        for lam, cycles in ((0.5, ref.POISSON_CYCLES_DEFAULT), (5.0, ref.POISSON_CYCLES_DEFAULT), (500.0, 32)):
            e = ref.correction(s, c, lam, cycles)
            print(hw, lam, cycles, 'sum e / sum |e| = %.3g' % (abs(e.sum()) / np.abs(e).sum()))
            assert np.abs(e).max() > 1 and abs(e.sum()) <= 1e-9 * np.abs(e).sum()
        for lam in (0.5, 5.0, 500.0):
            exact = ref.direct(s, c, lam)
            assert abs(exact.sum()) <= 1e-9 * np.abs(exact).sum()
            e = ref.correction(s, c, lam, 2)
            r = ref.rhs(s, c, lam) - ref.apply_operator(e, lam)
            assert abs(e.sum() + r.sum()) <= 1e-9 * (np.abs(e).sum() + np.abs(r).sum())


def test_the_energy_falls():
    for hw in SHAPES[:2]:
        s, c = ref.case(*hw)
        for lam in LAMBDAS:
            f = np.float64(s) + ref.correction(s, c, lam)
            ef, es, ec = (ref.energy(p, s, c, lam) for p in (f, s, c))
            print(hw, lam, 'energy at f %.6g, at s %.6g, at c %.6g' % (ef, es, ec))
            assert ef <= es and ef <= ec


def test_the_residual_after_the_default_cycles():
    for hw in SHAPES:
        s, c = ref.case(*hw)
        b = ref.rhs(s, c, 5.0)
        r = ref.residual(ref.correction(s, c, 5.0), b, 5.0)
        print(hw, '|b - A e| / |b| = %.3g' % (np.abs(r).max() / np.abs(b).max()))
        assert np.abs(r).max() < 1e-6 * np.abs(b).max()
        assert np.abs(r - (b - ref.apply_operator(ref.correction(s, c, 5.0), 5.0))).max() <= 1e-9 * np.abs(b).max()


def test_restriction_and_prolongation():
    r = np.arange(15, dtype=np.float64).reshape(3, 5)
    assert np.array_equal(ref.restrict(r), [[(0 + 1 + 5 + 6) / 4, (2 + 3 + 7 + 8) / 4, (4 + 9) / 2],
                                            [(10 + 11) / 2, (12 + 13) / 2, 14]])
    # a constant is prolonged to itself, a linear ramp exactly inside (cell centres: x' = (x - 0.5) / 2)
    assert np.array_equal(ref.prolong(np.full((2, 3), 7.0), 3, 5), np.full((3, 5), 7.0))
    ramp = np.tile(np.arange(4, dtype=np.float64), (2, 1))
    want = (np.arange(8) - 0.5) / 2
    assert np.array_equal(ref.prolong(ramp, 4, 8)[:, 1:-1], np.tile(want, (4, 1))[:, 1:-1])
    assert np.array_equal(ref.prolong(ramp, 4, 8)[:, [0, -1]], np.tile([0.0, 3.0], (4, 1)))     # clamped at the edge


# --------------------------------------------------------------------------------------------------- host logic
@pytest.mark.parametrize('h,w,lam,count', [(1, 1, 5.0, 1), (2, 7, 500.0, 1), (7, 2, 5.0, 1), (33, 31, 0.04, 1),
                                           (33, 31, 0.05, 1), (33, 31, 0.2, 2), (33, 31, 0.5, 3), (33, 31, 5.0, 5),
                                           (33, 31, 500.0, 5), (3, 5, 500.0, 2), (190, 257, 500.0, 8),
                                           (2048, 2048, 5.0, 5), (2048, 2048, 1000.0, 9), (4096, 4096, 500.0, 8)])
def test_level_counts(h, w, lam, count):
    assert ref.level_count(h, w, lam) == len(poisson.levels(h, w, lam)) == count
    assert poisson.levels(h, w, lam) == ref.levels(h, w, lam)
    assert poisson.launch_count(h, w, lam) == ref.launch_count(h, w, lam)


def test_levels_and_launches_of_one_case():
    assert poisson.levels(33, 31, 5.0) == [(33, 31, 5.0), (17, 16, 1.25), (9, 8, 0.3125), (5, 4, 0.078125),
                                           (3, 2, 0.01953125)]
    # per cycle 10 launches at each of 1 + 2 + 4 + 8 visits and 40 at each of 16 coarsest visits
    assert poisson.launch_count(33, 31, 5.0, 1) == 2 + 15 * 10 + 16 * 40
    assert poisson.launch_count(33, 31, 0.04, 3) == 2 + 3 * 40


def _parse(extra):
    return config_system.parse_args(argparse.Namespace(), ['-ci', 'c.png', '-si', 's.png'] + extra, config_py=False)


def test_the_options_are_absent_unless_set():
    args = _parse([])
    assert 'poisson_lambda' not in args and 'poisson_cycles' not in args
    assert config_system.check_poisson_options(args) is None
    args = _parse(['--poisson-lambda', '5'])
    assert 'poisson_lambda' in args and 'poisson_cycles' not in args
    assert config_system.check_poisson_options(args) == (5.0, 9)
    assert config_system.check_poisson_options(_parse(['--poisson-lambda', '1/2', '--poisson-cycles', '3'])) == (0.5, 3)
    assert config_system.check_poisson_options(_parse(['--poisson-lambda', '1000', '--poisson-cycles', '32'])) == (1000.0, 32)


@pytest.mark.parametrize('extra,option', [
    (['--poisson-cycles', '4'], '--poisson-cycles'),
    (['--poisson-lambda', '0'], '--poisson-lambda'),
    (['--poisson-lambda', '-1'], '--poisson-lambda'),
    (['--poisson-lambda', '1000.5'], '--poisson-lambda'),
    (['--poisson-lambda', '5', '--poisson-cycles', '0'], '--poisson-cycles'),
    (['--poisson-lambda', '5', '--poisson-cycles', '33'], '--poisson-cycles'),
])
def test_refusals_on_the_command_line(extra, option):
    with pytest.raises(ValueError) as err:
        _parse(extra)
    assert str(err.value).startswith(option)


@pytest.mark.parametrize('name,value,option', [
    ('poisson_lambda', float('nan'), '--poisson-lambda'), ('poisson_lambda', float('inf'), '--poisson-lambda'),
    ('poisson_lambda', True, '--poisson-lambda'), ('poisson_lambda', '5', '--poisson-lambda'),
    ('poisson_cycles', 2.0, '--poisson-cycles'), ('poisson_cycles', True, '--poisson-cycles'),
])
def test_refusals_of_values_from_a_config_file(name, value, option):
    values = dict(poisson_lambda=5.0)
    values[name] = value
    with pytest.raises(ValueError) as err:
        config_system.check_poisson_options(argparse.Namespace(**values))
    assert str(err.value).startswith(option)


def test_the_module_command_line_refuses_before_an_engine_exists():
    opts = poisson.parse_poisson_args(['r.png', 'c.png', 'o.png', '--poisson-lambda', '5'])
    assert (opts.poisson_lambda, opts.poisson_cycles, opts.device) == (5.0, 9, 0)
    for extra, option in ((['--poisson-lambda', '0'], '--poisson-lambda'),
                          (['--poisson-lambda', '2000'], '--poisson-lambda'),
                          (['--poisson-lambda', '5', '--poisson-cycles', '40'], '--poisson-cycles'),
                          (['--poisson-lambda', '5', '--device', '-1'], '--device')):
        with pytest.raises(ValueError) as err:
            poisson.parse_poisson_args(['r.png', 'c.png', 'o.png'] + extra)
        assert str(err.value).startswith(option)
    with pytest.raises(SystemExit):         # (argparse: the option is required)
        poisson.parse_poisson_args(['r.png', 'c.png', 'o.png'])


# ------------------------------------------------------------------------------ where the stage sits (no GPU)
class FakeArray:
    def __init__(self, shape, log, name):
        self.shape, self.log, self.name = tuple(shape), log, name

    def free(self):
        self.log.append(('free', self.name))


class FakeEngine:
    def __init__(self, log):
        self.log = log

    def to_device(self, host):
        self.log.append(('to_device', host.shape))
        return FakeArray(host.shape, self.log, 'content')


class FakeFarm:
    def __init__(self, log):
        self.master = FakeEngine(log)

    def layers(self):
        return []


def _transfer(monkeypatch, extra):
    log = []
    st = transfer.StyleTransfer(FakeFarm(log), _parse(extra), argparse.Namespace())

    def fake_poisson(engine, img, content, lam, cycles=None):
        log.append(('poisson', img.name, content.name, lam, cycles))
        return FakeArray(img.shape, log, 'solved')
    monkeypatch.setattr(image_ops, 'poisson', fake_poisson)
    monkeypatch.setattr(image_ops, 'to_u8', lambda engine, img, mean: log.append(('to_u8', img.name)) or 'u8')
    monkeypatch.setattr(image_ops, 'to_u8_luma',
                        lambda engine, img, content, mean: log.append(('to_u8_luma', img.name, content.name)) or 'luma')
    return st, log


def test_output_goes_through_the_stage_first_and_the_temporary_is_freed(monkeypatch):
    picture = Image.fromarray(np.zeros((6, 9, 3), np.uint8))
    iterate = FakeArray((3, 6, 9), [], 'iterate')
    # ---- off: no content picture is kept, the output is to_u8 of the iterate
    st, log = _transfer(monkeypatch, [])
    assert st.poisson is None
    st._keep_content_picture(picture)
    assert st.content_picture is None and st.output_u8(iterate) == 'u8' and log == [('to_u8', 'iterate')]
    # ---- on: the picture is kept as for luma; Poisson, then the output kernel on its result, then the free
    st, log = _transfer(monkeypatch, ['--poisson-lambda', '5'])
    assert st.poisson == (5.0, 9)
    st._keep_content_picture(picture)
    assert st.content_picture.shape == (3, 6, 9) and log == [('to_device', (3, 6, 9))]
    assert st.output_u8(iterate) == 'u8'
    assert log[1:] == [('poisson', 'iterate', 'content', 5.0, 9), ('to_u8', 'solved'), ('free', 'solved')]
    # ---- with luma beside it: Poisson first, then luma on its result
    st, log = _transfer(monkeypatch, ['--poisson-lambda', '2', '--poisson-cycles', '3', '--preserve-color', 'luma'])
    st._keep_content_picture(picture)
    assert st.output_u8(iterate) == 'luma'
    assert log[1:] == [('poisson', 'iterate', 'content', 2.0, 3), ('to_u8_luma', 'solved', 'content'), ('free', 'solved')]
    # ---- the next scale's picture replaces this one
    st._keep_content_picture(Image.fromarray(np.zeros((12, 18, 3), np.uint8)))
    assert log[-2:] == [('free', 'content'), ('to_device', (3, 12, 18))]
    # ---- an output kernel that fails still frees the temporary
    def broken(*a):
        raise RuntimeError('no')
    monkeypatch.setattr(image_ops, 'to_u8_luma', broken)
    with pytest.raises(RuntimeError):
        st.output_u8(FakeArray((3, 12, 18), [], 'iterate'))
    assert log[-1] == ('free', 'solved')


def test_a_content_picture_of_another_size_is_refused_as_for_luma(monkeypatch):
    st, log = _transfer(monkeypatch, ['--poisson-lambda', '5'])
    with pytest.raises(ValueError) as err:
        st.output_u8(FakeArray((3, 6, 9), [], 'iterate'))                   # none is kept
    assert str(err.value).startswith('--poisson-lambda: no content picture of size 9x6 is kept')
    st._keep_content_picture(Image.fromarray(np.zeros((6, 9, 3), np.uint8)))
    with pytest.raises(ValueError) as err:
        st.output_u8(FakeArray((3, 12, 18), [], 'iterate'))
    assert str(err.value).startswith('--poisson-lambda: no content picture of size 18x12 is kept')
    assert not any(entry[0] == 'poisson' for entry in log)
    luma, _ = _transfer(monkeypatch, ['--preserve-color', 'luma'])
    with pytest.raises(ValueError) as err:
        luma.output_u8(FakeArray((3, 6, 9), [], 'iterate'))
    assert str(err.value) == str(err.value).replace('--poisson-lambda', '--preserve-color luma')
    assert str(err.value).startswith('--preserve-color luma: no content picture of size 9x6 is kept')


def test_values_from_a_config_file_are_refused_at_construction():
    for values, option in ((dict(poisson_lambda=-2.0), '--poisson-lambda'), (dict(poisson_cycles=3), '--poisson-cycles'),
                           (dict(poisson_lambda=5.0, poisson_cycles=99), '--poisson-cycles')):
        args = _parse([])
        for name, value in values.items():
            setattr(args, name, value)
        with pytest.raises(ValueError) as err:
            transfer.StyleTransfer(FakeFarm([]), args, argparse.Namespace())
        assert str(err.value).startswith(option)


# ------------------------------------------------------------------------------------------------- the ABI
def test_the_entry_point_is_declared_bound_and_refuses_nulls():
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(repo, 'include', 'stx.h')).read(), flags=re.S)
    assert re.search(r'\bint\s+stx_image_poisson\s*\(', header)
    assert len(lib.SIGNATURES['stx_image_poisson']) == 8
    so = lib.load()
    assert so.stx_image_poisson(None, None, None, None, 4, 4, 5.0, 2) == -1
    assert 'stx_image_poisson' in so.stx_last_error().decode()
    for name in ('INTEGRATION.md', 'README.md', 'PAPERS.md', 'DESIGN.md'):
        assert 'poisson' in open(os.path.join(repo, name)).read().lower(), name
