"""The nearest-neighbour feature matching term (--nnfm-weight) on the GPU: the kernels of nnfm.hip through
stx_op_nnfm_terms and stx_nnfm_bank, the tile path and the command line -- against tests/nnfm_ref.py (float64
on the same float32 inputs).

Bounds.
  * Planted inputs (column i = a_i b_pi(i) + 1e-3 unit noise, a_i in [1e-2, 1e3]; the float64 winner beats the
    runner-up by more than 1e-2, verified before the GPU is asked): every index equals the reference's.
  * Exact ties (duplicated bank rows across block and slice boundaries): the lowest index, exactly.
  * Random inputs: cos64(x_i, b_jgpu) >= max_j cos64 - tau for every column, tau = 4 x the worst
    |emulated score - float64 score| of the case (nnfm_ref.search_error; the 4 covers summation orders inside
    the matrix core that the emulation does not enumerate).
  * E, sum |S| (relative) and S (of max |S_ref|) to 1e-5 (tests/gpu_helpers.TIGHT) against the reference
    evaluated AT THE GPU'S OWN INDICES, on the random inputs, the sliced case and the case with zeros.  On the
    planted inputs the three are printed only: a column lies within 1e-1 .. 1e-6 rad of its winner, a float32
    c_i carries 6e-8, and both 1 - c_i and b - c_i x_i are cancelled differences there (a map of one column
    with a_i = 1e3 has nothing else), whose relative error the number format does not bound by 1e-5.
  * stx_nnfm_bank: the row count, rows to 1e-6 of the reference's unit rows.
  * The tile path: the loss to TIGHT of the float64 term on the GPU's activations, the gradient to TIGHT of
    the oracle's backward pass on the GPU's activations fed the reference's S (tests/gpu_helpers.check_tile's
    clause for identical decisions).

Observed worst values on an MI355X over the 48 op-level shapes: emulated search error 1.13e-7 (tau 4.5e-7), the
GPU's worst excess over the float64 maximum 0 (every column took the float64 argmax), E 1.4e-7, sum |S| 2.6e-7,
S 1.8e-7 of its maximum; bank rows 5.1e-8; the tiles' loss 3.1e-7, their gradient 9.9e-7 of its maximum; the
command-line run lowers E / 2 from 0.044087 to 0.025068 in 20 Adam steps.  Every case prints its figures before it asserts (pytest -s)."""

import ctypes
import functools
import re

import numpy as np
import pytest
from PIL import Image

from oracle.caffe_net import synthetic_weights
from style_transfer_amd import lib
from style_transfer_amd.netspec import builtin_net
from tests import nnfm_ref
from tests.gpu_helpers import TIGHT, gpu_engine, max_rel

pytestmark = pytest.mark.gpu

CHANNELS = [64, 256, 512]                       # one, several and the most K steps
MAPS = [(1, 1), (3, 5), (31, 33), (45, 47)]     # one column; less than an MFMA tile; ragged query blocks, h w odd
ROWS = [1, 31, 129, 1000]                       # ragged last bank blocks
ERR_ARG, ERR_UNSUPPORTED = -1, -4


def _unit_rows(rng, m, c):
    b = rng.standard_normal((m, c))
    return (b / np.linalg.norm(b, axis=1, keepdims=True)).astype(np.float32)


def _op(eng, feat, bank, profile=False):
    """(S, j, E, sum |S|[, the search's slice count]) of stx_op_nnfm_terms."""
    c, h, w = feat.shape
    d_feat, d_bank = eng.to_device(feat), eng.to_device(bank)
    s_out = eng.empty((c, h, w))
    idx = eng.empty((h * w,), np.int32)
    out = (ctypes.c_double * 2)()
    if profile:
        eng.profile(True)
    try:
        lib.call('stx_op_nnfm_terms', eng.handle, d_feat.ptr, c, h, w, d_bank.ptr, bank.shape[0], s_out.ptr, idx.ptr,
                 out)
        result = (s_out.get(), idx.get().astype(np.int64), out[0], out[1])
        if profile:
            labels = [row[0] for row in eng.profile_read()]
            slices = [int(m.group(1)) for m in (re.fullmatch(r'nnfm search op x(\d+)', l) for l in labels) if m]
            assert len(slices) == 1, labels
            result += (slices[0],)
    finally:
        if profile:
            eng.profile(False)
        for arr in (d_feat, d_bank, s_out, idx):
            arr.free()
    return result


def _planted(rng, bank, h, w):
    m, c = bank.shape
    pick = rng.randint(0, m, h * w)
    alpha = 10.0 ** rng.uniform(-2, 3, h * w)
    noise = rng.standard_normal((h * w, c))
    noise /= np.linalg.norm(noise, axis=1, keepdims=True)
    cols = alpha[:, None] * bank[pick].astype(np.float64) + 1e-3 * noise
    return np.ascontiguousarray(cols.T.reshape(c, h, w), np.float32)


def _held_at_own_indices(tag, feat, bank, s, j, e, asum, hold=True):
    e_ref, s_ref, asum_ref, _ = nnfm_ref.terms_at(feat, bank, j)
    s_err = max_rel(s, s_ref) if np.abs(s_ref).max() > 0 else float(np.abs(s).max())
    e_err = abs(e / e_ref - 1) if e_ref else abs(e)
    a_err = abs(asum / asum_ref - 1) if asum_ref else abs(asum)
    print('%s: E %.6g (%.2e), sum|S| %.6g (%.2e), S %.2e of max' % (tag, e, e_err, asum, a_err, s_err))
    assert np.all(np.isfinite(s)) and np.isfinite(e) and np.isfinite(asum)
    if hold:
        assert s_err <= TIGHT and a_err <= TIGHT and e_err <= TIGHT


@pytest.mark.parametrize('m', ROWS)
@pytest.mark.parametrize('h,w', MAPS)
@pytest.mark.parametrize('c', CHANNELS)
def test_nnfm_kernels_against_float64(c, h, w, m):
    eng = gpu_engine()
    rng = np.random.RandomState(c + 7 * h + 13 * w + m)
    bank = _unit_rows(rng, m, c)
    tag = 'C %d %dx%d M %d' % (c, h, w, m)
    # --- planted inputs: exact indices
    feat = _planted(rng, bank, h, w)
    scores = nnfm_ref.scores64(feat, bank)
    j_ref = np.argmax(scores, axis=1)
    if m > 1:
        top2 = np.partition(scores, -2, axis=1)[:, -2:]
        assert np.all(top2[:, 1] - top2[:, 0] > 1e-2), 'the planted winner is not separated'
    s, j, e, asum = _op(eng, feat, bank)
    assert np.array_equal(j, j_ref), (tag, np.flatnonzero(j != j_ref)[:8])
    _held_at_own_indices(tag + ' planted', feat, bank, s, j, e, asum, hold=False)
    # --- random inputs: the near-tie rule, then everything else at the GPU's own indices; twice
    feat = rng.standard_normal((c, h, w)).astype(np.float32)
    scores = nnfm_ref.scores64(feat, bank)
    tau = 4 * nnfm_ref.search_error(feat, bank)
    s, j, e, asum = _op(eng, feat, bank)
    assert j.min() >= 0 and j.max() < m
    excess = scores.max(axis=1) - scores[np.arange(h * w), j]
    print('%s random: emulated worst %.2e, tau %.2e, worst excess %.2e, %d of %d columns off the float64 argmax'
          % (tag, tau / 4, tau, excess.max(), np.count_nonzero(j != np.argmax(scores, axis=1)), h * w))
    assert np.all(excess <= tau), (tag, float(excess.max()), tau)
    _held_at_own_indices(tag + ' random', feat, bank, s, j, e, asum)
    s2, j2, e2, asum2 = _op(eng, feat, bank)
    assert s.tobytes() == s2.tobytes() and np.array_equal(j, j2) and e == e2 and asum == asum2


def test_the_sliced_bank_path():
    """n = 64 columns against M = 6000 rows: one query block, the bank cut across workgroups and merged."""
    eng = gpu_engine()
    rng = np.random.RandomState(6000)
    c, h, w, m = 64, 8, 8, 6000
    bank = _unit_rows(rng, m, c)
    feat = _planted(rng, bank, h, w)
    j_ref = nnfm_ref.nearest(feat, bank)
    s, j, e, asum, slices = _op(eng, feat, bank, profile=True)
    print('sliced: %d slices' % slices)
    assert slices > 1
    assert np.array_equal(j, j_ref)
    feat = rng.standard_normal((c, h, w)).astype(np.float32)
    scores = nnfm_ref.scores64(feat, bank)
    tau = 4 * nnfm_ref.search_error(feat, bank)
    s, j, e, asum = _op(eng, feat, bank)
    excess = scores.max(axis=1) - scores[np.arange(h * w), j]
    print('sliced random: tau %.2e, worst excess %.2e' % (tau, excess.max()))
    assert np.all(excess <= tau)
    _held_at_own_indices('sliced random', feat, bank, s, j, e, asum)


@pytest.mark.parametrize('h,w', [(8, 8), (181, 181)])
def test_exact_ties_take_the_lowest_index(h, w):
    """Bank rows duplicated across the 128-row blocks -- which are the slices of the 8 x 8 map (one query block)
    and the steps of one workgroup's walk for the 181 x 181 map (256 query blocks: no slicing): columns that
    are exact multiples of such a row score the same on every copy."""
    eng = gpu_engine()
    rng = np.random.RandomState(h)
    c, m = 64, 700
    bank = _unit_rows(rng, m, c)
    groups = [(5, 130), (127, 128), (100, 300, 650), (255, 256, 699)]
    for g in groups:
        for k in g[1:]:
            bank[k] = bank[g[0]]
    pick = rng.randint(0, m, h * w)
    copies = [k for g in groups for k in g]
    pick[:len(copies) * 3] = np.tile(copies, 3)
    alpha = (2.0 ** rng.randint(-6, 10, h * w)).astype(np.float32)        # exact multiples: no rounding
    feat = np.ascontiguousarray((alpha[:, None] * bank[pick]).T.reshape(c, h, w))
    j_ref = nnfm_ref.nearest(feat, bank)
    lowest = {k: g[0] for g in groups for k in g}
    assert all(j_ref[i] == lowest.get(pick[i], pick[i]) for i in range(h * w))
    s, j, e, asum, slices = _op(eng, feat, bank, profile=True)
    print('ties %dx%d: %d slices' % (h, w, slices))
    assert (slices > 1) == (h == 8)
    assert np.array_equal(j, j_ref), np.flatnonzero(j != j_ref)[:8]


def test_zero_columns_and_zero_rows():
    eng = gpu_engine()
    rng = np.random.RandomState(3)
    c, h, w, m = 64, 9, 11, 140
    bank = _unit_rows(rng, m, c)
    bank[[0, 7, 128, 139]] = 0
    feat = rng.standard_normal((c, h, w)).astype(np.float32)
    feat[:, 0, 0] = 0
    feat[:, 4, 5] = 0
    feat[:, 8, 10] = 0
    # a column that every real row scores negative takes the first zero row: c = 0, S = 0
    feat[:, 2, 2] = -bank[1:].sum(axis=0)
    s, j, e, asum = _op(eng, feat, bank)
    zero = [0, 4 * w + 5, 8 * w + 10]
    flat = s.reshape(c, -1)
    assert np.all(np.isfinite(s)) and np.isfinite(e) and np.isfinite(asum)
    assert np.all(j[zero] == 0) and not flat[:, zero].any()
    assert np.array_equal(j, nnfm_ref.nearest(feat, bank))
    _held_at_own_indices('zeros', feat, bank, s, j, e, asum)


def test_a_bank_of_the_blob_itself_matches_every_column_to_itself():
    eng = gpu_engine()
    rng = np.random.RandomState(17)
    c, h, w = 64, 31, 33
    feat = rng.standard_normal((c, h, w)).astype(np.float32)
    d_bank = eng.nnfm_bank(feat)
    bank = d_bank.get()
    d_bank.free()
    tau = 4 * nnfm_ref.search_error(feat, bank)
    s, j, e, asum = _op(eng, feat, bank)
    print('self-match: tau %.2e, E %.3e' % (tau, e))
    assert np.array_equal(j, np.arange(h * w))
    assert 0 <= e + 1e-7 and e <= 2 * tau


def test_argument_errors_leave_the_output_alone():
    eng = gpu_engine()
    feat = eng.to_device(np.ones((64, 4, 4), np.float32))
    bank = eng.to_device(np.ones((3, 64), np.float32) / 8)
    s_out = eng.to_device(np.full((64, 4, 4), 7.0, np.float32))
    idx = eng.to_device(np.full((16,), 9, np.int32), np.int32)
    out = (ctypes.c_double * 2)(5.0, 5.0)
    call = lambda c, bank_ptr, rows: lib.call('stx_op_nnfm_terms', eng.handle, feat.ptr, c, 4, 4, bank_ptr, rows,
                                              s_out.ptr, idx.ptr, out)
    for args, code in (((48, bank.ptr, 3), ERR_UNSUPPORTED), ((64, None, 3), ERR_ARG), ((64, bank.ptr, 0), ERR_ARG)):
        with pytest.raises(lib.StxError) as err:
            call(*args)
        assert err.value.code == code, (args, err.value.code)
    assert np.all(s_out.get() == 7.0) and np.all(idx.get() == 9) and list(out) == [5.0, 5.0]
    with pytest.raises(lib.StxError) as err:        # channels that are not the layer's; a layer that does not exist
        eng.set_nnfm_targets({'conv3_1': np.ones((3, 64), np.float32)})
    assert err.value.code == ERR_ARG
    with pytest.raises(lib.StxError):
        eng.set_nnfm_targets({'conv9_9': np.ones((3, 64), np.float32)})
    call(64, bank.ptr, 3)       # and the same arrays in order are taken
    assert np.all(np.isfinite(s_out.get())) and np.all(idx.get() < 3)
    for arr in (feat, bank, s_out, idx):
        arr.free()


@pytest.mark.parametrize('h,w', [(5, 7), (31, 33)])
@pytest.mark.parametrize('stride', [1, 2, 3])
def test_nnfm_bank_against_float64(stride, h, w):
    eng = gpu_engine()
    rng = np.random.RandomState(h + stride)
    feat = np.maximum(rng.standard_normal((64, h, w)), 0).astype(np.float32)
    feat[:, 0, 0] = 0
    ref = nnfm_ref.bank_of(feat, stride)
    d_bank = eng.nnfm_bank(eng.to_device(feat), stride)
    bank = d_bank.get()
    again = eng.nnfm_bank(feat, stride).get()       # from the host
    assert bank.shape == ref.shape == (nnfm_ref.bank_rows(h, w, stride), 64)
    err = float(np.abs(bank - ref).max())
    print('bank %dx%d stride %d: %d rows, %.2e' % (h, w, stride, bank.shape[0], err))
    assert err <= 1e-6 and not bank[0].any()
    assert np.all(np.abs(np.linalg.norm(np.float64(bank[1:]), axis=1) - 1) <= 1e-6)
    assert bank.tobytes() == again.tobytes()


# --------------------------------------------------------------------------------- the tile path
SL = ['conv1_1', 'conv2_1', 'conv3_1']
SW = {l: 1 / 3 for l in SL}
LW = {'conv3_1': 1.5}
NNFM_W = {'conv3_1': 0.7}
TILE_CASES = {'alone': ([], []), 'gram': ([], SL), 'content': (['conv3_2'], [])}


@functools.lru_cache(maxsize=None)
def _scene():
    """Oracle with targets of a 64 x 64 frame and the conv3_1 bank of a 40 x 44 style picture, computed once."""
    net = builtin_net('vgg19')
    om = nnfm_ref.NnfmOracleModel(net.as_dicts(), synthetic_weights(net.as_dicts(), 0))
    rng = np.random.RandomState(29)
    full = rng.uniform(-110, 120, (3, 64, 64)).astype(np.float32)
    style = rng.uniform(-110, 120, (3, 40, 44)).astype(np.float32)
    om.styles = [om.style_grams([style], SL, 512)]
    om.contents = [om.prepare_features(full, ['conv3_2'], 512)]
    bank = nnfm_ref.bank_of(om.features_tile(style, ['conv3_1'])['conv3_1']).astype(np.float32)
    return om, full, bank


@pytest.mark.parametrize('case', list(TILE_CASES))
def test_nnfm_tile_against_the_oracle(case):
    """The term alone (no tap at all), beside a Gram term on the same blob (two gradient terms: the stand-alone
    injection) and beside a content term on the blob above (the fused epilogue)."""
    om, full, bank = _scene()
    cl, sl = TILE_CASES[case]
    cw = {l: 0.05 for l in cl}
    eng = gpu_engine()
    start, roll = (0, 0), (0, 0)
    eng.set_contents_and_styles(om.contents, om.styles)
    plain = eng.sc_grad_tile(full, start, roll, cl, sl, LW, cw, SW) if cl or sl else None
    eng.set_nnfm_targets({'conv3_1': bank}, NNFM_W)
    om.nnfm_banks, om.nnfm_weights = {'conv3_1': np.float64(bank)}, dict(NNFM_W)
    try:
        loss, grad = eng.sc_grad_tile(full, start, roll, cl, sl, LW, cw, SW)
        again = eng.sc_grad_tile(full, start, roll, cl, sl, LW, cw, SW)
        deepest = om.deep_to_shallow(cl + sl + ['conv3_1'])[0]
        blobs = om.blob_names[:om.blob_names.index(deepest) + 1]
        acts = eng.features_tile(full, blobs)
        same_loss, same_grad = om.sc_grad_tile(full, start, cl, sl, LW, cw, SW, activations=acts)
        term64 = om.nnfm_loss64(acts, LW)
    finally:
        om.nnfm_banks, om.nnfm_weights = {}, {}
        eng.set_nnfm_targets({})
    stats = dict(loss=abs(loss / same_loss - 1), term=term64, grad=max_rel(grad, same_grad),
                 moved=max_rel(grad, plain[1]) if plain else None)
    print('nnfm tile', case, stats)
    assert np.all(np.isfinite(grad)) and grad.any()
    assert again[0] == loss and np.array_equal(again[1], grad)
    assert loss == pytest.approx(same_loss, rel=TIGHT), (loss, same_loss)
    if plain:
        assert loss - plain[0] == pytest.approx(term64, abs=2 * TIGHT * loss)
        assert stats['moved'] > 1e-3        # the term is not lost in the others
    else:
        assert loss == pytest.approx(term64, rel=TIGHT)
    assert stats['grad'] < TIGHT, stats


def test_cleared_targets_change_no_bit(monkeypatch):
    om, full, bank = _scene()
    eng = gpu_engine()
    cl, cw = ['conv3_2'], {'conv3_2': 0.05}
    run = lambda: eng.sc_grad_tile(full, (0, 0), (0, 0), cl, SL, LW, cw, SW)
    eng.set_contents_and_styles(om.contents, om.styles)
    before = run()
    eng.set_nnfm_targets({'conv3_1': bank}, NNFM_W)
    moved = run()
    monkeypatch.setenv('STX_SUMS_LATE', '0')            # in-place sums (the fixture re-reads the switches)
    in_place = run()
    monkeypatch.delenv('STX_SUMS_LATE')
    assert moved[0] != before[0] and not np.array_equal(moved[1], before[1])
    assert in_place[0] == moved[0] and np.array_equal(in_place[1], moved[1])
    eng.set_contents_and_styles(om.contents, om.styles)                  # clears the banks
    cleared = run()
    assert cleared[0] == before[0] and np.array_equal(cleared[1], before[1])
    with pytest.raises(lib.StxError):       # no targets: the empty tap list is refused again
        eng.sc_grad_tile(full, (0, 0), (0, 0), [], [], {}, {}, {})


# ------------------------------------------------------------------------------ the command line
def _cli_run(tmp_path, monkeypatch, capsys, name, extra):
    import csv
    import glob
    from style_transfer_amd import cli
    where = tmp_path / name
    where.mkdir()
    monkeypatch.chdir(where)
    argv = ['-ci', '../c.png', '--size', '128', '--min-size', '128', '--tile-size', '128', '--model', 'vgg19',
            '--weights', 'synthetic:0', '--devices', '0', '-oi', 'out.png'] + extra
    assert cli.main(argv) == 0
    printed = capsys.readouterr().out
    final = Image.open(where / 'out.png')
    logs = glob.glob(str(where / '*_log.csv'))
    assert len(logs) == 1
    with open(logs[0], newline='') as f:
        losses = [float(row['loss']) for row in csv.DictReader(f)]
    return np.asarray(final.convert('RGB')), final.text['Comment'], losses, printed


def _bank_rows(sizes_hw, stride):
    """Rows of the concatenated conv3_1 bank (two poolings: ceil(size / 4) a side) of style pictures of these
    sizes.  The pictures of the test fit --size 128 and --style-scale 1 never enlarges one: they are used as given."""
    return sum(nnfm_ref.bank_rows(-(-hh // 4), -(-ww // 4), stride) for hh, ww in sizes_hw)


def test_cli_nnfm_runs_lower_the_term_and_concatenate_the_banks(tmp_path, monkeypatch, capsys):
    rng = np.random.RandomState(5)
    picture = lambda hw: Image.fromarray(np.uint8(rng.uniform(0, 255, hw + (3,))))
    picture((96, 128)).save(tmp_path / 'c.png')
    picture((96, 128)).save(tmp_path / 's.png')
    picture((64, 80)).save(tmp_path / 't.png')
    # the term alone: no Gram, the content term at weight 0, no regulariser -- the logged loss is weight E / 2
    alone = ['--nnfm-weight', '1', '--nnfm-layers', 'conv3_1', '--style-layers', '--content-layers', 'conv3_2', '-cw', '0', '-tw', '0',
             '-pw', '0']
    one = _cli_run(tmp_path, monkeypatch, capsys, 'one', ['-si', '../s.png', '-i', '20'] + alone)
    print('20 Adam steps, E / 2: %.6f -> %.6f' % (one[2][0], one[2][-1]))
    assert one[0].shape == (96, 128, 3) and len(one[2]) == 20 and np.all(np.isfinite(one[2]))
    assert one[2][-1] < one[2][0]
    assert re.search(r'nnfm_weight=1\.0', one[1]) and 'nnfm_stride' not in one[1]
    assert 'NNFM bank rows: conv3_1 %d\n' % _bank_rows([(96, 128)], 1) in one[3], one[3]
    two = _cli_run(tmp_path, monkeypatch, capsys, 'two',
                   ['-si', '../s.png', '../t.png', '-i', '2', '--nnfm-stride', '2'] + alone)
    both = [(96, 128), (64, 80)]
    assert _bank_rows(both, 2) == 12 * 16 + 8 * 10
    assert 'NNFM bank rows: conv3_1 %d\n' % _bank_rows(both, 2) in two[3], two[3]
    bare = _cli_run(tmp_path, monkeypatch, capsys, 'bare', ['-si', '../s.png', '-i', '2'])
    assert 'nnfm' not in bare[1] and 'NNFM' not in bare[3]
