"""Every loss term of the tile path armed in one call: masked and unmasked style targets, masked content targets,
statistics targets and a Deep-Dream term, on taps that share blobs and on taps of their own.  The per-feature
files arm one kind at a time; here the kinds meet, so their places in the shared scratch, in the scalar arena
and in the taps' gradient buffers are walked one behind the other.

Nothing here is held against an oracle (the per-feature files do that).  Held are:
  * finite results, the same bits on a second run, under STX_SUMS_LATE=0 and under STX_TERMS_LATE=1;
  * additivity with the forward pass held fixed: the call is repeated once per family (content, style, statistics,
    dream) with the weights of the other families set to zero.  Zero weights keep every tap, every kernel choice
    and every fusing decision, so the activations and the ReLU / pooling decisions are those of the full call and
    each run's loss and gradient are that family's share.
    Loss: the per-term scalars are the same floats in every run; the host adds fewer than 64 of them in double,
    only the order differs, all terms of a family share a sign: |loss - sum loss_f| <= 64 * 2^-52 * sum |loss_f|.
    Gradient: fp32 rounding and the power-of-two scales of the fp16-split kernels differ between the runs:
    max |g - sum g_f| <= GRAD_TOL * sum_f max |g_f|, no pixel excluded.
What additivity cannot see: a mistake in the layout.  If two terms' slots or scratch regions overlap, the full run and
every share run read the same overwritten memory and the shares still add up to the whole (run once: plan_terms with
the SWD slot laid over the NNFM slot passes this file).  tests/test_gpu_terms_meet.py holds the combined evaluation --
with NNFM, SWD and self-similarity targets too -- against an independent reference of all terms at once.
Every case prints its figures before it asserts (pytest -s).

Observed on an MI355X, before and after the term list was planned (the same bits): loss off by 0 on both tiles
(bounds 7.0e-6 and 5.6e-6); gradient off by 3.9e-7 and 4.5e-7 of the sum of the shares' maxima, which were 139 /
152 / 157 / 163 and 98 / 91 / 167 / 135 for content / style / statistics / dream."""

import functools

import numpy as np
import pytest

from style_transfer_amd import lib
from tests.gpu_helpers import TIGHT, gpu_engine
from tests.test_gpu_style_masks import FRAME, _smooth_mask, _tile

pytestmark = pytest.mark.gpu

SL = ['conv1_1', 'conv2_1', 'conv3_1']          # two style sets: set 0 through a mask, set 1 unmasked
CL = ['conv3_1', 'conv2_2']                     # both through the content mask; conv3_1 is a style tap too
STAT_W = {'conv2_1': 1.0, 'conv1_2': 2.0}       # conv2_1 is a style tap; conv1_2 is tapped by nothing else
DL = ['conv3_2']                                # the deepest tap
LW = {'conv2_1': 1.5}
# (every term's gradient is normalised by its sum of magnitudes: the weights below bring the four families'
# gradients within an order of magnitude of each other, so that the bound on their sum binds each of them)
CW = {'conv3_1': 2.0, 'conv2_2': 0.8}
SW = {l: 1.0 for l in SL}
DW = {'conv3_2': 1.0}
FAMILIES = ['content', 'style', 'statistics', 'dream']
# max |g_all - sum g_f| / sum_f max |g_f|, measured on an MI355X on the commit before the term list was planned:
# 3.9e-7 (64 x 48 tile) and 4.5e-7 (37 x 53 tile).  Both lie below TIGHT / 4 = 2.5e-6, so the bound is TIGHT; the
# factor of four covers that the observed value is the maximum of two tiles only.
GRAD_TOL = TIGHT


@functools.lru_cache(maxsize=None)
def _scene():
    """Targets of a 128 x 128 frame from the engine's own feature maps, computed once."""
    eng = gpu_engine()
    rng = np.random.RandomState(11)
    full = rng.uniform(-110, 120, (3,) + FRAME).astype(np.float32)
    pictures = [rng.uniform(-110, 120, (3, 40, 44)).astype(np.float32) for _ in range(2)]
    contents = [eng.features_tile(full, CL)]
    feats = [eng.features_tile(p, SL + ['conv1_2']) for p in pictures]
    styles = [{l: eng.gram_matrix(f[l]) for l in SL} for f in feats]
    stats = {l: eng.feature_stats(feats[0][l]) for l in STAT_W}
    return full, contents, styles, stats, [_smooth_mask(FRAME), None], _smooth_mask(FRAME, 1)


def _zeros(weights):
    return {l: 0.0 for l in weights}


@pytest.mark.parametrize('th,tw,start,roll', [(64, 48, (0, 0), (0, 0)), (37, 53, (64, 32), (-24, 40))])
def test_all_terms_together(th, tw, start, roll, monkeypatch):
    full, contents, styles, stats, style_masks, content_mask = _scene()
    eng = gpu_engine()
    eng.set_contents_and_styles(contents, styles)
    eng.set_style_masks(style_masks)
    eng.set_content_mask(content_mask)
    tile = _tile(full, th, tw, start, roll)

    def run(only=None):
        on = lambda family, weights: weights if only in (None, family) else _zeros(weights)
        eng.set_stat_targets(stats, on('statistics', STAT_W))
        return eng.sc_grad_tile(tile, start, roll, CL, SL, LW, on('content', CW), on('style', SW),
                                dd_layers=DL, dd_weight=on('dream', DW))

    try:
        first, again = run(), run()
        assert np.isfinite(first[0]) and np.all(np.isfinite(first[1]))
        assert first[0] == again[0] and np.array_equal(first[1], again[1])          # deterministic
        for name, value in (('STX_SUMS_LATE', '0'), ('STX_TERMS_LATE', '1')):
            monkeypatch.setenv(name, value)
            lib.reread_env()
            other = run()
            monkeypatch.delenv(name)
            lib.reread_env()
            assert other[0] == first[0] and np.array_equal(other[1], first[1]), name
        shares = [run(f) for f in FAMILIES]
    finally:
        eng.set_stat_targets({})
        eng.set_content_mask(None)
        eng.set_style_masks([])
    losses = np.array([s[0] for s in shares], np.float64)
    grads = [np.float64(s[1]) for s in shares]
    assert np.all(np.isfinite(losses)) and all(np.all(np.isfinite(g)) for g in grads)
    loss_err = abs(first[0] - losses.sum())
    loss_bound = 64 * 2.0 ** -52 * np.abs(losses).sum()
    scale = sum(np.abs(g).max() for g in grads)
    grad_err = float(np.abs(np.float64(first[1]) - sum(grads)).max() / scale)
    print('all terms %dx%d at %s roll %s: loss %.17g, shares %s, off by %.3e (bound %.3e); gradient shares %s, '
          'off by %.3e of their sum'
          % (th, tw, start, roll, first[0], dict(zip(FAMILIES, losses)), loss_err, loss_bound,
             {f: float(np.abs(g).max()) for f, g in zip(FAMILIES, grads)}, grad_err))
    assert all(l != 0 for l in losses) and losses[3] < 0        # every family is armed; dream subtracts
    assert loss_err <= loss_bound
    assert grad_err <= GRAD_TOL
