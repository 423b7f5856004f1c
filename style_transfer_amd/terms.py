"""The optional loss terms of a run (none but SWT is an option of the reference), behind two small protocols: the
schedule in ``transfer.py`` loops over two lists built from the options and names no term.  Target terms keep targets
in the engines beside the Grams; image terms add to the loss of the whole image.  The order of a list is the order
of the library's calls and of the loss's sum.  ``st`` below is the StyleTransfer.
"""

import warnings

import numpy as np
from PIL import Image

from . import image_ops
from .farm import tile_grid
from .config_system import (LAP_POOLS_DEFAULT, SWD_QUANTILES, ValuePlaceholder, check_lap_pools, check_nnfm_options,
                            check_photo_options, check_selfsim_options, check_stat_options, check_swd_options, ffloat,
                            nnfm_bank_rows, nnfm_layer_args, nnfm_cover, nnfm_k, nnfm_patch, nnfm_stride, option_on,
                            selfsim_layer_args, selfsim_points, stat_layer_args, swd_dirs, swd_directions,
                            swd_layer_args, check_shift_options, check_shift_tile, shift_layer_args, shift_offsets,
                            check_cx_bank, check_cx_options, cx_bank_rows, cx_h, cx_layer_args, cx_points, cx_rows,
                            check_temporal_options, flow_value, temporal_prev_contents)
from .flow import estimate_flow, read_flo
from .resample import resample_device


def parse_weights(args, master_weight):
    """['name', 'name:2', ...] -> (names, {name: weight normalised to sum |w| = master})
    (style_transfer.py:684-698)."""
    names, weights, total = [], {}, 0
    for arg in args:
        name, _, w = arg.partition(':')
        names.append(name)
        weights[name] = ffloat(w) if w else 1
        total += abs(weights[name])
    return names, {n: w * master_weight / total for n, w in weights.items()}


def lap_pool_weights(pools, lap_weight):
    """--lap-pools ['4', '16:3'] and --lap-weight 30 -> ([4, 16], [7.5, 22.5]): the pool sizes and their
    weights, normalised to sum |w| = lap_weight exactly as a layer list's are (parse_weights)."""
    names, weights = parse_weights(list(pools), lap_weight)
    return [int(name) for name in names], [weights[name] for name in names]


def mask_at_size(mask, size_hw):
    """A greyscale PIL mask at one scale: Lanczos-resized to (H, W), as float32 in [0, 1] (clipped)."""
    h, w = int(size_hw[0]), int(size_hw[1])
    return np.clip(np.float32(mask.convert('L').resize((w, h), Image.LANCZOS)) / np.float32(255), 0, 1)


def rolled_mask(mask, roll):
    """An [H, W] mask moved with the picture by ``roll`` = (x, y) pixels (--jitter), wrapping; None: as it is."""
    if roll is None:
        return mask
    return np.roll(mask, (int(roll[1]), int(roll[0])), (0, 1))


# ---------------------------------------------------------------------------------------- target terms
def _nothing(self, *args, **kwargs):
    pass


class TargetTerm:
    """A term whose targets live in the engines.  Per scale ``read(st)`` comes first.  When the style targets are
    made (preprocess_images) the term sees every variant's feature maps at its ``layers``: ``begin()``,
    ``take(st, layer, feat)`` per variant and layer, ``picture_done(st, index)`` behind the variants of style
    picture ``index``, ``finish(st, count, quiet)`` with the variant count.
    ``send(st, roll)`` follows every set_contents_and_styles, which clears the engines' copy (``roll``: the
    iteration's shift under --jitter).  ``drop()`` goes with the style targets.  ``content_layers``: the layers whose
    content maps the term reads; preprocess_images takes the content features there too."""
    layers = content_layers = ()
    read = begin = take = picture_done = finish = send = drop = _nothing


class LayerTargets(TargetTerm):
    """One target per layer of a ``LAYER[:weight]`` list, which is read once per scale like the other layer lists.
    The targets may be older (--style-multiscale): a layer that a later reading drops gets no term, and one that
    it adds has no target and is refused."""
    weights = targets = None    # {layer: weight} of the scale; {layer: target}, or None while there are none

    def read(self, st):
        self.layers, self.weights = parse_weights(self.layer_args(st.args), getattr(st.args, self.WEIGHT))

    def begin(self):
        self._parts = {layer: [] for layer in self.layers}

    def drop(self):
        self.targets = None

    def send(self, st, roll=None):
        if not self.weights:
            return
        missing = [layer for layer in self.weights if layer not in self.targets]
        if missing:
            raise ValueError('%s %s: no %s was taken there; with --style-multiscale the layers are those of the '
                             'first scale' % (self.FLAG, ' '.join(missing), self.WHAT))
        self.set_targets(st.farm, {layer: self.targets[layer] for layer in self.weights})


class StatTargets(LayerTargets):
    """--stat-weight / --stat-layers (the mean / std style term): per-channel mean and sd of the style pictures'
    feature maps, averaged like the Grams; ``targets`` = {layer: (mean [C], sd [C])}."""
    FLAG, WEIGHT, WHAT, layer_args = '--stat-layers', 'stat_weight', 'statistics target', staticmethod(stat_layer_args)

    def take(self, st, layer, feat):
        self._parts[layer].append(np.stack(st.farm.feature_stats(feat)))

    def finish(self, st, count, quiet):
        self.targets = {layer: tuple(sum(parts[1:], parts[0]) / np.float32(count))
                        for layer, parts in self._parts.items() if parts}

    def set_targets(self, farm, targets):
        farm.set_stat_targets(targets, self.weights)


class NnfmBanks(LayerTargets):
    """--nnfm-weight / --nnfm-layers / --nnfm-stride / --nnfm-patch / --nnfm-k / --nnfm-cover (nearest-neighbour feature matching):
    per layer one bank of the style pictures' unit feature vectors (3 x 3 patches of them with --nnfm-patch 3), built
    on the master GPU and concatenated over the variants; ``targets`` = {layer: DeviceArray [rows, patch^2 C]}.  The
    banks do not depend on --nnfm-k or --nnfm-cover, which are read once per scale and go with the targets.
    --nnfm-masks (``st.nnfm_masks``): the rows of a style picture -- of all its ladder sizes with --style-multiscale
    -- are one segment of a bank, ``segments`` = {layer: [rows of picture 0, of picture 1, ...]}, and the masks,
    resized to the scale and rolled under --jitter like the style masks, go to the engines with the banks."""
    FLAG, WEIGHT, WHAT, layer_args = '--nnfm-layers', 'nnfm_weight', 'bank', staticmethod(nnfm_layer_args)
    targets_patch = 1       # --nnfm-patch of the banks in ``targets``
    masks = segments = _roll = None     # [H, W] float32 arrays in [0, 1] of the scale; {layer: [rows per picture]}

    def read(self, st):
        super().read(st)
        self.stride, self.patch, self.k = nnfm_stride(st.args), nnfm_patch(st.args), nnfm_k(st.args)
        self.cover = nnfm_cover(st.args)
        if getattr(st, 'nnfm_masks', None) is not None:
            self.masks = [mask_at_size(mask, st.img.shape[1:]) for mask in st.nnfm_masks]

    def begin(self):
        super().begin()
        self._seg_rows = {layer: [] for layer in self.layers}

    def picture_done(self, st, index):
        for layer, parts in self._parts.items():
            self._seg_rows[layer].append(sum(part.shape[0] for part in parts) - sum(self._seg_rows[layer]))

    def take(self, st, layer, feat):
        # (a bank past the library's offsets is refused before this part is allocated)
        nnfm_bank_rows(*feat.shape, self.stride, self.patch, sum(part.shape[0] for part in self._parts[layer]))
        self._parts[layer].append(st.farm.nnfm_bank(feat, self.stride, self.patch))

    def finish(self, st, count, quiet):
        self.targets = {layer: st.engine.concat_rows(parts) for layer, parts in self._parts.items()}
        self.targets_patch = self.patch
        self.segments = {layer: list(rows) for layer, rows in self._seg_rows.items()}
        if not quiet:
            def seg_note(layer):
                return ' (%s)' % ' + '.join(map(str, self.segments[layer])) if self.masks is not None else ''
            print('NNFM bank rows: ' + ', '.join('%s %d%s' % (layer, bank.shape[0], seg_note(layer))
                                                 for layer, bank in self.targets.items()) +
                  ('; patch %d' % self.patch if self.patch != 1 else '') + ('; k %d' % self.k if self.k != 1 else '') +
                  ('; cover %g' % self.cover if self.cover != 0 else ''))

    def drop(self):
        for bank in (self.targets or {}).values():
            bank.free()
        self.targets = None

    def send(self, st, roll=None):
        self._roll = roll       # (the masks move with the picture)
        super().send(st, roll)

    def set_targets(self, farm, targets):
        if self.masks is not None:
            counts = {len(self.segments[layer]) for layer in targets}
            if counts - {len(self.masks)}:
                raise ValueError('--nnfm-masks: %d mask(s) for %s style picture(s)'
                                 % (len(self.masks), ' / '.join(map(str, sorted(counts)))))
            farm.set_nnfm_targets(targets, self.weights, self.targets_patch, self.k, self.cover,
                                  segments={layer: self.segments[layer] for layer in targets},
                                  masks=[rolled_mask(mask, self._roll) for mask in self.masks])
        elif self.cover != 0:
            farm.set_nnfm_targets(targets, self.weights, self.targets_patch, self.k, self.cover)
        else:
            farm.set_nnfm_targets(targets, self.weights, self.targets_patch, self.k)


class SwdTargets(LayerTargets):
    """--swd-weight / --swd-layers / --swd-dirs (the sliced Wasserstein style term): per layer fixed directions V
    (swd_directions: from --seed and the layer's name, the same for the whole run) and, per direction, the quantile
    function of the style pictures' projections at SWD_QUANTILES samples, averaged over the variants like the Grams
    -- the mean of quantile functions is the 1-D Wasserstein barycentre and stays non-decreasing; ``targets`` =
    {layer: (V [D, C], Tq [D, Q])}."""
    FLAG, WEIGHT, WHAT, layer_args = '--swd-layers', 'swd_weight', 'quantile target', staticmethod(swd_layer_args)

    def __init__(self):
        self._directions = {}       # {layer: V}, drawn at first use

    def directions(self, st, layer, channels):
        if layer not in self._directions:
            self._directions[layer] = swd_directions(getattr(st.args, 'seed', 0), layer, channels,
                                                     swd_dirs(st.args) or channels)
        return self._directions[layer]

    def take(self, st, layer, feat):
        self._parts[layer].append(st.farm.swd_target(feat, self.directions(st, layer, feat.shape[0]), SWD_QUANTILES))

    def finish(self, st, count, quiet):
        self.targets = {layer: (self._directions[layer], sum(parts[1:], parts[0]) / np.float32(count))
                        for layer, parts in self._parts.items() if parts}

    def set_targets(self, farm, targets):
        farm.set_swd_targets(targets, self.weights)


class SelfsimTargets(TargetTerm):
    """--selfsim-weight / --selfsim-layers / --selfsim-points (the self-similarity content term): the term reads the
    content maps at its layers (``content_layers``) and has no data of its own -- per layer the most grid positions
    and a weight.  Under --jitter the maps are retaken every iteration with the contents, and ``send`` re-arms the
    term behind them."""
    weights = points = None     # {layer: weight} of the scale; --selfsim-points

    def read(self, st):
        names, self.weights = parse_weights(selfsim_layer_args(st.args), getattr(st.args, 'selfsim_weight'))
        self.content_layers, self.points = tuple(names), selfsim_points(st.args)

    def send(self, st, roll=None):
        # (the term goes with content maps: under --jitter there are none until the first step)
        if self.weights and st.contents:
            st.farm.set_selfsim_targets({layer: self.points for layer in self.weights}, self.weights)


class ShiftTargets(LayerTargets):
    """--shift-weight / --shift-layers / --shift-offsets (the shifted-Gram style term): per layer the Gram matrices
    of the style pictures' feature maps against themselves moved by every offset, averaged over the variants like the
    Grams; ``targets`` = {layer: (offsets [(dy, dx), ...], T [n, C, C])}.  The offsets are read once per scale; an
    offset that leaves a tile's blob of the scale without a pair of pixels is refused there, before any GPU work.
    Kept targets (--style-multiscale) go to the engines with the offsets they were taken at."""
    FLAG, WEIGHT, WHAT, layer_args = '--shift-layers', 'shift_weight', 'shifted-Gram target', staticmethod(shift_layer_args)
    offsets = None      # [(dy, dx), ...] of the scale

    def read(self, st):
        super().read(st)
        self.offsets = shift_offsets(st.args)
        tiles = {(y1 - y0, x1 - x0) for y0, y1, x0, x1 in tile_grid(st.img.shape[1:], st.args.tile_size)}
        for layer in self.layers:
            for tile_hw in sorted(tiles):
                check_shift_tile(self.offsets, layer, st.farm.layer_info(layer)[0], tile_hw)

    def take(self, st, layer, feat):
        self._parts[layer].append(st.farm.shift_gram(feat, self.offsets))

    def finish(self, st, count, quiet):
        self.targets = {layer: (list(self.offsets), sum(parts[1:], parts[0]) / np.float32(count))
                        for layer, parts in self._parts.items() if parts}

    def set_targets(self, farm, targets):
        farm.set_shift_targets(targets, self.weights)


class CxTargets(LayerTargets):
    """--cx-weight / --cx-layers / --cx-points / --cx-rows / --cx-h (the contextual style term): per layer one bank
    of the style pictures' RAW feature vectors on a grid of at most --cx-rows positions per picture and size,
    gathered on the master GPU and concatenated over the variants; ``targets`` = {layer: DeviceArray [rows, C]}.  The
    engines centre and normalise the rows when they take them.  Points and bandwidth are read once per scale and go
    with the targets; a bank past the library's limits is refused before its part is allocated."""
    FLAG, WEIGHT, WHAT, layer_args = '--cx-layers', 'cx_weight', 'bank', staticmethod(cx_layer_args)
    points = rows = h = None    # --cx-points, --cx-rows, --cx-h of the scale

    def read(self, st):
        super().read(st)
        self.points, self.rows, self.h = cx_points(st.args), cx_rows(st.args), cx_h(st.args)

    def take(self, st, layer, feat):
        cx_bank_rows(feat.shape[1], feat.shape[2], self.rows, sum(part.shape[0] for part in self._parts[layer]),
                     self.points)
        self._parts[layer].append(st.farm.cx_rows(feat, self.rows))

    def finish(self, st, count, quiet):
        self.targets = {layer: st.engine.concat_rows(parts) for layer, parts in self._parts.items()}
        if not quiet:
            print('CX bank rows: ' + ', '.join('%s %d' % (layer, bank.shape[0]) for layer, bank in self.targets.items()))

    def drop(self):
        for bank in (self.targets or {}).values():
            bank.free()
        self.targets = None

    def send(self, st, roll=None):
        for layer in self.weights or ():        # (kept banks of an earlier scale against this scale's points)
            if self.targets and layer in self.targets:
                check_cx_bank(self.targets[layer].shape[0], self.points, self.rows)
        super().send(st, roll)

    def set_targets(self, farm, targets):
        farm.set_cx_targets(targets, self.weights, self.points, self.h)


class Masks(TargetTerm):
    """--style-masks / --content-mask (spatial control): ``st.style_masks`` and ``st.content_mask`` resized to the
    scale's content size.  Under --jitter the engines hold content maps of the rolled picture and shift nothing,
    so the masks are rolled too.  Without masks nothing here runs."""
    style = content = None      # [H, W] float32 arrays in [0, 1] of the scale being optimised

    def read(self, st):
        if st.style_masks is not None:
            self.style = [mask_at_size(mask, st.img.shape[1:]) for mask in st.style_masks]
        if st.content_mask is not None:
            self.content = mask_at_size(st.content_mask, st.img.shape[1:])

    def send(self, st, roll=None):
        if self.style is not None:
            if len(st.styles) != len(self.style):
                raise ValueError('--style-masks: %d mask(s) for %d style set(s)' % (len(self.style), len(st.styles)))
            st.farm.set_style_masks([rolled_mask(mask, roll) for mask in self.style])
        # (the content mask goes with content targets only: under --jitter there are none until the first step)
        if self.content is not None and st.contents:
            st.farm.set_content_mask(rolled_mask(self.content, roll))


def target_terms(args, known_layers):
    """The target terms of a run, in the order they are sent; a bad option is refused here, before any GPU work.
    (The masks are handed to transfer_multiscale, so their term is always listed.)"""
    checked = ((check_stat_options, StatTargets), (check_nnfm_options, NnfmBanks), (check_swd_options, SwdTargets),
               (check_selfsim_options, SelfsimTargets), (check_shift_options, ShiftTargets),
               (check_cx_options, CxTargets))
    return [cls() for check, cls in checked if check(args, known_layers)] + [Masks()]


# ----------------------------------------------------------------------------------------- image terms
class ImageTerm:
    """A term of the whole image.  Per scale ``prepare(st, picture)``: ``picture`` is ``st.content_picture``, which
    StyleTransfer owns -- there for a term that ``needs_content``, and still there at every ``add()`` for one that
    ``keeps_content``; a term frees only what it made.  ``add(st, loss, params, roll)`` adds the term to ``loss``
    and its gradient to ``st.grad``; weights are read at every evaluation (a config file may bind them)."""
    needs_content = keeps_content = False
    __init__ = prepare = add = _nothing


class SwtTerm(ImageTerm):
    """--swt-weight (style_transfer.py:716-720) calls PyWavelets, which is not part of the reference tree; its
    transform is restated for the Haar wavelet only, at any level count (oracle/num_ops.py,
    tests/swt_levels_ref.py)."""

    def __init__(self, args):
        if str(args.swt_wavelet) not in ('haar', 'db1'):
            raise NotImplementedError('--swt-wavelet %s: only the Haar wavelet (haar / db1) is '
                                      'implemented' % args.swt_wavelet)
        if int(args.swt_levels) < 1:
            raise ValueError('--swt-levels %s: at least one level is needed' % args.swt_levels)
        warnings.warn('--swt-weight: the Haar SWT term is a restatement of PyWavelets\' '
                      'swt2 / iswt2, which is not part of the reference tree and not '
                      'installed here; it has never been compared with it (parity unpinned)')

    def prepare(self, st, picture):
        # pywt.swt2 refuses more levels than log2 of the padded side (num_utils.py:186-191):
        # the reference stops at its first evaluation of such a scale
        args, (h, w) = st.args, st.img.shape[1:]
        side = image_ops.swt_padded_side(h, w)
        if 2 ** int(args.swt_levels) > side:
            raise ValueError('--swt-levels %d: a %d x %d image is padded to a square of side %d, '
                             'which takes %d levels at most (raise --min-size or lower the level '
                             'count)' % (args.swt_levels, w, h, side, side.bit_length() - 1))

    def add(self, st, loss, params, roll):
        args = st.args
        if args.swt_weight:
            loss.add(image_ops.swt_haar(st.engine, params, st.grad, st.layer_weights['data'] * args.swt_weight,
                                        args.swt_power, roll=roll, levels=int(args.swt_levels)), st.engine)


class LapTerm(ImageTerm):
    """--lap-weight / --lap-pools (the Laplacian loss): ``target`` is D P_p u of the scale's first content
    picture for every pool size, on the master GPU; the previous scale's is freed when the next one is made."""
    needs_content = True

    def __init__(self, args):
        self.pools = check_lap_pools(args)
        self.target = None
        self._key = self._weights = None    # the last (--lap-pools, lap_weight) parsed

    def prepare(self, st, picture):
        target = image_ops.lap_target(st.engine, picture, self.pools)
        if self.target is not None:
            self.target.free()
        self.target = target

    def add(self, st, loss, params, roll):
        lap_weight = getattr(st.args, 'lap_weight', 0)
        if lap_weight:
            # the pool weights carry --lap-weight (sum |w| = lap_weight), the scale the data layer's factor
            loss.add(image_ops.lap_loss(st.engine, params, st.grad, self.target, self.pools,
                                        self.weights(st.args, lap_weight), st.layer_weights['data']), st.engine)

    def weights(self, args, lap_weight):
        """The weights of the target's pool sizes for this evaluation.  The sizes are those the target was
        made for: the target's layout follows from them, so an ``args.lap_pools`` that names other sizes
        by now is refused and never reaches the kernels."""
        spec = getattr(args, 'lap_pools', None) or LAP_POOLS_DEFAULT
        key = (tuple([spec] if isinstance(spec, str) else spec), lap_weight)
        if key != self._key:
            pools, weights = lap_pool_weights(key[0], lap_weight)
            if pools != self.pools:
                raise ValueError('--lap-pools changed from %s to %s during the run; the pool sizes are fixed '
                                 'when the run starts, only their weights may move' % (self.pools, pools))
            self._key, self._weights = key, weights
        return self._weights


class PhotoTerm(ImageTerm):
    """--photo-weight / --photo-eps (the photorealism regulariser): the matting Laplacian of the scale's first
    content picture, which stays on the master GPU for it."""
    needs_content = keeps_content = True

    def prepare(self, st, picture):
        if min(st.img.shape[1:]) < 3:
            raise ValueError('--photo-weight: a %d x %d image holds no 3 x 3 window (raise --min-size)'
                             % (st.img.shape[2], st.img.shape[1]))

    def add(self, st, loss, params, roll):
        photo_weight = getattr(st.args, 'photo_weight', 0)
        if photo_weight:
            eps = check_photo_options(st.args)
            if isinstance(eps, ValuePlaceholder):
                raise ValueError('--photo-eps is bound to run state that does not exist at an evaluation')
            loss.add(image_ops.photo_loss(st.engine, params, st.grad, st.content_picture, eps,
                                          st.layer_weights['data'] * photo_weight), st.engine)


class TemporalTerm(ImageTerm):
    """--temporal-weight / --prev-images / --flows / --flows-fwd / --temporal-init (temporal consistency for
    video): the earlier stylised frames and their flows are read when the run is set up; the flows go to the
    master GPU at first use and stay there.  Per scale ``target`` [3,H,W] and ``weight`` [H,W] are the composite
    of the earlier frames warped to this frame (image_ops.flow_warp, closest frame first); the previous
    scale's are freed when the next ones are made.  With --prev-contents no flow is read: both flows of every
    earlier frame are estimated on the master GPU at first use (flow.estimate_flow, at the content picture's size as
    loaded) -- ``flows_b[k]`` from the current content frame into earlier frame k, ``flows_f[k]`` the other way --
    and from there the path is the same."""

    def __init__(self, args):
        prev, flows, fwd = check_temporal_options(args)
        self.pictures = [Image.open(path).convert('RGB') for path in prev]
        with Image.open(args.content_image) as content:
            self.size0 = content.size           # (W0, H0): the content picture as loaded, the flows' frame
            self.frames = []                    # (--prev-contents: the current content frame, then the earlier ones)
            if temporal_prev_contents(args):
                self.frames.append(content.convert('RGB'))
        for path in temporal_prev_contents(args):
            frame = Image.open(path).convert('RGB')
            if frame.size != tuple(self.size0):
                raise ValueError('--prev-contents %s: a frame of %d x %d, but the content picture %s is %d x %d'
                                 % (path, frame.size[0], frame.size[1], args.content_image, *self.size0))
            self.frames.append(frame)
        self.flow_params = dict(alpha=flow_value(args, 'flow_alpha'), gamma=flow_value(args, 'flow_gamma'))

        def load(path):
            flow = read_flo(path)
            if (flow.shape[2], flow.shape[1]) != tuple(self.size0):
                raise ValueError('%s: a flow of %d x %d, but the content picture %s is %d x %d'
                                 % (path, flow.shape[2], flow.shape[1], args.content_image, *self.size0))
            return flow
        self.flows_b = [load(path) for path in flows]
        self.flows_f = [load(path) for path in fwd] or [None] * len(flows)
        self.target = self.weight = None
        self._on_device = False

    def composite(self, st, hw):
        """Makes ``target`` and ``weight`` for a scale of h x w, unless they are that scale's already."""
        h, w = int(hw[0]), int(hw[1])
        if self.weight is not None and tuple(self.weight.shape) == (h, w):
            return
        eng = st.engine
        if not self._on_device:
            if self.frames:
                current, earlier = self.frames[0], self.frames[1:]
                self.flows_b = [estimate_flow(eng, current, frame, **self.flow_params) for frame in earlier]
                self.flows_f = [estimate_flow(eng, frame, current, **self.flow_params) for frame in earlier]
                self.frames = []
            else:
                self.flows_b = [eng.to_device(flow) for flow in self.flows_b]
                self.flows_f = [eng.to_device(flow) if flow is not None else None for flow in self.flows_f]
            self._on_device = True
        target, weight = eng.empty((3, h, w)), eng.empty((h, w))
        su, sv = w / self.size0[0], h / self.size0[1]
        for index, (picture, flow_b, flow_f) in enumerate(zip(self.pictures, self.flows_b, self.flows_f)):
            # exactly as aux_image is brought to a scale
            prev = eng.to_device(st.pil_to_image(picture.resize((w, h), Image.LANCZOS)))
            # The flows are resampled like pictures.  An unknown marker (1e10) smears through the Lanczos window
            # into values that are still huge: they point far outside the frame, so c = 0 there -- around an
            # unknown pixel a few more pixels go free, which is the conservative outcome.
            scaled_b = resample_device(eng, flow_b, (h, w))
            scaled_f = resample_device(eng, flow_f, (h, w)) if flow_f is not None else None
            image_ops.flow_warp(eng, prev, scaled_b, scaled_f, su, sv, index == 0, target, weight)
            for arr in (prev, scaled_b, scaled_f):
                if arr is not None:
                    arr.free()
        for arr in (self.target, self.weight):
            if arr is not None:
                arr.free()
        self.target, self.weight = target, weight

    def prepare(self, st, picture):
        self.composite(st, st.img.shape[1:])

    def start_image(self, st, content):
        """--temporal-init: the start image [3,h,w] (host) of the scale whose content picture is the PIL image
        ``content`` -- the composite where its weight is set, the content picture elsewhere."""
        self.composite(st, (content.size[1], content.size[0]))
        return np.where(self.weight.get()[None] > 0, self.target.get(), st.pil_to_image(content))

    def add(self, st, loss, params, roll):
        temporal_weight = getattr(st.args, 'temporal_weight', 0)
        if temporal_weight:
            loss.add(image_ops.temporal_loss(st.engine, params, st.grad, self.target, self.weight,
                                             st.layer_weights['data'] * temporal_weight), st.engine)


def image_terms(args):
    """The image terms of a run, in the order they join the loss; a bad option is refused here."""
    weights = (('swt_weight', SwtTerm), ('lap_weight', LapTerm), ('photo_weight', PhotoTerm),
               ('temporal_weight', TemporalTerm))
    check_temporal_options(args)        # (--temporal-init without the term has no term to refuse it)
    return [cls(args) for name, cls in weights if option_on(args, name)]
