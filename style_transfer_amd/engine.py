"""Python face of one libstx tile engine (one GPU).

Mirrors the server side of the reference's tile-worker protocol: the three requests a
``TileWorker`` answers (``style_transfer.py:215-259``) become three methods with the same
argument meaning --

    FeatureMapRequest(img, layers)                    -> features_tile(img, layers)
    SCGradRequest(img, roll, start, content_layers,   -> sc_grad_tile(img, start, roll, ...)
                  style_layers, dd_layers, layer_weights,
                  content_weight, style_weight, dd_weight)
    SetContentsAndStyles(contents, styles)            -> set_contents_and_styles(contents, styles)

-- and the arithmetic behind them (``CaffeModel.eval_features_tile`` / ``eval_sc_grad_tile``,
``style_transfer.py:421-427,556-612``) runs in the HIP kernels of libstx.  Arrays may be numpy
(host) or ``DeviceArray`` (resident on the engine's GPU).
"""

import ctypes

import numpy as np

from . import lib
from .config_system import nnfm_bank_rows, selfsim_grid
from .netspec import NetSpec

_TYPE_CODES = {'Input': lib.LAYER_INPUT, 'Convolution': lib.LAYER_CONV, 'ReLU': lib.LAYER_RELU,
               'Pooling': lib.LAYER_POOL}
# the targets that tap layers of their own, in the order of their taps
EXTRA_TAP_KINDS = ('stat', 'nnfm', 'swd', 'selfsim', 'shift', 'cx')


class DeviceArray:
    """A float32 (or uint8) array living on an engine's GPU."""

    def __init__(self, engine, shape, dtype=np.float32):
        self.engine = engine
        self.shape = tuple(int(s) for s in shape)
        self.dtype = np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        ptr = ctypes.c_void_p()
        lib.call('stx_malloc', engine.handle, self.nbytes, ctypes.byref(ptr))
        self.ptr = ptr.value

    @classmethod
    def from_pointer(cls, engine, ptr, shape, dtype=np.float32, owner=None):
        """A view of device memory somebody else owns (e.g. a torch tensor: pass it as ``owner``
        to keep it alive).  ``free()`` does nothing."""
        arr = cls.__new__(cls)
        arr.engine, arr.shape, arr.dtype = engine, tuple(int(v) for v in shape), np.dtype(dtype)
        arr.nbytes = int(np.prod(arr.shape, dtype=np.int64)) * arr.dtype.itemsize
        arr.ptr, arr.owner = int(ptr), owner
        arr.free = lambda: None
        return arr

    @property
    def size(self):
        return int(np.prod(self.shape, dtype=np.int64))

    @property
    def __cuda_array_interface__(self):
        """Lets torch (``torch.as_tensor(arr, device=...)``) view the array without a copy, e.g.
        as the source of an RCCL broadcast.  The caller orders the streams (``engine.sync()``)."""
        return {'shape': self.shape, 'typestr': self.dtype.str, 'data': (int(self.ptr), False),
                'version': 2, 'strides': None}

    def set(self, host):
        host = np.ascontiguousarray(host, self.dtype)
        assert host.shape == self.shape, (host.shape, self.shape)
        lib.call('stx_memcpy_async', self.engine.handle, self.ptr, lib.DEVICE, host.ctypes.data,
                 lib.HOST, self.nbytes)
        self.engine.sync()
        return self

    def copy_from(self, other):
        assert other.nbytes == self.nbytes
        lib.call('stx_memcpy_async', self.engine.handle, self.ptr, lib.DEVICE, other.ptr,
                 lib.DEVICE, self.nbytes)
        return self

    def zero(self):
        lib.call('stx_memset_async', self.engine.handle, self.ptr, 0, self.nbytes)
        return self

    def get(self):
        out = np.empty(self.shape, self.dtype)
        lib.call('stx_memcpy_async', self.engine.handle, out.ctypes.data, lib.HOST, self.ptr,
                 lib.DEVICE, self.nbytes)
        self.engine.sync()
        return out

    def free(self):
        if self.ptr and self.engine.handle:
            lib.call('stx_free', self.engine.handle, self.ptr)
        self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:  # pylint: disable=broad-except
            pass


def _as_arg(arr):
    """(pointer, mem tag, keep-alive object) for a numpy array, a DeviceArray or a float32 torch
    tensor (on a GPU: used in place; on the CPU: its memory is the host buffer)."""
    if isinstance(arr, DeviceArray):
        return arr.ptr, lib.DEVICE, arr
    if hasattr(arr, 'data_ptr') and hasattr(arr, 'is_cuda'):        # torch.Tensor, no import
        t = arr.contiguous()
        if str(t.dtype) != 'torch.float32':
            t = t.float()
        return t.data_ptr(), (lib.DEVICE if t.is_cuda else lib.HOST), t
    host = np.ascontiguousarray(arr, np.float32)
    return host.ctypes.data, lib.HOST, host


def _shift_offsets(offsets):
    """Offsets [n, 2] = (dy, dx) of the shifted-Gram term as a C int array of 2 n entries (the library checks them)."""
    flat = np.asarray(offsets)
    if flat.ndim != 2 or flat.shape[1] != 2 or flat.shape[0] < 1 or flat.dtype.kind not in 'iu':
        raise ValueError('shifted-Gram offsets %r: an [n, 2] list of integer (dy, dx) pairs is expected' % (offsets,))
    return (ctypes.c_int * flat.size)(*[int(v) for v in flat.ravel()])


class PendingTile:
    """Result of an asynchronous sc_grad_tile: valid after ``engine.sync()``."""

    def __init__(self, grad, keep):
        self._loss = ctypes.c_double(float('nan'))
        self.grad = grad
        self._keep = keep

    @property
    def loss(self):
        return self._loss.value


class TileEngine:
    """One GPU's worker: the network, its weights and the current targets."""

    def __init__(self, net, device=0, weights=None, share=None):
        """``share``: an engine on the same GPU whose weights, packed filter banks and targets
        this one uses (stx_engine_create_shared); ``weights`` is then ignored."""
        assert isinstance(net, NetSpec)
        self.net = net
        self.device = device
        self.handle = None
        self._names = {}
        self.primary = share.primary if share is not None else self
        handle = ctypes.c_void_p()
        if share is not None:
            assert share.device == device and share.net is net
            lib.call('stx_engine_create_shared', share.handle, ctypes.byref(handle))
        else:
            descs = (lib.LayerDesc * len(net.layers))()
            for d, lay in zip(descs, net.layers):
                d.name = self._cstr(lay.name)
                d.type = _TYPE_CODES[lay.type]
                d.bottom = self._cstr(lay.bottom) if lay.bottom else None
                d.top = self._cstr(lay.top)
                d.num_output = lay.num_output if lay.type != 'Input' else \
                    (lay.shape[1] if lay.shape else 3)
                d.kernel_size, d.pad, d.stride = lay.kernel_size, lay.pad, lay.stride
                d.pool_mode = lib.POOL_AVE if lay.pool == 'AVE' else lib.POOL_MAX
            lib.call('stx_engine_create', device, descs, len(net.layers), ctypes.byref(handle))
        self.handle = handle
        self._results = []
        self._info = {b: net.layer_info(b) for b in net.blob_names()}
        self.n_styles = 0
        # (of the primary) the layers that the group's extra targets tap, by kind: kept like the library keeps
        # the targets -- emptied by set_contents_and_styles, one kind replaced by its setter
        self.extra_taps = {kind: [] for kind in EXTRA_TAP_KINDS}
        if weights and share is None:
            for name, (w, b) in weights.items():
                self.set_weights(name, w, b)

    def _cstr(self, s):
        """Encoded layer name, kept alive for as long as the engine (one entry per distinct
        name: tap tables are rebuilt on every call)."""
        b = self._names.get(s)
        if b is None:
            b = self._names[s] = s.encode()
        return b

    def close(self):
        if self.handle:
            lib.load().stx_engine_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # pylint: disable=broad-except
            pass

    # ------------------------------------------------------------------------------ basics
    def sync(self):
        lib.call('stx_sync', self.handle)
        self._results = []
        self._fence_marks = {}
        self._dropped = 0

    def keep_until_sync(self, result):
        """Holds a reference to an object the library will write into at the next sync (a
        pending loss): it must not be collected before, even if its owner lets go of it.  The
        library publishes pending values whenever it drains its scalar arena, also inside calls
        that never come back through ``sync()``.  Entries are dropped when their values have been
        published: at ``sync()`` and at ``wait_fence()`` (everything queued before that fence).  The
        count below is a backstop for callers that never do either -- the library drains its arena
        every few hundred evaluations, so an entry 2048 evaluations old has long been written.  (Each
        entry pins a tile-sized host buffer: the cap stays small.)"""
        self._results.append(result)
        if len(self._results) > 4096:
            del self._results[:2048]
            self._dropped = getattr(self, '_dropped', 0) + 2048
        return result

    def fence(self):
        """Closes the pending values queued so far behind an event and returns a ticket for
        ``wait_fence`` (stx_fence): the host can queue the next iteration first and collect this
        one's losses afterwards, without waiting for the newer work."""
        ticket = ctypes.c_ulonglong(0)
        lib.call('stx_fence', self.handle, ctypes.byref(ticket))
        if not hasattr(self, '_fence_marks'):
            self._fence_marks, self._dropped = {}, 0
        self._fence_marks[ticket.value] = self._dropped + len(self._results)
        return ticket.value

    def wait_fence(self, ticket):
        """Waits for the fence's event only and publishes the values it closed; the objects
        those values were written into are released from ``keep_until_sync``."""
        lib.call('stx_fence_wait', self.handle, int(ticket))
        mark = getattr(self, '_fence_marks', {}).pop(int(ticket), None)
        if mark is not None:
            n = mark - self._dropped
            if n > 0:
                del self._results[:n]
                self._dropped += n

    def wait_for(self, other):
        """Orders this engine's stream behind what ``other`` has queued so far (no host wait)."""
        if other is not self:
            lib.call('stx_engine_wait', self.handle, other.handle)

    def query(self, what):
        """One of the lib.Q_* counters."""
        v = ctypes.c_double(0)
        lib.call('stx_engine_query', self.handle, int(what), ctypes.byref(v))
        return v.value

    def empty(self, shape, dtype=np.float32):
        return DeviceArray(self, shape, dtype)

    def to_device(self, host, dtype=np.float32):
        host = np.ascontiguousarray(host, dtype)
        return DeviceArray(self, host.shape, dtype).set(host)

    def layer_info(self, layer):
        """(scale, channels) -- CaffeModel.layer_info, style_transfer.py:415-419."""
        return self._info[layer]

    def feature_shape(self, layer, th, tw):
        if layer not in self._info:
            raise lib.StxError('feature_shape', -1, "unknown layer '%s'" % layer)
        scale, ch = self._info[layer]
        h, w = th, tw
        s = 1
        while s < scale:          # one ceil-mode halving per pooling stage
            h, w, s = (h + 1) // 2, (w + 1) // 2, s * 2
        return ch, h, w

    def set_weights(self, conv_layer, w, b):
        """w [Cout,Cin,k,k], b [Cout]: numpy, DeviceArray or torch tensors (device-resident
        sources are copied on the engine's stream, e.g. straight out of an RCCL broadcast)."""
        wp, wmem, wkeep = _as_arg(w)
        bp, bmem, bkeep = _as_arg(b)
        if wmem != bmem:
            raise ValueError('weights and bias must live on the same side')
        lib.call('stx_set_conv_weights', self.handle, conv_layer.encode(), wp, bp, wmem)
        if wmem == lib.DEVICE:
            self.sync()          # the sources may be released once this returns
        del wkeep, bkeep

    # ------------------------------------------------------------- SetContentsAndStyles
    def set_contents_and_styles(self, contents, styles):
        """contents: list of {layer: [C,h,w] full-image feature map}; styles: list of
        {layer: [C,C] lower-triangular Gram} (style_transfer.py:243-254)."""
        keep = []
        n_c = sum(len(c) for c in contents)
        n_s = sum(len(s) for s in styles)
        ctargets = (lib.ContentTarget * max(1, n_c))()
        starget = (lib.StyleTarget * max(1, n_s))()
        i = 0
        for ci, content in enumerate(contents):
            for layer, feat in content.items():
                ptr, mem, obj = _as_arg(feat)
                keep.append(obj)
                t = ctargets[i]
                t.content_index, t.layer = ci, self._cstr(layer)
                t.channels, t.height, t.width = obj.shape
                t.features, t.mem = ptr, mem
                i += 1
        i = 0
        for si, style in enumerate(styles):
            for layer, gram in style.items():
                ptr, mem, obj = _as_arg(gram)
                keep.append(obj)
                t = starget[i]
                t.style_index, t.layer, t.channels = si, self._cstr(layer), obj.shape[0]
                t.gram, t.mem = ptr, mem
                i += 1
        lib.call('stx_set_contents_and_styles', self.handle, ctargets, n_c, starget, n_s)
        self.n_styles = len(styles)
        # (the library clears the extra targets with these)
        self.primary.extra_taps = {kind: [] for kind in EXTRA_TAP_KINDS}

    def set_stat_targets(self, targets, weights=None):
        """targets: {layer: (mean [C], sd [C])} -- what ``feature_stats`` gives for a style picture's
        feature map -- and weights: {layer: factor} (default 1 each); an empty dict: no targets
        (stx_set_stat_targets).  Call it after ``set_contents_and_styles``, which clears them.  A layer
        with a target is part of every tile evaluation of the group from then on."""
        keep, n = [], len(targets)
        table = (lib.StatTarget * max(1, n))()
        for t, (layer, (mean, sd)) in zip(table, targets.items()):
            mp, mmem, mobj = _as_arg(mean)
            sp, smem, sobj = _as_arg(sd)
            if mmem != smem or mobj.shape != sobj.shape or len(mobj.shape) != 1:
                raise ValueError('statistics target %s: mean and sd are two [C] arrays on the same side' % layer)
            keep += [mobj, sobj]
            t.layer, t.channels, t.mean, t.sd, t.mem = self._cstr(layer), int(mobj.shape[0]), mp, sp, mmem
            t.weight = float(weights.get(layer, 1.0)) if weights is not None else 1.0
        lib.call('stx_set_stat_targets', self.handle, table, n)
        self.primary.extra_taps['stat'] = list(targets)
        del keep

    def set_nnfm_targets(self, banks, weights=None, patch=1, k=1, cover=0.0, segments=None, masks=None):
        """banks: {layer: B [rows, C]} -- unit rows, what ``nnfm_bank`` gives for a style picture's feature map
        (banks of several pictures concatenated) -- and weights: {layer: factor} (default 1 each); an empty
        dict: none.  The library copies a bank and builds its fp16 pieces once, here.  Call it after ``set_contents_and_styles``, which clears the banks.  A layer with a bank is part of
        every tile evaluation of the group from then on.  ``patch`` 3: banks of 3 x 3 patches, [rows, 9 C] as
        ``nnfm_bank(feat, stride, 3)`` gives them.  Both forms are patch targets of the library
        (stx_set_nnfm_patch_targets), the plain one with patch 1.  ``k`` 2 to 4: every vector is pulled towards
        the mean of its k best rows (stx_set_nnfm_knn_targets); with k = 1 the calls are those without it.
        ``cover`` above 0: that factor times the coverage part -- every bank row pulls its most similar vector
        towards itself -- is added (stx_set_nnfm_cover_targets; patch 1 only); with 0 the calls are those
        without it.  ``segments`` = {layer: [rows of style picture 0's part of the bank, of picture 1's, ...]} and
        ``masks`` = one [H, W] array in [0, 1] per style picture, in the frame of the current targets: the guided
        term (stx_set_nnfm_guided_targets; patch 1, no cover) -- a feature vector looks into a picture's rows with
        the weight of that picture's mask."""
        if (segments is None) != (masks is None):
            raise ValueError('NNFM banks: segments and masks go together')
        if masks is not None:
            return self._set_nnfm_guided_targets(banks, weights, patch, k, cover, segments, masks)
        if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= 4:
            raise ValueError('NNFM banks, k %r: an integer from 1 to 4 is expected' % (k,))
        if isinstance(cover, bool) or not isinstance(cover, (int, float)) or not 0 <= cover < float('inf'):
            raise ValueError('NNFM banks, cover %r: a finite number >= 0 is expected' % (cover,))
        if cover != 0 and patch != 1:
            raise ValueError('NNFM banks, cover %r with patch %r: the coverage part matches single vectors only'
                             % (cover, patch))
        keep, n = [], len(banks)
        kind, call = ((lib.NnfmCoverTarget, 'stx_set_nnfm_cover_targets') if cover != 0 else
                      (lib.NnfmPatchTarget, 'stx_set_nnfm_patch_targets') if k == 1 else
                      (lib.NnfmKnnTarget, 'stx_set_nnfm_knn_targets'))
        table = (kind * max(1, n))()
        for t, (layer, bank) in zip(table, banks.items()):
            ptr, mem, obj = _as_arg(bank)
            if patch == 1 and len(obj.shape) != 2:
                raise ValueError('NNFM bank %s: a [rows, C] array is expected' % layer)
            if patch != 1 and (len(obj.shape) != 2 or isinstance(patch, bool) or patch != 3 or obj.shape[1] % 9):
                raise ValueError('NNFM bank %s, patch %r: a [rows, patch * patch * C] array and patch 1 or 3 are '
                                 'expected' % (layer, patch))
            keep.append(obj)
            t.layer, t.patch, t.rows = self._cstr(layer), int(patch), int(obj.shape[0])
            t.channels, t.bank, t.mem = int(obj.shape[1]) // (t.patch * t.patch), ptr, mem
            t.weight = float(weights.get(layer, 1.0)) if weights is not None else 1.0
            if k != 1 or cover != 0:
                t.k = k
            if cover != 0:
                t.cover = float(cover)
        lib.call(call, self.handle, table, n)
        self.primary.extra_taps['nnfm'] = list(banks)
        del keep

    def _set_nnfm_guided_targets(self, banks, weights, patch, k, cover, segments, masks):
        if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= 4:
            raise ValueError('NNFM banks, k %r: an integer from 1 to 4 is expected' % (k,))
        if patch != 1 or cover != 0:
            raise ValueError('NNFM banks with masks, patch %r and cover %r: the guided term matches single vectors '
                             'and has no coverage part' % (patch, cover))
        if not 1 <= len(masks) <= lib.NNFM_MAX_SEGMENTS:
            raise ValueError('NNFM banks with masks: %d masks (1 to %d are expected)' % (len(masks),
                                                                                       lib.NNFM_MAX_SEGMENTS))
        keep, n, shape, mems = [], len(banks), None, set()
        mask_ptrs = (ctypes.c_void_p * len(masks))()
        for si, mask in enumerate(masks):
            ptr, mem, obj = _as_arg(mask)
            if len(obj.shape) != 2 or (shape is not None and tuple(obj.shape) != shape):
                raise ValueError('NNFM mask %d: [H, W] arrays of one size are expected, not %s' % (si, tuple(obj.shape)))
            shape = tuple(obj.shape)
            keep.append(obj)
            mems.add(mem)
            mask_ptrs[si] = ptr
        if len(mems) != 1:
            raise ValueError('NNFM masks: all on the host or all on the device')
        table = (lib.NnfmGuidedTarget * max(1, n))()
        for t, (layer, bank) in zip(table, banks.items()):
            ptr, mem, obj = _as_arg(bank)
            rows = [int(r) for r in segments[layer]]
            if len(obj.shape) != 2 or len(rows) != len(masks) or sum(rows) != int(obj.shape[0]):
                raise ValueError('NNFM bank %s: a [rows, C] array and %d segment row counts that add up to its rows '
                                 'are expected, not %s and %s' % (layer, len(masks), tuple(obj.shape), rows))
            if min(rows) < k:
                raise ValueError('NNFM bank %s: a segment of %d rows, fewer than k = %d' % (layer, min(rows), k))
            seg_rows = (ctypes.c_int * len(rows))(*rows)
            keep += [obj, seg_rows]
            t.layer, t.channels, t.k, t.segments, t.seg_rows = self._cstr(layer), int(obj.shape[1]), k, len(rows), seg_rows
            t.bank, t.mem = ptr, mem
            t.weight = float(weights.get(layer, 1.0)) if weights is not None else 1.0
        lib.call('stx_set_nnfm_guided_targets', self.handle, table, n, mask_ptrs, len(masks), int(shape[0]),
                 int(shape[1]), mems.pop())
        self.primary.extra_taps['nnfm'] = list(banks)
        del keep

    def set_swd_targets(self, targets, weights=None):
        """targets: {layer: (V [D, C], Tq [D, Q])} -- unit directions and, per direction, the quantile function
        that ``swd_target`` gives for a style picture's feature map -- and weights: {layer: factor} (default 1
        each); an empty dict: none (stx_set_swd_targets).  The library copies both.  Call it after
        ``set_contents_and_styles``, which clears them.  A layer with a target is part of every tile evaluation
        of the group from then on."""
        keep, n = [], len(targets)
        table = (lib.SwdTarget * max(1, n))()
        for t, (layer, (V, Tq)) in zip(table, targets.items()):
            vp, vmem, vobj = _as_arg(V)
            qp, qmem, qobj = _as_arg(Tq)
            if vmem != qmem or len(vobj.shape) != 2 or len(qobj.shape) != 2 or vobj.shape[0] != qobj.shape[0]:
                raise ValueError('sliced Wasserstein target %s: V [D, C] and Tq [D, Q] on the same side are expected'
                                 % layer)
            keep += [vobj, qobj]
            t.layer, t.channels, t.dirs, t.quantiles = (self._cstr(layer), int(vobj.shape[1]), int(vobj.shape[0]),
                                                        int(qobj.shape[1]))
            t.V, t.Tq, t.mem = vp, qp, vmem
            t.weight = float(weights.get(layer, 1.0)) if weights is not None else 1.0
        lib.call('stx_set_swd_targets', self.handle, table, n)
        self.primary.extra_taps['swd'] = list(targets)
        del keep

    def set_selfsim_targets(self, points, weights=None):
        """points: {layer: the most grid positions, 2 .. 4096} -- one self-similarity target per layer, each at a layer
        that holds a content map of content_index 0, which is all the term reads -- and weights: {layer: factor}
        (default 1 each); an empty dict: none (stx_set_selfsim_targets).  Call it after ``set_contents_and_styles``,
        which clears them.  A layer with a target is part of every tile evaluation of the group from then on."""
        n = len(points)
        table = (lib.SelfsimTarget * max(1, n))()
        for t, (layer, count) in zip(table, points.items()):
            t.layer, t.points = self._cstr(layer), int(count)
            t.weight = float(weights.get(layer, 1.0)) if weights is not None else 1.0
        lib.call('stx_set_selfsim_targets', self.handle, table, n)
        self.primary.extra_taps['selfsim'] = list(points)

    def set_shift_targets(self, targets, weights=None):
        """targets: {layer: (offsets [n, 2] = dy, dx, T [n, C, C])} -- what ``shift_gram`` gives for a style picture's
        feature map at those offsets -- and weights: {layer: factor} (default 1 each); an empty dict: none
        (stx_set_shift_targets).  The library copies both.  Call it after ``set_contents_and_styles``, which clears
        them.  A layer with a target is part of every tile evaluation of the group from then on."""
        keep, n = [], len(targets)
        table = (lib.ShiftTarget * max(1, n))()
        for t, (layer, (offsets, grams)) in zip(table, targets.items()):
            offs = _shift_offsets(offsets)
            gp, gmem, gobj = _as_arg(grams)
            if len(gobj.shape) != 3 or gobj.shape[0] != len(offs) // 2 or gobj.shape[1] != gobj.shape[2]:
                raise ValueError('shifted-Gram target %s: T %s for %d offsets; [n, C, C] is expected'
                                 % (layer, tuple(gobj.shape), len(offs) // 2))
            keep += [offs, gobj]
            t.layer, t.channels, t.n_offsets, t.offsets = self._cstr(layer), int(gobj.shape[1]), len(offs) // 2, offs
            t.grams, t.mem = gp, gmem
            t.weight = float(weights.get(layer, 1.0)) if weights is not None else 1.0
        lib.call('stx_set_shift_targets', self.handle, table, n)
        self.primary.extra_taps['shift'] = list(targets)
        del keep

    def shift_gram(self, feat, offsets):
        """X [n, C, C] float32: the shifted Grams of a [C,h,w] feature map at ``offsets`` [n, 2] = (dy, dx), each
        (0, d) or (d, 0) with d >= 1 (stx_shift_gram): the targets of the shifted-Gram style term."""
        ptr, mem, keep = _as_arg(feat)
        c, h, w = (int(v) for v in keep.shape)
        offs = _shift_offsets(offsets)
        out = np.empty((len(offs) // 2, c, c), np.float32)
        lib.call('stx_shift_gram', self.handle, ptr, mem, c, h, w, offs, len(offs) // 2, out.ctypes.data)
        return out

    def set_cx_targets(self, banks, weights=None, points=1024, h=0.5):
        """banks: {layer: Y [rows, C]} -- RAW feature vectors, what ``cx_rows`` gives for a style picture's feature
        map (rows of several pictures concatenated) -- and weights: {layer: factor} (default 1 each); an empty dict:
        none (stx_set_cx_targets).  The library copies the rows and builds their mean and the centred unit rows
        once, here.  ``points``: the most sample positions per tile, 2 to 4096; ``h``: the bandwidth, above 0.
        Call it after ``set_contents_and_styles``, which clears the targets.  A layer with a target is part of
        every tile evaluation of the group from then on."""
        keep, n = [], len(banks)
        table = (lib.CxTarget * max(1, n))()
        for t, (layer, rows) in zip(table, banks.items()):
            ptr, mem, obj = _as_arg(rows)
            if len(obj.shape) != 2:
                raise ValueError('contextual bank %s: a [rows, C] array is expected' % layer)
            keep.append(obj)
            t.layer, t.channels, t.rows = self._cstr(layer), int(obj.shape[1]), int(obj.shape[0])
            t.raw_rows, t.mem, t.points, t.h = ptr, mem, int(points), float(h)
            t.weight = float(weights.get(layer, 1.0)) if weights is not None else 1.0
        lib.call('stx_set_cx_targets', self.handle, table, n)
        self.primary.extra_taps['cx'] = list(banks)
        del keep

    def cx_rows(self, feat, rows):
        """The raw rows of a [C,h,w] feature map for a contextual bank as a DeviceArray [N, C]: its columns on the
        grid of a budget of ``rows`` positions (config_system.selfsim_grid), raster order (stx_cx_rows).  Nothing
        travels through the host when ``feat`` is on the device."""
        ptr, mem, keep = _as_arg(feat)
        c, h, w = (int(v) for v in keep.shape)
        _, gh, gw = selfsim_grid(h, w, int(rows))
        out = DeviceArray(self, (gh * gw, c))
        lib.call('stx_cx_rows', self.handle, ptr, mem, c, h, w, int(rows), out.ptr, lib.DEVICE)
        return out

    def swd_target(self, feat, V, Q):
        """Tq [D, Q] float32: per direction of V [D, C] the quantile function of a [C,h,w] feature map's
        projections, sampled at (q + 1/2) / Q (stx_swd_target); with Q = h w the sorted projections themselves."""
        ptr, mem, keep = _as_arg(feat)
        c, h, w = (int(v) for v in keep.shape)
        V = np.ascontiguousarray(V, np.float32)
        if V.ndim != 2 or V.shape[1] != c:
            raise ValueError('swd_target: V %s for a map of %d channels; [D, C] is expected' % (V.shape, c))
        out = np.empty((V.shape[0], int(Q)), np.float32)
        lib.call('stx_swd_target', self.handle, ptr, mem, c, h, w, V.ctypes.data, int(V.shape[0]), int(Q),
                 out.ctypes.data)
        return out

    def nnfm_bank(self, feat, stride=1, patch=1):
        """The bank of a [C,h,w] feature map as a DeviceArray [rows, C]: its unit-normalised columns at every
        ``stride``-th row and column, raster order.  Nothing travels through the host when ``feat`` is on the
        device.  ``patch`` 3: the unit 3 x 3 patches centred there, [rows, 9 C]; a bank past the library's 2^31
        offsets is refused before it is allocated.  One call for both (stx_nnfm_patch_bank, patch 1 or 3)."""
        ptr, mem, keep = _as_arg(feat)
        c, h, w = (int(v) for v in keep.shape)
        rows = nnfm_bank_rows(c, h, w, stride, patch)
        out = DeviceArray(self, (rows, patch * patch * c))
        lib.call('stx_nnfm_patch_bank', self.handle, ptr, mem, c, h, w, int(patch), int(stride), out.ptr, lib.DEVICE)
        return out

    def concat_rows(self, parts):
        """One DeviceArray [sum of rows, C] of the DeviceArrays ``parts`` ([rows_k, C] each), in their order,
        copied on the device; the parts are freed."""
        if len(parts) == 1:
            return parts[0]
        out = DeviceArray(self, (sum(p.shape[0] for p in parts), parts[0].shape[1]))
        at = 0
        for p in parts:
            lib.call('stx_memcpy_async', self.handle, out.ptr + at, lib.DEVICE, p.ptr, lib.DEVICE, p.nbytes)
            at += p.nbytes
        self.sync()
        for p in parts:
            p.free()
        return out

    def feature_stats(self, feat):
        """(mean [C], sd [C]) of a [C,h,w] feature map, sd = sqrt(population variance + 1e-5), as float32
        (stx_feature_stats): the targets of the mean / std style term."""
        ptr, mem, keep = _as_arg(feat)
        c = keep.shape[0]
        hw = int(np.prod(keep.shape[1:]))
        mean, sd = np.empty(c, np.float32), np.empty(c, np.float32)
        lib.call('stx_feature_stats', self.handle, ptr, mem, c, hw, mean.ctypes.data, sd.ctypes.data, lib.HOST)
        return mean, sd

    def set_style_masks(self, masks):
        """masks: one entry per style set of the current targets, in their order -- an [H, W] array
        in [0, 1] in the content picture's frame (numpy, DeviceArray or torch tensor; white = the style
        applies) or None (that style acts everywhere) -- or an empty list: no masks
        (stx_set_style_masks).  Call it after ``set_contents_and_styles``, which clears them."""
        keep, entries = [], []
        for si, mask in enumerate(masks):
            if mask is None:
                continue
            ptr, mem, obj = _as_arg(mask)
            if len(obj.shape) != 2:
                raise ValueError('style mask %d: an [H, W] array is expected, not %s' % (si, tuple(obj.shape)))
            keep.append(obj)
            entries.append((si, int(obj.shape[0]), int(obj.shape[1]), ptr, mem))
        table = (lib.StyleMask * max(1, len(entries)))()
        for t, (si, h, w, ptr, mem) in zip(table, entries):
            t.style_index, t.H, t.W, t.mask, t.mem = si, h, w, ptr, mem
        lib.call('stx_set_style_masks', self.handle, table, len(entries))
        del keep

    def set_content_mask(self, mask):
        """mask: an [H, W] array in [0, 1] in the content picture's frame (numpy, DeviceArray or torch tensor;
        white = the content picture is held there, black = the content term is off there), applied to every
        content target, or None: no mask (stx_set_content_mask).  Call it after ``set_contents_and_styles``,
        which clears it."""
        if mask is None:
            lib.call('stx_set_content_mask', self.handle, None, 0, 0, lib.HOST)
            return
        ptr, mem, keep = _as_arg(mask)
        if len(keep.shape) != 2:
            raise ValueError('content mask: an [H, W] array is expected, not %s' % (tuple(keep.shape),))
        lib.call('stx_set_content_mask', self.handle, ptr, int(keep.shape[0]), int(keep.shape[1]), mem)
        del keep

    # --------------------------------------------------------------------- FeatureMapRequest
    def features_tile(self, img, layers):
        """Post-ReLU feature maps of one tile: {layer: [C, ceil(th/s), ceil(tw/s)] ndarray}."""
        ptr, mem, keep = _as_arg(img)
        th, tw = keep.shape[-2:]
        outs = [np.empty(self.feature_shape(l, th, tw), np.float32) for l in layers]
        names = (ctypes.c_char_p * len(layers))(*[l.encode() for l in layers])
        ptrs = (ctypes.c_void_p * len(layers))(*[o.ctypes.data for o in outs])
        lib.call('stx_features_tile', self.handle, ptr, mem, th, tw, names, len(layers), ptrs,
                 lib.HOST)
        self.sync()
        return dict(zip(layers, outs))

    def features_tile_device(self, img, layers, out=None):
        """Like features_tile, but the maps stay on the GPU: {layer: DeviceArray}.  ``out`` may
        supply the destination arrays (reused across tiles).  Asynchronous."""
        ptr, mem, keep = _as_arg(img)
        th, tw = keep.shape[-2:]
        if out is None:
            out = {}
        for l in layers:
            shape = self.feature_shape(l, th, tw)
            if l not in out or out[l].shape != shape:
                out[l] = self.empty(shape)
        names = (ctypes.c_char_p * len(layers))(*[l.encode() for l in layers])
        ptrs = (ctypes.c_void_p * len(layers))(*[out[l].ptr for l in layers])
        lib.call('stx_features_tile', self.handle, ptr, mem, th, tw, names, len(layers), ptrs,
                 lib.DEVICE)
        if mem == lib.HOST:
            self.sync()
        return out

    def map_place(self, dst, y0, x0, src):
        """dst[:, y0:y0+h, x0:x0+w] = src on the device (feature-map stitch)."""
        c, h, w = src.shape
        lib.call('stx_map_place', self.handle, dst.ptr, c, dst.shape[1], dst.shape[2], int(y0),
                 int(x0), src.ptr, h, w)

    def map_roll_add(self, acc, src, roll_xy, alpha, init_divisor=0.0):
        """acc = roll2(src, roll_xy) / init_divisor, or acc += alpha * roll2(src, roll_xy)."""
        c, h, w = src.shape
        roll = (ctypes.c_int * 2)(int(roll_xy[0]), int(roll_xy[1]))
        lib.call('stx_map_roll_add', self.handle, acc.ptr, src.ptr, c, h, w, roll, float(alpha),
                 float(init_divisor))

    # --------------------------------------------------------------------------- SCGradRequest
    def _taps(self, content_layers, style_layers, layer_weights, content_weight, style_weight,
              dd_layers=(), dd_weight=None):
        # (a layer that only a statistics target names is tapped for nothing: the tap carries its layer weight)
        names = list(dict.fromkeys(list(content_layers) + list(style_layers) + list(dd_layers) +
                                   sum(self.primary.extra_taps.values(), [])))
        taps = (lib.Tap * len(names))()
        for t, name in zip(taps, names):
            t.layer = self._cstr(name)
            t.layer_weight = float(layer_weights.get(name, 1.0)) if layer_weights else 1.0
            t.is_content = int(name in content_layers)
            t.content_weight = float(content_weight.get(name, 0.0)) if t.is_content else 0.0
            t.is_style = int(name in style_layers)
            t.style_weight = float(style_weight.get(name, 0.0)) if t.is_style else 0.0
            t.is_dd = int(name in dd_layers)
            t.dd_weight = float(dd_weight.get(name, 0.0)) if t.is_dd and dd_weight else 0.0
        return taps, len(names)

    def io_buffers(self, th, tw):
        """(tile, gradient) DeviceArray views of the engine's own input blob and of the blob its
        gradient is left in: a tile written into the first and evaluated with grad_out = the
        second needs no copies (stx_tile_buffers).  Query before every use."""
        tin, gout = ctypes.c_void_p(), ctypes.c_void_p()
        lib.call('stx_tile_buffers', self.handle, int(th), int(tw), ctypes.byref(tin), ctypes.byref(gout))
        return (DeviceArray.from_pointer(self, tin.value, (3, th, tw)),
                DeviceArray.from_pointer(self, gout.value, (3, th, tw)))

    def sc_grad_tile_async(self, img, start, roll, content_layers, style_layers, layer_weights,
                           content_weight, style_weight, grad_out=None, dd_layers=(),
                           dd_weight=None):
        """Enqueues one tile evaluation; returns a PendingTile (read it after ``sync()``)."""
        ptr, mem, keep = _as_arg(img)
        th, tw = keep.shape[-2:]
        if grad_out is None:
            grad_out = np.empty((3, th, tw), np.float32)
        gptr, gmem, gkeep = (grad_out.ptr, lib.DEVICE, grad_out) \
            if isinstance(grad_out, DeviceArray) else (grad_out.ctypes.data, lib.HOST, grad_out)
        taps, n_taps = self._taps(content_layers, style_layers, layer_weights, content_weight,
                                  style_weight, dd_layers, dd_weight)
        roll_c = (ctypes.c_int * 2)(int(roll[0]), int(roll[1])) if roll is not None \
            else (ctypes.c_int * 2)(0, 0)
        start_c = (ctypes.c_int * 2)(int(start[0]), int(start[1]))
        pending = self.keep_until_sync(PendingTile(gkeep, (keep, taps)))
        lib.call('stx_sc_grad_tile', self.handle, ptr, mem, th, tw, roll_c, start_c, taps, n_taps,
                 ctypes.byref(pending._loss), gptr, gmem, 0)
        return pending

    def sc_grad_tile(self, img, start, roll, content_layers, style_layers, layer_weights,
                     content_weight, style_weight, dd_layers=(), dd_weight=None):
        """(loss, grad[3,th,tw]) of one tile -- CaffeModel.eval_sc_grad_tile with the worker's
        content roll (style_transfer.py:230-241,556-612)."""
        pending = self.sc_grad_tile_async(img, start, roll, content_layers, style_layers,
                                          layer_weights, content_weight, style_weight,
                                          dd_layers=dd_layers, dd_weight=dd_weight)
        self.sync()
        return pending.loss, pending.grad

    def gram_matrix(self, feat):
        """Lower-triangular Gram of a [C,h,w] feature map (num_utils.py:143-147)."""
        ptr, mem, keep = _as_arg(feat)
        c = keep.shape[0]
        hw = int(np.prod(keep.shape[1:]))
        out = np.empty((c, c), np.float32)
        lib.call('stx_gram_matrix', self.handle, ptr, mem, c, hw, out.ctypes.data, lib.HOST)
        return out

    def profile(self, on=True):
        """Turns per-kernel-group event timing on or off (clears the record)."""
        lib.call('stx_profile_enable', self.handle, int(on))

    def profile_read(self, clock=False):
        """[(label, milliseconds, algorithmic flops)] recorded since the last read; with
        ``clock=True`` a fourth field: the shader clock in MHz inside the group's convolution kernel
        (0 unless clock_marks is on and the group is a 2-D Winograd launch)."""
        buf = ctypes.create_string_buffer(1 << 20)
        lib.call('stx_profile_read', self.handle, buf, len(buf), None)
        rows = []
        for line in buf.value.decode().splitlines():
            label, ms, flops, mhz = line.split('\t')
            rows.append((label, float(ms), float(flops), float(mhz)) if clock else
                        (label, float(ms), float(flops)))
        return rows

    def amax_audit(self, on=True):
        """Turns the audit of the maxima handed from kernel to kernel on or off (stx_amax_audit; clears the
        record).  For the tests: while on, every hand-off costs a copy and a pass over the consumer's input."""
        lib.call('stx_amax_audit', self.handle, int(on))

    def amax_audit_read(self):
        """[(consumer, blob, 'data' | 'diff', blob whose slots were read, recorded, measured)] of the hand-offs
        since the last read, the two maxima as float32 bit patterns (ints): recorded >= measured is what the
        fp16-split kernels rely on.  Empty while the audit is off."""
        buf = ctypes.create_string_buffer(1 << 20)
        lib.call('stx_amax_audit_read', self.handle, buf, len(buf), None)
        rows = []
        for line in buf.value.decode().splitlines():
            consumer, blob, kind, source, recorded, measured = line.split('\t')
            rows.append((consumer, blob, kind, source, int(recorded, 16), int(measured, 16)))
        return rows

    def last_tile_flops(self):
        """(algorithmic, issued) matrix-core FLOP of the convolutions of the last tile call."""
        a, b = ctypes.c_double(0), ctypes.c_double(0)
        lib.call('stx_last_tile_flops', self.handle, ctypes.byref(a), ctypes.byref(b))
        return a.value, b.value

    def clock_marks(self, on):
        """While on, one workgroup of every 2-D Winograd convolution launch of this engine times its
        chunk loop with the core-cycle counter and the constant 100 MHz counter (stx_clock_marks):
        the shader clock inside the kernel that does most of the work."""
        lib.call('stx_clock_marks', self.handle, 1 if on else 0)

    def clock_marks_read(self, max_values=16384):
        """MHz of the marks recorded since the last read, launch order (0: a loop too short to
        tell); synchronises this engine's stream and clears the record."""
        mhz = (ctypes.c_double * max_values)()
        n = ctypes.c_int(0)
        lib.call('stx_clock_marks_read', self.handle, mhz, max_values, ctypes.byref(n))
        return [mhz[i] for i in range(n.value)]

    def last_tile_ms(self):
        ms = ctypes.c_float(0)
        lib.call('stx_last_tile_ms', self.handle, ctypes.byref(ms))
        return ms.value
