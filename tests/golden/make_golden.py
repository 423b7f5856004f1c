#!/usr/bin/env python3
"""Generates the golden vectors under tests/golden/ by RUNNING THE REFERENCE'S OWN PYTHON.

Run in the build container only (it imports crowsonkb/style_transfer from /root/reference,
which does not exist on the GPU box):

    python tests/golden/make_golden.py
    STX_GOLDEN_APPEND=e2e_sm python tests/golden/make_golden.py    # add one section's arrays only

(A full regeneration reproduces the committed arrays to 1e-7 .. 5e-6 relative, not bit for bit --
the thread order of the reference's multi-threaded BLAS calls -- so new sections are appended and
the committed arrays stay as they were when the tests were tuned against them.)

What executes unmodified from the reference: ``num_utils`` (scipy-BLAS helpers, TV / p-norm),
``optimizers`` (Adam, L-BFGS), ``config_system.parse_args`` and, from ``style_transfer``,
``CaffeModel.eval_features_tile / eval_features_once / prepare_features / preprocess_images /
eval_sc_grad_tile / eval_sc_grad / roll``, ``TileWorker.process_one_request``,
``TileWorkerPool.request / set_contents_and_styles``, ``StyleTransfer.eval_loss_and_grad /
transfer / transfer_multiscale``.

What is substituted, because it is absent from /root/reference and from this container:
  * ``caffe``          -> ``oracle.caffe_net`` (pycaffe-shaped shim over numpy Caffe-layer
                          arithmetic, seeded synthetic weights: no .caffemodel exists offline)
  * ``average.EWMA``   -> the standard bias-corrected EWMA (same class as oracle.optim.Ewma)
  * ``shared_ndarray`` -> an in-process stand-in (``.array``, ``.copy()``, ``.unlink()``)
  * ``pywt``, ``aiohttp_index`` -> empty modules (never called on this path)
  * worker processes   -> a synchronous in-process queue around the reference's worker method

Only data is written: inputs, arguments and the outputs the reference produced.
"""

import collections
import os
import sys
import types

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = '/root/reference'
sys.path.insert(0, REPO)

from oracle import caffe_net  # noqa: E402


# ------------------------------------------------------------------ stand-ins for absent deps
class _SharedNDArray:
    def __init__(self, array):
        self.array = array

    @classmethod
    def copy(cls, arr):
        return cls(np.array(arr, copy=True))

    def unlink(self):
        pass


class _EWMA:
    def __init__(self, shape=(), dtype=np.float64, beta=0.9, correct_bias=True):
        self.beta = beta
        self.beta_accum = 1 if correct_bias else 0
        self.value = np.zeros(shape, dtype)

    @classmethod
    def like(cls, arr, beta=0.9, correct_bias=True):
        return cls(arr.shape, arr.dtype, beta, correct_bias)

    def get(self):
        return self.value / (1 - self.beta_accum)

    def update(self, datum):
        self.beta_accum *= self.beta
        self.value *= self.beta
        self.value += (1 - self.beta) * datum
        return self.get()


def install_stubs():
    for name, attrs in (('pywt', {}), ('aiohttp_index', {'IndexMiddleware': object}),
                        ('shared_ndarray', {'SharedNDArray': _SharedNDArray}),
                        ('average', {'EWMA': _EWMA})):
        mod = types.ModuleType(name)
        mod.__dict__.update(attrs)
        sys.modules[name] = mod
    sys.modules['caffe'] = caffe_net
    sys.path.insert(0, REF)


class _SyncQueue:
    """put() hands the request straight to the worker; get() pops what is stored."""

    def __init__(self, on_put=None):
        self.items = collections.deque()
        self.on_put = on_put

    def put(self, item):
        self.items.append(item)
        if self.on_put:
            self.on_put()

    def get(self):
        return self.items.popleft()


def make_sync_pool(st, model_args, n_workers=1, pool_cls=None):
    """A TileWorkerPool whose workers run the reference's process_one_request in-process."""
    pool = object.__new__(pool_cls or st.TileWorkerPool)
    pool.workers, pool.req_count, pool.next_worker, pool.is_healthy = [], 0, 0, True
    pool.resp_q = _SyncQueue()
    for _ in range(n_workers):
        worker = object.__new__(st.TileWorker)
        worker.resp_q = pool.resp_q
        worker.model = st.CaffeModel(*model_args)
        worker.model.img = np.zeros((3, 1, 1), np.float32)
        worker.proc = types.SimpleNamespace(exitcode=None, terminate=lambda: None)
        worker.req_q = _SyncQueue(on_put=worker.process_one_request)
        pool.workers.append(worker)
    return pool


def smooth_image(seed, h, w):
    """Low-pass filtered seeded noise as a uint8 RGB picture (no photos ship with the reference)."""
    rng = np.random.RandomState(seed)
    small = rng.uniform(0, 255, (max(2, h // 8), max(2, w // 8), 3)).astype(np.uint8)
    img = Image.fromarray(small).resize((w, h), Image.BICUBIC)
    arr = np.asarray(img).astype(np.float32) + rng.uniform(-20, 20, (h, w, 3))
    return np.uint8(np.clip(arr, 0, 255))


def main():
    install_stubs()
    sys.argv = ['style_transfer.py', '-ci', 'c.png', '-si', 's.png']
    import config_system
    import num_utils
    import optimizers
    import style_transfer as st

    out = {}

    # ---------------------------------------------------------------- 1. numeric helpers
    rng = np.random.RandomState(1)
    feat = np.maximum(rng.standard_normal((64, 17, 23)), 0).astype(np.float32)
    other = rng.standard_normal((64, 64)).astype(np.float32)
    gram = num_utils.gram_matrix(feat)
    symm_in = np.tril(gram - np.tril(other) * 0.01)
    out['num/feat'] = feat
    out['num/gram'] = gram
    out['num/symm_in'] = symm_in
    out['num/symm_out'] = num_utils.ssymm(symm_in, feat.reshape(64, -1))
    out['num/norm2'] = np.float64(num_utils.norm2(symm_in))
    out['num/normalize'] = num_utils.normalize(feat.copy())
    img = rng.uniform(-120, 130, (3, 21, 34)).astype(np.float32)
    out['num/img'] = img
    for beta in (2, 1.5):
        loss, grad = num_utils.tv_norm(img / 127.5, beta=beta)
        out['num/tv_loss_%g' % beta] = np.float64(loss)
        out['num/tv_grad_%g' % beta] = grad
    loss, grad = num_utils.p_norm(img / 127.5, p=6.0)
    out['num/p6_loss'], out['num/p6_grad'] = np.float64(loss), grad
    out['num/roll_3_-5'] = num_utils.roll2(img.copy(), np.array([3, -5]))

    # ------------------------------------------------- 2. tile path over the caffe shim
    mean = (103.939, 116.779, 123.68)
    cases = [
        dict(tag='vgg19', proto='vgg19.prototxt', shapes=st.VGG19_SHAPES, content=(96, 112),
             styles=[(80, 72)], tile=64, roll=(16, -24)),
        dict(tag='vgg16avg', proto='vgg16_avgpool.prototxt', shapes=st.VGG16_SHAPES,
             content=(75, 93), styles=[(66, 59), (50, 71)], tile=48, roll=(-8, 40)),
    ]
    for ci, case in enumerate(cases):
        tag = 'tile/%s/' % case['tag']
        model_args = (os.path.join(REF, case['proto']), 'synthetic', mean, case['shapes'])
        st.ARGS = config_system.parse_args(st.STATE)
        master = st.CaffeModel(*model_args, placeholder=True)
        pool = make_sync_pool(st, model_args, n_workers=2)
        content_u8 = smooth_image(10 + ci, *case['content'])
        style_u8 = [smooth_image(20 + ci * 5 + j, *hw) for j, hw in enumerate(case['styles'])]
        content_layers, content_weight = st.StyleTransfer.parse_weights(['conv4_2'], 0.05)
        style_layers, style_weight = st.StyleTransfer.parse_weights(
            ['conv1_1', 'conv2_1', 'conv3_1', 'conv4_1', 'conv5_1'], 1)
        np.random.seed(123)
        master.preprocess_images(pool, [Image.fromarray(content_u8)],
                                 [Image.fromarray(s) for s in style_u8],
                                 content_layers, style_layers, case['tile'])
        pool.set_contents_and_styles(master.contents, master.styles)
        layer_weights = {layer: 1.0 for layer in master.layers() + ['data']}
        layer_weights['conv3_1'] = 1.5
        img = master.pil_to_image(Image.fromarray(smooth_image(30 + ci, *case['content'])))
        master.img = img.copy()
        roll = np.array(case['roll'])
        st.roll2(master.img, roll)
        loss, grad = master.eval_sc_grad(pool, roll, content_layers, style_layers, [],
                                         layer_weights, content_weight, style_weight, {},
                                         case['tile'])
        out[tag + 'content_u8'] = content_u8
        for j, s in enumerate(style_u8):
            out[tag + 'style%d_u8' % j] = s
        out[tag + 'img_rolled'] = master.img
        out[tag + 'roll'] = roll
        out[tag + 'tile_size'] = np.int64(case['tile'])
        out[tag + 'loss'] = np.float64(loss)
        out[tag + 'grad'] = grad
        out[tag + 'lw_conv3_1'] = np.float64(1.5)
        # spot pins of the targets (full Grams / feature maps are too large to commit)
        for layer, g in master.styles[0].grams.items():
            out[tag + 'gram_sum/' + layer] = np.float64(g.sum(dtype=np.float64))
            out[tag + 'gram_diag8/' + layer] = np.diag(g)[:8].copy()
        cf = master.contents[0].features['conv4_2']
        out[tag + 'content_feat_shape'] = np.int64(cf.shape)
        out[tag + 'content_feat_sum'] = np.float64(cf.sum(dtype=np.float64))
        out[tag + 'content_feat_c0'] = cf[0].copy()

        # one standalone tile with a non-zero start, straight through eval_sc_grad_tile
        worker_model = pool.workers[0].model
        tile = master.img[:, 8:8 + 40, 16:16 + 56].copy()
        layers = [l for l in reversed(master.layers()) if l in content_layers + style_layers]
        tloss, tgrad = worker_model.eval_sc_grad_tile(
            tile, np.array([8, 16]), layers, content_layers, style_layers, [], layer_weights,
            content_weight, style_weight, {})
        out[tag + 'single/loss'] = np.float64(tloss)
        out[tag + 'single/grad'] = tgrad.copy()
        # the same tile with a Deep-Dream term on two layers (style_transfer.py:602-604)
        dd_layers, dd_weight = st.StyleTransfer.parse_weights(['conv4_3', 'conv2_2:3'], 0.04)
        dlayers = [l for l in reversed(master.layers())
                   if l in content_layers + style_layers + dd_layers]
        dloss, dgrad = worker_model.eval_sc_grad_tile(
            tile, np.array([8, 16]), dlayers, content_layers, style_layers, dd_layers,
            layer_weights, content_weight, style_weight, dd_weight)
        out[tag + 'dream/loss'] = np.float64(dloss)
        out[tag + 'dream/grad'] = dgrad.copy()
        feats = worker_model.eval_features_tile(tile, ['conv1_1', 'pool1', 'conv5_1'])
        out[tag + 'single/feat_conv5_1'] = feats['conv5_1'].copy()
        out[tag + 'single/feat_pool1_sum'] = np.float64(feats['pool1'].sum(dtype=np.float64))

    # ------------------------------------------------------------ 3. optimizer trajectories
    def quad_opfunc(target):
        def f(x):
            d = x - target
            return float(np.sum(d * d, dtype=np.float64)), (2 * d).astype(np.float32)
        return f

    rng = np.random.RandomState(7)
    target = rng.uniform(-100, 100, (3, 12, 20)).astype(np.float32)
    x0 = rng.uniform(-100, 100, (3, 12, 20)).astype(np.float32)
    rolls = [(3, -2), (0, 0), (-5, 4), (1, 1), (7, 0)]
    out['opt/target'], out['opt/x0'], out['opt/rolls'] = target, x0, np.int64(rolls)
    for biased in (False, True):
        params = x0.copy()
        tgt = target.copy()
        opt = optimizers.AdamOptimizer(params, step_size=15, bp1=1 - 1 / 20, decay=0.05,
                                       power=0.5, biased_g1=biased)
        traj, losses = [], []
        for xy in rolls:
            xy = np.array(xy)
            num_utils.roll2(params, xy), num_utils.roll2(tgt, xy)
            opt.roll(xy)
            avg, loss = opt.update(quad_opfunc(tgt))
            num_utils.roll2(params, -xy), num_utils.roll2(tgt, -xy)
            opt.roll(-xy)
            traj.append(avg.copy()), losses.append(loss)
        key = 'opt/adam_biased%d/' % biased
        out[key + 'avg'], out[key + 'loss'] = np.stack(traj), np.float64(losses)
        out[key + 'params'] = params.copy()
    params = x0.copy()
    tgt = target.copy()
    scale = np.linspace(0.5, 2, target.size).reshape(target.shape).astype(np.float32)

    def lb_opfunc(x):
        d = (x - tgt) * scale
        return float(np.sum(d * d, dtype=np.float64)), (2 * d * scale).astype(np.float32)
    opt = optimizers.LBFGSOptimizer(params)
    traj, losses = [], []
    for _ in range(14):
        p, loss = opt.update(lb_opfunc)
        traj.append(p.copy()), losses.append(loss)
    out['opt/lbfgs/scale'] = scale
    out['opt/lbfgs/params'], out['opt/lbfgs/loss'] = np.stack(traj), np.float64(losses)

    # --------------------------------------------- 4. the whole multi-scale schedule, tiny
    sys.argv = ['style_transfer.py', '-ci', 'c.png', '-si', 's.png', '--size', '96',
                '--min-size', '60', '--tile-size', '48', '--iterations', '3', '2',
                '--display', 'none', '--seed', '5']
    st.ARGS = config_system.parse_args(st.STATE)
    st.STATS = st.StatLogger()
    st.STATE.__dict__.clear()
    model_args = (os.path.join(REF, 'vgg19.prototxt'), 'synthetic', mean, st.VGG19_SHAPES)
    ref_pool_cls = st.TileWorkerPool
    st.TileWorkerPool = lambda model, devices, caffe_path=None: \
        make_sync_pool(st, model_args, 1, ref_pool_cls)
    model = st.CaffeModel(*model_args, placeholder=True)
    transfer = st.StyleTransfer(model)
    content_u8 = smooth_image(40, 96, 80)
    style_u8 = smooth_image(41, 70, 90)
    log = []

    class Cb:
        def set_steps(self, steps):
            self.steps = steps

        def __call__(self, **kw):
            log.append((kw['step'], kw['update_size'], kw['loss'], kw['tv_loss']))
    np.random.seed(st.ARGS.seed)
    transfer.transfer_multiscale([Image.fromarray(content_u8)], [Image.fromarray(style_u8)],
                                 None, None, callback=Cb())
    out['e2e/content_u8'], out['e2e/style_u8'] = content_u8, style_u8
    out['e2e/argv'] = np.array(' '.join(sys.argv[1:]))
    out['e2e/log'] = np.float64(log)
    out['e2e/final_raw'] = transfer.current_raw.copy()
    out['e2e/final_u8'] = np.asarray(transfer.current_output)

    # ----------------- 4b. L-BFGS, VGG-16 with AVE pooling, two style images (configs 4 and 5)
    sys.argv = ['style_transfer.py', '-ci', 'c.png', '-si', 's1.png', 's2.png', '--size', '80',
                '--min-size', '50', '--tile-size', '40', '--iterations', '3', '2', '-o', 'lbfgs',
                '--model', 'vgg16_avgpool.prototxt', '--display', 'none', '--seed', '9']
    st.ARGS = config_system.parse_args(st.STATE)
    st.STATS = st.StatLogger()
    st.STATE.__dict__.clear()
    model_args2 = (os.path.join(REF, 'vgg16_avgpool.prototxt'), 'synthetic', mean, st.VGG16_SHAPES)
    st.TileWorkerPool = lambda model, devices, caffe_path=None: \
        make_sync_pool(st, model_args2, 1, ref_pool_cls)
    model = st.CaffeModel(*model_args2, placeholder=True)
    transfer = st.StyleTransfer(model)
    content_u8 = smooth_image(50, 64, 80)
    styles_u8 = [smooth_image(51, 60, 48), smooth_image(52, 40, 72)]
    log = []
    np.random.seed(st.ARGS.seed)
    transfer.transfer_multiscale([Image.fromarray(content_u8)],
                                 [Image.fromarray(s) for s in styles_u8], None, None, callback=Cb())
    out['e2e_lbfgs/content_u8'] = content_u8
    out['e2e_lbfgs/style0_u8'], out['e2e_lbfgs/style1_u8'] = styles_u8
    out['e2e_lbfgs/argv'] = np.array(' '.join(sys.argv[1:]))
    out['e2e_lbfgs/log'] = np.float64(log)
    out['e2e_lbfgs/final_raw'] = transfer.current_raw.copy()

    # ------- 4c. BASELINE config 4 in miniature: VGG-19 (MAX pooling) x L-BFGS x a 3 x 3 tiling
    # whose last row / column is larger (style_transfer.py:619-632), two scales.  The step lines
    # the reference's own Progress prints (style_transfer.py:950-951), its CSV log
    # (style_transfer.py:121-130) and its PNG comment (style_transfer.py:1003-1010) are kept too.
    import contextlib
    import io
    import tempfile
    sys.argv = ['style_transfer.py', '-ci', 'c.png', '-si', 's.png', '--size', '100',
                '--min-size', '64', '--tile-size', '40', '--iterations', '3', '2', '-o', 'lbfgs',
                '--display', 'none', '--seed', '13', '--save-every', '2']
    st.ARGS = config_system.parse_args(st.STATE)
    st.STATS = st.StatLogger()
    st.STATE.__dict__.clear()
    st.TileWorkerPool = lambda model, devices, caffe_path=None: \
        make_sync_pool(st, model_args, 1, ref_pool_cls)
    model = st.CaffeModel(*model_args, placeholder=True)
    transfer = st.StyleTransfer(model)
    content_u8 = smooth_image(60, 92, 100)
    style_u8 = smooth_image(61, 80, 70)
    log = []
    tmp = tempfile.mkdtemp()
    st.RUN = os.path.join(tmp, 'run')
    web_if = types.SimpleNamespace(put_event=lambda ev: None)
    progress = st.Progress(transfer, save_every=st.ARGS.save_every, web_if=web_if,
                           callback=None)
    saved = []

    def cb(**kw):
        log.append((kw['step'], kw['update_size'], kw['loss'], kw['tv_loss']))
        progress(**kw)
    cb.set_steps = progress.set_steps
    np.random.seed(st.ARGS.seed)
    stdout = io.StringIO()
    with contextlib.redirect_stdout(stdout):
        transfer.transfer_multiscale([Image.fromarray(content_u8)], [Image.fromarray(style_u8)],
                                     None, None, callback=cb)
    st.STATS.dump()
    with open(st.RUN + '_log.csv') as f:
        csv_lines = f.read().splitlines()
    saved = sorted(n[len('run'):] for n in os.listdir(tmp) if n.endswith('.png'))
    out['e2e_cfg4/content_u8'], out['e2e_cfg4/style_u8'] = content_u8, style_u8
    out['e2e_cfg4/argv'] = np.array(' '.join(sys.argv[1:]))
    out['e2e_cfg4/log'] = np.float64(log)
    out['e2e_cfg4/final_raw'] = transfer.current_raw.copy()
    out['e2e_cfg4/final_u8'] = np.asarray(transfer.current_output)
    out['e2e_cfg4/step_lines'] = np.array('\n'.join(
        l for l in stdout.getvalue().splitlines() if l.startswith('Step ')))
    out['e2e_cfg4/tile_lines'] = np.array('\n'.join(
        l for l in stdout.getvalue().splitlines() if l.startswith('Using ')))
    out['e2e_cfg4/csv_header'] = np.array(csv_lines[0])
    out['e2e_cfg4/csv_rows'] = np.array('\n'.join(csv_lines[1:]))
    out['e2e_cfg4/saved_files'] = np.array(' '.join(saved))
    out['e2e_cfg4/image_comment'] = np.array(st.get_image_comment())

    # ------- 4e. the auxiliary-image term (--aux-image, style_transfer.py:729-733): the reference
    # rolls the image by the iteration's shift but not the auxiliary image.  One scale, 2 x 2 tiles,
    # three Adam steps.
    sys.argv = ['style_transfer.py', '-ci', 'c.png', '-si', 's.png', '--aux-image', 'a.png',
                '--size', '72', '--min-size', '72', '--tile-size', '48', '--iterations', '3',
                '--display', 'none', '--seed', '21']
    st.ARGS = config_system.parse_args(st.STATE)
    st.STATS = st.StatLogger()
    st.STATE.__dict__.clear()
    st.TileWorkerPool = lambda model, devices, caffe_path=None: \
        make_sync_pool(st, model_args, 1, ref_pool_cls)
    model = st.CaffeModel(*model_args, placeholder=True)
    transfer = st.StyleTransfer(model)
    content_u8 = smooth_image(70, 64, 72)
    style_u8 = smooth_image(71, 60, 50)
    aux_u8 = smooth_image(72, 64, 72)
    log = []
    np.random.seed(st.ARGS.seed)
    transfer.transfer_multiscale([Image.fromarray(content_u8)], [Image.fromarray(style_u8)],
                                 None, Image.fromarray(aux_u8), callback=Cb())
    out['e2e_aux/content_u8'], out['e2e_aux/style_u8'], out['e2e_aux/aux_u8'] = \
        content_u8, style_u8, aux_u8
    out['e2e_aux/argv'] = np.array(' '.join(sys.argv[1:]))
    out['e2e_aux/log'] = np.float64(log)
    out['e2e_aux/final_raw'] = transfer.current_raw.copy()

    # ------- 4f. --jitter (content maps recomputed every iteration from the shifted picture,
    # any pixel shift: style_transfer.py:757-763,780-794) together with a Deep-Dream term
    # (style_transfer.py:602-604).  One scale, 2 x 2 tiles, three Adam steps.
    sys.argv = ['style_transfer.py', '-ci', 'c.png', '-si', 's.png', '--jitter', '--dd-weight',
                '0.02', '--dd-layers', 'conv4_3', 'conv3_2:2', '--size', '80', '--min-size', '80',
                '--tile-size', '48', '--iterations', '3', '--display', 'none', '--seed', '31']
    st.ARGS = config_system.parse_args(st.STATE)
    st.STATS = st.StatLogger()
    st.STATE.__dict__.clear()
    st.TileWorkerPool = lambda model, devices, caffe_path=None: \
        make_sync_pool(st, model_args, 1, ref_pool_cls)
    model = st.CaffeModel(*model_args, placeholder=True)
    transfer = st.StyleTransfer(model)
    content_u8 = smooth_image(80, 72, 80)
    style_u8 = smooth_image(81, 56, 64)
    log = []
    np.random.seed(st.ARGS.seed)
    transfer.transfer_multiscale([Image.fromarray(content_u8)], [Image.fromarray(style_u8)],
                                 None, None, callback=Cb())
    out['e2e_jitter/content_u8'], out['e2e_jitter/style_u8'] = content_u8, style_u8
    out['e2e_jitter/argv'] = np.array(' '.join(sys.argv[1:]))
    out['e2e_jitter/log'] = np.float64(log)
    out['e2e_jitter/final_raw'] = transfer.current_raw.copy()

    # ------- 4g. --style-multiscale MIN MAX (style_transfer.py:493-531): the style Gram is the mean
    # over a sqrt(2) ladder of resamplings of the style picture (here 48, 68, 96 of a 96 x 120
    # picture).  One scale, one tile, two Adam steps.
    sys.argv = ['style_transfer.py', '-ci', 'c.png', '-si', 's.png', '--style-multiscale', '48', '96',
                '--size', '64', '--min-size', '64', '--tile-size', '64', '--iterations', '2',
                '--display', 'none', '--seed', '41']
    st.ARGS = config_system.parse_args(st.STATE)
    st.STATS = st.StatLogger()
    st.STATE.__dict__.clear()
    st.TileWorkerPool = lambda model, devices, caffe_path=None: \
        make_sync_pool(st, model_args, 1, ref_pool_cls)
    model = st.CaffeModel(*model_args, placeholder=True)
    transfer = st.StyleTransfer(model)
    content_u8 = smooth_image(90, 56, 64)
    style_u8 = smooth_image(91, 96, 120)
    log = []
    np.random.seed(st.ARGS.seed)
    stdout = io.StringIO()
    with contextlib.redirect_stdout(stdout):
        transfer.transfer_multiscale([Image.fromarray(content_u8)], [Image.fromarray(style_u8)],
                                     None, None, callback=Cb())
    out['e2e_sm/content_u8'], out['e2e_sm/style_u8'] = content_u8, style_u8
    out['e2e_sm/argv'] = np.array(' '.join(sys.argv[1:]))
    out['e2e_sm/log'] = np.float64(log)
    out['e2e_sm/final_raw'] = transfer.current_raw.copy()
    out['e2e_sm/style_lines'] = np.array('\n'.join(
        l for l in stdout.getvalue().splitlines() if l.startswith('Processing style')))

    # ------- 4h. a run that leaves the defaults in many places at once: --init-image (the biased
    # first-moment start of Adam, style_transfer.py:883-897), --style-scale, --div, --step-decay,
    # --avg-window, --tv-power, --p-power, --mean, weighted non-default content / style layers.
    # Two scales, 2 x 2 tiles at the second, Adam.
    sys.argv = ['style_transfer.py', '-ci', 'c.png', '-si', 's.png', '--init-image', 'i.png',
                '--style-scale', '0.75', '--div', '8', '--step-decay', '0.1', '0.6',
                '--avg-window', '5', '--tv-power', '1.5', '--p-power', '4', '--tv-weight', '3',
                '--mean', '100', '110', '120', '--content-layers', 'conv3_2', 'conv4_2:0.5',
                '--style-layers', 'conv1_2', 'conv3_1:0.5', 'conv4_1', '--content-weight', '0.1',
                '--size', '80', '--min-size', '56', '--tile-size', '48', '--iterations', '2', '3',
                '--step-size', '10', '--display', 'none', '--seed', '51']
    st.ARGS = config_system.parse_args(st.STATE)
    st.STATS = st.StatLogger()
    st.STATE.__dict__.clear()
    # (the model and the workers get --mean the way style_transfer.py:1106-1110 hands it over)
    model_args_h = (model_args[0], model_args[1], st.ARGS.mean, model_args[3])
    st.TileWorkerPool = lambda model, devices, caffe_path=None: \
        make_sync_pool(st, model_args_h, 1, ref_pool_cls)
    model = st.CaffeModel(*model_args_h, placeholder=True)
    transfer = st.StyleTransfer(model)
    content_u8 = smooth_image(100, 64, 80)
    style_u8 = smooth_image(101, 72, 60)
    init_u8 = smooth_image(102, 40, 50)
    log = []
    np.random.seed(st.ARGS.seed)
    stdout = io.StringIO()
    with contextlib.redirect_stdout(stdout):
        transfer.transfer_multiscale([Image.fromarray(content_u8)], [Image.fromarray(style_u8)],
                                     Image.fromarray(init_u8), None, callback=Cb())
    out['e2e_opts/content_u8'], out['e2e_opts/style_u8'], out['e2e_opts/init_u8'] = \
        content_u8, style_u8, init_u8
    out['e2e_opts/argv'] = np.array(' '.join(sys.argv[1:]))
    out['e2e_opts/log'] = np.float64(log)
    out['e2e_opts/final_raw'] = transfer.current_raw.copy()
    out['e2e_opts/lines'] = np.array('\n'.join(
        l for l in stdout.getvalue().splitlines()
        if l.startswith(('Processing style', 'Scale ', 'Using '))))

    # ------- 4i. the remaining branches of the style-size rule (style_transfer.py:862-872):
    # an absolute --style-scale (>= 32) and --max-style-size with --style-scale-up.  One scale,
    # one tile, one Adam step each.
    for tag, extra in (('abs', ['--style-scale', '48']),
                       ('max', ['--style-scale', '2', '--max-style-size', '52', '--style-scale-up'])):
        sys.argv = ['style_transfer.py', '-ci', 'c.png', '-si', 's.png'] + extra + [
            '--size', '64', '--min-size', '64', '--tile-size', '64', '--iterations', '1',
            '--display', 'none', '--seed', '61']
        st.ARGS = config_system.parse_args(st.STATE)
        st.STATS = st.StatLogger()
        st.STATE.__dict__.clear()
        st.TileWorkerPool = lambda model, devices, caffe_path=None: \
            make_sync_pool(st, model_args, 1, ref_pool_cls)
        model = st.CaffeModel(*model_args, placeholder=True)
        transfer = st.StyleTransfer(model)
        content_u8 = smooth_image(110, 56, 64)
        style_u8 = smooth_image(111, 40, 44)
        log = []
        np.random.seed(st.ARGS.seed)
        transfer.transfer_multiscale([Image.fromarray(content_u8)], [Image.fromarray(style_u8)],
                                     None, None, callback=Cb())
        out['e2e_ss/%s.argv' % tag] = np.array(' '.join(sys.argv[1:]))
        out['e2e_ss/%s.log' % tag] = np.float64(log)
        out['e2e_ss/%s.final_raw' % tag] = transfer.current_raw.copy()
    out['e2e_ss/content_u8'], out['e2e_ss/style_u8'] = content_u8, style_u8

    # ------- 4j. the L-BFGS multi-tile run at a size where the reference has ONE trajectory (VERDICT r5
    # item 2f): VGG-19 with AVE pooling x L-BFGS x a ragged 2 x 2 tiling, 194 x 198 (tiles of 97 x 99) then
    # 275 x 280 (137/138 x 140), 3 + 2 iterations -- tests/golden/fixtures_lbfgs.py `stable`, run as is.
    # tests/golden/branch_sets.py stable: with its Convolution layer computed by 14 other float32
    # implementations and under calibrated noise (8 runs) the reference's losses stay within 5.4e-5 of this
    # run at every step.  (MAX pooling does not get there at any size: the 280-pixel VGG-19 run differs from
    # itself by 2e-4 at step 2 and 2.4e-3 at step 5 between its own SGEMM and torch's conv2d.)
    if os.environ.get('STX_GOLDEN_APPEND', 'e2e_stable') == 'e2e_stable':
        import fixtures_lbfgs
        st.TileWorkerPool = ref_pool_cls          # (the sections above left their stand-in behind)
        log, raw, content_u8, styles_u8, argv = fixtures_lbfgs.run_fixture(st, config_system, num_utils, 'stable')
        out['e2e_stable/content_u8'], out['e2e_stable/style_u8'] = content_u8, styles_u8[0]
        out['e2e_stable/argv'] = np.array(' '.join(argv))
        out['e2e_stable/log'] = log
        out['e2e_stable/final_raw'] = raw

    # ----------- 4d. the six deploy prototxts the reference ships, as parsed layer tuples (data
    # for the --model reader): (name, type, bottom, top, num_output, pad, kernel,
    # stride, pool).  Two independent readings must agree: the oracle's protobuf-text parser and
    # a per-block regular-expression scan.
    import json
    import re
    protos = {}
    for fn in sorted(os.listdir(REF)):
        if not fn.endswith('.prototxt'):
            continue
        with open(os.path.join(REF, fn)) as f:
            text = f.read()
        rows = []
        for lay in caffe_net.layers_from_prototxt(text):
            rows.append([lay['name'], lay['type'], lay['bottom'], lay['top'],
                         lay.get('num_output', 0), lay.get('pad', 0), lay.get('kernel_size', 0),
                         lay.get('stride', 1 if lay['type'] != 'Pooling' else 0),
                         lay.get('pool', '') if lay['type'] == 'Pooling' else '',
                         list(lay.get('shape', ()))])
        scan = []
        for block in re.findall(r'layer\s*\{(.*?)\n\}', text, re.S):
            def grab(key, cast=str, default=None):
                m = re.search(r'\b%s\s*:\s*"?([\w.]+)"?' % key, block)
                return cast(m.group(1)) if m else default
            scan.append([grab('name'), grab('type'), grab('bottom'), grab('top'),
                         grab('num_output', int, 0), grab('pad', int, 0)])
        assert [r[:6] for r in rows] == scan, fn
        protos[fn] = rows
    out['proto/layers_json'] = np.array(json.dumps(protos, sort_keys=True))

    # ------------------------------------------------------------------ 5. parse_args defaults
    sys.argv = ['style_transfer.py', '-ci', 'c.png', '-si', 's.png']
    args = config_system.parse_args(st.STATE)
    defaults = {k: getattr(args, k) for k in args}
    out['args/defaults_repr'] = np.array(repr(sorted((k, str(v)) for k, v in defaults.items())))

    import vectors      # (HERE is on sys.path: reference_vectors*.npz, parts of at most 1 MiB)
    # STX_GOLDEN_APPEND=<section>: keep the committed arrays as they are (a regeneration differs
    # from them at the 1e-7 level: the thread order of the reference's BLAS calls) and only add
    # the arrays of that section
    section = os.environ.get('STX_GOLDEN_APPEND')
    if section and os.path.exists(vectors.part_path(0)):
        old = vectors.load()
        old.update({k.replace('/', '.'): v for k, v in out.items() if k.startswith(section + '/')})
        out = old
    else:
        out = {k.replace('/', '.'): v for k, v in out.items()}
    paths = vectors.save(out)
    print('wrote %s (%d arrays, %.1f KiB)' % (', '.join(paths), len(out),
                                             sum(os.path.getsize(p) for p in paths) / 1024))
    num_utils.POOL.shutdown()


if __name__ == '__main__':
    main()
