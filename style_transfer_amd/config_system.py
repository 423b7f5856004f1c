"""Command-line / config-file options, compatible with the reference's ``config_system.py``.

Same flag names, short aliases, types and defaults (``config_system.py:46-119``), same
precedence -- built-in defaults < ``config.py`` next to the CLI script < flags given on the
command line < the file named by ``--config`` (``config_system.py:121-135``) -- and the same
"lazy" values: a config file is executed as Python and may bind an option to a callable of the
run state (``scale``, ``step``, ``steps``, ``img_size``), which is then re-evaluated on every
read (``config_system.py:151-163``).  ``detect_devices()`` asks the HIP runtime instead of
``nvidia-smi`` (``config_system.py:17-24``).
"""

import argparse
from fractions import Fraction
import math
import os
from pathlib import Path
import sys
import zlib

import numpy as np


def detect_devices():
    """List of visible GPU indices, or [-1] when there is none (the reference's CPU marker)."""
    try:
        from . import lib
        n = lib.device_count()
    except Exception:  # pylint: disable=broad-except
        n = 0
    return list(range(n)) if n else [-1]


def ffloat(text):
    """Floats written as decimals or fractions ('1/3')."""
    return float(Fraction(text))


# (flags, argparse keyword arguments)
_OPTIONS = [
    (('--content-image', '-ci'), dict(help='content image file')),
    (('--style-images', '-si'), dict(nargs='+', default=[], metavar='STYLE_IMAGE',
                                     help='one or more style image files')),
    (('--output-image', '-oi'), dict(help='where to write the result')),
    (('--init-image', '-ii'), dict(metavar='IMAGE', help='start from this image')),
    (('--aux-image', '-ai'), dict(metavar='IMAGE', help='auxiliary image to stay close to')),
    (('--config',), dict(type=Path, help='Python file with option assignments')),
    (('--list-layers',), dict(action='store_true', help='print the model layers and exit')),
    (('--caffe-path',), dict(help='accepted for compatibility; unused (no Caffe involved)')),
    (('--devices',), dict(nargs='+', metavar='DEVICE', type=int, default=[-1],
                          help='GPU indices to farm tiles over (-1: first GPU)')),
    (('--iterations', '-i'), dict(nargs='+', type=int, default=[200, 100],
                                  help='iterations per scale (last value repeats)')),
    (('--size', '-s'), dict(type=int, default=256, help='output size (long edge)')),
    (('--min-size',), dict(type=int, default=182, help='smallest scale of the pyramid')),
    (('--style-scale', '-ss'), dict(type=ffloat, default=1, help='style size relative to content')),
    (('--max-style-size',), dict(type=int, help='upper bound for the style size')),
    (('--style-scale-up',), dict(default=False, action='store_true',
                                 help='allow enlarging style images')),
    (('--style-multiscale', '-sm'), dict(type=int, nargs=2, metavar=('MIN_SCALE', 'MAX_SCALE'),
                                         default=None, help='pool style Grams over these scales')),
    (('--tile-size',), dict(type=int, default=512, help='largest tile edge evaluated at once')),
    (('--optimizer', '-o'), dict(default='adam', choices=['adam', 'lbfgs'], help='optimizer')),
    (('--step-size', '-st'), dict(type=ffloat, default=15, help='Adam step size')),
    (('--step-decay', '-sd'), dict(nargs=2, metavar=('DECAY', 'POWER'), type=ffloat,
                                   default=[0.05, 0.5], help='step size / (1 + DECAY*i)^POWER')),
    (('--avg-window',), dict(type=ffloat, default=20, help='iterate-averaging window')),
    (('--layer-weights',), dict(help='JSON file of per-layer weight factors')),
    (('--content-weight', '-cw'), dict(type=ffloat, default=0.05, help='content factor')),
    (('--dd-weight', '-dw'), dict(type=ffloat, default=0, help='Deep Dream factor')),
    (('--tv-weight', '-tw'), dict(type=ffloat, default=5, help='total-variation factor')),
    (('--tv-power', '-tp'), dict(metavar='BETA', type=ffloat, default=2, help='TV exponent')),
    (('--swt-weight', '-ww'), dict(metavar='WEIGHT', type=ffloat, default=0, help='SWT factor')),
    (('--swt-wavelet', '-wt'), dict(metavar='WAVELET', default='haar', help='SWT wavelet')),
    (('--swt-levels', '-wl'), dict(metavar='LEVELS', default=1, type=int, help='SWT levels')),
    (('--swt-power', '-wp'), dict(metavar='P', default=2, type=ffloat, help='SWT exponent')),
    (('--p-weight', '-pw'), dict(type=ffloat, default=2, help='p-norm factor')),
    (('--p-power', '-pp'), dict(metavar='P', type=ffloat, default=6, help='p-norm exponent')),
    (('--aux-weight', '-aw'), dict(type=ffloat, default=10, help='auxiliary image factor')),
    (('--content-layers',), dict(nargs='*', default=['conv4_2'], metavar='LAYER',
                                 help='content layers (name or name:weight)')),
    (('--style-layers',), dict(nargs='*', metavar='LAYER',
                               default=['conv1_1', 'conv2_1', 'conv3_1', 'conv4_1', 'conv5_1'],
                               help='style layers (name or name:weight)')),
    (('--dd-layers',), dict(nargs='*', metavar='LAYER', default=[], help='Deep Dream layers')),
    (('--port', '-p'), dict(type=int, default=8000, help='accepted for compatibility')),
    (('--display',), dict(default='browser', choices=['browser', 'gui', 'none'],
                          help='accepted for compatibility (no live view)')),
    (('--browser',), dict(default=None, help='accepted for compatibility')),
    (('--model',), dict(default='vgg19.prototxt', help='deploy prototxt or a stock model name')),
    (('--weights',), dict(default='vgg19.caffemodel', help='.caffemodel / .npz weights')),
    (('--mean',), dict(nargs=3, metavar=('B_MEAN', 'G_MEAN', 'R_MEAN'),
                       default=(103.939, 116.779, 123.68), help='per-channel mean, BGR')),
    (('--save-every',), dict(metavar='N', type=int, default=0, help='save every N steps')),
    (('--seed',), dict(type=int, default=0, help='random seed')),
    (('--div',), dict(metavar='FACTOR', type=int, default=1,
                      help='make image sizes divisible by FACTOR')),
    (('--jitter',), dict(action='store_true', help='per-iteration content features (slow)')),
    (('--debug',), dict(action='store_true', help='verbose logging')),
]


# Options the reference does not have.  The option namespace (and with it the PNG comment) holds the
# reference's names and nothing else unless one of these is SET -- on the command line, in config.py
# or in the --config file -- so they have no default there: read them with
# getattr(args, name, <the default named in the help text>).
_EXTENSIONS = [
    (('--preserve-color',), dict(choices=['none', 'luma', 'match'],
                                 help="keep the content picture's colours: 'luma' puts the luminance "
                                      "of the result on the chroma of the content picture when a "
                                      "picture is written, 'match' recolours every style picture to "
                                      "the content picture's colour mean and covariance before its "
                                      "Grams are taken (default: none)")),
    (('--style-masks',), dict(nargs='+', metavar='MASK',
                              help='spatial control: one greyscale picture per style image, in the content '
                                   "picture's frame; a style applies where its mask is white.  With masks "
                                   'every style image is a style set of its own instead of one average '
                                   '(default: no masks)')),
    (('--content-mask',), dict(metavar='MASK',
                               help="spatial control of the content term: a greyscale picture in the content "
                                    "picture's frame; the content picture is held where it is white and the "
                                    'content term is off where it is black (default: no mask)')),
    (('--lap-weight',), dict(metavar='WEIGHT', type=ffloat,
                             help="Laplacian loss factor: holds the result to the content picture's edges "
                                  '(the Laplacian of the average-pooled result against that of the '
                                  'average-pooled content picture); 0 or absent: off (default: 0)')),
    (('--lap-pools',), dict(nargs='+', metavar='POOL',
                            help='pool sizes of the Laplacian loss as P or P:weight, one to four distinct '
                                 'powers of two from 1 to 64; the weights are normalised to --lap-weight '
                                 'like those of a layer list (default: 4)')),
    (('--stat-weight',), dict(metavar='WEIGHT', type=ffloat,
                              help="mean / std style factor: holds every channel's mean and standard deviation "
                                   'at the --stat-layers to those of the style picture(s) -- palette, contrast '
                                   "and texture energy without the Gram's patterns; read once per scale; "
                                   '0 or absent: off (default: 0)')),
    (('--stat-layers',), dict(nargs='+', metavar='LAYER',
                              help='layers of the mean / std style term as name or name:weight; the weights are '
                                   'normalised to --stat-weight like those of a layer list and read once per '
                                   'scale; with --style-multiscale the layers themselves stay those of the '
                                   "first scale, whose targets are kept (default: the --style-layers' names "
                                   'with weight 1 each; its built-in list when --style-layers is empty)')),
    (('--nnfm-weight',), dict(metavar='WEIGHT', type=ffloat,
                              help='nearest-neighbour feature matching factor (ARF, NNST): pulls every feature '
                                   'vector of the result at the --nnfm-layers towards the most similar feature '
                                   'vector of the style picture(s), by cosine -- keeps small motifs that the '
                                   'global statistics average away; read once per scale; 0 or absent: off '
                                   '(default: 0)')),
    (('--nnfm-layers',), dict(nargs='+', metavar='LAYER',
                              help='layers of the nearest-neighbour term as name or name:weight; the weights are '
                                   'normalised to --nnfm-weight like those of a layer list and read once per '
                                   'scale; with --style-multiscale the layers themselves stay those of the '
                                   'first scale, whose banks are kept (default: conv3_1 conv4_1)')),
    (('--nnfm-stride',), dict(metavar='S', type=int,
                              help="keeps every S-th row and column of the style picture's feature maps in the "
                                   'bank of the nearest-neighbour term, an integer >= 1 (default: 1)')),
    (('--nnfm-patch',), dict(metavar='P', type=int,
                             help='matches P x P patches of feature vectors in the nearest-neighbour term instead '
                                  'of single vectors (CNNMRF, NNST), 1 or 3: a 3 x 3 patch carries the local '
                                  'arrangement -- strokes, hatching, small motifs -- and makes the search nine '
                                  'times as long; read once per scale (default: 1)')),
    (('--nnfm-k',), dict(metavar='K', type=int,
                         help='pulls every feature vector (or patch) of the nearest-neighbour term towards the mean '
                              'of its K most similar bank rows instead of the single best one, an integer from 1 '
                              'to 4: steadier targets where two rows are nearly tied and with --nnfm-stride above '
                              '1; the search is done once whatever K is; read once per scale (default: 1)')),
    (('--nnfm-cover',), dict(metavar='LAMBDA', type=ffloat,
                             help='adds LAMBDA times the coverage part to the nearest-neighbour term (the other half '
                                  "of STROTSS's relaxed earth mover's distance): every bank row also looks for its "
                                  'most similar feature vector of the result and pulls that one towards itself, so '
                                  'that the whole style bank is used and not only the rows that are easiest to '
                                  'reach; every tile is asked to cover the whole bank, so --nnfm-stride matters '
                                  'more; a finite number >= 0, not with --nnfm-patch 3; read once per scale; 0 or '
                                  'absent: off (default: 0)')),
    (('--nnfm-masks',), dict(nargs='+', metavar='MASK',
                             help='region-guided nearest-neighbour matching ("semantic" or "doodle" style transfer): '
                                  "one greyscale picture per style image, in the content picture's frame; where a "
                                  'mask is white the feature vectors of the result pick rows of THAT style picture '
                                  'only, so sky takes from sky and town from town.  Restricts the nearest-neighbour '
                                  'term alone (the Gram term stays one averaged style set); one to 8 style images, '
                                  'not with --nnfm-patch 3, --nnfm-cover or --style-masks (default: no masks)')),
    (('--swd-weight',), dict(metavar='WEIGHT', type=ffloat,
                             help='sliced Wasserstein style factor (Heitz et al.): holds the whole distribution of '
                                  'the feature vectors at the --swd-layers to that of the style picture(s), along '
                                  'fixed random directions and by an exact sort -- contrast and rare colours that '
                                  'the Gram term washes out; read once per scale; 0 or absent: off (default: 0)')),
    (('--swd-layers',), dict(nargs='+', metavar='LAYER',
                             help='layers of the sliced Wasserstein term as name or name:weight; the weights are '
                                  'normalised to --swd-weight like those of a layer list and read once per scale; '
                                  'with --style-multiscale the layers themselves stay those of the first scale, '
                                  'whose targets are kept.  The term is not cheap: at a 1024 x 1024 tile the default '
                                  'layers together take about 1.1 times the tile evaluation itself (4.2 ms beside '
                                  '3.8 ms on an MI355X), and conv1_1 alone -- 64 rows of a million values to sort '
                                  '-- 6.2 ms, 1.6 tile evaluations, which is why the default leaves it out '
                                  '(default: conv2_1 conv3_1 conv4_1)')),
    (('--swd-dirs',), dict(metavar='D', type=int,
                           help='directions per layer of the sliced Wasserstein term, an integer from 1 to 4096: '
                                'orthonormal bases drawn once per run from --seed and the layer name (default: the '
                                "layer's channel count, one basis)")),
    (('--selfsim-weight',), dict(metavar='WEIGHT', type=ffloat,
                                 help='self-similarity content factor (STROTSS, NNST): holds the pattern of '
                                      'similarities between positions of the content picture -- places that look '
                                      'alike there should look alike in the result, places that differ should '
                                      'differ -- and leaves the feature values free, so it does not fight the '
                                      'per-pixel style terms (--nnfm-weight, --swd-weight) as the content term '
                                      'does; with -cw 0 or an empty --content-layers it replaces that term.  '
                                      '--content-mask weights the content term only and leaves this one alone.  '
                                      'At its default (conv4_2, 1024 points) the term takes 0.41 ms beside a 3.8 ms '
                                      'evaluation of a 1024 x 1024 tile on an MI355X, a ninth of it, and about as '
                                      'much beside the 0.83 ms of a 256 x 256 tile; with --selfsim-points 4096, 1.5 '
                                      'ms; read once per scale; 0 or absent: off (default: 0)')),
    (('--selfsim-layers',), dict(nargs='+', metavar='LAYER',
                                 help='layers of the self-similarity term as name or name:weight; the weights are '
                                      'normalised to --selfsim-weight like those of a layer list and read once per '
                                      'scale; a content map is taken at every one of them (default: the names of '
                                      '--content-layers, or conv4_2 when that list is empty)')),
    (('--selfsim-points',), dict(metavar='N', type=int,
                                 help='most sample positions of the self-similarity term per tile and layer, an '
                                      'integer from 2 to 4096: the blob is thinned to every g-th row and column, g '
                                      'the smallest step that fits; the term forms two N x N matrices, so its cost '
                                      'grows with N squared (default: 1024)')),
    (('--shift-weight',), dict(metavar='WEIGHT', type=ffloat,
                               help='shifted-Gram style factor (Berger & Memisevic): holds the Gram matrices of the '
                                    'feature maps at the --shift-layers against copies of themselves moved by the '
                                    '--shift-offsets to those of the style picture(s) -- the arrangement of a '
                                    'regular texture (brickwork, weave, hatching at a fixed pitch), which every '
                                    'other style term is blind to.  The term is not cheap: at its defaults it '
                                    'takes 8.2 ms beside a 3.8 ms evaluation of a 1024 x 1024 tile on an MI355X, 2.2 '
                                    'tile evaluations (0.8 ms beside 0.8 ms at 256 x 256); fewer --shift-offsets or '
                                    '--shift-layers cut it in proportion; read once per scale; 0 or absent: off '
                                    '(default: 0)')),
    (('--shift-layers',), dict(nargs='+', metavar='LAYER',
                               help='layers of the shifted-Gram term as name or name:weight; the weights are '
                                    'normalised to --shift-weight like those of a layer list and read once per scale; '
                                    'with --style-multiscale the layers themselves stay those of the first scale, '
                                    'whose targets are kept (default: conv1_1 conv2_1 conv3_1)')),
    (('--shift-offsets',), dict(nargs='+', metavar='D', type=int,
                                help="distances of the shifted-Gram term in the layer's own pixels, one to 8 positive "
                                     'integers; each D gives the offsets (0, D) and (D, 0).  A tile blob must be '
                                     'larger than D on both axes; read once per scale (default: 2 4 8)')),
    (('--cx-weight',), dict(metavar='WEIGHT', type=ffloat,
                            help='contextual style factor (Mechrez et al., the contextual loss): soft, scale-free '
                                 'matching of feature vectors -- at the --cx-layers every sampled feature vector of '
                                 'the result spreads a softmax over a bank of the style picture(s)\' feature vectors '
                                 'at a temperature that follows its own best distance, and every bank row is credited '
                                 'with the best share any vector gives it; between the global statistics (Gram, '
                                 '--stat-weight, --swd-weight) and the hard matches of --nnfm-weight.  The term '
                                 'belongs to one tile: every tile\'s sample is asked to cover the whole bank, as '
                                 'with --nnfm-cover.  At its defaults (two layers, 1024 points, a bank of 4096 rows) '
                                 'the term takes 0.52 ms beside a 3.7 ms evaluation of a 1024 x 1024 tile on an '
                                 'MI355X, 0.14 tile evaluations (0.47 ms beside 0.82 ms at 256 x 256, 0.57); read '
                                 'once per scale; 0 or absent: off (default: 0)')),
    (('--cx-layers',), dict(nargs='+', metavar='LAYER',
                            help='layers of the contextual term as name or name:weight; the weights are normalised '
                                 'to --cx-weight like those of a layer list and read once per scale; with '
                                 '--style-multiscale the layers themselves stay those of the first scale, whose '
                                 'banks are kept (default: conv3_2 conv4_2)')),
    (('--cx-points',), dict(metavar='N', type=int,
                            help='most sample positions per tile and layer of the contextual term, an integer from '
                                 '2 to 4096: the blob is thinned to every g-th row and column, g the smallest step '
                                 'that fits; the term forms two N x M matrices against a bank of M rows, and N x M '
                                 'may not pass 2^24 (default: 1024)')),
    (('--cx-rows',), dict(metavar='M', type=int,
                          help='most bank rows of the contextual term per style picture and size, by the same grid '
                               'rule; the banks of all style pictures (and, with --style-multiscale, sizes) are '
                               'concatenated, to 16384 rows at most (default: 4096)')),
    (('--cx-h',), dict(metavar='H', type=ffloat,
                       help='bandwidth of the contextual term, a number above 0: the softmax temperature of a '
                            'feature vector is H times (its best cosine distance + 1e-5) (default: 0.5)')),
    (('--photo-weight',), dict(metavar='WEIGHT', type=ffloat,
                               help='photorealism factor (Luan et al., Deep Photo Style Transfer): penalises a '
                                    "result that is not locally an affine function of the content picture's "
                                    'colours, the quadratic form of the matting Laplacian; keeps straight edges '
                                    'and flat regions when the style is a photograph; 0 or absent: off '
                                    '(default: 0)')),
    (('--photo-eps',), dict(metavar='EPS', type=ffloat,
                            help='regularisation of the matting Laplacian\'s 3 x 3 window covariances, finite '
                                 'and positive (default: 1e-7)')),
    (('--temporal-weight',), dict(metavar='WEIGHT', type=ffloat,
                                  help='temporal-consistency factor for video (Ruder et al., Artistic Style Transfer '
                                       'for Videos): holds the result to the --prev-images, warped to this frame by '
                                       'the --flows, wherever the flow is reliable; disoccluded regions and motion '
                                       'boundaries stay free.  One invocation stylises one frame.  On a 2048 x 2048 picture '
                                       'the term takes 0.039 ms per evaluation on an MI355X, 0.76 of what the '
                                       '--aux-image term takes; 0 or absent: off (default: 0)')),
    (('--prev-images',), dict(nargs='+', metavar='IMAGE',
                              help='one to four earlier stylised frames, closest in time first (default: none)')),
    (('--flows',), dict(nargs='+', metavar='FLO',
                        help='one backward optical flow per earlier frame, from the current content frame to that '
                             "frame, as a Middlebury .flo file of the content picture's size (default: none)")),
    (('--flows-fwd',), dict(nargs='+', metavar='FLO',
                            help='one forward optical flow per earlier frame, from that frame to the current one, '
                                 'for the forward-backward consistency test; without them only motion boundaries '
                                 'and the frame\'s edge make a pixel unreliable (default: none)')),
    (('--prev-contents',), dict(nargs='+', metavar='IMAGE',
                                help='the earlier CONTENT frames, one per --prev-images entry, closest first: the '
                                     "backward and the forward flow of every earlier frame are estimated on the GPU "
                                     "from the content frames at the content picture's size as loaded (Brox et al. "
                                     '2004, a variational solver in float64), instead of being read from --flows / '
                                     '--flows-fwd; the consistency test is always on.  Both flows of one earlier '
                                     'frame at 1024 x 1024 take 35 ms on an MI355X (11.5 ms of device time each), '
                                     'once per run: 0.019 of a whole --size 1024 run; python -m '
                                     'style_transfer_amd.flow writes the same flows as .flo files (default: none)')),
    (('--flow-alpha',), dict(metavar='ALPHA', type=ffloat,
                             help='smoothness weight of the flow estimator, finite and above 0 (default: 18)')),
    (('--flow-gamma',), dict(metavar='GAMMA', type=ffloat,
                             help='weight of the gradient-constancy term of the flow estimator, finite and 0 or '
                                  'more (default: 6)')),
    (('--temporal-init',), dict(action='store_true',
                                help='start from the warped earlier frame(s), and from the content picture where no '
                                     'flow is reliable, instead of noise (default: off)')),
    (('--poisson-lambda',), dict(metavar='LAMBDA', type=ffloat,
                                 help='screened-Poisson output stage (Mechrez et al., Photorealistic Style Transfer '
                                      'with Screened Poisson Equation): every written picture keeps the colours of the '
                                      "result and has its gradients pulled to the content picture's with weight "
                                      'LAMBDA, which takes out wobbling edges and texture in flat regions; finite, '
                                      'above 0 and up to 1000 (5 is a moderate value).  Changes no step of the '
                                      'optimisation; with --preserve-color luma the stage comes first.  A multigrid '
                                      'solve in float64 on the GPU, run at every --save-every picture and at the final '
                                      'one: at 2048 x 2048 with LAMBDA 5 one solve takes 24 ms on an MI355X, '
                                      '0.005 of a whole --size 2048 --tile-size 1024 run; python -m '
                                      'style_transfer_amd.poisson applies the stage to existing pictures (default: '
                                      'off)')),
    (('--poisson-cycles',), dict(metavar='N', type=int,
                                 help='multigrid W-cycles of the screened-Poisson stage, an integer from 1 to 32; a '
                                      'cycle leaves 0.1 to 0.3 of the error (default: 9)')),
]


def build_parser():
    parser = argparse.ArgumentParser(
        description='Tiled neural style transfer on AMD MI355X.',
        formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    for flags, kwargs in _OPTIONS:
        parser.add_argument(*flags, **kwargs)
    for flags, kwargs in _EXTENSIONS:
        parser.add_argument(*flags, default=argparse.SUPPRESS, **kwargs)
    return parser


class ValuePlaceholder:
    """What a lazy option reads as while the run state it depends on does not exist yet
    (config_system.py:147-163 of the reference)."""

    def __repr__(self):
        return 'ValuePlaceholder()'


class LazyArgs:
    """Namespace whose callable values are called with the run-state object on every read."""

    def __init__(self, state, **values):
        object.__setattr__(self, 'state_obj', state)
        object.__setattr__(self, 'ns', argparse.Namespace(**values))

    def __getattr__(self, name):
        value = getattr(object.__getattribute__(self, 'ns'), name)
        if callable(value):
            try:
                return value(object.__getattribute__(self, 'state_obj'))
            except AttributeError:
                return ValuePlaceholder()
        return value

    def __setattr__(self, name, value):
        setattr(self.ns, name, value)

    def __iter__(self):
        return iter(vars(self.ns))

    def __contains__(self, key):
        return key in self.ns

    def __repr__(self):
        return 'LazyArgs(%r)' % vars(self.ns)


CONFIG_SCOPE = dict(detect_devices=detect_devices, math=math, np=np)


def eval_config(path):
    """Runs a config file; its top-level assignments become option values."""
    code = compile(Path(path).read_text(), str(path), 'exec')
    scope = {}
    exec(code, dict(CONFIG_SCOPE), scope)  # pylint: disable=exec-used
    return scope


def raw_option(args, name, default=0):
    """An option as it was given: a value bound to the run state stays the callable it is (reading it through a
    LazyArgs would call it)."""
    return getattr(getattr(args, 'ns', args), name, default)


def option_on(args, name):
    """Whether a weight option switches its term on: a number that is not 0, or a callable of the run state
    (what it will return is not known before the run)."""
    raw = raw_option(args, name)
    return bool(callable(raw) or raw)


def check_style_masks(args):
    """--style-masks names one mask per style image: anything else is refused before any GPU work."""
    masks = getattr(args, 'style_masks', None)
    if masks and len(masks) != len(args.style_images):
        raise ValueError('--style-masks: %d mask(s) for %d style image(s); one per style image is needed'
                         % (len(masks), len(args.style_images)))
    return list(masks) if masks else []


def check_content_mask(args):
    """--content-mask weights the content term: without content layers there is nothing to weight, which is
    refused before any GPU work.  Returns the path, or None."""
    path = getattr(args, 'content_mask', None)
    if path and not args.content_layers:
        raise ValueError('--content-mask needs a content term: --content-layers is empty')
    return path or None


LAP_POOLS_DEFAULT = ('4',)
LAP_POOL_SIZES = (1, 2, 4, 8, 16, 32, 64)


def check_lap_pools(args):
    """The pool sizes of --lap-pools (``P`` or ``P:weight`` each), or of its default when only --lap-weight
    is set, as integers: one to four distinct powers of two from 1 to 64.  Anything else is refused
    before any GPU work.  [] when neither option is set."""
    if getattr(args, 'lap_pools', None) is None and not hasattr(args, 'lap_weight'):
        return []
    given = getattr(args, 'lap_pools', None) or LAP_POOLS_DEFAULT
    if isinstance(given, str):
        given = [given]
    pools = []
    for item in given:
        name, _, weight = str(item).partition(':')
        try:
            size = int(name)
            if weight:
                ffloat(weight)
        except (ValueError, ZeroDivisionError):
            raise ValueError('--lap-pools %s: P or P:weight is expected' % item) from None
        if size not in LAP_POOL_SIZES:
            raise ValueError('--lap-pools %s: the pool size must be a power of two from 1 to 64' % item)
        if size in pools:
            raise ValueError('--lap-pools: pool size %d is given twice' % size)
        pools.append(size)
    if len(pools) > 4:
        raise ValueError('--lap-pools: %d pool sizes, but four at most are taken' % len(pools))
    return pools


PHOTO_EPS_DEFAULT = 1e-7


def check_photo_options(args):
    """--photo-eps regularises 3 x 3 covariances that are singular wherever a window's colours lie on a line:
    a value that is not finite and positive is refused before any GPU work.  (A value bound to the run state
    reads as a placeholder until the run exists and is checked at every evaluation instead.)  Returns
    the eps in force."""
    eps = getattr(args, 'photo_eps', PHOTO_EPS_DEFAULT)
    if isinstance(eps, ValuePlaceholder):
        return eps
    try:
        ok = math.isfinite(float(eps)) and float(eps) > 0
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError('--photo-eps %s: a finite positive value is needed' % (eps,))
    return float(eps)


TEMPORAL_MAX_FRAMES = 4
FLOW_DEFAULTS = dict(flow_alpha=18.0, flow_gamma=6.0)


def flow_value(args, name):
    """--flow-alpha (finite, above 0) or --flow-gamma (finite, 0 or more) as a float, or its default."""
    value = getattr(args, name, FLOW_DEFAULTS[name])
    option = '--' + name.replace('_', '-')
    try:
        number = float(value)
        ok = math.isfinite(number) and (number > 0 if name == 'flow_alpha' else number >= 0)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError('%s %s: a finite value %s is needed' % (option, value,
                                                                  'above 0' if name == 'flow_alpha' else 'of 0 or more'))
    return number


def temporal_prev_contents(args):
    """The --prev-contents paths (closest first), [] when not given; ``check_temporal_options`` checks them."""
    given = getattr(args, 'prev_contents', None)
    return [given] if isinstance(given, str) else list(given or [])


def check_temporal_options(args):
    """--temporal-weight / --prev-images / --flows / --flows-fwd / --temporal-init: refused before any GPU work
    are a weight that is on without earlier frames or without flows, lists of different lengths, more than four
    frames, and --temporal-init together with --init-image or without the term.  Returns (pictures, backward
    flows, forward flows) as lists of paths, all empty when the term is off.  With --prev-contents
    (``temporal_prev_contents`` returns them) the flows are estimated: both lists of flows are then empty, and
    refused are --flows or --flows-fwd beside it, a count other than --prev-images', and --prev-contents, --flow-alpha
    or --flow-gamma without the term or, the latter two, without --prev-contents or out of range."""
    def paths(name):
        given = getattr(args, name, None)
        return [given] if isinstance(given, str) else list(given or [])
    on = option_on(args, 'temporal_weight')
    if getattr(args, 'temporal_init', False):
        if getattr(args, 'init_image', None):
            raise ValueError('--temporal-init and --init-image both name the start image; give one of them')
        if not on:
            raise ValueError('--temporal-init starts from the warped --prev-images, which only the temporal term '
                             'makes: --temporal-weight is off')
    contents = paths('prev_contents')
    for name, option in (('flow_alpha', '--flow-alpha'), ('flow_gamma', '--flow-gamma')):
        if hasattr(args, name):
            if not contents:
                raise ValueError('%s sets the flow estimator of --prev-contents, which is not given' % option)
            flow_value(args, name)
    if contents and not on:
        raise ValueError('--prev-contents gives the frames that the flows of the temporal term are estimated from: '
                         '--temporal-weight is off')
    if not on:
        return [], [], []
    prev, flows, fwd = paths('prev_images'), paths('flows'), paths('flows_fwd')
    if not prev:
        raise ValueError('--temporal-weight needs the earlier stylised frame(s): --prev-images is missing')
    if contents:
        for name, given in (('--flows', flows), ('--flows-fwd', fwd)):
            if given:
                raise ValueError('--prev-contents estimates both flows of every earlier frame, and %s names files to '
                                 'read them from; give one of them' % name)
        if len(prev) > TEMPORAL_MAX_FRAMES:
            raise ValueError('--prev-images: %d frames, but %d at most are taken' % (len(prev), TEMPORAL_MAX_FRAMES))
        if len(contents) != len(prev):
            raise ValueError('--prev-contents: %d content frame(s) for %d --prev-images; one per earlier frame is needed'
                             % (len(contents), len(prev)))
        return prev, [], []
    if not flows:
        raise ValueError('--temporal-weight needs a backward flow per earlier frame: --flows is missing')
    if len(prev) > TEMPORAL_MAX_FRAMES:
        raise ValueError('--prev-images: %d frames, but %d at most are taken' % (len(prev), TEMPORAL_MAX_FRAMES))
    if len(flows) != len(prev):
        raise ValueError('--flows: %d flow(s) for %d --prev-images; one per earlier frame is needed'
                         % (len(flows), len(prev)))
    if fwd and len(fwd) != len(flows):
        raise ValueError('--flows-fwd: %d flow(s) for %d --flows; none, or one per backward flow, is needed'
                         % (len(fwd), len(flows)))
    return prev, flows, fwd


POISSON_LAMBDA_MAX = 1000.0
POISSON_CYCLES_DEFAULT = 9      # (the smallest count that meets the cap on every case, plus 2)
POISSON_MAX_CYCLES = 32


def poisson_lambda(args):
    """--poisson-lambda as a finite float above 0 and up to 1000, or None without the option; anything else, bools
    and strings included, is a ValueError."""
    raw = raw_option(args, 'poisson_lambda', None)
    if raw is None:
        return None
    if (isinstance(raw, bool) or not isinstance(raw, (int, float, np.integer, np.floating)) or not np.isfinite(raw)
            or not 0 < raw <= POISSON_LAMBDA_MAX):
        raise ValueError('--poisson-lambda %r: a finite number above 0 and up to %g is expected'
                         % (raw, POISSON_LAMBDA_MAX))
    return float(raw)


def poisson_cycles(args):
    """--poisson-cycles as an integer from 1 to 32 (default 9); anything else, bools and floats included, is a
    ValueError."""
    raw = raw_option(args, 'poisson_cycles', POISSON_CYCLES_DEFAULT)
    if isinstance(raw, bool) or not isinstance(raw, (int, np.integer)) or not 1 <= raw <= POISSON_MAX_CYCLES:
        raise ValueError('--poisson-cycles %r: an integer from 1 to %d is expected' % (raw, POISSON_MAX_CYCLES))
    return int(raw)


def check_poisson_options(args):
    """--poisson-lambda / --poisson-cycles: refused before any GPU work are a lambda that is not a finite number above
    0 and up to 1000, a cycle count outside 1 .. 32, and --poisson-cycles without --poisson-lambda.  Returns (lambda,
    cycles), or None when the stage is off."""
    lam = poisson_lambda(args)
    if lam is None:
        if raw_option(args, 'poisson_cycles', None) is not None:
            raise ValueError('--poisson-cycles sets the screened-Poisson stage, which is off: --poisson-lambda is '
                             'not given')
        return None
    return lam, poisson_cycles(args)


# the built-in --style-layers list (read from its entry above: one statement of it)
STYLE_LAYERS_DEFAULT = tuple(next(kw['default'] for flags, kw in _OPTIONS if flags[0] == '--style-layers'))


def stat_layer_args(args):
    """The layer list of the mean / std style term (``name`` or ``name:weight`` each): --stat-layers, or the
    names of the --style-layers when only --stat-weight is set (of its built-in list when it is empty: the
    Gram term can be switched off that way).  [] when the term is off (no --stat-weight, or 0)."""
    if not option_on(args, 'stat_weight'):
        return []
    given = getattr(args, 'stat_layers', None)
    if not given:
        given = [str(item).partition(':')[0] for item in args.style_layers] or STYLE_LAYERS_DEFAULT
    return [given] if isinstance(given, str) else list(given)


def check_layer_list(args, items, weight_flag, layers_flag, one_set, known_layers=None, style_side=True):
    """A ``LAYER[:weight]`` list of a style term that has one set of targets (``one_set`` says of what): refused
    together with --style-masks, with a malformed entry, with a layer named twice, with weights that are all 0
    or -- when the network's layers are known -- with a layer it does not have.  Returns the layer names.
    ``style_side`` False: the list of a content-side term, which --style-masks leaves alone."""
    if style_side and getattr(args, 'style_masks', None):
        raise ValueError('%s cannot be combined with --style-masks: there is %s, and masks make every style '
                         'picture a style set of its own' % (weight_flag, one_set))
    names, total = [], 0.0
    for item in items:
        name, _, weight = str(item).partition(':')
        try:
            total += abs(ffloat(weight)) if weight else 1.0
        except (ValueError, ZeroDivisionError):
            raise ValueError('%s %s: LAYER or LAYER:weight is expected' % (layers_flag, item)) from None
        if not name or name in names:
            raise ValueError('%s %s: a layer name, given once, is expected' % (layers_flag, item))
        if known_layers is not None and (name not in known_layers or name == 'data'):
            raise ValueError("%s %s: the network has no layer '%s'" % (layers_flag, item, name))
        names.append(name)
    if not total:
        raise ValueError('%s %s: at least one layer weight must not be 0 (they are normalised to %s)'
                         % (layers_flag, ' '.join(map(str, items)), weight_flag))
    return names


def check_stat_options(args, known_layers=None):
    """--stat-weight / --stat-layers: refused before any GPU work together with --style-masks (there is one
    statistics set and, with masks, one style set per picture) and with a bad layer list (check_layer_list).
    Returns the layer names."""
    items = stat_layer_args(args)
    if not items:
        return []
    return check_layer_list(args, items, '--stat-weight', '--stat-layers', 'one set of statistics targets',
                            known_layers)


NNFM_LAYERS_DEFAULT = ('conv3_1', 'conv4_1')


def nnfm_layer_args(args):
    """The layer list of the nearest-neighbour term (``name`` or ``name:weight`` each): --nnfm-layers, or
    conv3_1 conv4_1.  [] when the term is off (no --nnfm-weight, or 0)."""
    if not option_on(args, 'nnfm_weight'):
        return []
    given = getattr(args, 'nnfm_layers', None) or NNFM_LAYERS_DEFAULT
    return [given] if isinstance(given, str) else list(given)


def nnfm_stride(args):
    """--nnfm-stride as an integer >= 1 (default 1); anything else is a ValueError."""
    raw = raw_option(args, 'nnfm_stride', 1)
    if isinstance(raw, bool) or not isinstance(raw, (int, np.integer)) or raw < 1:
        raise ValueError('--nnfm-stride %r: an integer >= 1 is expected' % (raw,))
    return int(raw)


def nnfm_patch(args):
    """--nnfm-patch as the integer 1 or 3 (default 1); anything else, bools and floats included, is a
    ValueError."""
    raw = raw_option(args, 'nnfm_patch', 1)
    if isinstance(raw, bool) or not isinstance(raw, (int, np.integer)) or raw not in (1, 3):
        raise ValueError('--nnfm-patch %r: 1 or 3 is expected' % (raw,))
    return int(raw)


def nnfm_k(args):
    """--nnfm-k as an integer from 1 to 4 (default 1); anything else, bools and floats included, is a
    ValueError."""
    raw = raw_option(args, 'nnfm_k', 1)
    if isinstance(raw, bool) or not isinstance(raw, (int, np.integer)) or not 1 <= raw <= 4:
        raise ValueError('--nnfm-k %r: an integer from 1 to 4 is expected' % (raw,))
    return int(raw)


def nnfm_cover(args):
    """--nnfm-cover as a finite float >= 0 (default 0: no coverage part); anything else, bools and strings
    included, is a ValueError."""
    raw = raw_option(args, 'nnfm_cover', 0.0)
    if (isinstance(raw, bool) or not isinstance(raw, (int, float, np.integer, np.floating)) or not np.isfinite(raw)
            or raw < 0):
        raise ValueError('--nnfm-cover %r: a finite number >= 0 is expected' % (raw,))
    return float(raw)


def nnfm_bank_rows(channels, h, w, stride=1, patch=1, rows_before=0):
    """Rows that a [channels, h, w] feature map adds to a bank at this stride.  With ``patch`` 3 a bank that
    would reach the library's limit -- (rows_before + rows) x 9 x channels below 2^31 -- is a ValueError, raised
    before anything is allocated."""
    rows = -(-h // stride) * -(-w // stride)
    if patch != 1 and (rows_before + rows) * patch * patch * channels >= 2 ** 31:
        raise ValueError('the NNFM bank of %d x %d x %d-channel patches would have %d rows of %d values, past the '
                         "library's 2^31 offsets: raise --nnfm-stride (now %d), or use --nnfm-patch 1"
                         % (patch, patch, channels, rows_before + rows, patch * patch * channels, stride))
    return rows


NNFM_MAX_SEGMENTS = 8       # style pictures that --nnfm-masks can tell apart (STX_NNFM_MAX_SEGMENTS)


def nnfm_masks(args):
    """The paths of --nnfm-masks as a list; [] without the option."""
    given = getattr(args, 'nnfm_masks', None)
    if not given:
        return []
    return [given] if isinstance(given, str) else list(given)


def check_nnfm_options(args, known_layers=None):
    """--nnfm-weight / --nnfm-layers / --nnfm-stride / --nnfm-patch / --nnfm-k / --nnfm-cover: refused before any GPU
    work together with --style-masks (there is one bank and, with masks, one style set per picture), with a stride
    below 1, with a patch that is not 1 or 3, with a k outside 1 .. 4, with a cover that is not a finite number >= 0,
    with a cover other than 0 beside patch 3 (the coverage part has no patch form) and with a bad layer list
    (check_layer_list).  --nnfm-masks: refused without the term, with a mask count that is not the style images',
    with more than 8 style images, with --nnfm-patch 3 and with a cover other than 0 (the guided term matches single
    vectors and has no coverage part).  Returns the layer names."""
    items = nnfm_layer_args(args)
    masks = nnfm_masks(args)
    if not items:
        if masks and not getattr(args, 'style_masks', None):
            raise ValueError('--nnfm-masks guides the nearest-neighbour term: --nnfm-weight is needed')
        return []
    if not getattr(args, 'style_masks', None):      # (the refusal of --style-masks comes first)
        nnfm_stride(args)
        nnfm_patch(args)
        nnfm_k(args)
        if nnfm_cover(args) != 0 and nnfm_patch(args) != 1:
            raise ValueError('--nnfm-cover %g cannot be combined with --nnfm-patch 3: the coverage part matches '
                             'single feature vectors only' % nnfm_cover(args))
        if masks:
            styles = getattr(args, 'style_images', None)
            if styles is not None and len(masks) != len(styles):
                raise ValueError('--nnfm-masks: %d mask(s) for %d style image(s); one mask per style image is needed'
                                 % (len(masks), len(styles)))
            if len(masks) > NNFM_MAX_SEGMENTS:
                raise ValueError('--nnfm-masks: %d masks; at most %d style images can be told apart'
                                 % (len(masks), NNFM_MAX_SEGMENTS))
            if nnfm_patch(args) != 1:
                raise ValueError('--nnfm-masks cannot be combined with --nnfm-patch 3: the guided term matches '
                                 'single feature vectors only')
            if nnfm_cover(args) != 0:
                raise ValueError('--nnfm-masks cannot be combined with --nnfm-cover %g: the guided term has no '
                                 'coverage part' % nnfm_cover(args))
    return check_layer_list(args, items, '--nnfm-weight', '--nnfm-layers', 'one bank of style features',
                            known_layers)


SWD_LAYERS_DEFAULT = ('conv2_1', 'conv3_1', 'conv4_1')
SWD_QUANTILES = 4096        # samples of a direction's target quantile function
SWD_MAX_DIRS = 4096


def swd_layer_args(args):
    """The layer list of the sliced Wasserstein term (``name`` or ``name:weight`` each): --swd-layers, or
    conv2_1 conv3_1 conv4_1.  [] when the term is off (no --swd-weight, or 0)."""
    if not option_on(args, 'swd_weight'):
        return []
    given = getattr(args, 'swd_layers', None) or SWD_LAYERS_DEFAULT
    return [given] if isinstance(given, str) else list(given)


def swd_dirs(args):
    """--swd-dirs as an integer from 1 to 4096, or None (the default: every layer's channel count); anything
    else, bools and floats included, is a ValueError."""
    raw = raw_option(args, 'swd_dirs', None)
    if raw is None:
        return None
    if isinstance(raw, bool) or not isinstance(raw, (int, np.integer)) or not 1 <= raw <= SWD_MAX_DIRS:
        raise ValueError('--swd-dirs %r: an integer from 1 to %d is expected' % (raw, SWD_MAX_DIRS))
    return int(raw)


def swd_directions(seed, layer, channels, dirs):
    """The directions V [dirs, channels] (float32, unit rows) of the sliced Wasserstein term at one layer:
    ceil(dirs / channels) independent orthonormal bases -- the Q factors of Gaussian matrices drawn from PCG64
    seeded with [seed, crc32(layer name)] -- concatenated and cut to ``dirs`` rows.  The same for the whole run:
    L-BFGS and --style-multiscale need one objective, and targets of several scales are averaged."""
    rng = np.random.Generator(np.random.PCG64([int(seed) & 0xffffffff, zlib.crc32(layer.encode())]))
    bases = []
    for _ in range(-(-int(dirs) // int(channels))):
        q, r = np.linalg.qr(rng.standard_normal((channels, channels)))
        bases.append((q * np.sign(np.diag(r))).T)       # (the sign that makes the factorisation unique)
    return np.ascontiguousarray(np.concatenate(bases)[:dirs], np.float32)


def check_swd_options(args, known_layers=None):
    """--swd-weight / --swd-layers / --swd-dirs: refused before any GPU work together with --style-masks (there
    is one set of targets and, with masks, one style set per picture), with --swd-dirs outside 1 .. 4096 and with
    a bad layer list (check_layer_list).  Returns the layer names."""
    items = swd_layer_args(args)
    if not items:
        return []
    if not getattr(args, 'style_masks', None):      # (the refusal of --style-masks comes first)
        swd_dirs(args)
    return check_layer_list(args, items, '--swd-weight', '--swd-layers', 'one set of sliced Wasserstein targets',
                            known_layers)


SELFSIM_POINTS_DEFAULT = 1024
SELFSIM_MAX_POINTS = 4096


def selfsim_layer_args(args):
    """The layer list of the self-similarity content term (``name`` or ``name:weight`` each): --selfsim-layers, or
    the names of --content-layers, or conv4_2 when that list is empty.  [] when the term is off (no
    --selfsim-weight, or 0)."""
    if not option_on(args, 'selfsim_weight'):
        return []
    given = getattr(args, 'selfsim_layers', None)
    if not given:
        content = getattr(args, 'content_layers', None) or []
        content = [content] if isinstance(content, str) else list(content)
        given = [str(item).partition(':')[0] for item in content] or ['conv4_2']
    return [given] if isinstance(given, str) else list(given)


def selfsim_points(args):
    """--selfsim-points as an integer from 2 to 4096 (default 1024); anything else, bools and floats included, is a
    ValueError."""
    raw = raw_option(args, 'selfsim_points', SELFSIM_POINTS_DEFAULT)
    if isinstance(raw, bool) or not isinstance(raw, (int, np.integer)) or not 2 <= raw <= SELFSIM_MAX_POINTS:
        raise ValueError('--selfsim-points %r: an integer from 2 to %d is expected' % (raw, SELFSIM_MAX_POINTS))
    return int(raw)


def selfsim_grid(h, w, points):
    """(g, rows, columns) of the term's sample grid on an h x w blob: g is the smallest integer >= 1 with
    ceil(h / g) ceil(w / g) <= points; the positions are (a g, b g) in raster order (include/stx.h)."""
    g = 1
    while -(-h // g) * -(-w // g) > points:
        g += 1
    return g, -(-h // g), -(-w // g)


def check_selfsim_options(args, known_layers=None):
    """--selfsim-weight / --selfsim-layers / --selfsim-points: refused before any GPU work with --selfsim-points
    outside 2 .. 4096 and with a bad layer list (check_layer_list).  A content-side term: --style-masks and
    --content-mask leave it alone.  Returns the layer names."""
    items = selfsim_layer_args(args)
    if not items:
        return []
    selfsim_points(args)
    return check_layer_list(args, items, '--selfsim-weight', '--selfsim-layers', '', known_layers, style_side=False)


SHIFT_LAYERS_DEFAULT = ('conv1_1', 'conv2_1', 'conv3_1')
SHIFT_OFFSETS_DEFAULT = (2, 4, 8)
SHIFT_MAX_DISTANCES = 8


def shift_layer_args(args):
    """The layer list of the shifted-Gram term (``name`` or ``name:weight`` each): --shift-layers, or conv1_1
    conv2_1 conv3_1.  [] when the term is off (no --shift-weight, or 0)."""
    if not option_on(args, 'shift_weight'):
        return []
    given = getattr(args, 'shift_layers', None) or SHIFT_LAYERS_DEFAULT
    return [given] if isinstance(given, str) else list(given)


def shift_offsets(args):
    """--shift-offsets as the term's offsets [(dy, dx), ...]: every distance D gives (0, D) and (D, 0), in the
    order given (default 2 4 8).  One to 8 distinct positive integers; anything else, bools and floats included, is
    a ValueError."""
    raw = raw_option(args, 'shift_offsets', None)
    if raw is None:
        raw = SHIFT_OFFSETS_DEFAULT
    if isinstance(raw, (int, np.integer)) and not isinstance(raw, bool):
        raw = [raw]
    if not isinstance(raw, (list, tuple)) or not 1 <= len(raw) <= SHIFT_MAX_DISTANCES:
        raise ValueError('--shift-offsets %r: one to %d positive integers are expected' % (raw, SHIFT_MAX_DISTANCES))
    offsets = []
    for d in raw:
        if isinstance(d, bool) or not isinstance(d, (int, np.integer)) or d < 1:
            raise ValueError('--shift-offsets %r: a positive integer is expected' % (d,))
        if (0, int(d)) in offsets:
            raise ValueError('--shift-offsets: distance %d is given twice' % d)
        offsets += [(0, int(d)), (int(d), 0)]
    return offsets


def check_shift_tile(offsets, layer, scale, tile_hw):
    """An offset that leaves a tile's blob at ``layer`` (``scale`` image pixels per blob pixel, ceil mode) without a
    pair of pixels is refused before any GPU work."""
    h, w = (-(-int(v) // int(scale)) for v in tile_hw)
    for dy, dx in offsets:
        if h - dy < 1 or w - dx < 1:
            raise ValueError('--shift-offsets %d: a %d x %d tile is a %d x %d map at layer %s, which holds no pair of '
                             'pixels at that distance (raise --min-size or drop the offset)'
                             % (max(dy, dx), tile_hw[1], tile_hw[0], w, h, layer))


def check_shift_options(args, known_layers=None):
    """--shift-weight / --shift-layers / --shift-offsets: refused before any GPU work together with --style-masks
    (there is one set of targets and, with masks, one style set per picture), with bad offsets and with a bad layer
    list (check_layer_list).  Returns the layer names."""
    items = shift_layer_args(args)
    if not items:
        return []
    if not getattr(args, 'style_masks', None):      # (the refusal of --style-masks comes first)
        shift_offsets(args)
    return check_layer_list(args, items, '--shift-weight', '--shift-layers', 'one set of shifted-Gram targets',
                            known_layers)


CX_LAYERS_DEFAULT = ('conv3_2', 'conv4_2')
CX_POINTS_DEFAULT = 1024
CX_MAX_POINTS = 4096
CX_ROWS_DEFAULT = 4096
CX_MAX_ROWS = 16384
CX_MAX_CELLS = 2 ** 24
CX_H_DEFAULT = 0.5


def cx_layer_args(args):
    """The layer list of the contextual term (``name`` or ``name:weight`` each): --cx-layers, or conv3_2 conv4_2.
    [] when the term is off (no --cx-weight, or 0)."""
    if not option_on(args, 'cx_weight'):
        return []
    given = getattr(args, 'cx_layers', None) or CX_LAYERS_DEFAULT
    return [given] if isinstance(given, str) else list(given)


def cx_points(args):
    """--cx-points as an integer from 2 to 4096 (default 1024); anything else, bools and floats included, is a
    ValueError."""
    raw = raw_option(args, 'cx_points', CX_POINTS_DEFAULT)
    if isinstance(raw, bool) or not isinstance(raw, (int, np.integer)) or not 2 <= raw <= CX_MAX_POINTS:
        raise ValueError('--cx-points %r: an integer from 2 to %d is expected' % (raw, CX_MAX_POINTS))
    return int(raw)


def cx_rows(args):
    """--cx-rows as an integer from 1 to 16384 (default 4096); anything else, bools and floats included, is a
    ValueError."""
    raw = raw_option(args, 'cx_rows', CX_ROWS_DEFAULT)
    if isinstance(raw, bool) or not isinstance(raw, (int, np.integer)) or not 1 <= raw <= CX_MAX_ROWS:
        raise ValueError('--cx-rows %r: an integer from 1 to %d is expected' % (raw, CX_MAX_ROWS))
    return int(raw)


def cx_h(args):
    """--cx-h as a finite float above 0 (default 0.5); anything else, bools and strings included, is a ValueError."""
    raw = raw_option(args, 'cx_h', CX_H_DEFAULT)
    if (isinstance(raw, bool) or not isinstance(raw, (int, float, np.integer, np.floating)) or not np.isfinite(raw)
            or not np.float32(raw) > 0):
        raise ValueError('--cx-h %r: a finite number above 0 is expected' % (raw,))
    return float(raw)


def check_cx_bank(total, points, rows):
    """A contextual bank of ``total`` rows past the library's limits -- 16384 rows, points x rows up to 2^24 -- is a
    ValueError that names both options."""
    if total > CX_MAX_ROWS or points * total > CX_MAX_CELLS:
        raise ValueError('the contextual bank would have %d rows: with --cx-points %d at most %d are possible; lower '
                         '--cx-rows (now %d) or --cx-points'
                         % (total, points, min(CX_MAX_ROWS, CX_MAX_CELLS // points), rows))


def cx_bank_rows(h, w, rows, rows_before=0, points=CX_POINTS_DEFAULT):
    """Rows that an h x w feature map adds to a contextual bank under a budget of ``rows`` (the grid rule of
    selfsim_grid); a bank past the limits (check_cx_bank) is refused before anything is allocated."""
    _, gh, gw = selfsim_grid(h, w, rows)
    check_cx_bank(rows_before + gh * gw, points, rows)
    return gh * gw


def check_cx_options(args, known_layers=None):
    """--cx-weight / --cx-layers / --cx-points / --cx-rows / --cx-h: refused before any GPU work together with
    --style-masks (there is one bank and, with masks, one style set per picture, as for --nnfm-weight), with points
    outside 2 .. 4096, rows outside 1 .. 16384, a bandwidth that is not a finite number above 0, and with a bad
    layer list (check_layer_list).  Returns the layer names."""
    items = cx_layer_args(args)
    if not items:
        return []
    if not getattr(args, 'style_masks', None):      # (the refusal of --style-masks comes first)
        cx_points(args)
        cx_rows(args)
        cx_h(args)
    return check_layer_list(args, items, '--cx-weight', '--cx-layers', 'one contextual bank', known_layers)


def parse_args(state=None, argv=None, config_py=None):
    """Returns the merged options.  ``config_py`` defaults to ``config.py`` beside the entry
    script of THIS package (the repository's ``style_transfer.py``), like the reference, which
    looks next to its own config_system.py -- never next to whatever launcher started the process
    (pytest, torch.distributed.run, ...).  ``config_py=False`` reads no default file."""
    parser = build_parser()
    defaults = vars(parser.parse_args([]))
    given = vars(parser.parse_args(argv))
    merged = dict(defaults)
    if config_py is None:
        config_py = Path(__file__).resolve().parent.parent / 'config.py'
    if config_py and Path(config_py).exists():
        merged.update(eval_config(config_py))
    # (an extension option is in `given` only when the command line names it, and never in `defaults`)
    merged.update({k: v for k, v in given.items() if k not in defaults or defaults[k] != v})
    if given['config']:
        merged.update(eval_config(given['config']))
    args = LazyArgs(state, **merged)
    if args.debug:
        os.environ['DEBUG'] = '1'
    if not args.list_layers and (not args.content_image or not args.style_images):
        parser.print_help()
        sys.exit(1)
    check_style_masks(args)
    check_content_mask(args)
    check_lap_pools(args)
    check_stat_options(args)
    check_nnfm_options(args)
    check_swd_options(args)
    check_selfsim_options(args)
    check_shift_options(args)
    check_cx_options(args)
    check_photo_options(args)
    check_temporal_options(args)
    check_poisson_options(args)
    return args
