"""The screened-Poisson output stage of --poisson-lambda (stx_image_poisson, include/stx.h: Mechrez, Shechtman,
Zelnik-Manor, BMVC 2017, as a fixed count of multigrid W-cycles in float64 on the GPU), its level and launch counts,
and a command line that applies it to existing pictures:

    python -m style_transfer_amd.poisson RESULT.png CONTENT.png OUT.png --poisson-lambda L [--poisson-cycles N]

OUT.png keeps the colours of RESULT.png and has its gradients pulled to those of CONTENT.png, which is resized to
RESULT.png's size with the pipeline's Lanczos resize first.
"""

import argparse
import sys

import numpy as np

from .config_system import POISSON_CYCLES_DEFAULT, POISSON_LAMBDA_MAX, POISSON_MAX_CYCLES    # noqa: F401

POISSON_COARSEST_LAMBDA = 0.05
POISSON_PRE, POISSON_POST, POISSON_COARSEST = 2, 2, 20      # sweeps before and after the coarse visits; at the coarsest
MEAN_BGR = (103.939, 116.779, 123.68)


def levels(height, width, lam):
    """The multigrid's levels as [(h, w, lambda)] from the picture down: h' = ceil(h / 2), w' = ceil(w / 2), lambda'
    = lambda / 4; a level is the coarsest when min(h, w) <= 2 or lambda <= 0.05."""
    out = [(int(height), int(width), float(lam))]
    while not (min(out[-1][0], out[-1][1]) <= 2 or out[-1][2] <= POISSON_COARSEST_LAMBDA):
        h, w, l = out[-1]
        out.append(((h + 1) // 2, (w + 1) // 2, l / 4.0))
    return out


def launch_count(height, width, lam, cycles=POISSON_CYCLES_DEFAULT):
    """Kernel launches of one solve (csrc/poisson.hip): the right-hand side and the output, and per W-cycle, with
    2^l visits of level l, 40 half-sweeps at a visit of the coarsest level and, at a visit of any other, 8
    half-sweeps, one residual + restriction and one prolongation + add."""
    n = len(levels(height, width, lam))
    per_cycle = sum((2 ** l) * (2 * POISSON_COARSEST if l == n - 1 else 2 * (POISSON_PRE + POISSON_POST) + 2)
                    for l in range(n))
    return 2 + cycles * per_cycle


def pil_to_picture(picture, mean_bgr=MEAN_BGR):
    """RGB PIL picture -> BGR CHW float32 minus mean, as the pipeline keeps its pictures."""
    arr = np.float32(picture.convert('RGB')).transpose((2, 0, 1))[::-1]
    return np.ascontiguousarray(arr - np.float32(mean_bgr).reshape((3, 1, 1)))


def apply(engine, pil_result, pil_content, lam, cycles=None, mean_bgr=MEAN_BGR):
    """RGB HWC uint8 array of ``pil_result`` through the stage against ``pil_content`` (resized to its size with
    Lanczos when it differs).  The device pictures are freed."""
    from PIL import Image
    from . import image_ops
    if pil_content.size != pil_result.size:
        pil_content = pil_content.convert('RGB').resize(pil_result.size, Image.LANCZOS)
    s, c = engine.to_device(pil_to_picture(pil_result, mean_bgr)), engine.to_device(pil_to_picture(pil_content, mean_bgr))
    solved = None
    try:
        solved = image_ops.poisson(engine, s, c, lam, cycles)
        return image_ops.to_u8(engine, solved, np.float32(mean_bgr).reshape((3, 1, 1)))
    finally:
        engine.sync()           # (the pictures are read by the queued launches)
        for array in (s, c, solved):
            if array is not None:
                array.free()


def build_poisson_parser():
    ap = argparse.ArgumentParser(prog='python -m style_transfer_amd.poisson',
                                 description='The screened-Poisson output stage on existing pictures: OUT keeps the '
                                             "colours of RESULT and has its gradients pulled to CONTENT's.")
    ap.add_argument('result', metavar='RESULT', help='the stylised picture')
    ap.add_argument('content', metavar='CONTENT', help="the content picture; resized to RESULT's size (Lanczos)")
    ap.add_argument('out', metavar='OUT', help='where the picture is written')
    ap.add_argument('--poisson-lambda', type=float, required=True, metavar='LAMBDA',
                    help='weight of the gradient term, finite, above 0 and up to 1000')
    ap.add_argument('--poisson-cycles', type=int, default=argparse.SUPPRESS, metavar='N',
                    help='multigrid W-cycles, from 1 to 32 (default: %d)' % POISSON_CYCLES_DEFAULT)
    ap.add_argument('--device', type=int, default=0, metavar='N', help='the GPU (default: %(default)s)')
    return ap


def parse_poisson_args(argv=None):
    """The command line's options, checked: everything that can be refused before an engine exists is refused here
    (a ValueError that names the option)."""
    from .config_system import check_poisson_options
    opts = build_poisson_parser().parse_args(argv)
    opts.poisson_lambda, opts.poisson_cycles = check_poisson_options(opts)
    if opts.device < 0:
        raise ValueError('--device %d: a device number of 0 or more is needed' % opts.device)
    return opts


def main(argv=None):
    from PIL import Image
    from .engine import TileEngine
    from .netspec import builtin_net
    opts = parse_poisson_args(argv)
    engine = TileEngine(builtin_net('vgg19'), opts.device)         # (no weights: only the image entries are used)
    try:
        with Image.open(opts.result) as result, Image.open(opts.content) as content:
            picture = apply(engine, result, content, opts.poisson_lambda, opts.poisson_cycles)
        Image.fromarray(picture).save(opts.out)
    finally:
        engine.close()
    return 0


if __name__ == '__main__':
    sys.exit(main())
