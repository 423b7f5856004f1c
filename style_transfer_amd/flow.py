"""Optical flow files in the Middlebury ``.flo`` format, which the temporal term reads (--flows, --flows-fwd):
little endian; the float32 magic 202021.25; int32 width, int32 height; then H * W interleaved (u, v) float32
pairs, row by row.  A vector with a component above 1e9 in magnitude marks a pixel whose flow is unknown.
"""

import numpy as np

FLO_MAGIC = np.float32(202021.25)
FLO_UNKNOWN = np.float32(1e10)       # what writers put where the flow is unknown (anything above 1e9 counts)


def read_flo(path):
    """A ``.flo`` file as a float32 array [2, H, W]: plane 0 horizontal, plane 1 vertical.  A wrong magic, a
    non-positive size or a short file is a ValueError that names the file."""
    with open(path, 'rb') as f:
        data = f.read()
    if len(data) < 12:
        raise ValueError('%s: %d byte(s) hold no .flo header (12 bytes)' % (path, len(data)))
    if np.frombuffer(data, '<f4', 1)[0] != FLO_MAGIC:
        raise ValueError('%s: not a .flo file (the magic number 202021.25 is missing)' % (path,))
    w, h = (int(v) for v in np.frombuffer(data, '<i4', 2, 4))
    if w <= 0 or h <= 0:
        raise ValueError('%s: a flow of %d x %d' % (path, w, h))
    if len(data) < 12 + 8 * w * h:
        raise ValueError('%s: %d bytes are too few for a flow of %d x %d (%d)' % (path, len(data), w, h, 12 + 8 * w * h))
    pairs = np.frombuffer(data, '<f4', 2 * w * h, 12).reshape(h, w, 2)
    return np.ascontiguousarray(pairs.transpose(2, 0, 1), np.float32)


def write_flo(path, array):
    """Writes a flow [2, H, W] (anything ``np.float32`` takes) as a ``.flo`` file."""
    flow = np.asarray(array, np.float32)
    if flow.ndim != 3 or flow.shape[0] != 2 or flow.shape[1] < 1 or flow.shape[2] < 1:
        raise ValueError('write_flo: an array of shape %s, but [2, H, W] is needed' % (flow.shape,))
    with open(path, 'wb') as f:
        f.write(np.float32(FLO_MAGIC).astype('<f4').tobytes())
        f.write(np.array([flow.shape[2], flow.shape[1]], '<i4').tobytes())
        f.write(np.ascontiguousarray(flow.transpose(1, 2, 0)).astype('<f4').tobytes())
