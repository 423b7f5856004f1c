"""The reference vectors (make_golden.py's output) on disk: one set of named arrays stored as
reference_vectors.npz, reference_vectors_1.npz, reference_vectors_2.npz, ... so that no file
passes 1 MiB (the repository's limit for a committed file).  Arrays go to the parts in key order,
a new part when the next array would take the current one past PART_BYTES; load() merges them.

Numpy only: the tests' `golden` fixture, make_golden.py / branch_sets.py and tools/ all use it."""

import io
import os
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
STEM = 'reference_vectors'
PART_BYTES = 960 * 1024          # estimated compressed bytes per part (the written files are checked)
MAX_FILE_BYTES = 1 << 20


def part_path(k, folder=HERE):
    return os.path.join(folder, '%s.npz' % STEM if k == 0 else '%s_%d.npz' % (STEM, k))


def load(folder=HERE):
    """{name: array} over every part."""
    out, k = {}, 0
    while os.path.exists(part_path(k, folder)):
        with np.load(part_path(k, folder)) as z:
            for name in z.files:
                assert name not in out, (name, part_path(k, folder))
                out[name] = z[name]
        k += 1
    if not k:
        raise FileNotFoundError(part_path(0, folder))
    return out


def _packed_size(a):
    buf = io.BytesIO()
    np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
    return len(zlib.compress(buf.getvalue(), 6)) + 256


def save(arrays, folder=HERE):
    """Writes {name: array} as parts (np.savez_compressed each) and removes parts left over from a
    larger earlier set.  Returns the paths written."""
    parts, size = [[]], 0
    for name in sorted(arrays):
        n = _packed_size(arrays[name])
        if parts[-1] and size + n > PART_BYTES:
            parts.append([])
            size = 0
        parts[-1].append(name)
        size += n
    paths = []
    for k, names in enumerate(parts):
        path = part_path(k, folder)
        np.savez_compressed(path, **{name: arrays[name] for name in names})
        if os.path.getsize(path) > MAX_FILE_BYTES:
            raise RuntimeError('%s is %d bytes (over %d): lower PART_BYTES'
                               % (path, os.path.getsize(path), MAX_FILE_BYTES))
        paths.append(path)
    k = len(parts)
    while os.path.exists(part_path(k, folder)):
        os.remove(part_path(k, folder))
        k += 1
    return paths
