"""Reading and writing the fixtures of tests/golden/ within the 1 MiB limit of a committed file.

A fixture `NAME.npz` that would be larger than PART_BYTES is stored as `NAME.part0.npz`, `NAME.part1.npz`, ... (every
array unchanged, compressed, in its original order); an array that alone does not fit one part is stored flat in pieces
`KEY::piece0`, `KEY::piece1`, ... after `KEY::shape`.  `load(path)` takes the name of the logical fixture (`NAME.npz`)
and returns a read-only mapping with the interface of numpy's NpzFile that the tests use (`.files`, `[key]`, `in`,
`keys()` / `items()`, `close()`, `with`), whichever way the fixture is stored.  The generators write through `save`.
"""
import glob
import io
import math
import os
import re
from collections.abc import Mapping

import numpy as np

PART_BYTES = 960 * 1024      # target size of one part file (the limit for a committed file is 1 MiB)
_SEP = "::"


def _parts(path):
    stem = path[:-len(".npz")] if path.endswith(".npz") else path
    found = glob.glob(glob.escape(stem) + ".part*.npz")
    found = [(int(m.group(1)), f) for f in found for m in [re.search(r"\.part(\d+)\.npz$", f)] if m]
    return [f for _, f in sorted(found)]


class Fixture(Mapping):
    """The logical fixture over its part files (arrays are read on access, like NpzFile)."""

    def __init__(self, paths):
        self._npz = [np.load(p) for p in paths]
        self._where, self._pieces, self.files = {}, {}, []
        for z in self._npz:
            for k in z.files:
                if _SEP not in k:
                    self._where[k] = z
                    self.files.append(k)
                    continue
                key, tag = k.rsplit(_SEP, 1)
                if tag == "shape":
                    self._where[key] = None
                    self._pieces[key] = [z[k]]
                    self.files.append(key)
                else:
                    self._pieces[key].append((z, k))

    def __getitem__(self, key):
        z = self._where[key]
        if z is not None:
            return z[key]
        shape, pieces = self._pieces[key][0], self._pieces[key][1:]
        return np.concatenate([p[k] for p, k in pieces]).reshape(tuple(int(s) for s in shape))

    def __iter__(self):
        return iter(self.files)

    def __len__(self):
        return len(self.files)

    def __contains__(self, key):
        return key in self._where

    def close(self):
        for z in self._npz:
            z.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def load(path):
    """`path` names the logical fixture (`.../NAME.npz`): the single file when it exists, else its parts"""
    if os.path.exists(path):
        return np.load(path)
    paths = _parts(path)
    if not paths:
        raise FileNotFoundError(path)
    return Fixture(paths)


def _compressed_size(arrays):
    buf = io.BytesIO()
    np.savez_compressed(buf, **arrays)
    return buf.tell()


def save(path, **arrays):
    """np.savez_compressed(path, **arrays), split into parts of at most PART_BYTES when the single file would be larger"""
    for old in _parts(path) + ([path] if os.path.exists(path) else []):
        os.remove(old)
    arrays = {k: np.asarray(v) for k, v in arrays.items()}
    if _compressed_size(arrays) <= PART_BYTES:
        np.savez_compressed(path, **arrays)
        return [path]
    budget = PART_BYTES - 32 * 1024           # room for the zip directory of a part
    items = []                                # (name, array, compressed size) in the fixture's order
    for k, v in arrays.items():
        assert _SEP not in k, k
        size = _compressed_size({k: v})
        if size <= budget:
            items.append((k, v, size))
            continue
        n = math.ceil(size / (0.8 * budget))
        items.append((k + _SEP + "shape", np.array(v.shape, np.int64), 0))
        for i, piece in enumerate(np.array_split(v.reshape(-1), n)):
            items.append(("%s%spiece%d" % (k, _SEP, i), piece, _compressed_size({"x": piece})))
    groups, cur, used = [], {}, 0
    for k, v, size in items:
        if cur and used + size > budget:
            groups.append(cur)
            cur, used = {}, 0
        cur[k] = v
        used += size
    groups.append(cur)
    stem = path[:-len(".npz")]
    written = []
    for i, g in enumerate(groups):
        p = "%s.part%d.npz" % (stem, i)
        np.savez_compressed(p, **g)
        assert os.path.getsize(p) <= 1024 * 1024, (p, os.path.getsize(p))
        written.append(p)
    return written
