"""TEST INFRASTRUCTURE -- read and write the golden .npz archives of ``tests/golden/``.

A committed file stays under 1 MiB, so an archive larger than that is stored as ``<name>.part1.npz``, ``<name>.part2.npz``, ...
(``save``), and ``load`` merges the parts back into one mapping that reads like ``np.load``'s: ``[key]`` and ``.files``, keys in
the order they were written.  An archive small enough to be one file is written and read as ``<name>.npz`` as before.
"""
from __future__ import annotations

import glob
import os
import re

import numpy as np

PART_BYTES = 900 * 1024             # budget per part, under the 1 MiB limit with room for the zip and .npy headers
_ENTRY_OVERHEAD = 400               # zip local + central header and .npy header of one entry, bytes (generous)


class Parts(dict):
    """The merged arrays of a split archive."""

    @property
    def files(self):
        return list(self)


def _parts(path: str):
    base = path[:-len(".npz")]
    found = glob.glob(glob.escape(base) + ".part*.npz")
    num = {p: re.fullmatch(r"\.part(\d+)\.npz", p[len(base):]) for p in found}
    return sorted((p for p, m in num.items() if m), key=lambda p: int(num[p].group(1)))


def load(path: str):
    """``np.load(path)`` for an archive stored whole, the merged parts for one stored split."""
    if os.path.exists(path):
        return np.load(path)
    parts = _parts(path)
    if not parts:
        raise FileNotFoundError(path)
    out = Parts()
    for p in parts:
        with np.load(p) as z:
            out.update((k, z[k]) for k in z.files)
    return out


def save(path: str, store: dict, compressed: bool = False) -> list:
    """Write ``store`` as ``path`` if it fits one part, else as ``<path minus .npz>.partN.npz`` files of at most PART_BYTES of
    payload each, in key order; stale parts or a stale whole file of the same archive are removed.  -> the files written."""
    groups, cur, size = [], {}, 0
    for k, v in store.items():
        n = np.asarray(v).nbytes + _ENTRY_OVERHEAD
        if cur and size + n > PART_BYTES:
            groups.append(cur)
            cur, size = {}, 0
        cur[k] = v
        size += n
    groups.append(cur)
    write = np.savez_compressed if compressed else np.savez
    for stale in _parts(path) + ([path] if os.path.exists(path) else []):
        os.remove(stale)
    if len(groups) == 1:
        write(path, **groups[0])
        return [path]
    names = [f"{path[:-len('.npz')]}.part{i + 1}.npz" for i in range(len(groups))]
    for name, g in zip(names, groups):
        write(name, **g)
    return names
