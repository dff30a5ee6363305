"""Host-side reference of the clip augmentation (include/fgcn.h), shared by tests/test_augment.py and
tests/test_augment_gpu.py (no test in here).  numpy float64 throughout, written from the contract's formulas and independent of
csrc/fgcn_augment.hip; the generator is tests/dropout_ref.py's Philox.

* ``params``: the table row of a sample from (sample, site, epoch, seed) and the magnitudes, as the contract states it.
* ``transform``: the augmented rows from a GIVEN table (the device's own, in the GPU tests: that separates the transform from the
  trigonometric functions), source rows, and valid frame counts.
"""
import numpy as np

from dropout_ref import M32, philox4x32_10

U24 = 2.0 ** -24          # half an ulp of a float32 in [1, 2): the relative rounding error of one float32 operation


def uniforms(sample, site, epoch, seed):
    """-> the eight uniforms of a sample, words 0..3 of block j = 0 then of block j = 1: u = (w >> 8) * 2^-24"""
    key = (seed & M32, (seed >> 32) & M32)
    words = np.concatenate([philox4x32_10((sample & M32, site & M32, epoch & M32, j), key) for j in (0, 1)])
    return (words >> np.uint32(8)).astype(np.float64) * U24


def rotation(tx, ty, tz):
    cx, sx, cy, sy, cz, sz = np.cos(tx), np.sin(tx), np.cos(ty), np.sin(ty), np.cos(tz), np.sin(tz)
    rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return rz @ ry @ rx


def params(sample, site, epoch, seed, max_angle, scale, min_window):
    """-> (12,) float64: A = s Rz Ry Rx row-major, o, r, 0.  The magnitudes are taken as the float32 values the C ABI receives."""
    u = uniforms(sample, site, epoch, seed)
    ang = [float(np.float32(a)) for a in max_angle]
    scale, min_window = float(np.float32(scale)), float(np.float32(min_window))
    theta = [(2.0 * u[a] - 1.0) * ang[a] for a in range(3)]
    s = 1.0 + (2.0 * u[3] - 1.0) * scale
    r = min_window + u[4] * (1.0 - min_window)
    o = u[5] * (1.0 - r)
    return np.concatenate([(s * rotation(*theta)).reshape(9), [o, r, 0.0]])


def transform(src, idx, table, valid=None, joints=None):
    """src: (rows, M, T, V, C) or (rows, T, S); idx: (b) source rows; table: (b, 12); valid: None or (rows) frame counts indexed by
    source row; joints: None or (lo, hi) -> (b, ...) float64: interpolation first, then the matrix on joints [lo, hi)."""
    src, table = np.asarray(src, dtype=np.float64), np.asarray(table, dtype=np.float64)
    x5 = src if src.ndim == 5 else src[:, None, :, None, :]
    T = x5.shape[2]
    out = np.empty((len(idx), *x5.shape[1:]))
    for k, s in enumerate(np.asarray(idx).tolist()):
        o, r = table[k, 9], table[k, 10]
        v = T if valid is None else int(valid[s])
        for t in range(T):
            pos = (o + r * (t / (T - 1) if T > 1 else 0.0)) * (v - 1)
            f0 = min(max(int(np.floor(pos)), 0), v - 1)
            f1 = min(f0 + 1, v - 1)
            w = pos - f0
            out[k, :, t] = (1.0 - w) * x5[s, :, f0] + w * x5[s, :, f1]
        if joints is not None:
            lo, hi = joints
            out[k, :, :, lo:hi] = out[k, :, :, lo:hi] @ table[k, :9].reshape(3, 3).T
    return out.reshape(len(idx), *src.shape[1:])


def ulps32(got, want):
    """|got - want| in units of the float32 spacing at ``want``"""
    want = np.asarray(want, dtype=np.float64)
    return np.abs(np.asarray(got, dtype=np.float64) - want) / np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)


def check_table(table, ref, scale):
    """The bounds the table is held to, on the host and on the device alike: o, r within 4 float32 ulps; entries of A within
    16 * 2^-24 * (1 + scale) absolute (three trigonometric factors at <= 2 ulp each, two products and a sum); A A^T = s^2 I to the same
    bound; det A > 0.  ``ref``: ``params`` of the same rows."""
    table, ref = np.asarray(table, dtype=np.float64).reshape(-1, 12), np.asarray(ref, dtype=np.float64).reshape(-1, 12)
    bound = 16 * U24 * (1.0 + scale)
    assert np.all(ulps32(table[:, 9:11], ref[:, 9:11]) <= 4), (table[:, 9:11], ref[:, 9:11])
    assert np.all(table[:, 11] == 0)
    assert np.abs(table[:, :9] - ref[:, :9]).max() <= bound, np.abs(table[:, :9] - ref[:, :9]).max()
    for row, want in zip(table, ref):
        a = row[:9].reshape(3, 3)
        s2 = np.linalg.det(want[:9].reshape(3, 3)) ** (2.0 / 3.0)            # det(s R) = s^3
        assert np.abs(a @ a.T - s2 * np.eye(3)).max() <= bound, np.abs(a @ a.T - s2 * np.eye(3)).max()
        assert np.linalg.det(a) > 0
