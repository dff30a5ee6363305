"""Host-side reference of the sensor augmentation (include/fgcn.h), shared by tests/test_sensors.py and
tests/test_sensors_gpu.py (no test in here).  numpy float64 throughout, written from the contract's formulas and independent of
csrc/fgcn_sensors.hip; the generator is tests/dropout_ref.py's Philox.

* ``params``: the table row of a sample -- rotation, then gain, drop flag and knots per sensor -- from (sample, site, epoch, seed).
* ``catmull_rom`` / ``warp``: the magnitude factor of a frame from a sensor's knots.
* ``noise``: the three standard normal values of (frame, sensor), Box-Muller on the block's words.
* ``transform``: the augmented rows from a GIVEN table (the device's own, in the GPU tests: that separates the transform from the
  trigonometric functions) and the restatement's own noise.
* ``minmax32``: the float32 min-max formula of fgcn_signal_prepare's contract, in numpy float32.
"""
import numpy as np

from augment_ref import rotation, ulps32
from dropout_ref import M32, philox4x32_10, threshold

U24 = 2.0 ** -24
JITTER_BASE = 1 << 20


def _block(sample, site, epoch, seed, j):
    return philox4x32_10((sample & M32, site & M32, epoch & M32, j & M32), (seed & M32, (seed >> 32) & M32))


def _uniform(words):
    return (np.asarray(words) >> np.uint32(8)).astype(np.float64) * U24


def row_floats(sensors):
    return 12 + 12 * sensors


def params(sample, site, epoch, seed, sensors, max_angle, scale, warp, knots, drop):
    """-> (12 + 12 G,) float64: R = Rz Ry Rx row-major, 0, 0, 0, then per sensor s_g, the drop flag, 0, 0, d_{g,0..7}.  The magnitudes are
    taken as the float32 values the C ABI receives."""
    ang = [float(np.float32(a)) for a in max_angle]
    scale, warp = float(np.float32(scale)), float(np.float32(warp))
    u = _uniform(_block(sample, site, epoch, seed, 3))
    row = [rotation(*[(2.0 * u[a] - 1.0) * ang[a] for a in range(3)]).reshape(9), np.zeros(3)]
    for g in range(sensors):
        j = 16 + 4 * g
        w = _block(sample, site, epoch, seed, j)
        ku = np.concatenate([_uniform(_block(sample, site, epoch, seed, j + 1)), _uniform(_block(sample, site, epoch, seed, j + 2))])
        d = np.where(np.arange(8) < knots, (2.0 * ku - 1.0) * warp, 0.0)
        row.append(np.concatenate([[1.0 + (2.0 * _uniform(w[0]) - 1.0) * scale, float(int(w[1]) < threshold(drop)), 0.0, 0.0], d]))
    return np.concatenate(row)


def catmull_rom(d, knots, t, v):
    """delta of frame t of v valid frames: the Catmull-Rom value through the ``knots`` values ``d`` at q = t (K - 1) / (v - 1), end knots
    repeated"""
    q = t * (knots - 1) / (v - 1) if v > 1 else 0.0
    i = min(int(np.floor(q)), knots - 2)
    f = q - i
    p0, p1, p2, p3 = d[max(i - 1, 0)], d[i], d[i + 1], d[min(i + 2, knots - 1)]
    return 0.5 * ((-f ** 3 + 2 * f ** 2 - f) * p0 + (3 * f ** 3 - 5 * f ** 2 + 2) * p1 + (-3 * f ** 3 + 4 * f ** 2 + f) * p2 + (f ** 3 - f ** 2) * p3)


def warp(d, knots, t, v):
    return 1.0 if knots == 0 else 1.0 + catmull_rom(d, knots, t, v)


def noise(sample, site, epoch, seed, t, g, sensors):
    """-> (3,) float64: n_0, n_1 the two branches of (w0, w1), n_2 the cosine branch of (w2, w3) of block 2^20 + t G + g"""
    w = [int(x) >> 8 for x in _block(sample, site, epoch, seed, JITTER_BASE + t * sensors + g)]
    rad = [np.sqrt(-2.0 * np.log((w[e] + 1) * U24)) for e in (0, 2)]              # u1 in (0, 1]
    phi = [2.0 * np.pi * (w[e] * U24) for e in (1, 3)]                           # 2 pi u2
    return np.array([rad[0] * np.cos(phi[0]), rad[0] * np.sin(phi[0]), rad[1] * np.cos(phi[1])])


def transform(src, idx, ids, table, *, seed, epoch, site, knots, jitter, valid=None, joints=None):
    """src: (rows, M, T, V, 3) with joints = (lo, hi) or (rows, T, S) (joints None: all S / 3 triples); idx: (b) source rows; ids: (b) sample
    ids; table: (b, 12 + 12 G), whose rotation, gains, drop flags and knots are used as they are; jitter: a scalar or (G) -> (b, ...) float64:
    gain and rotation, warp, jitter, drop on the valid frames of the sensors, everything else copied."""
    src, table = np.asarray(src, dtype=np.float64), np.asarray(table, dtype=np.float64)
    x5 = src if src.ndim == 5 else src.reshape(src.shape[0], 1, src.shape[1], src.shape[2] // 3, 3)
    lo, hi = joints if joints is not None else (0, x5.shape[3])
    G, T = hi - lo, x5.shape[2]
    sigma = np.broadcast_to(np.asarray(jitter, dtype=np.float32).astype(np.float64), (G,))
    out = x5[np.asarray(idx)].copy()
    for k, s in enumerate(np.asarray(idx).tolist()):
        R = table[k, :9].reshape(3, 3)
        v = T if valid is None else min(max(int(valid[s]), 1), T)
        for g in range(G):
            grp = table[k, 12 + 12 * g:24 + 12 * g]
            for t in range(v):
                y = grp[0] * (x5[s, :, t, lo + g] @ R.T) * warp(grp[4:], knots, t, v)          # (M, 3): every body alike
                if sigma[g] != 0.0:
                    y = y + sigma[g] * noise(int(ids[k]), site, epoch, seed, t, g, G)
                out[k, :, t, lo + g] = 0.0 if grp[1] != 0.0 else y
    return out.reshape(len(idx), *src.shape[1:])


def minmax32(y):
    """(b, T, S) float32 -> (the normalised clips, (b, 2) mn / mx), every clip by mn = min, mx = fl32(max - mn), fl32(fl32(y - mn) / mx)"""
    y = np.asarray(y, dtype=np.float32)
    flat = y.reshape(len(y), -1)
    mn = flat.min(1)
    mx = (flat.max(1) - mn).astype(np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        out = ((y - mn[:, None, None]).astype(np.float32) / mx[:, None, None]).astype(np.float32)
    return out, np.stack([mn, mx], 1)


def check_table(table, ref, sensors):
    """The bounds the table is held to, on the host and on the device alike: R within 16 * 2^-24 absolute (three trigonometric factors at
    <= 2 ulp each, two products and a sum), R R^T = I to the same bound, det R > 0; s_g and the knots within 4 float32 ulps; the drop flags
    and the zeros exactly.  ``ref``: ``params`` of the same rows."""
    n = row_floats(sensors)
    table, ref = np.asarray(table, dtype=np.float64).reshape(-1, n), np.asarray(ref, dtype=np.float64).reshape(-1, n)
    bound = 16 * U24
    assert np.abs(table[:, :9] - ref[:, :9]).max() <= bound, np.abs(table[:, :9] - ref[:, :9]).max()
    assert np.all(table[:, 9:12] == 0)
    for row in table:
        r = row[:9].reshape(3, 3)
        assert np.abs(r @ r.T - np.eye(3)).max() <= bound, np.abs(r @ r.T - np.eye(3)).max()
        assert np.linalg.det(r) > 0
    got, want = table[:, 12:].reshape(len(table), sensors, 12), ref[:, 12:].reshape(len(ref), sensors, 12)
    assert np.array_equal(got[:, :, 1:4], want[:, :, 1:4]), (got[:, :, 1:4], want[:, :, 1:4])
    assert np.all(ulps32(got[:, :, 0], want[:, :, 0]) <= 4)
    nz = want[:, :, 4:] != 0
    assert np.all(got[:, :, 4:][~nz] == 0) and np.all(ulps32(got[:, :, 4:][nz], want[:, :, 4:][nz]) <= 4)
