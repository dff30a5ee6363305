"""Host-side reference of the clip window and of the valid-frame count (include/fgcn.h), shared by
tests/test_window.py and tests/test_window_gpu.py (no test in here).  numpy float64, written from the contract's formulas and independent
of csrc/fgcn_window.hip; the generator is tests/augment_ref.py's Philox (tests/dropout_ref.py).

* ``params``: the table row {o, r} of a sample from (sample, site, epoch, seed), the interval and the mode, as the contract states it.
* ``transform``: the windowed rows from a GIVEN table (the device's own, in the GPU tests), source rows and valid frame counts.
* ``reads32``: the frames f0, f1 and the weight w of every output frame in the contract's OWN float32 arithmetic -- which source frames an
  output reads is a discrete fact, and a float64 position that differs from the float32 one in its last bits can fall on the other side of
  a frame boundary; ``classes`` uses it to say which outputs a non-finite source value reaches, and as what.
* ``valid_frames``: the count of a clip's valid frames.
"""
import numpy as np

from augment_ref import U24, ulps32  # noqa: F401  (ulps32: for the tests)
from dropout_ref import M32, philox4x32_10

RANDOM, CENTRE = 0, 1                     # enum fgcn_window_mode


def words(sample, site, epoch, seed, j=2):
    """the four words of the block at counter word ``j``: the window draws from j = 2, the augmentation from j = 0 and 1"""
    key = (seed & M32, (seed >> 32) & M32)
    return philox4x32_10((sample & M32, site & M32, epoch & M32, j), key)


def uniforms(sample, site, epoch, seed):
    """-> u0, u1: words 0 and 1 of block j = 2, u = (w >> 8) * 2^-24"""
    return ((words(sample, site, epoch, seed)[:2] >> np.uint32(8)).astype(np.float64) * U24).tolist()


def params(sample, site, epoch, seed, lo, hi, mode):
    """-> (o, r) float64.  lo and hi are taken as the float32 values the C ABI receives."""
    lo, hi = float(np.float32(lo)), float(np.float32(hi))
    if mode == CENTRE:
        return (1.0 - hi) / 2.0, hi
    u0, u1 = uniforms(sample, site, epoch, seed)
    r = lo + u0 * (hi - lo)
    return u1 * (1.0 - r), r


def clamp_valid(v, T):
    return T if v is None else min(max(int(v), 1), T)


def _as5(src):
    src = np.asarray(src)
    return src if src.ndim == 5 else src[:, None, :, None, :]


def transform(src, idx, table, W, valid=None):
    """src: (rows, M, T, V, C) or (rows, T, S); idx: (b) source rows; table: (b, 2) = o, r; valid: None or (rows) frame counts indexed by
    source row (clamped into [1, T], as the kernel does) -> (b, M, W, V, C) or (b, W, S) float64"""
    src = np.asarray(src, dtype=np.float64)
    x5, table = _as5(src), np.asarray(table, dtype=np.float64)
    T = x5.shape[2]
    out = np.empty((len(idx), x5.shape[1], W, *x5.shape[3:]))
    for k, s in enumerate(np.asarray(idx).tolist()):
        o, r = table[k]
        v = clamp_valid(None if valid is None else valid[s], T)
        for t in range(W):
            pos = (o + r * (t / (W - 1) if W > 1 else 0.0)) * (v - 1)
            f0 = min(max(int(np.floor(pos)), 0), v - 1)
            f1 = min(f0 + 1, v - 1)
            w = pos - f0
            out[k, :, t] = (1.0 - w) * x5[s, :, f0] + w * x5[s, :, f1]
    return out.reshape((len(idx), x5.shape[1], W, *src.shape[3:]) if src.ndim == 5 else (len(idx), W, src.shape[2]))


def _fma32(a, b, c):
    """fma of three float32: the product of two float32 is exact in float64, the sum is rounded to float64 and then to float32 (the two
    roundings differ from one only where the float64 sum lies within 2^-29 relative of a float32 tie: not at the tests' values)"""
    return np.float32(np.float64(a) * np.float64(b) + np.float64(c))


def reads32(o, r, W, v):
    """-> [(f0, f1, w)] for t = 0 .. W-1 in the contract's float32 arithmetic; o, r: the table's float32 values, v: the clamped count"""
    o, r, vm1 = np.float32(o), np.float32(r), np.float32(v - 1)
    ratio = vm1 / np.float32(W - 1) if W > 1 else np.float32(0.0)
    out = []
    for t in range(W):
        pos = _fma32(r * np.float32(t), ratio, o * vm1)
        f0 = min(max(int(np.floor(pos)), 0), v - 1)
        out.append((f0, min(f0 + 1, v - 1), np.float32(pos - np.float32(f0))))
    return out


def classify(a):
    """0 finite, 1 NaN, 2 +inf, 3 -inf"""
    a = np.asarray(a)
    return np.where(np.isnan(a), 1, np.where(a == np.inf, 2, np.where(a == -np.inf, 3, 0))).astype(np.int8)


def classes(src, idx, table, W, valid=None):
    """-> (reads, cls): per output element, whether it reads a non-finite source value, and the class (``classify``) of
    fma(w, x[f1] - x[f0], x[f0]) with the frames and weights of ``reads32``"""
    src = np.asarray(src, dtype=np.float32)
    x5 = _as5(src)
    T = x5.shape[2]
    shape = (len(idx), x5.shape[1], W, *x5.shape[3:])
    reads, y = np.zeros(shape, dtype=bool), np.empty(shape, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        for k, s in enumerate(np.asarray(idx).tolist()):
            v = clamp_valid(None if valid is None else valid[s], T)
            for t, (f0, f1, w) in enumerate(reads32(table[k][0], table[k][1], W, v)):
                x0, x1 = x5[s, :, f0].astype(np.float64), x5[s, :, f1].astype(np.float64)
                reads[k, :, t] = ~np.isfinite(x0) | ~np.isfinite(x1)
                y[k, :, t] = np.float64(w) * (x1 - x0) + x0
    final = (len(idx), x5.shape[1], W, *src.shape[3:]) if src.ndim == 5 else (len(idx), W, src.shape[2])
    return reads.reshape(final), classify(y).reshape(final)


def valid_frames(src, idx=None):
    """-> (b) int32: 1 + the last frame in which any body of source row idx[k] holds a value that is not zero (-0 is zero, a NaN is a
    value); 1 for a clip that holds none"""
    x5 = _as5(src)
    idx = range(len(x5)) if idx is None else np.asarray(idx).tolist()
    out = []
    for s in idx:
        holds = (x5[s] != 0).any(axis=(0, 2, 3))                               # per frame; NaN != 0 is True, -0.0 != 0 is False
        out.append(int(np.flatnonzero(holds)[-1]) + 1 if holds.any() else 1)
    return np.asarray(out, dtype=np.int32)
