"""Host-side restatement of the preparation of raw inertial recordings (include/fgcn.h), shared by
tests/test_inertial.py and tests/test_inertial_gpu.py (no test in here).  numpy, written from the contract's formulas and independent of
csrc/fgcn_imu.hip.  Every step is integer arithmetic, float32 arithmetic that numpy rounds correctly, or a copy: the tests compare
value for value, with no tolerance.

The reference's SkeletonProcessor("imu_enhanced") imports (tools/gen_golden_inertial.py records through it), so ``enhanced`` below is
checked against its output; it restates the eleven lines that assemble the array (processor/skeleton.py:89-104).
"""
import numpy as np


def resample_indices(Li, Ls):
    """-> (Ls) int64: the frame of a recording of Li frames that every frame of its resampling to Ls frames reads."""
    if Li == Ls:
        return np.arange(Ls, dtype=np.int64)
    if Ls == 1:
        return np.zeros(1, dtype=np.int64)
    factor = np.float64(Li - 1) / np.float64(Ls - 1)                 # the quotient first
    return np.clip(np.rint(np.arange(Ls, dtype=np.float64) * factor).astype(np.int64), 0, Li - 1)      # rint: ties to even


def padded(imu, Li, Ls, T):
    """imu (L >= Li, S) float32 -> (T, S) float32: resampled to Ls frames, zero from frame Ls on."""
    imu = np.asarray(imu, dtype=np.float32)
    out = np.zeros((T, imu.shape[1]), dtype=np.float32)
    out[:Ls] = imu[:Li][resample_indices(Li, Ls)]
    return out


def signal(imu, Li, Ls, T, minmax=True):
    """-> (out (T, S) float32, stats (2) float32 = mn, mx): min-max normalised over the padded array, the padding's zeros included."""
    x = padded(imu, Li, Ls, T)
    if not minmax:
        return x, np.array([0.0, 1.0], dtype=np.float32)
    mn = x.min()
    shifted = x - mn                                                 # float32
    mx = shifted.max()
    with np.errstate(invalid="ignore", divide="ignore"):
        out = shifted / mx                                           # float32, correctly rounded; 0 / 0 for a constant array
    assert out.dtype == np.float32
    return out, np.array([mn, mx], dtype=np.float32)


def enhanced(skeleton, imu, Li, Ls):
    """skeleton (M, T, V, C) float32, NORMALISED, C = 2 or 3 -> (M, T, V + S / 3, 3) float32: the padded recording (not min-max normalised)
    appended as joints of three values to every body; a third coordinate of zero where the skeleton has two."""
    skeleton = np.asarray(skeleton, dtype=np.float32)
    M, T, V, C = skeleton.shape
    x = padded(imu, Li, Ls, T)
    S = x.shape[1]
    assert S % 3 == 0 and C in (2, 3)
    out = np.zeros((M, T, V + S // 3, 3), dtype=np.float32)
    out[:, :, :V, :C] = skeleton
    out[:, :, V:] = x.reshape(1, T, S // 3, 3)
    return out
