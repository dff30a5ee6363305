"""The input streams of include/fgcn.h (fgcn_clip_streams) restated in numpy, from the header's contract and not from
the kernel (a helper module: no test).  float32 throughout: every value is one correctly rounded float32 subtraction, a copy or a zero, which
is what numpy's float32 subtraction gives, so the comparison with the kernel is bit for bit."""
import numpy as np

STREAMS = ("joint", "bone", "motion", "bone_motion")


def clamp_valid(valid, T: int) -> int:
    """the valid frame count the kernel uses: T without a table, a value outside [1, T] clamped into it"""
    return T if valid is None else int(min(max(int(valid), 1), T))


def bone(x: np.ndarray, parents) -> np.ndarray:
    """x (M, T, V, C) float32 -> x[t, v] - x[t, parents[v]]; parents[v] == -1: x[t, v] itself"""
    assert x.dtype == np.float32 and x.ndim == 4 and len(parents) == x.shape[2]
    out = np.empty_like(x)
    for v, p in enumerate(parents):
        out[:, :, v] = x[:, :, v] if p == -1 else x[:, :, v] - x[:, :, p]
    return out


def motion(x: np.ndarray, valid=None) -> np.ndarray:
    """x (M, T, V, C) float32 -> x[t + 1] - x[t] for t < L - 1, +0 from frame L - 1 on; no frame at or behind L takes part"""
    assert x.dtype == np.float32 and x.ndim == 4
    L = clamp_valid(valid, x.shape[1])
    out = np.zeros_like(x)
    out[:, :L - 1] = x[:, 1:L] - x[:, :L - 1]
    return out


def streams(x: np.ndarray, parents, valid=None) -> dict:
    """all four streams of one clip"""
    b = bone(x, parents)
    return {"joint": x.copy(), "bone": b, "motion": motion(x, valid), "bone_motion": motion(b, valid)}


def batch(src: np.ndarray, idx, parents, valid=None) -> dict:
    """src (rows, M, T, V, C), idx (b) -> {stream: (b, M, T, V, C)}; valid: None or one count per SOURCE row"""
    clips = [streams(src[r], parents, None if valid is None else valid[r]) for r in idx]
    return {s: np.stack([c[s] for c in clips]) for s in STREAMS}


def same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32),
                                                                                      np.ascontiguousarray(b).view(np.uint32))


def same_values(a: np.ndarray, b: np.ndarray) -> bool:
    """where NaN is expected: NaN where NaN (whatever its payload), the same bits elsewhere"""
    if not (a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b))):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(a[ok].view(np.uint32), b[ok].view(np.uint32))
