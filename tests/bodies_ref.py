"""The body selection of include/fgcn.h (fgcn_clip_bodies) restated in numpy float64, from the header's text and not from the reference:
``scores(x)``, ``order(scores)``, ``select(x, M)`` for one clip ``x`` of shape (Mr, T, V, C)."""
import numpy as np


def non_null(body: np.ndarray) -> np.ndarray:
    """(T) bool: the frames of a (T, V, C) body that hold a value (-0 is zero, a NaN is a value)"""
    return (body != 0).reshape(len(body), -1).any(axis=1)


def scores(x: np.ndarray) -> np.ndarray:
    x = np.asarray(x)
    out = np.zeros(len(x), dtype=np.float64)
    for m, body in enumerate(x):
        frames = body[non_null(body)].astype(np.float64)
        n = frames.shape[0] * frames.shape[1]
        if n == 0:
            continue                                        # +0
        with np.errstate(invalid="ignore", over="ignore"):
            for c in range(frames.shape[2]):
                mean = frames[:, :, c].sum() / n
                out[m] += np.sqrt(((frames[:, :, c] - mean) ** 2).sum() / n)
    return out


def order(s: np.ndarray) -> np.ndarray:
    """descending; a NaN above every number; equal keys: the higher source index first"""
    keys = [(1, 0.0, m) if np.isnan(v) else (0, float(v), m) for m, v in enumerate(s)]
    return np.array(sorted(range(len(keys)), key=keys.__getitem__, reverse=True), dtype=np.int32)


def select(x: np.ndarray, M: int) -> np.ndarray:
    return np.asarray(x)[order(scores(x))[:M]]


def frames_counted(x: np.ndarray) -> np.ndarray:
    """(Mr): n = |F| * V of every body, the number of terms of each of its sums (the tolerance of the device's scores scales with it)"""
    x = np.asarray(x)
    return np.array([non_null(body).sum() * x.shape[2] for body in x], dtype=np.int64)
