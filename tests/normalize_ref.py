"""Host-side restatement of the skeleton normalisation (include/fgcn.h), shared by tests/test_normalize.py and
tests/test_normalize_gpu.py (no test in here).  numpy, written from the contract's formulas and independent of csrc/fgcn_normalize.hip:
the frame map of every body, then float64 arithmetic from the float32 input -- centring, the mask of missing joints, both rotations
and their product -- and ONE rounding to float32 at the end.

A frame of a body is null when all its V * C values are zero (-0 counts as zero); a body is invalid when all its frames are null; a
joint of a frame is missing when its C values are zero.  (The reference tests ``sum() == 0``: the two differ only where non-zero values
cancel exactly; tools/gen_golden_normalize.py asserts that the golden inputs have no such frame or joint.)
"""
import numpy as np

EPS = 1e-6                # the reference's epsilon: a bone, a rotation axis or an angle below it skips the pass
U23 = 2.0 ** -23          # one float32 ulp at 1: the bound of the rotated result, relative to the clip's largest magnitude


def frame_map(clip):
    """clip (M, T, V, C) -> (maps (M, T) int32, valid (M) bool): output frame t of body m is source frame maps[m, t]."""
    clip = np.asarray(clip)
    M, T = clip.shape[:2]
    maps = np.tile(np.arange(T, dtype=np.int32), (M, 1))
    valid = np.zeros(M, dtype=bool)
    t = np.arange(T)
    for m in range(M):
        nonnull = np.any(clip[m] != 0, axis=(1, 2))
        if not nonnull.any():
            continue                                                 # an invalid body: the identity map
        valid[m] = True
        base = np.flatnonzero(nonnull) if not nonnull[0] else np.arange(np.flatnonzero(nonnull)[-1] + 1)
        f = len(base)
        maps[m] = np.where(t < f, base[np.minimum(t, f - 1)], base[(t - f) % f])
    return maps, valid


def centred(clip, origin_joint):
    """Stages 1 and 2 -> (float64 (M, T, V, C), maps, valid): padded, the centre of body 0 subtracted, missing joints zero."""
    maps, valid = frame_map(clip)
    x = np.asarray(clip).astype(np.float64)
    padded = np.stack([x[m, maps[m]] for m in range(x.shape[0])])
    centre = padded[0, :, origin_joint:origin_joint + 1, :]          # (T, 1, C); zero when body 0 is invalid
    present = np.any(padded != 0, axis=-1, keepdims=True)
    return np.where(present, padded - centre, 0.0), maps, valid


def rodrigues(bone, axis_index):
    """The matrix that turns ``bone`` to the unit axis ``axis_index``, or None where the contract skips the pass."""
    bone = np.asarray(bone, dtype=np.float64)
    axis = np.zeros(3)
    axis[axis_index] = 1.0
    if np.abs(bone).sum() < EPS:
        return None
    k = np.cross(bone, axis)
    theta = np.arccos(np.clip(bone[axis_index] / np.sqrt((bone * bone).sum()), -1.0, 1.0))
    if np.abs(k).sum() < EPS or abs(theta) < EPS:
        return None
    k = k / np.sqrt((k * k).sum())
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(theta) * K + (1.0 - np.cos(theta)) * (K @ K)


def normalize(clip, origin_joint, z_axis_joints=None, x_axis_joints=None):
    """-> dict: ``out`` float32 (M, T, V, C), ``out64`` the value before the rounding, ``centred`` float32 (stages 1 and 2 alone),
    ``frame_map`` (M, T) int32, ``params`` (12) float64 = R row-major, z applied, x applied, the number of valid bodies."""
    c, maps, valid = centred(clip, origin_joint)
    R, applied = np.eye(3), [0.0, 0.0]
    if z_axis_joints is not None:
        j0, j1 = z_axis_joints
        Rz = rodrigues(c[0, 0, j1] - c[0, 0, j0], 2)
        if Rz is not None:
            R, applied[0] = Rz, 1.0
    if x_axis_joints is not None:
        j0, j1 = x_axis_joints
        Rx = rodrigues(R @ c[0, 0, j1] - R @ c[0, 0, j0], 0)          # the bone of the clip as it stands: after the z pass
        if Rx is not None:
            R, applied[1] = Rx @ R, 1.0
    out64 = c @ R.T if any(applied) else c
    return {"out": out64.astype(np.float32), "out64": out64, "centred": c.astype(np.float32), "frame_map": maps,
            "params": np.concatenate([R.reshape(9), applied, [float(valid.sum())]])}
