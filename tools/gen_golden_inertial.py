#!/usr/bin/env python3
"""Writes tests/golden/inertial.npz from the REFERENCE's own inertial preprocessing (util/preprocessing: interpolator.py, sequence.py,
signal.py, processor/skeleton.py, processor/inertial.py), CPU only, on a machine that has the reference checked out
(``FGCN_REFERENCE``).  Nothing of the reference is copied: the file holds the inputs this script draws and the arrays the reference's
functions return for them.  Two runs write the same bytes (fixed seed, fixed archive time stamps).

Index tables, for Li in LI and every Ls in 2 .. 128:

    idx_<Li>          NearestNeighborInterpolator._compute_indices(Li, Ls), the tables of all Ls one behind the other (Ls = 2 first;
                      the table of Ls starts at (Ls - 2) (Ls + 1) / 2), stored as int16 (no value exceeds 325)

For every clip case (DESIGN.md section 8h lists them):

    <case>_skel       float32 (M, T, V, C): the raw skeleton recording, Ls frames, zero from frame Ls on
    <case>_imu        float32 (Li, S): the raw inertial recording
    <case>_dims       Ls, Li, T as integers
    <case>_args       origin joint, z pair, x pair of the skeleton normalisation as five integers (-1, -1 = no pair)
    <case>_padded     float32 (T, S): pad_sequence_numpy(imu[_compute_indices(Li, Ls)], T, (Li, S)) -- imu itself where Li == Ls
    <case>_signal     float32 (T, S): InertialProcessor(None).process(...), asserted equal to normalize_signal(<case>_padded)
    <case>_enhanced   float32 (M, T, V + S / 3, 3): SkeletonProcessor("imu_enhanced").process(...); its joints [0, V) are the
                      reference's normalised skeleton, which the tests feed back as the skeleton source

Asserted while writing: the half-up formula floor(x + 0.5) and the multiply-first formula rint(t (Li - 1) / (Ls - 1)) each differ from the
reference on at least one recorded table; every recorded array has the dtype above; the appended joints of <case>_enhanced equal
<case>_padded reshaped, on every body; no recorded signal is constant.

Stubs.  The reference's modules import, at the top, libraries that no value recorded here needs: ``cv2`` (video decoding),
``util.preprocessing.cnn_features`` (torchvision encoders) and ``tqdm`` (progress bars); each is replaced by a permissive stub module when
it cannot be imported.  ``np.int``, which the interpolator uses, was removed from NumPy 1.24: it is set to ``int``, which is what it was.
"""
import os
import sys
import types
import zipfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("FGCN_REFERENCE", "/root/reference")
sys.dont_write_bytecode = True


class _Stub(types.ModuleType):
    """a module whose every attribute exists (annotations such as cv2.VideoCapture are evaluated at import) and does nothing"""

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return lambda *a, **kw: None


if not hasattr(np, "int"):
    np.int = int
for _name in ("cv2", "tqdm", "util.preprocessing.cnn_features"):
    try:
        if _name.startswith("util."):
            raise ImportError                            # torchvision and its model downloads: never wanted here
        __import__(_name)
    except ImportError:
        sys.modules[_name] = _Stub(_name)
if isinstance(sys.modules.get("tqdm"), _Stub):
    sys.modules["tqdm"].tqdm = lambda it, **kw: it
sys.path.insert(0, REF)
from util.preprocessing import sequence as ref_sequence, signal as ref_signal          # noqa: E402
from util.preprocessing.data_loader import SequenceStructure                            # noqa: E402
from util.preprocessing.interpolator import NearestNeighborInterpolator                 # noqa: E402
from util.preprocessing.processor.inertial import InertialProcessor                     # noqa: E402
from util.preprocessing.processor.skeleton import SkeletonProcessor                     # noqa: E402

LI = (2, 4, 6, 180, 326)
LS = range(2, 129)
SEED = 20261019
ARGS7 = (2, (3, 2), (4, 6))             # origin joint, z pair, x pair of the 7-joint cases (tests/golden/normalize.npz uses the same)
UTD = (2, None, None)                   # the 20-joint UTD-MHAD cases: centred only, so that the float32 result is exact to the bit


def tables():
    out = {}
    half_up = multiply_first = 0
    for li in LI:
        rows = []
        for ls in LS:
            idx = NearestNeighborInterpolator._compute_indices(li, ls)
            assert idx.shape == (ls,) and idx.min() == 0 and idx.max() == li - 1
            t = np.arange(ls)
            half_up += not np.array_equal(idx, np.floor(t * ((li - 1) / (ls - 1)) + 0.5).astype(int))
            multiply_first += not np.array_equal(idx, np.rint(t * (li - 1) / (ls - 1)).astype(int))
            rows.append(idx)
        out[f"idx_{li}"] = np.concatenate(rows).astype(np.int16)
    assert half_up > 0 and multiply_first > 0, (half_up, multiply_first)
    print(f"index tables: {len(LI) * len(LS)}; half-up differs on {half_up}, multiply-first on {multiply_first}")
    return out


def cases():
    """-> [(name, M, T, V, C, S, Ls, Li, normalisation args, all-positive signal)]"""
    return [
        ("c01_full", 1, 13, 7, 3, 6, 13, 29, ARGS7, False),                  # Ls == T: no padding
        ("c02_padded_positive", 1, 13, 7, 3, 6, 9, 29, ARGS7, True),         # Ls < T, the minimum is the padding's zero
        ("c03_equal_lengths", 1, 13, 7, 3, 6, 9, 9, ARGS7, False),           # Li == Ls: taken as it is
        ("c04_upsampling", 1, 13, 7, 3, 6, 11, 4, ARGS7, False),             # Li < Ls
        ("c05_two_frames", 1, 13, 7, 3, 6, 2, 29, ARGS7, False),             # Ls == 2: the first and the last frame
        ("c06_326_to_79", 1, 128, 7, 3, 6, 79, 326, ARGS7, False),           # where multiply-first differs; T = 128
        ("c07_two_coordinates", 1, 13, 7, 2, 6, 10, 29, (1, None, None), False),
        ("c08_two_bodies", 2, 13, 7, 3, 6, 8, 21, ARGS7, False),
        ("c09_three_values", 1, 13, 7, 3, 3, 7, 12, ARGS7, False),           # S == 3: one appended joint
        ("c10_utd_a", 1, 16, 20, 3, 6, 12, 40, UTD, False),                  # the two clips of the end-to-end test: T = 16
        ("c11_utd_b", 1, 16, 20, 3, 6, 16, 33, UTD, False),
    ]


def run_reference(skel, imu, Ls, Li, T, args):
    """-> (padded, signal, enhanced) through the reference's processors; skel (M, T, V, C) raw, imu (Li, S) raw"""
    M, _, V, C = skel.shape
    S = imu.shape[1]
    interp = {"skeleton": NearestNeighborInterpolator(), "inertial": NearestNeighborInterpolator()}
    structure = {"skeleton": SequenceStructure(T, (T, V, C, M), np.float32), "inertial": SequenceStructure(326, (326, S), np.float32)}
    lengths = {"skeleton": Ls, "inertial": Li}
    # the leaf functions, one by one
    resampled = imu if Li == Ls else imu[NearestNeighborInterpolator._compute_indices(Li, Ls)]
    padded = ref_sequence.pad_sequence_numpy(resampled, T, (Li, S))
    leaf_signal = ref_signal.normalize_signal(padded.copy())
    # the processors (the loaders' layout of a skeleton recording is (frames, joints, coordinates, bodies))
    p = InertialProcessor(None)
    p.set_input_structure({"inertial": structure["inertial"]}, T)
    signal = p.process({"inertial": imu.copy()}, {"inertial": Li}, {"inertial": _target(Ls)}, None)
    assert np.array_equal(signal, leaf_signal)
    p = SkeletonProcessor("imu_enhanced")
    p.set_input_structure(structure, T)
    origin, zp, xp = args
    enhanced = p.process({"skeleton": np.ascontiguousarray(skel[:, :Ls].transpose(1, 2, 3, 0)), "inertial": imu.copy()}, lengths, interp, None,
                         skeleton_center_joint=origin, skeleton_z_joints=zp, skeleton_x_joints=xp, imu_num_signals=S // 3)
    assert enhanced.shape == (M, T, V + S // 3, 3)
    for m in range(M):
        assert np.array_equal(enhanced[m, :, V:], padded.reshape(T, S // 3, 3))
    assert all(a.dtype == np.float32 for a in (padded, signal, enhanced))
    assert np.isfinite(signal).all() and signal.min() == 0.0 and signal.max() == 1.0
    return padded, signal, enhanced


def _target(Ls):
    """InertialProcessor alone resamples to its own length; the data group sets the main modality's length on the interpolator
    (datagroup.py:131-135: global_target_sequence_length), which is what this does"""
    it = NearestNeighborInterpolator()
    it.global_target_sequence_length = Ls
    return it


def record():
    rng = np.random.default_rng(SEED)
    out = {"seed": np.int64(SEED)}
    out.update(tables())
    for name, M, T, V, C, S, Ls, Li, args, positive in cases():
        skel = rng.uniform(0.5, 3.0, (M, T, V, C)).astype(np.float32)
        skel[:, Ls:] = 0
        imu = (rng.uniform(0.25, 2.0, (Li, S)) if positive else rng.standard_normal((Li, S))).astype(np.float32)
        padded, signal, enhanced = run_reference(skel, imu, Ls, Li, T, args)
        if positive:
            assert Ls < T and padded.min() == 0.0 and padded[:Ls].min() > 0.0
        origin, zp, xp = args
        out[f"{name}_skel"], out[f"{name}_imu"] = skel, imu
        out[f"{name}_dims"] = np.array([Ls, Li, T], dtype=np.int64)
        out[f"{name}_args"] = np.array([origin, *(zp or (-1, -1)), *(xp or (-1, -1))], dtype=np.int64)
        out[f"{name}_padded"], out[f"{name}_signal"], out[f"{name}_enhanced"] = padded, signal, enhanced
        print(f"{name}: skeleton {skel.shape}, recording {imu.shape}, Ls = {Ls}, T = {T}")
    return out


def main():
    out = record()
    path = os.path.join(REPO, "tests", "golden", "inertial.npz")
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:          # (np.savez stamps the entries with the time of day)
        for key, a in out.items():
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with z.open(info, "w") as f:
                np.lib.format.write_array(f, np.asanyarray(a), allow_pickle=False)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
