#!/usr/bin/env python3
"""Writes tests/golden/normalize.npz from the REFERENCE's own skeleton preprocessing (util/preprocessing/skeleton.py), CPU only, on a
machine that has the reference checked out (``FGCN_REFERENCE``).  Nothing of the reference is copied: the file holds the inputs this
script draws and the arrays the reference's functions return for them.

For every case (DESIGN.md section 8g lists them):

    <case>_x          the float32 input clip (M, T, V, C)
    <case>_args       origin joint, z pair, x pair as five integers (-1, -1 = no pair)
    <case>_centred    float32: move_skeleton_origin(pad_null_frames(x), origin) run on the float32 array
    <case>_gold64     float64: normalize_skeleton(x.astype(float64), origin, z pair, x pair)
    <case>_applied    whether the reference applied the z and the x rotation (0 / 1)

Asserted while writing: (a) the reference's ``sum() == 0`` and the contract's "every value is zero" agree on every frame and joint
of every input; (b) every rotation the reference applies has an angle in [0.2, 2.9] rad -- away from the thresholds, where float64
round-off in the angle cannot decide anything; (c) a pass the reference skips leaves the array exactly as it was, and the cases built
to be skipped are skipped.

The reference module imports tqdm at the top for its progress bars; no value needs it, so it is stubbed when it is not installed.
"""
import importlib.util
import os
import sys
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("FGCN_REFERENCE", "/root/reference")
sys.dont_write_bytecode = True

try:
    import tqdm  # noqa: F401
except ImportError:
    _t = types.ModuleType("tqdm")
    _t.tqdm = lambda it, **kw: it
    sys.modules["tqdm"] = _t
_spec = importlib.util.spec_from_file_location("ref_skeleton", os.path.join(REF, "util", "preprocessing", "skeleton.py"))
ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref)

SHAPE = (2, 13, 7, 3)
ARGS = (2, (3, 2), (4, 6))          # origin joint, z pair, x pair of the (2, 13, 7, 3) cases: UTD-MHAD's pattern (z ends in the origin)
ANGLES = (0.2, 2.9)


def draw(rng, shape):
    return rng.uniform(0.5, 3.0, shape).astype(np.float32)


def null(x, body, frames):
    x[body, list(frames)] = 0
    return x


def cases(rng):
    """-> [(name, x, origin, z, x pair, expected (z applied, x applied) or None)]"""
    out = []

    def add(name, x, args=ARGS, expect=(1, 1)):
        out.append((name, x, *args, expect))

    add("c01_full", draw(rng, SHAPE))
    add("c02a_trailing_f9", null(null(draw(rng, SHAPE), 0, range(9, 13)), 1, range(5, 13)))
    add("c02b_trailing_f2", null(draw(rng, SHAPE), 0, range(2, 13)))
    add("c02c_trailing_f1", null(null(draw(rng, SHAPE), 0, range(1, 13)), 1, range(12, 13)))
    add("c03_compaction", null(null(draw(rng, SHAPE), 0, (0, 1, 5, 10, 11, 12)), 1, (0,)))
    add("c04_interior", null(null(draw(rng, SHAPE), 0, (6,)), 1, (3, 9, 10, 11, 12)))
    add("c05_body1_null", null(draw(rng, SHAPE), 1, range(13)))
    add("c06_body0_null", null(draw(rng, SHAPE), 0, range(13)), expect=(0, 0))
    x = draw(rng, SHAPE)
    x[:, :, 5] = 0
    add("c07_missing_joint", x)
    for name, z3, expect in (("c08_z_parallel", 1.0, (0, 1)), ("c09_z_antiparallel", 2.0, (0, 1)), ("c10_z_degenerate", 1.5, (0, 1))):
        x = draw(rng, SHAPE)
        x[0, 0, 2] = (1.25, 2.0, 1.5)                    # bone = x[2] - x[3] = (0, 0, 1.5 - z3), exact in float32
        x[0, 0, 3] = (1.25, 2.0, z3)
        add(name, x, expect=expect)
    add("c11_mmact_2d", null(draw(rng, (1, 5, 4, 2)), 0, (4,)), args=(1, None, None), expect=(0, 0))
    add("c12_long", null(draw(rng, (1, 130, 3, 3)), 0, list(range(0, 3)) + [70] + list(range(100, 130))), args=(1, (0, 1), (0, 2)))
    add("c13_v64", draw(rng, (1, 3, 64, 3)), args=(1, (0, 1), (4, 63)))
    return out


class AngleOutOfRange(Exception):
    pass


def angle(bone, axis):
    return float(np.arccos(np.dot(bone / np.linalg.norm(bone), axis)))


def run_reference(x, origin, zpair, xpair):
    """-> (centred float32, gold float64, applied): the reference's stages one by one, then checked against its normalize_skeleton."""
    for body in x:                                                                # (a) both definitions of "null" / "missing" agree
        for frame in body:
            assert (frame.sum() == 0) == (not frame.any()), "a frame whose non-zero values cancel"
            for joint in frame:
                assert (joint.sum() == 0) == (not joint.any()), "a joint whose non-zero values cancel"
    centred = ref.move_skeleton_origin(ref.pad_null_frames(x.copy()), origin)
    assert centred.dtype == np.float32
    s = ref.move_skeleton_origin(ref.pad_null_frames(x.astype(np.float64)), origin)
    applied = []
    for pair, axis in ((zpair, (0, 0, 1)), (xpair, (1, 0, 0))):
        if pair is None:
            applied.append(0)
            continue
        before = s.copy()
        bone = s[0, 0, pair[1]] - s[0, 0, pair[0]]
        try:
            s = ref.parallelize_joints_to_axis(s, pair, axis)
            theta = angle(bone, axis)
            if not ANGLES[0] <= theta <= ANGLES[1]:                                                       # (b)
                raise AngleOutOfRange(f"applied angle {theta} outside {ANGLES}")
            applied.append(1)
        except ref.InvalidSkeletonException:
            assert np.array_equal(s, before)                                                             # (c)
            applied.append(0)
    gold = ref.normalize_skeleton(x.astype(np.float64), origin, zpair, xpair)
    assert np.array_equal(gold, s)
    return centred, gold, applied


def record(seed):
    out = {"seed": np.int64(seed)}
    for name, x, origin, zpair, xpair, expect in cases(np.random.default_rng(seed)):
        assert x.dtype == np.float32
        centred, gold, applied = run_reference(x, origin, zpair, xpair)
        assert tuple(applied) == tuple(expect), (name, applied, expect)
        out[f"{name}_x"] = x
        out[f"{name}_args"] = np.array([origin, *(zpair or (-1, -1)), *(xpair or (-1, -1))], dtype=np.int64)
        out[f"{name}_centred"], out[f"{name}_gold64"] = centred, gold
        out[f"{name}_applied"] = np.array(applied, dtype=np.int64)
        print(f"{name}: {x.shape} applied {applied}")
    return out


def main():
    for seed in range(20261019, 20261019 + 64):          # the first seed whose draws keep every applied angle inside ANGLES
        try:
            out = record(seed)
            break
        except AngleOutOfRange as e:
            print(f"seed {seed}: {e}; next seed")
    else:
        raise SystemExit("no seed found")
    path = os.path.join(REPO, "tests", "golden", "normalize.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
