"""Normalisation of raw skeleton clips as ClipBatches loads them, the part that needs no GPU: the restatement of
tests/normalize_ref.py against the golden vectors recorded from the reference (tests/golden/normalize.npz, written by
tools/gen_golden_normalize.py), the host-side argument checks of fgcn_clip_normalize (they precede any launch), the arguments of
``Normalize``, and the promise of the Python surface that holds without a device: no host fallback.

Bound of the rotated result: |out - gold64| <= 2^-23 max|gold64| per clip.  The one rounding to float32 costs at most 2^-24 relative to
the value, i.e. to the clip's largest magnitude; the float64 differences between two evaluations of the rotation (this restatement's
Rodrigues formula against the reference's quaternion route) are of order 1e-15 at angles inside [0.2, 2.9], where no threshold is
near; the bound leaves a factor of two over the rounding."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import normalize_ref as N
from conftest import ROOT
from fusion_gcn_amd import _lib, build
from test_data import write_split

GOLDEN = os.path.join(ROOT, "tests", "golden", "normalize.npz")


def golden_cases():
    """-> [(name, x, origin, z pair or None, x pair or None, centred float32, gold float64, applied)]"""
    g = np.load(GOLDEN)
    out = []
    for name in sorted({k[:-2] for k in g.files if k.endswith("_x")}):
        a = g[f"{name}_args"].tolist()
        pair = lambda lo: None if a[lo] < 0 else (a[lo], a[lo + 1])      # noqa: E731
        out.append((name, g[f"{name}_x"], a[0], pair(1), pair(3), g[f"{name}_centred"], g[f"{name}_gold64"], g[f"{name}_applied"].tolist()))
    return out


CASES = golden_cases()


def test_the_golden_file_holds_the_cases_of_the_design():
    shapes = [c[1].shape for c in CASES]
    assert len(CASES) == 15 and shapes.count((2, 13, 7, 3)) == 12
    assert {(1, 5, 4, 2), (1, 130, 3, 3), (1, 3, 64, 3)} <= set(shapes)
    assert all(c[1].dtype == np.float32 and c[5].dtype == np.float32 and c[6].dtype == np.float64 for c in CASES)
    assert sorted(tuple(c[7]) for c in CASES).count((0, 1)) == 3 and [c[7] for c in CASES if c[0].startswith("c06")] == [[0, 0]]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_restatement_against_the_reference(case):
    name, x, origin, zp, xp, centred, gold, applied = case
    r = N.normalize(x, origin, zp, xp)
    assert r["out"].dtype == np.float32 and r["frame_map"].dtype == np.int32 and r["frame_map"].shape == x.shape[:2]
    assert np.array_equal(r["centred"], centred)                             # stages 1 and 2: the reference's float32 values (-0 == +0)
    assert r["params"][9:11].tolist() == applied
    bound = N.U23 * np.abs(gold).max()
    err = np.abs(r["out"].astype(np.float64) - gold).max()
    print(f"[normalize] {name}: max error {err:.3e}, bound {bound:.3e} ({err / bound:.3f})")
    assert err <= bound, (err, bound)
    if applied == [0, 0]:
        assert np.array_equal(r["out"], centred)                             # no rotation: value for value
    maps, valid = N.frame_map(x)
    assert r["params"][11] == valid.sum() and np.all((maps >= 0) & (maps < x.shape[1]))
    for m in range(x.shape[0]):                                              # every output frame of a valid body holds what its source frame held
        nonnull = np.any(x[m] != 0, axis=(1, 2))
        assert valid[m] == nonnull.any()
        kept_null = valid[m] and nonnull[0] and not nonnull[:np.flatnonzero(nonnull)[-1] + 1].all()      # an interior null that stays
        if valid[m] and not kept_null:
            assert nonnull[maps[m]].all(), (name, m)                         # a skeleton in every frame


def test_frame_map_of_the_contract_by_hand():
    def clip(nonnull):
        x = np.zeros((1, len(nonnull), 2, 3), dtype=np.float32)
        x[0, np.flatnonzero(nonnull)] = 1.0
        return x
    m = lambda flags: N.frame_map(clip(np.array(flags, dtype=bool)))[0][0].tolist()      # noqa: E731
    assert m([1, 1, 1, 1, 1]) == [0, 1, 2, 3, 4]
    assert m([1, 1, 0, 0, 0]) == [0, 1, 0, 1, 0]                             # f = 2, replicated
    assert m([1, 0, 0, 0, 0]) == [0, 0, 0, 0, 0]                             # f = 1
    assert m([0, 1, 0, 1, 0]) == [1, 3, 1, 3, 1]                             # frame 0 null: compaction, then replication
    assert m([1, 0, 1, 0, 0]) == [0, 1, 2, 0, 1]                             # frame 0 valid: the interior null stays, and is replicated
    assert m([0, 0, 0, 0, 0]) == [0, 1, 2, 3, 4]                             # an invalid body: the identity
    neg = clip(np.array([1, 0, 1], dtype=bool))
    neg[0, 1] = -0.0
    assert N.frame_map(neg)[0][0].tolist() == [0, 1, 2]                      # -0 counts as zero: frame 1 is null and stays


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def test_host_side_validation(lib):
    """include/fgcn.h's list: each refusal is FGCN_E_BADARG with a message, before any launch (no device is touched: this runs without one)."""
    buf = (C.c_double * 64)()
    p = C.addressof(buf)

    def call(src=p, idx=p + 64, out=p + 128, frame_map=p + 192, params=p + 256, b=1, M=2, T=4, V=7, Cc=3, origin=2, z0=3, z1=2, x0=4, x1=6):
        return lib.fgcn_clip_normalize(src, idx, out, frame_map, params, b, M, T, V, Cc, origin, z0, z1, x0, x1, None)

    def refused(text, **kw):
        assert call(**kw) == -1, kw
        assert text in lib.fgcn_last_error(), (kw, lib.fgcn_last_error())

    for name in ("src", "idx", "out", "frame_map", "params"):
        refused(b"null pointer", **{name: None})
    for name in ("b", "M", "T", "V"):
        for bad in (0, -3):
            refused(b"bad b/M/T/V", **{name: bad})
    refused(b"at most 64", V=65)
    for bad in (0, 1, 4, -3):
        refused(b"expected 2 or 3", Cc=bad)
    assert _lib.NORMALIZE_MAX_T >= 1024
    refused(b"frames, at most", T=_lib.NORMALIZE_MAX_T + 1)
    for bad in (-1, 7, 64):
        refused(b"origin joint", origin=bad)
    for axis in ("z", "x"):
        for j0, j1 in ((3, 7), (7, 3), (3, -1), (3, 3), (64, 2)):
            refused(b"axis joints", **{axis + "0": j0, axis + "1": j1})
    refused(b"needs C == 3", Cc=2)
    refused(b"needs C == 3", Cc=2, z0=-1)                                     # the x pair alone
    refused(b"alias", out=p)
    refused(b"more than one grid holds", b=2 ** 31 - 1, M=64, T=4096, V=64, z0=-1, x0=-1)
    # what is refused above is a pair: without one, two coordinates pass the checks up to the aliasing test
    refused(b"alias", Cc=2, z0=-1, x0=-1, out=p)


def test_normalize_object_validates_its_arguments():
    from fusion_gcn_amd.data import Normalize
    z = Normalize(2, (3, 2), (4, 8))
    assert (z.origin_joint, z.z_axis_joints, z.x_axis_joints, z.only) == (2, (3, 2), (4, 8), None)
    assert z.applies_to("skeleton") and not Normalize(1, only=["skeleton"]).applies_to("inertial")
    assert Normalize(1).z_axis_joints is None and Normalize(1).x_axis_joints is None
    for args in ((-1,), (1.5,), ("1",), (1, (3,)), (1, (3, 3)), (1, (3, -2)), (1, None, (4, 4)), (1, (0, 1, 2)), (1, (0.0, 1.0))):
        with pytest.raises(ValueError):
            Normalize(*args)
    for name, want in (("utd_mhad", (2, (3, 2), (4, 8))), ("UTD-MHAD", (2, (3, 2), (4, 8))), ("mmact", (1, None, None)),
                       ("ntu_rgb_d", (1, (0, 1), (4, 8)))):
        z = Normalize.for_dataset(name)
        assert (z.origin_joint, z.z_axis_joints, z.x_axis_joints) == want, name
    assert Normalize.for_dataset("ntu_rgb_d", only=["skeleton"]).only == frozenset(["skeleton"])


def test_no_host_fallback(tmp_path):
    from fusion_gcn_amd import ops
    from fusion_gcn_amd.data import ClipBatches, MultiModalDataset, Normalize, NumpyDatasetLoader
    write_split(str(tmp_path), "train", 9, {"skeleton": (2, 5, 25, 3)})
    ds = MultiModalDataset([(str(tmp_path), NumpyDatasetLoader())], "train")
    for resident in (True, False):
        with pytest.raises(_lib.FgcnError):
            ClipBatches(ds, 4, device="cpu", resident=resident, normalize=Normalize.for_dataset("ntu_rgb_d"))
    with pytest.raises(_lib.FgcnError):
        ops.clip_normalize(torch.zeros(3, 2, 5, 25, 3), torch.arange(2), origin_joint=1)
    it = ClipBatches(ds, 4, device="cpu", normalize=None)                    # the default: what it always was
    assert it.normalize is None and it.last_plan == {} and it.norm_keys == []
