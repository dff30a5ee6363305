"""Preparation of raw inertial recordings as ClipBatches loads them, the part that needs no GPU: the restatement
of tests/inertial_ref.py and the host entry point fgcn_resample_index against the golden vectors recorded from the reference
(tests/golden/inertial.npz, written by tools/gen_golden_inertial.py), the host-side argument checks of fgcn_signal_prepare and
fgcn_imu_enhance (they precede any launch), the arguments of ``Inertial``, and the promise of the Python surface that holds without a
device: no host fallback.  Every comparison is exact: the steps are integer arithmetic, correctly rounded float32 arithmetic or copies."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import inertial_ref as R
from conftest import ROOT
from fusion_gcn_amd import _lib, build
from test_data import write_split

GOLDEN = os.path.join(ROOT, "tests", "golden", "inertial.npz")
LI, LS = (2, 4, 6, 180, 326), range(2, 129)


def golden():
    g = np.load(GOLDEN)
    tables = {}
    for li in LI:
        flat, at = g[f"idx_{li}"], 0
        for ls in LS:
            tables[li, ls] = flat[at:at + ls].astype(np.int64)
            at += ls
        assert at == len(flat)
    cases = []
    for name in sorted({k[:-5] for k in g.files if k.endswith("_skel")}):
        Ls, Li, T = g[f"{name}_dims"].tolist()
        a = g[f"{name}_args"].tolist()
        pair = lambda lo: None if a[lo] < 0 else (a[lo], a[lo + 1])      # noqa: E731
        cases.append(dict(name=name, skel=g[f"{name}_skel"], imu=g[f"{name}_imu"], Ls=Ls, Li=Li, T=T, origin=a[0], z=pair(1), x=pair(3),
                          padded=g[f"{name}_padded"], signal=g[f"{name}_signal"], enhanced=g[f"{name}_enhanced"]))
    return tables, cases


TABLES, CASES = golden()
IDS = [c["name"] for c in CASES]


def normalised(case):
    """the reference's normalised skeleton of a case: joints [0, V) of its enhanced array, with the case's own coordinates"""
    M, T, V, Cc = case["skel"].shape
    return np.ascontiguousarray(case["enhanced"][:, :, :V, :Cc])


def test_the_golden_file_holds_the_cases_of_the_issue():
    assert os.path.getsize(GOLDEN) < 200_000
    assert len(TABLES) == 5 * 127 and all(len(t) == ls for (_, ls), t in TABLES.items())
    by = {c["name"][4:]: c for c in CASES}
    assert by["full"]["Ls"] == by["full"]["T"]
    c = by["padded_positive"]
    assert c["Ls"] < c["T"] and c["imu"].min() > 0 and c["padded"].min() == 0
    assert by["equal_lengths"]["Li"] == by["equal_lengths"]["Ls"] and by["upsampling"]["Li"] < by["upsampling"]["Ls"]
    assert by["two_frames"]["Ls"] == 2
    c = by["326_to_79"]
    assert (c["Li"], c["Ls"], c["T"]) == (326, 79, 128)
    assert by["two_coordinates"]["skel"].shape[3] == 2 and by["two_bodies"]["skel"].shape[0] == 2
    for c in CASES:
        M, T, V, Cc = c["skel"].shape
        S = c["imu"].shape[1]
        assert c["imu"].shape[0] == c["Li"] and T == c["T"] and not c["skel"][:, c["Ls"]:].any()
        assert c["padded"].shape == c["signal"].shape == (T, S) and c["enhanced"].shape == (M, T, V + S // 3, 3)
        assert all(c[k].dtype == np.float32 for k in ("skel", "imu", "padded", "signal", "enhanced"))
    # the formulas the contract rules out do differ on recorded tables
    t79 = np.arange(79)
    assert not np.array_equal(TABLES[326, 79], np.rint(t79 * 325 / 78).astype(np.int64))                 # multiply first
    assert TABLES[2, 3].tolist() == [0, 0, 1] and TABLES[6, 3].tolist() == [0, 2, 5]                     # half-up gives [0, 1, 1], [0, 3, 5]
    assert not np.array_equal(TABLES[4, 95], np.rint(np.arange(95, dtype=np.float32) * (np.float32(3) / np.float32(94))).astype(np.int64))


def test_restated_indices_equal_every_golden_table():
    for (li, ls), want in TABLES.items():
        assert np.array_equal(R.resample_indices(li, ls), want), (li, ls)
    assert R.resample_indices(9, 9).tolist() == list(range(9)) and R.resample_indices(1, 1).tolist() == [0]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_restatement_against_the_reference(case):
    Li, Ls, T = case["Li"], case["Ls"], case["T"]
    assert np.array_equal(R.padded(case["imu"], Li, Ls, T), case["padded"])
    out, stats = R.signal(case["imu"], Li, Ls, T)
    assert out.dtype == np.float32 and np.array_equal(out, case["signal"])
    assert stats[0] == case["padded"].min() and out.min() == 0.0 and out.max() == 1.0
    raw, stats = R.signal(case["imu"], Li, Ls, T, minmax=False)
    assert np.array_equal(raw, case["padded"]) and stats.tolist() == [0.0, 1.0]
    enh = R.enhanced(normalised(case), case["imu"], Li, Ls)
    assert enh.dtype == np.float32 and np.array_equal(enh, case["enhanced"])
    V = case["skel"].shape[2]
    assert not enh[:, Ls:, V:].any()                                         # the appended joints stay zero behind the recording ...
    if Ls < T:
        assert enh[:, Ls:, :V].any()                                         # ... where the normalisation repeated the skeleton
    # a row longer than the recording: the frames behind Li are never read
    longer = np.concatenate([case["imu"], np.full((3, case["imu"].shape[1]), np.nan, dtype=np.float32)])
    assert np.array_equal(R.padded(longer, Li, Ls, T), case["padded"])


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def test_host_entry_point_equals_every_golden_table(lib):
    out = C.c_int()

    def r(t, li, ls):
        assert lib.fgcn_resample_index(t, li, ls, C.byref(out)) == 0
        return out.value
    for (li, ls), want in TABLES.items():
        assert [r(t, li, ls) for t in range(ls)] == want.tolist(), (li, ls)
    assert [r(t, 7, 7) for t in range(7)] == list(range(7))                  # equal lengths: the frame itself
    assert r(0, 5, 1) == 0 and r(3, 5, 1) == 0 and r(0, 1, 1) == 0           # a single output frame
    assert r(-4, 29, 13) == 0 and r(500, 29, 13) == 28 and r(12, 7, 7) == 6 and r(2 ** 31 - 1, 326, 2) == 325      # clamped
    from fusion_gcn_amd import ops
    assert [ops.resample_index(t, 326, 79) for t in range(79)] == TABLES[326, 79].tolist()
    for bad in ((0, 0, 5, C.byref(out)), (0, 5, 0, C.byref(out)), (0, -1, 5, C.byref(out)), (0, 5, 5, None)):
        assert lib.fgcn_resample_index(*bad) == -1


def test_host_side_validation(lib):
    """include/fgcn.h's list: each refusal is FGCN_E_BADARG with a message, before any launch (null streams, no device is touched)."""
    buf = (C.c_double * 64)()
    p = C.addressof(buf)
    ptrs = dict(src=p, idx=p + 64, src_len=p + 128, dst_len=p + 192, out=p + 256, stats=p + 320)

    def signal(b=1, L=29, S=6, T=13, minmax=1, **kw):
        a = {**ptrs, **kw}
        return lib.fgcn_signal_prepare(a["src"], a["idx"], a["src_len"], a["dst_len"], a["out"], a["stats"], b, L, S, T, minmax, None)

    eptrs = dict(skel=p, skel_idx=p + 64, imu=p + 128, imu_idx=p + 192, src_len=p + 256, dst_len=p + 320, out=p + 384)

    def enhance(b=1, M=2, T=13, V=7, Cc=3, L=29, S=6, **kw):
        a = {**eptrs, **kw}
        return lib.fgcn_imu_enhance(a["skel"], a["skel_idx"], a["imu"], a["imu_idx"], a["src_len"], a["dst_len"], a["out"], b, M, T, V, Cc, L,
                                    S, None)

    def refused(call, text, **kw):
        assert call(**kw) == -1, kw
        assert text in lib.fgcn_last_error(), (kw, lib.fgcn_last_error())

    for name in ptrs:
        refused(signal, b"null pointer", **{name: None})
    for name in eptrs:
        refused(enhance, b"null pointer", **{name: None})
    for bad in (0, -3):
        for name in ("b", "L", "S", "T"):
            refused(signal, b"bad b/L/S/T", **{name: bad})
        for name in ("b", "M", "T", "V", "L", "S"):
            refused(enhance, b"bad b/M/T/V/L/S", **{name: bad})
    for bad in (0, 1, 4, -3):
        refused(enhance, b"expected 2 or 3", Cc=bad)
    for bad in (1, 2, 4, 7):
        refused(enhance, b"joints of three", S=bad)
    refused(signal, b"alias", out=p)
    refused(enhance, b"alias", out=p)
    refused(enhance, b"alias", out=p + 128)
    refused(signal, b"2^31 or more", b=2 ** 20, T=2 ** 10, S=6)
    refused(signal, b"2^31 or more", b=2 ** 31 - 1, T=2 ** 31 - 1, S=2 ** 31 - 1, L=2 ** 31 - 1)
    refused(signal, b"2^31 or more", L=2 ** 30, S=6)
    refused(enhance, b"2^31 or more", b=2 ** 20, T=2 ** 10)
    refused(enhance, b"2^31 or more", b=2 ** 31 - 1, M=2 ** 31 - 1, T=2 ** 31 - 1, V=2 ** 31 - 1, L=2 ** 31 - 1, S=3 * (2 ** 29))
    refused(enhance, b"2^31 or more", L=2 ** 30, S=6)
    # two coordinates and a signal that does not divide by three pass the checks of fgcn_signal_prepare / reach the aliasing test
    refused(enhance, b"alias", Cc=2, out=p)
    refused(signal, b"alias", S=7, out=p)


def test_header_and_signature_table_agree():
    """every argument of the three new prototypes of include/fgcn.h against the ctypes table: pointers to device memory travel as
    integers (c_void_p), the host result of fgcn_resample_index as a pointer to int"""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fgcn.h")).read(), flags=re.S)
    kinds = {"int": C.c_int, "void*": C.c_void_p, "float*": C.c_void_p, "const float*": C.c_void_p, "const long long*": C.c_void_p,
             "const int*": C.c_void_p}
    for name in ("fgcn_resample_index", "fgcn_signal_prepare", "fgcn_imu_enhance"):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, name
        args = []
        for a in m.group(1).split(","):
            kind = re.sub(r"\s+", " ", re.sub(r"\w+\s*$", "", a.strip())).strip().replace(" *", "*")
            args.append(C.POINTER(C.c_int) if (name, kind) == ("fgcn_resample_index", "int*") else kinds[kind])
        res, want = _lib.SIGNATURES[name]
        assert res is C.c_int and want == args, (name, want, args)


def _frames(n=9, T=5, L=11, seed=0):
    rng = np.random.default_rng(seed)
    ls = rng.integers(2, T + 1, n)
    return {"skeleton": ls, "inertial": rng.integers(2, L + 1, n)}


def test_inertial_object_validates_its_arguments():
    from fusion_gcn_amd.data import Inertial
    f = _frames()
    z = Inertial(frames=f)
    assert (z.main, z.signal, z.enhance, z.minmax, z.drop_signal) == ("skeleton", "inertial", False, True, False)
    assert z.frames["skeleton"].dtype == np.int32 and z.frames["inertial"].tolist() == f["inertial"].tolist()
    shapes = {"skeleton": (9, 2, 5, 25, 3), "inertial": (9, 11, 6)}
    z.check_shapes(shapes, 9)
    assert z.sample_shapes(shapes) == {"skeleton": (2, 5, 25, 3), "inertial": (5, 6)}
    e = Inertial(frames=f, enhance=True, drop_signal=True)
    e.check_shapes(shapes, 9)
    assert e.sample_shapes(shapes) == {"skeleton": (2, 5, 27, 3)}
    assert Inertial(frames=f, enhance=True).sample_shapes({"skeleton": (9, 1, 5, 25, 2), "inertial": (9, 11, 3)}) == \
        {"skeleton": (1, 5, 26, 3), "inertial": (5, 3)}
    named = Inertial(frames={"pose": f["skeleton"], "imu": f["inertial"]}, main="pose", signal="imu")
    named.check_shapes({"pose": shapes["skeleton"], "imu": shapes["inertial"], "depth": (9, 4)}, 9)
    for kw in (dict(frames={"skeleton": f["skeleton"]}), dict(frames={**f, "depth": f["skeleton"]}),       # feature ids
               dict(frames=f, main="pose"), dict(frames=f, signal="skeleton"), dict(frames=f, drop_signal=True),
               dict(frames={**f, "inertial": f["inertial"][:-1]}), dict(frames={**f, "skeleton": f["skeleton"] * 1.0}),
               dict(frames={**f, "skeleton": f["skeleton"] * 0}), dict(frames={**f, "inertial": f["inertial"] - 20}),
               dict(frames={**f, "skeleton": np.ones(9, dtype=int)})):                                     # Ls == 1 != Li
        with pytest.raises(ValueError):
            Inertial(**kw)
    Inertial(frames={"skeleton": np.ones(9, dtype=int), "inertial": np.ones(9, dtype=int)})                # Ls == 1 == Li is taken
    with pytest.raises(ValueError, match="does not have"):
        z.check_shapes({"skeleton": shapes["skeleton"]}, 9)
    with pytest.raises(ValueError, match=r"in \[1, 4\]"):
        z.check_shapes({"skeleton": (9, 2, 4, 25, 3), "inertial": (9, 11, 6)}, 9)                          # a count above T
    with pytest.raises(ValueError, match=r"in \[1, 10\]"):
        Inertial(frames={**f, "inertial": np.full(9, 11)}).check_shapes({"skeleton": shapes["skeleton"], "inertial": (9, 10, 6)}, 9)
    with pytest.raises(ValueError, match="expected 8 frame counts"):
        z.check_shapes(shapes, 8)
    with pytest.raises(_lib.FgcnError, match="expected"):
        z.check_shapes({"skeleton": (9, 5, 25, 3), "inertial": (9, 11, 6)}, 9)
    with pytest.raises(_lib.FgcnError, match="expected"):
        z.check_shapes({"skeleton": shapes["skeleton"], "inertial": (9, 1, 11, 6)}, 9)
    with pytest.raises(_lib.FgcnError, match="joints of three"):
        Inertial(frames=f, enhance=True).check_shapes({"skeleton": shapes["skeleton"], "inertial": (9, 11, 4)}, 9)
    z.check_shapes({"skeleton": shapes["skeleton"], "inertial": (9, 11, 4)}, 9)                            # without enhance, any S


def test_no_host_fallback(tmp_path):
    from fusion_gcn_amd import ops
    from fusion_gcn_amd.data import ClipBatches, Inertial, MultiModalDataset, NumpyDatasetLoader
    write_split(str(tmp_path), "train", 9, {"skeleton": (2, 5, 25, 3), "inertial": (11, 6)})
    ds = MultiModalDataset([(str(tmp_path), NumpyDatasetLoader())], "train")
    for resident in (True, False):
        with pytest.raises(_lib.FgcnError, match="no host fallback"):
            ClipBatches(ds, 4, device="cpu", resident=resident, inertial=Inertial(frames=_frames()))
    lens = torch.ones(3, dtype=torch.int32)
    with pytest.raises(_lib.FgcnError):
        ops.signal_prepare(torch.zeros(3, 11, 6), torch.arange(2), lens, lens, 5)
    with pytest.raises(_lib.FgcnError):
        ops.imu_enhance(torch.zeros(3, 2, 5, 25, 3), torch.arange(2), torch.zeros(3, 11, 6), torch.arange(2), lens, lens)
    it = ClipBatches(ds, 4, device="cpu", inertial=None)                     # the default: what it always was
    assert it.inertial is None and it.last_inertial is None and it.out_keys == it.keys == ["inertial", "skeleton"]
    feats, _, idx = next(iter(it))
    assert feats["inertial"].shape == (4, 11, 6) and feats["skeleton"].shape == (4, 2, 5, 25, 3)
