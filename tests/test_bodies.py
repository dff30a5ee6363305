"""Selection of a clip's most energetic bodies as ClipBatches loads it, the part that needs no GPU: the restatement
of tests/bodies_ref.py against the golden vectors recorded from the reference (tests/golden/bodies.npz, written by
tools/gen_golden_bodies.py), the ranking rule of the contract by hand, the host-side argument checks of fgcn_clip_bodies (they precede any
launch), the arguments of ``Bodies``, and the promise of the Python surface that holds without a device: no host fallback.

Bound of the scores: 1e-5 relative between the restatement (float64 throughout) and the reference's values, which numpy's std() forms in
float32 from the float32 array.  The generator asserts the same bound while writing and measured 1.1e-7 at worst."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import bodies_ref as B
from conftest import ROOT
from fusion_gcn_amd import _lib, build
from test_data import write_split

GOLDEN = os.path.join(ROOT, "tests", "golden", "bodies.npz")


def golden_cases():
    """-> [(name, x, the reference's scores, the reference's order, the selected array, tied)]"""
    g = np.load(GOLDEN)
    return [(name, g[f"{name}_x"], g[f"{name}_scores"], g[f"{name}_order"], g[f"{name}_sel"], bool(g[f"{name}_tied"]))
            for name in sorted({k[:-2] for k in g.files if k.endswith("_x")})]


CASES = golden_cases()


def test_the_golden_file_holds_the_cases_of_the_design():
    shapes = [c[1].shape for c in CASES]
    assert len(CASES) == 13 and set(shapes) == {(4, 13, 7, 3), (3, 5, 4, 2), (16, 9, 5, 3)}
    assert all(c[1].dtype == np.float32 and c[2].dtype.kind == "f" and c[4].dtype == np.float32 for c in CASES)
    kept = {(c[1].shape[0], c[4].shape[0]) for c in CASES}
    assert {(4, 1), (4, 2), (4, 4), (3, 1), (3, 3), (16, 2), (16, 16)} <= kept            # M = 1, 2 and Mr
    assert sum(c[5] for c in CASES) == 2
    null = lambda x: [int(B.non_null(b).sum()) for b in x]      # noqa: E731
    assert any(0 in null(c[1]) for c in CASES) and any(1 in null(c[1]) for c in CASES)      # an all-null body; exactly one frame
    assert any(not B.non_null(b)[0] and B.non_null(b).any() for c in CASES for b in c[1])   # first frames null
    assert [null(c[1]).count(0) for c in CASES if c[0].startswith("c09")] == [3]            # one actor, three empty slots
    assert os.path.getsize(GOLDEN) < 200 << 10


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_restatement_against_the_reference(case):
    name, x, scores, order, sel, tied = case
    s = B.scores(x)
    assert s.dtype == np.float64 and s.shape == (len(x),)
    err = np.abs(s - scores)
    print(f"[bodies] {name}: max relative difference {np.max(err / np.where(s > 0, s, 1)):.3e}")
    assert np.all(err <= 1e-5 * s), (s, scores)
    if not tied:
        assert np.array_equal(B.order(s), order)
    assert np.array_equal(B.select(x, len(sel)), sel)
    assert sorted(B.order(s).tolist()) == list(range(len(x)))


def test_one_actor_and_empty_slots_order():
    name, x, scores, order, sel, tied = next(c for c in CASES if c[0].startswith("c09"))
    assert B.order(B.scores(x)).tolist() == [2, 3, 1, 0] == order.tolist()               # [m, Mr - 1, ...]: the actor, then the higher index first


def test_ranking_rule_of_the_contract_by_hand():
    nan = float("nan")
    o = lambda s: B.order(np.array(s, dtype=np.float64)).tolist()      # noqa: E731
    assert o([.5, 0, 0, 0]) == [0, 3, 2, 1]
    assert o([.1, nan, .2, nan]) == [3, 1, 2, 0]                     # a NaN above every number, several NaNs by the higher index
    assert o([1., 2., 3.]) == [2, 1, 0]
    assert o([2., 2., 1., 2.]) == [3, 1, 0, 2]
    assert o([0., -0., 0.]) == [2, 1, 0]                             # -0 == +0
    assert o([float("inf"), nan, 1.]) == [1, 0, 2]
    assert o([7.]) == [0]
    for s in ([.5, 0, 0, 0], [.1, nan, .2, nan]):                    # what numpy's stable small-array sort, reversed, returns
        assert o(s) == np.array(s).argsort()[::-1].tolist()


def test_scores_of_the_contract_by_hand():
    x = np.zeros((3, 4, 2, 3), dtype=np.float32)
    x[0, 1] = [[1, 2, 3], [3, 2, 5]]                                # one frame: std over the two joints = (1, 0, 1)
    x[1, :, :, 0] = [[0, 2], [4, 6], [0, 0], [0, 0]]                # frames 2, 3 null: channel 0 = {0, 2, 4, 6}, std sqrt(5)
    assert np.allclose(B.scores(x), [2.0, np.sqrt(5.0), 0.0], rtol=1e-15)
    assert not np.signbit(B.scores(x)[2])
    x[2, 0, 0, 0], x[1, 3, 1, 2] = np.nan, np.inf                   # a NaN is a value; a body with a NaN or an inf scores NaN
    assert np.isnan(B.scores(x)[1:]).all() and B.order(B.scores(x)).tolist() == [2, 1, 0]
    x = np.full((1, 3, 2, 3), -0.0, dtype=np.float32)               # -0 frames are null
    x[0, 1, 0] = [1, 2, 3]
    assert B.non_null(x[0]).tolist() == [False, True, False] and B.frames_counted(x).tolist() == [2]


def test_a_frame_whose_values_cancel_is_valid():
    """the documented divergence from the reference's sum() != 0: such a frame counts (restatement only)"""
    x = np.zeros((1, 3, 2, 3), dtype=np.float32)
    x[0, 0] = [[1, 2, 3], [4, 5, 6]]
    x[0, 1] = [[1.5, -1.5, 0], [2, 0, -2]]                          # sums to zero, holds values
    assert x[0, 1].sum() == 0 and B.non_null(x[0]).tolist() == [True, True, False]
    with_it, without = B.scores(x)[0], B.scores(x[:, :1])[0]
    assert B.frames_counted(x).tolist() == [4] and with_it != without
    cols = x[0, :2].astype(np.float64).reshape(4, 3)
    assert np.isclose(with_it, cols.std(axis=0).sum(), rtol=1e-15)


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def test_host_side_validation(lib):
    """include/fgcn.h's list: each refusal is FGCN_E_BADARG with its own message, before any launch (no device is touched)."""
    buf = (C.c_double * 64)()
    p = C.addressof(buf)

    def call(src=p, idx=p + 64, out=p + 128, order=p + 192, scores=p + 256, b=1, Mr=4, M=2, T=4, V=7, Cc=3):
        return lib.fgcn_clip_bodies(src, idx, out, order, scores, b, Mr, M, T, V, Cc, None)

    def refused(text, **kw):
        assert call(**kw) == -1, kw
        assert text in lib.fgcn_last_error(), (kw, lib.fgcn_last_error())

    for name in ("src", "idx", "out", "order", "scores"):
        refused(b"null pointer", **{name: None})
    for name in ("b", "Mr", "M", "T", "V"):
        for bad in (0, -3):
            refused(b"bad b/Mr/M/T/V", **{name: bad})
    refused(b"bodies kept of", M=5)
    assert _lib.BODIES_MAX == 16
    refused(b"bodies, at most 16", Mr=17)
    refused(b"bodies, at most 16", Mr=17, M=17)
    for bad in (0, 1, 4, -3):
        refused(b"expected 2 or 3", Cc=bad)
    refused(b"more than a lane indexes", T=2 ** 20, V=2 ** 8, Cc=2)          # T * V * C = 2^29
    refused(b"more than a lane indexes", T=2 ** 30, V=2 ** 30)
    refused(b"their flags stay in LDS", T=_lib.BODIES_MAX_T + 1, V=1, Cc=2)
    refused(b"more than one grid holds", b=2 ** 27, Mr=16, M=1)               # b * Mr = 2^31
    refused(b"alias", out=p)
    refused(b"alias", out=p, Mr=16, M=16, Cc=2)


def test_the_abi_table_has_the_symbol():
    assert _lib.SIGNATURES["fgcn_clip_bodies"] == (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 6 + [C.c_void_p])
    header = open(os.path.join(ROOT, "include", "fgcn.h")).read()
    assert f"#define FGCN_BODIES_MAX {_lib.BODIES_MAX}\n" in header and f"#define FGCN_BODIES_MAX_T {_lib.BODIES_MAX_T}\n" in header


def test_bodies_object_validates_its_arguments():
    from fusion_gcn_amd.data import Bodies
    z = Bodies()
    assert (z.bodies, z.only, z.name, z.at_upload) == (2, None, "bodies", True)
    assert z.applies_to("skeleton") and not Bodies(1, only=["skeleton"]).applies_to("inertial")
    for bad in (0, -1, 17, 1.5, "2", True, None):
        with pytest.raises(ValueError):
            Bodies(bad)
    assert Bodies(np.int64(3)).bodies == 3 and Bodies(16).bodies == 16
    shapes, writes = Bodies(2, only=["skeleton"]).bind({"skeleton": (4, 300, 25, 3), "inertial": (50, 6)}, 9, ["skeleton", "inertial"])
    assert shapes == {"skeleton": (2, 300, 25, 3), "inertial": (50, 6)} and writes == ["skeleton"]
    assert Bodies(4).bind({"s": (4, 5, 3, 2)}, 1, ["s"]) == ({"s": (4, 5, 3, 2)}, ["s"])       # M == Mr: a pure reordering
    for shape, text in (((50, 6), "expected (samples, Mr, T, V, C)"), ((1, 5, 3, 3), "holds 1 bodies"), ((17, 5, 3, 3), "at most 16"),
                        ((4, 5, 3, 4), "expected 2 or 3"), ((4, 5, 3, 1), "expected 2 or 3")):
        with pytest.raises(_lib.FgcnError, match=text.replace("(", r"\(").replace(")", r"\)")):
            Bodies(2).bind({"s": shape}, 9, ["s"])
    with pytest.raises(ValueError, match="does not have"):
        Bodies(2, only=["nope"]).bind({"s": (4, 5, 3, 3)}, 9, ["s"])


def test_bodies_for_dataset():
    from fusion_gcn_amd.data import Bodies
    z = Bodies.for_dataset("ntu_rgb_d")
    assert z.bodies == 2 and z.only is None
    assert Bodies.for_dataset("NTU-RGB-D", only=["skeleton"]).only == frozenset(["skeleton"])
    for name in ("utd_mhad", "mmact"):
        with pytest.raises(ValueError, match="max_body_true"):
            Bodies.for_dataset(name)


def test_no_host_fallback(tmp_path):
    from fusion_gcn_amd import ops
    from fusion_gcn_amd.data import Bodies, ClipBatches, MultiModalDataset, NumpyDatasetLoader, valid_frames
    write_split(str(tmp_path), "train", 9, {"skeleton": (4, 5, 25, 3)})
    ds = MultiModalDataset([(str(tmp_path), NumpyDatasetLoader())], "train")
    for resident in (True, False):
        with pytest.raises(_lib.FgcnError, match="no host fallback"):
            ClipBatches(ds, 4, device="cpu", resident=resident, bodies=Bodies())
    with pytest.raises(_lib.FgcnError):
        ops.clip_bodies(torch.zeros(3, 4, 5, 25, 3), torch.arange(2), bodies=2)
    with pytest.raises(_lib.FgcnError, match="no host fallback"):
        valid_frames(ds, "skeleton", device="cpu", bodies=Bodies())
    it = ClipBatches(ds, 4, device="cpu", bodies=None)                        # the default: what it always was
    assert it.stages == [] and it.bodies is None and it.last_bodies == {} and it.shapes == {"skeleton": (4, 5, 25, 3)}
    assert ClipBatches(ds, 4, device="cpu").stages == []
