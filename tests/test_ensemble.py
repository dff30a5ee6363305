"""Score fusion of stream models, the part that needs no device: the two entry points refuse malformed calls on
the host before any launch (validation precedes HIP, as in test_abi.py), the host layer refuses what it documents, the score files make the
round trip from ``StreamScores.save`` to ``ScoreStore.load``, and the numpy restatement the device tests compare against (ensemble_ref.py)
resolves ties and NaN as include/fgcn.h says."""
import ctypes as C

import numpy as np
import pytest
import torch

import ensemble_ref as R
from fusion_gcn_amd import _lib, build


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def _fuse_in(ptr, S=2, ld=4):
    arg = _lib.FuseIn()
    for s in range(S):
        arg.scores[s], arg.ld[s], arg.weight[s] = ptr + 64 * s, ld, 1.0
    return arg


def test_both_entry_points_refuse_malformed_calls_before_any_launch(lib):
    buf = (C.c_double * 64)()
    p = C.addressof(buf)
    out, cand, labels, counts = p + 256, p + 320, p + 384, p + 448
    assert p % 8 == 0
    ok = _fuse_in(p)

    def fuse(arg=ok, S=2, transform=0, out=out, ld_out=4, rows=3, classes=4):
        return lib.fgcn_score_fuse(None if arg is None else C.byref(arg), S, transform, out, ld_out, rows, classes, None)

    def sweep(arg=ok, S=2, transform=0, cand=cand, G=3, labels=labels, rows=3, classes=4, k=2, counts=counts):
        return lib.fgcn_fuse_sweep(None if arg is None else C.byref(arg), S, transform, cand, G, labels, rows, classes, k, counts, None)

    def refused(rc, code, text):
        assert rc == code and text in lib.fgcn_last_error(), (rc, lib.fgcn_last_error())

    for call, name in ((fuse, b"score_fuse"), (sweep, b"fuse_sweep")):
        refused(call(arg=None), -1, name + b": null pointer (in)")
        hole = _fuse_in(p)
        hole.scores[1] = None
        refused(call(arg=hole), -1, name + b": null pointer (scores[1])")
        # entries [S, 8) are not read: with S = 1 the same struct passes the scores loop and meets a LATER refusal (no call here may pass validation)
        later = dict(out=None) if call is fuse else dict(k=0)
        refused(call(arg=hole, S=1, **later), -1, name + (b": null pointer (out)" if call is fuse else b": bad k"))
        for S in (0, 9, -1):
            refused(call(S=S), -1, name + b": bad stream count")
        for transform in (2, -1):
            refused(call(transform=transform), -1, name + b": unknown transform")
        for rows in (0, -5):
            refused(call(rows=rows), -1, name + b": bad row count")
        for classes in (0, _lib.CLS_MAX_CLASSES + 1):
            refused(call(classes=classes), -1, name + b": bad class count")
        refused(call(arg=_fuse_in(p, ld=3)), -1, name + b": bad row stride ld[0]=3 < classes=4")
    refused(fuse(out=None), -1, b"score_fuse: null pointer (out)")
    refused(fuse(ld_out=3), -1, b"score_fuse: bad row stride ld_out")
    refused(fuse(out=p + 64), -1, b"score_fuse: out must not alias an input (scores[1])")
    for missing in ("cand", "labels", "counts"):
        refused(sweep(**{missing: None}), -1, b"fuse_sweep: null pointer")
    for k in (0, 5):
        refused(sweep(k=k), -1, b"fuse_sweep: bad k")
    for G in (0, -1, _lib.FUSE_MAX_CANDIDATES + 1):
        refused(sweep(G=G), -1, b"fuse_sweep: bad candidate count")
    refused(sweep(counts=counts + 4), -2, b"fuse_sweep: counts must be 8-byte aligned")
    assert _lib.FUSE_PASS < _lib.FUSE_MAX_CANDIDATES and _lib.FUSE_MAX_STREAMS == 8


def test_header_constants_match_the_binding():
    import os
    import re
    from conftest import ROOT
    text = open(os.path.join(ROOT, "include", "fgcn.h")).read()
    define = lambda name: re.search(rf"#define {name} (\d+)\s", text).group(1)      # noqa: E731
    assert int(define("FGCN_FUSE_MAX_STREAMS")) == _lib.FUSE_MAX_STREAMS and int(define("FGCN_FUSE_PASS")) == _lib.FUSE_PASS
    assert int(define("FGCN_FUSE_MAX_CANDIDATES")) == _lib.FUSE_MAX_CANDIDATES
    assert "FGCN_FUSE_NONE = 0, FGCN_FUSE_SOFTMAX = 1" in text and _lib.FUSE_TRANSFORMS == {"none": 0, "softmax": 1}
    assert C.sizeof(_lib.FuseIn) == 8 * 8 + 4 * 8 + 4 * 8


def test_cpu_tensors_raise_fgcn_error():
    """the tensor checks come before the device check, so the refusal of a host tensor is the same with and without a device"""
    from fusion_gcn_amd import metrics, ops
    z, y = torch.zeros(3, 4), torch.zeros(3, dtype=torch.int64)
    with pytest.raises(_lib.FgcnError, match=r"score_fuse: scores\[0\] must be a float32 \(rows, classes\) tensor on the device.*no host path"):
        ops.score_fuse([z, z.clone()], [1.0, 1.0])
    with pytest.raises(_lib.FgcnError, match=r"fuse_sweep: scores\[0\] must be .* on the device.*no host path"):
        ops.fuse_sweep([z, z.clone()], [[1.0, 1.0]], y, 1)
    with pytest.raises(_lib.FgcnError, match="expected 1..8 score tensors"):
        ops.score_fuse([], [])
    with pytest.raises(_lib.FgcnError, match="transform='log_softmax'"):
        ops.score_fuse([z], [1.0], transform="log_softmax")
    with pytest.raises(_lib.FgcnError, match="no host path"):
        metrics.StreamScores("validation_scores", 3, 4).update((z, y), indices=torch.arange(3))


def test_simplex_grid_counts_and_order():
    from math import comb

    from fusion_gcn_amd.ensemble import simplex_grid
    assert simplex_grid(2, 4).tolist() == [[0, 1], [.25, .75], [.5, .5], [.75, .25], [1, 0]]
    assert simplex_grid(1, 7).tolist() == [[1.0]]
    assert simplex_grid(3, 2).tolist() == [[0, 0, 1], [0, .5, .5], [0, 1, 0], [.5, 0, .5], [.5, .5, 0], [1, 0, 0]]
    for S, steps in ((4, 20), (3, 5), (8, 3)):
        grid = simplex_grid(S, steps)
        ints = np.rint(grid * steps).astype(int)
        assert grid.shape == (comb(steps + S - 1, S - 1), S) and grid.dtype == np.float64
        assert (ints >= 0).all() and (ints.sum(axis=1) == steps).all() and np.array_equal(ints / steps, grid)
        assert [tuple(r) for r in ints] == sorted(set(tuple(r) for r in ints))            # lexicographic, no repeats
    assert simplex_grid(4, 20).shape[0] == 1771
    for bad in ((0, 4), (9, 4), (2, 0)):
        with pytest.raises(ValueError):
            simplex_grid(*bad)


def test_stream_ensemble_refuses_what_it_documents():
    from fusion_gcn_amd.ensemble import StreamEnsemble
    a, b = torch.nn.Linear(4, 3), torch.nn.Linear(4, 3)
    members = {"joint": (a, "skeleton"), "bone": (b, {"x": "skeleton_bone"})}
    ens = StreamEnsemble(members)
    assert ens.weights == [1.0, 1.0] and ens.names == ("joint", "bone") and not ens.training and not a.training
    assert StreamEnsemble(members, weights={"bone": 0.5, "joint": 2}).weights == [2.0, 0.5]
    assert StreamEnsemble(members, weights=(0.25, 0.75), transform="softmax").weights == [0.25, 0.75]
    assert len(list(ens.parameters())) == 4
    with pytest.raises(ValueError, match="weights names"):
        StreamEnsemble(members, weights={"joint": 1.0, "motion": 1.0})
    with pytest.raises(ValueError, match="weights names"):
        StreamEnsemble(members, weights={"joint": 1.0})
    with pytest.raises(ValueError, match="3 weights"):
        StreamEnsemble(members, weights=[1, 2, 3])
    with pytest.raises(ValueError, match="transform"):
        StreamEnsemble(members, transform="log_softmax")
    for bad in ({}, {"joint": a}, {"joint": (a, 3)}, {"joint": ("skeleton", a)}, {"joint": (a, {})}, {str(i): (a, "x") for i in range(9)}):
        with pytest.raises(ValueError):
            StreamEnsemble(bad)
    ens.train()
    with pytest.raises(RuntimeError, match="joint fine-tuning through the fused score is not built"):
        ens({"skeleton": torch.zeros(2, 4), "skeleton_bone": torch.zeros(2, 4)})
    ens.eval()
    with pytest.raises(KeyError, match="skeleton_bone"):
        ens({"skeleton": torch.zeros(2, 4)})
    with pytest.raises(ValueError, match="dict of features"):
        ens(torch.zeros(2, 4))


def _filled_metric(name, scores, labels, filled=None):
    from fusion_gcn_amd.metrics import StreamScores
    m = StreamScores(name, *scores.shape)
    m._load_arrays(scores, labels, np.ones(len(labels), bool) if filled is None else filled)
    return m


def test_score_files_round_trip_and_the_refusals(tmp_path):
    from fusion_gcn_amd.ensemble import ScoreStore
    from fusion_gcn_amd.metrics import Metric, StreamScores
    rng = np.random.default_rng(3)
    N, classes = 11, 6
    labels = rng.integers(0, classes, N)
    scores = {n: rng.standard_normal((N, classes)).astype(np.float32) for n in ("joint", "bone")}
    paths = {}
    for n, z in scores.items():
        m = _filled_metric(f"validation_scores_{n}", z, labels)
        assert isinstance(m, Metric) and m._to_summary(None, 0) is None
        paths[n] = str(tmp_path / f"{n}.npz")
        m.save(paths[n])
        with np.load(paths[n]) as f:
            assert sorted(f.files) == ["filled", "labels", "scores"]
            assert f["scores"].dtype == np.float32 and f["labels"].dtype == np.int64 and f["filled"].dtype == np.bool_
            assert f["scores"].shape == (N, classes) and f["filled"].all()
    store = ScoreStore.load(paths, transform="softmax")
    assert store.names == ("joint", "bone") and store.num_samples == N and store.num_classes == classes and store.transform == "softmax"
    assert all(np.array_equal(store.scores[n].view(np.uint32), scores[n].view(np.uint32)) for n in scores) and np.array_equal(store.labels, labels)
    same = ScoreStore.from_metrics({n: _filled_metric("validation_" + n, z, labels) for n, z in scores.items()})
    assert all(np.array_equal(same.scores[n], scores[n]) for n in scores)

    def saved(name, z, y, filled=None):
        path = str(tmp_path / f"{name}.npz")
        _filled_metric("validation_x", z, y, filled).save(path)
        return path
    with pytest.raises(ValueError, match="12 samples"):
        ScoreStore.load({**paths, "motion": saved("n", np.zeros((N + 1, classes), np.float32), np.zeros(N + 1, np.int64))})
    with pytest.raises(ValueError, match="7 classes"):
        ScoreStore.load({**paths, "motion": saved("c", np.zeros((N, classes + 1), np.float32), labels)})
    other = labels.copy()
    other[4] = (other[4] + 1) % classes
    with pytest.raises(ValueError, match="labels of stream 'motion' differ"):
        ScoreStore.load({**paths, "motion": saved("y", scores["bone"], other)})
    holes = np.ones(N, bool)
    holes[[2, 9]] = False
    with pytest.raises(ValueError, match=r"2 unfilled rows \(first: 2\)"):
        ScoreStore.load({**paths, "motion": saved("f", scores["bone"], labels, holes)})
    with pytest.raises(ValueError, match="unfilled"):          # a metric no update reached
        ScoreStore.from_metrics({"joint": StreamScores("validation_scores", N, classes)})
    np.savez(str(tmp_path / "alien.npz"), scores=scores["bone"])
    with pytest.raises(ValueError, match="lacks"):
        ScoreStore.load({"joint": str(tmp_path / "alien.npz")})
    with pytest.raises(ValueError, match="weights names"):
        store.fuse({"joint": 1.0})
    with pytest.raises(ValueError, match="candidates"):
        store.search(np.ones((3, 3)))
    with pytest.raises(ValueError, match="k=7"):
        store.search(np.ones((3, 2)), k=7)
    for bad in ((0, 3), (3, 0), (3, _lib.CLS_MAX_CLASSES + 1)):
        with pytest.raises(ValueError):
            StreamScores("validation_scores", *bad)
    m = StreamScores("validation_scores", N, classes)
    value = m.value
    assert value[0].shape == (N, classes) and (value[1] == -1).all() and not value[2].any()
    with pytest.raises(ValueError, match="_load_arrays"):
        m._load_arrays(np.zeros((N, classes + 1)), labels, holes)
    m._load_arrays(scores["bone"], labels, holes)
    m.reset()
    assert not m.value[0].any() and (m.value[1] == -1).all() and not m.value[2].any()


def test_best_candidate_order():
    from fusion_gcn_amd.ensemble import best_candidate
    for table in ([[3, 9], [5, 6], [5, 7], [5, 7], [4, 9]], [[0, 0]], [[2, 2], [2, 2]], [[1, 5], [2, 1]]):
        assert best_candidate(np.asarray(table)) == R.best(table)
    assert best_candidate(np.asarray([[3, 9], [5, 6], [5, 7], [5, 7], [4, 9]])) == 2


def test_the_restatement_resolves_ties_and_nan_as_the_header_says():
    nan, inf = np.nan, np.inf
    rows = np.asarray([[1.0, 3.0, 3.0, 2.0],        # a tie of the maximum: the lower index wins
                       [1.0, 3.0, 3.0, 2.0],
                       [0.0, nan, 5.0, nan],        # NaN is the maximum, the FIRST NaN the prediction
                       [0.0, nan, 5.0, nan],
                       [2.0, 2.0, 2.0, 2.0],        # all equal: rank(y) = y
                       [-inf, 1.0, inf, 0.0],
                       [1.0, 2.0, 3.0, 4.0],
                       [1.0, 2.0, 3.0, 4.0],
                       [1.0, 2.0, 3.0, 4.0]], np.float32)
    labels = np.asarray([1, 2, 3, 2, 2, 2, -100, 4, -1])
    got = R.classify(rows, labels, k=2)
    assert got["pred"].tolist() == [1, 1, 1, 1, 0, 2, -1, -1, -1]
    assert (got["examples"], got["ignored"], got["invalid"]) == (6, 1, 2)
    assert got["top1"] == 2                          # rows 0 and 5
    assert got["topk"] == 4                          # rows 0, 1 (rank 1), 3 is rank 2 (two NaN above), 2 is rank 1 (one NaN at a lower index), 5
    assert R.classify(rows[4:5], [2], k=2)["topk"] == 0 and R.classify(rows[4:5], [2], k=3)["topk"] == 1
    # the fused value: float64 accumulation, one rounding -- 2^24 + 1 is no float32, and 1 + 2^-30 + (-1) survives only in float64
    a = np.asarray([[2.0 ** 24]], np.float32)
    b = np.asarray([[1.0]], np.float32)
    assert R.fuse([a, b, b], [1, 1, 1]).tolist() == [[2.0 ** 24 + 2]]            # float32 steps would stay at 2^24
    tiny = np.asarray([[2.0 ** -30]], np.float32)
    assert R.fuse([b, tiny, b], [1, 1, -1]).tolist() == [[2.0 ** -30]]
    assert R.fuse([np.asarray([[-0.0]], np.float32)], [1.0]).view(np.uint32).tolist() == [[0]]            # acc starts at +0.0
    assert R.fuse([b], [0.1]).tolist() == [[float(np.float32(0.1))]]            # weights are float32 first
    sm = R.transform(np.asarray([[0.0, 0.0], [nan, 1.0], [inf, 1.0], [-inf, -inf], [-inf, 0.0]], np.float32), R.SOFTMAX)
    assert sm[0].tolist() == [0.5, 0.5] and np.isnan(sm[1:4]).all() and sm[4].tolist() == [0.0, 1.0]
    header, hits = R.sweep([rows, rows], [[1, 1], [0.5, 0.5], [0, 0]], labels, 2)
    assert header.tolist() == [6, 1, 2] and hits[0].tolist() == [2, 4] and hits[1].tolist() == [2, 4]
    # zero weights: 0 x NaN and 0 x inf are NaN and every other value is +0, so rank(y) = the equal values at lower indices: no row has
    # rank 0 (row 0: label 1, rank 1), and rows 0, 2 (one NaN in front of the label's) and 5 (the label's NaN behind one) have rank 1
    assert hits[2].tolist() == [0, 3]
