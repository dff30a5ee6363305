"""fgcn_score_fuse / fgcn_fuse_sweep and the host layer above them on the device, against the numpy restatement of
tests/ensemble_ref.py and against fgcn_classify_update.

Mode NONE is defined bit for bit (a float32 times a float32 is exact in float64; one rounding), so the uint32 views are equal.  Mode
SOFTMAX forms exp(z - m) / sum in float64 on both sides; the two float64 values differ by the order of the sum's additions and the two
exp implementations, ~1e-15 relative, so after the ONE rounding to float32 they differ by at most one float32 spacing, and the fused
value of S streams by at most sum_s |w_s| spacing(t_s) + spacing(fused) (positive weights: no cancellation).  The sweep's counts are
integers: equal, in both transforms, to what fgcn_classify_update counts on fgcn_score_fuse's output candidate by candidate.

Shapes: the smallest at which the kernels take another path -- 1 row and 260 (more than one workgroup of four waves), 1, 2, 27, 64, 65 and
130 classes (below, at and above one 64-lane walk), padded rows, 1 / 2 / 4 / 8 streams (the sweep stages one stream per wave: 8 streams are
two rounds of its four waves), more rows than the sweep's grid holds, and one candidate more than fits one pass.  Everything runs on
guarded allocations, inputs placed with guarded.put: a load past a row reaches NaN, a store past `out` a margin."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ensemble_ref as R
from test_data import write_split

import guarded
from guarded import guarded_allocations  # noqa: F401  (the fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_allocations")]
DEV = torch.device("cuda:0")
ROWS, CLASSES = (1, 5, 67, 260), (1, 2, 27, 64, 65, 130)
PAD_FILL = 7.0


def _put(a, pad=0):
    """(rows, classes) float32 on the device; pad > 0: a view of rows that are `pad` floats longer, the padding NaN"""
    a = np.ascontiguousarray(a, np.float32)
    if not pad:
        return guarded.put(torch.from_numpy(a), device=DEV)
    wide = np.full((a.shape[0], a.shape[1] + pad), np.nan, np.float32)
    wide[:, :a.shape[1]] = a
    return guarded.put(torch.from_numpy(wide), device=DEV)[:, :a.shape[1]]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _fuse(scores, weights, transform, pad):
    """ops.score_fuse into a padded `out` whose padding must stay as it was -> the fused rows on the host"""
    from fusion_gcn_amd import ops
    rows, classes = scores[0].shape
    dev = [_put(z, pad if s % 2 == 0 else 0) for s, z in enumerate(scores)]
    wide = guarded.put(torch.full((rows, classes + pad), PAD_FILL), device=DEV)
    out = ops.score_fuse(dev, weights, transform, out=wide[:, :classes])
    assert out.data_ptr() == wide.data_ptr()
    again = ops.score_fuse(dev, weights, transform)                       # its own output buffer; two calls give the same bits
    torch.cuda.synchronize()
    host = wide.cpu().numpy()
    assert (host[:, classes:] == PAD_FILL).all()
    assert np.array_equal(_bits(again.cpu().numpy()), _bits(host[:, :classes]))
    return np.ascontiguousarray(host[:, :classes])


def _draw(rng, kind, S, rows, classes):
    if kind == "random":
        return [rng.standard_normal((rows, classes)).astype(np.float32) * 3 for _ in range(S)], rng.standard_normal(S).astype(np.float32)
    scores = [(rng.integers(-4, 5, (rows, classes)) / 4).astype(np.float32) for _ in range(S)]          # ties are frequent and exact
    return scores, rng.choice(np.asarray([1.0, 0.5, 0.25], np.float32), S)


@pytest.mark.parametrize("kind", ["random", "quarters"])
@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("S", [1, 2, 4, 8])
def test_score_fuse_raw_scores_bit_for_bit(S, pad, kind):
    rng = np.random.default_rng(100 * S + 10 * pad + len(kind))
    for rows in ROWS:
        for classes in CLASSES:
            scores, w = _draw(rng, kind, S, rows, classes)
            got = _fuse(scores, w, "none", pad)
            want = R.fuse(scores, w, R.NONE)
            assert np.array_equal(_bits(got), _bits(want)), (rows, classes, int((_bits(got) != _bits(want)).sum()))


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("S", [1, 2, 4, 8])
def test_score_fuse_softmax_within_the_rounding_bound(S, pad):
    rng = np.random.default_rng(7 * S + pad)
    for rows in ROWS:
        for classes in CLASSES:
            scores = [rng.standard_normal((rows, classes)).astype(np.float32) * 3 for _ in range(S)]
            w = np.ones(1, np.float32) if S == 1 else rng.uniform(0.1, 1.0, S).astype(np.float32)      # positive: no cancellation
            got = _fuse(scores, w, "softmax", pad).astype(np.float64)
            want = R.fuse(scores, w, R.SOFTMAX)
            # S = 1, weight 1: the fused value IS the probability, one float32 spacing; otherwise the header's sum
            bound = np.spacing(want).astype(np.float64) if S == 1 else R.spacing_bound(scores, w, R.SOFTMAX)
            err = np.abs(got - want.astype(np.float64))
            worst = float((err / bound).max())
            print(f"softmax S={S} rows={rows} classes={classes} pad={pad}: worst error / bound = {worst:.3f}")
            assert (err <= bound).all(), (rows, classes, worst)
            assert np.allclose(got.sum(axis=1), float(w.astype(np.float64).sum()), rtol=1e-5)


def _sweep_case(rng, rows, classes, S):
    scores = [(rng.integers(-4, 5, (rows, classes)) / 4).astype(np.float32) for _ in range(S)]
    labels = rng.integers(0, classes, rows).astype(np.int64)
    if rows > 8:
        labels[1], labels[2], labels[3], labels[5] = -100, classes, -1, 10 ** 12      # ignored, and three invalid ones
        scores[S - 1][4, min(1, classes - 1)] = np.nan                                # a NaN in one stream of a row that counts
        scores[0][6] = 0.5                                                            # a row that is one tie in stream 0
    return scores, labels


SWEEPS = [(67, 27, 4, 5, 1), (67, 27, 4, 5, 3), (67, 27, 4, 5, "pass+3"), (37, 130, 8, 3, 3), (2100, 5, 2, 2, 3), (5, 1, 1, 1, 3), (9, 64, 3, 64, 2)]


@pytest.mark.parametrize("transform", ["none", "softmax"])
@pytest.mark.parametrize("rows,classes,S,k,G", SWEEPS, ids=["x".join(map(str, c)) for c in SWEEPS])
def test_fuse_sweep_counts_what_classify_update_counts_on_the_fused_scores(rows, classes, S, k, G, transform):
    from fusion_gcn_amd import _lib, ops
    G = _lib.FUSE_PASS + 3 if G == "pass+3" else G
    rng = np.random.default_rng(rows + classes + S + G)
    scores, labels = _sweep_case(rng, rows, classes, S)
    cand = rng.choice(np.asarray([0.0, 0.25, 0.5, 1.0], np.float32), (G, S))
    dev = [_put(z, 3 if s % 2 else 0) for s, z in enumerate(scores)]
    y = torch.from_numpy(labels).to(DEV)
    counts = torch.zeros(_lib.FUSE_HEADER + 2 * G, dtype=torch.int64, device=DEV)
    hits, header = ops.fuse_sweep(dev, cand, y, k, transform, counts=counts)
    assert hits.data_ptr() == counts.data_ptr() + 8 * _lib.FUSE_HEADER and tuple(hits.shape) == (G, 2) and hits.dtype == torch.int64
    once = counts.cpu().numpy().copy()
    # candidates on the device, as float64: converted to float32 in a buffer of ops' own (the values are exact in float32); the call ADDS
    ops.fuse_sweep(dev, guarded.put(torch.from_numpy(cand.astype(np.float64)), device=DEV), y, k, transform, counts=counts)
    assert np.array_equal(counts.cpu().numpy(), 2 * once)
    fresh_hits, fresh_header = ops.fuse_sweep(dev, cand, y, k, transform)                                   # a zeroed buffer of its own
    assert np.array_equal(np.concatenate([fresh_header.cpu().numpy(), fresh_hits.cpu().numpy().reshape(-1)]), once)
    # candidate by candidate: fgcn_classify_update on fgcn_score_fuse's output, one state per candidate, no wait in between
    words = ops.classify_state_bytes(classes) // 8
    states = torch.zeros((G, words), dtype=torch.int64, device=DEV)
    fused = guarded.put(torch.zeros(rows, classes), device=DEV)
    for g in range(G):
        ops.score_fuse(dev, cand[g], transform, out=fused)
        ops.classify_update(fused, y, states[g], k=k)
    states = states.cpu().numpy()
    assert np.array_equal(once[_lib.FUSE_HEADER:].reshape(G, 2), states[:, [_lib.CLS_TOP1, _lib.CLS_TOPK]])
    want_header = [int((labels >= 0).sum() - (labels >= classes).sum()), int((labels == -100).sum()),
                   int(((labels < 0) & (labels != -100)).sum() + (labels >= classes).sum())]
    assert once[:_lib.FUSE_HEADER].tolist() == want_header
    assert (states[:, [_lib.CLS_EXAMPLES, _lib.CLS_IGNORED, _lib.CLS_INVALID]] == np.asarray(want_header)).all()
    if transform == "none":
        ref_header, ref_hits = R.sweep(scores, cand, labels, k, R.NONE)
        assert np.array_equal(ref_hits, once[_lib.FUSE_HEADER:].reshape(G, 2)) and ref_header.tolist() == want_header
    if rows > 8:
        assert want_header[1] == 1 and want_header[2] == 3 and 0 < once[_lib.FUSE_HEADER:].reshape(G, 2)[:, 1].max() <= want_header[0]


# ---- the host layer: two tiny AGCN models on the joint and the bone stream ---------------------------------------------------------------
@pytest.fixture
def two_stream_setup(tmp_path):
    from fusion_gcn_amd.data import ClipBatches, MultiModalDataset, NumpyDatasetLoader, Streams
    from fusion_gcn_amd.datasets.utd_mhad import constants as utd
    from fusion_gcn_amd.models.mmargcn.agcn import Model
    from fusion_gcn_amd.util import Graph
    from oracle import filler
    shape, classes, n = (1, 16, 20, 3), 5, 12
    write_split(str(tmp_path), "train", n, {"skeleton": shape}, classes=classes, seed=11)
    ds = MultiModalDataset([(str(tmp_path), NumpyDatasetLoader())], "train")
    models = []
    for salt in (0, 1):
        model = Model(shape, classes, Graph(utd.skeleton_edges, center_joint=utd.center_joint), num_layers=2)
        filler.fill_state_dict(model.state_dict(), salt=salt)
        models.append(guarded.to(model, DEV).eval())
    loader = ClipBatches(ds, 4, device=DEV, streams=Streams.for_dataset("utd_mhad", streams=("joint", "bone")))
    return models, loader, classes, n


def test_stream_ensemble_and_score_store_on_two_models(two_stream_setup):
    from fusion_gcn_amd import ops
    from fusion_gcn_amd.ensemble import ScoreStore, StreamEnsemble, simplex_grid
    from fusion_gcn_amd.metrics import StreamScores, build_metrics
    from fusion_gcn_amd.session.session import Session
    from fusion_gcn_amd.session.procedures.batch_train import DefaultBatchProcessor
    from fusion_gcn_amd.session.procedures.step import DefaultStep
    (joint, bone), loader, classes, n = two_stream_setup
    weights = {"joint": 1.0, "bone": 0.5}
    ens = StreamEnsemble({"joint": (joint, "skeleton"), "bone": (bone, "skeleton_bone")}, weights=weights)
    # forward is bitwise ops.score_fuse of the members' own eval outputs
    own = {"joint": np.zeros((n, classes), np.float32), "bone": np.zeros((n, classes), np.float32)}
    labels = np.zeros(n, np.int64)
    batches = 0
    for feats, y, idx in loader:
        assert sorted(feats) == ["skeleton", "skeleton_bone"]
        with torch.no_grad():
            zj, zb = joint(feats["skeleton"]), bone(feats["skeleton_bone"])
        want = ops.score_fuse([zj, zb], [1.0, 0.5])
        got = ens(feats)
        assert not got.requires_grad and torch.equal(got, want)
        at = idx.cpu().numpy()
        own["joint"][at], own["bone"][at], labels[at] = zj.cpu().numpy(), zb.cpu().numpy(), y.cpu().numpy()
        batches += 1
    assert batches == 3 and not np.array_equal(own["joint"], own["bone"])
    ref = R.classify(R.fuse([own["joint"], own["bone"]], [1.0, 0.5]), labels, k=2)
    # ... through Session.validate_epoch with an unchanged container; the members' scores are collected in a pass each
    container = build_metrics(classes, k=2, is_eval=True)
    Session.validate_epoch(DefaultBatchProcessor(DefaultStep()), ens, F.cross_entropy, loader, None, container)
    counts = container.state_snapshot("val")["counts"]
    from fusion_gcn_amd import _lib
    assert (int(counts[_lib.CLS_EXAMPLES]), int(counts[_lib.CLS_TOP1]), int(counts[_lib.CLS_TOPK])) == (ref["examples"], ref["top1"], ref["topk"])
    assert ref["examples"] == n and container["validation_accuracy"].value == ref["top1"] / n
    stores = {}
    for name, model, key in (("joint", joint, "skeleton"), ("bone", bone, "skeleton_bone")):
        stores[name] = StreamScores(f"validation_scores_{name}", n, classes)
        member = StreamEnsemble({name: (model, key)})              # one member, weight 1: the fused score is the model's own, bit for bit
        Session.validate_epoch(DefaultBatchProcessor(DefaultStep()), member, F.cross_entropy, loader, None,
                               build_metrics(classes, k=2, is_eval=True, additional_metrics=[stores[name]]))
        scores, got_labels, filled = stores[name].value
        assert filled.all() and np.array_equal(got_labels, labels) and np.array_equal(_bits(scores), _bits(own[name]))
    store = ScoreStore.from_metrics(stores)
    assert store.evaluate(weights, k=2) == {"top1": ref["top1"], "topk": ref["topk"], "examples": n}
    assert np.array_equal(_bits(store.fuse(weights).cpu().numpy()), _bits(R.fuse([own["joint"], own["bone"]], [1.0, 0.5])))
    grid = simplex_grid(2, 4)
    found = store.search(grid, k=2)
    ref_header, ref_hits = R.sweep([own["joint"], own["bone"]], grid, labels, 2)
    assert np.array_equal(found["counts"], ref_hits) and found["best"] == R.best(ref_hits) and found["examples"] == n
    assert found["weights"].tolist() == grid[found["best"]].tolist()
    stores["joint"].reset()
    assert not stores["joint"].value[2].any()


def test_stream_ensemble_forward_in_training_mode_raises(two_stream_setup):
    from fusion_gcn_amd.ensemble import StreamEnsemble
    (joint, bone), loader, _, _ = two_stream_setup
    ens = StreamEnsemble({"joint": (joint, "skeleton"), "bone": (bone, "skeleton_bone")}).train()
    feats, _, _ = next(iter(loader))
    with pytest.raises(RuntimeError, match="joint fine-tuning through the fused score is not built"):
        ens(feats)
    assert ens.eval()(feats).shape == (4, 5)
