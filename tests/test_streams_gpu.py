"""fgcn_clip_streams on the device against the numpy restatement of tests/streams_ref.py.  Every comparison is exact
-- each value is one correctly rounded float32 subtraction, a copy or a zero -- so there is no tolerance to derive: the uint32 views are
equal, and where NaN is expected NaN stands where NaN stands.  The shapes are the smallest at which the kernel can go wrong: rows of 21,
27 and 75 floats (no 16-byte alignment), two coordinates, two bodies, T = 1 and T = 2, 3000 lanes (more than one workgroup, no multiple of
256); the parents are not in topological order.  Every test runs on guarded allocations: a read of frame T behind the last row, or a
store past a row, reaches NaN or a margin.  Then the promises of ClipBatches: the same bits on the resident and the streaming path, the
streams of what the stages before left (normalised, IMU-enhanced, augmented -- also where the augmentation leaves a feature out, so that the
two features are read through different rows), and a model that trains on the bone stream."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import streams_ref as R
from test_data import write_split

import guarded
from guarded import guarded_allocations  # noqa: F401  (the fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_allocations")]
DEV = torch.device("cuda:0")
DERIVED = R.STREAMS[1:]


def _f(a):
    return guarded.to(torch.as_tensor(np.ascontiguousarray(a)), DEV)


def _parents(V):
    """not in topological order: joint 0's and joint 4's parents have higher numbers, 2 is the root (its own parent), 5 is copied through"""
    assert V >= 7
    return [2, 0, 2, 1, 6, -1, 3] + list(range(6, V - 1))


def _run(src, idx, parents, streams, valid=None):
    from fusion_gcn_amd import ops
    got = ops.clip_streams(_f(src), torch.as_tensor(idx, dtype=torch.int64), parents, streams=streams,
                           valid=None if valid is None else torch.as_tensor(np.asarray(valid), dtype=torch.int32).to(DEV))
    torch.cuda.synchronize()
    assert list(got) == list(streams)
    return {s: t.cpu().numpy() for s, t in got.items()}


CASES = [(1, 5, 7, 3), (2, 13, 7, 3), (1, 13, 9, 2), (2, 1, 7, 3), (1, 2, 7, 3), (1, 40, 25, 3)]


@pytest.mark.parametrize("M,T,V,C", CASES, ids=["x".join(map(str, c)) for c in CASES])
def test_kernel_against_the_restatement(M, T, V, C):
    """five source rows gathered as [4, 0, 4]: all four outputs in one launch, then each derived output alone; two calls give the same bits"""
    rng = np.random.default_rng(M * 1000 + T * 10 + V + C)
    src = rng.standard_normal((5, M, T, V, C)).astype(np.float32)
    idx, par = [4, 0, 4], _parents(V)
    want = R.batch(src, idx, par)
    got = _run(src, idx, par, R.STREAMS)
    for s in R.STREAMS:
        assert got[s].shape == (3, M, T, V, C) and R.same_bits(got[s], want[s]), s
    assert not got["bone"][:, :, :, 2].any() and R.same_bits(got["bone"][:, :, :, 5], src[idx][:, :, :, 5])       # the root, the sensor joint
    assert not got["motion"][:, :, T - 1:].any() and not got["bone_motion"][:, :, T - 1:].any()
    again = _run(src, idx, par, R.STREAMS)
    assert all(R.same_bits(again[s], got[s]) for s in R.STREAMS)
    for s in DERIVED:                                                         # the launches that load less
        alone = _run(src, idx, par, (s,))
        assert list(alone) == [s] and R.same_bits(alone[s], want[s]), s
    from fusion_gcn_amd import ops
    on_dev = _run(src, idx, ops.stream_parents(par, DEV), ("joint", "bone_motion"))      # the table built once, as the stage does
    assert R.same_bits(on_dev["joint"], want["joint"]) and R.same_bits(on_dev["bone_motion"], want["bone_motion"])


@pytest.mark.parametrize("M,T,V,C", [(2, 13, 7, 3), (1, 5, 9, 2)])
def test_valid_frames_bound_what_the_motions_read(M, T, V, C):
    """valid in {1, 2, T-1, T}; the source is NaN at and behind L, so a motion value that read such a frame would be NaN"""
    rng = np.random.default_rng(T + V)
    src = rng.standard_normal((5, M, T, V, C)).astype(np.float32)
    valid = [1, 2, T - 1, T, 2]
    for r, L in enumerate(valid):
        src[r, :, L:] = np.nan
    idx, par = [4, 0, 4, 1, 2, 3], _parents(V)
    want = R.batch(src, idx, par, valid)
    got = _run(src, idx, par, R.STREAMS, valid)
    for s in ("motion", "bone_motion"):
        assert not np.isnan(got[s]).any() and R.same_bits(got[s], want[s]), s
    for s in ("joint", "bone"):                                               # they cover all T frames: NaN exactly where the source has it
        assert R.same_values(got[s], want[s]), s
        assert np.array_equal(np.isnan(got[s]), np.isnan(src[idx])), s
    for s in ("motion", "bone_motion"):
        alone = _run(src, idx, par, (s,), valid)
        assert R.same_bits(alone[s], want[s]), s
    # a count outside [1, T] is clamped before it becomes an address: 0 reads as 1, T + 3 as T (the restatement clamps the same way)
    src = rng.standard_normal((3, M, T, V, C)).astype(np.float32)
    src[0, :, 1:] = np.nan
    valid = [0, T + 3, -7]
    want = R.batch(src, [2, 1, 0], par, valid)
    got = _run(src, [2, 1, 0], par, R.STREAMS, valid)
    assert all(R.same_values(got[s], want[s]) for s in R.STREAMS)
    assert not got["motion"][0].any() and not got["motion"][2].any() and R.same_bits(got["motion"][1], R.motion(src[1]))
    assert not np.isnan(got["motion"]).any() and not np.isnan(got["bone_motion"]).any()


def test_wrapper_refusals():
    from fusion_gcn_amd import _lib, ops
    src = torch.zeros(5, 2, 13, 7, 3, device=DEV)
    par = _parents(7)
    with pytest.raises(_lib.FgcnError, match="rows outside"):
        ops.clip_streams(src, torch.tensor([5]), par)
    with pytest.raises(_lib.FgcnError, match="int64"):
        ops.clip_streams(src, torch.arange(5, dtype=torch.int32), par)
    with pytest.raises(_lib.FgcnError, match="parents"):
        ops.clip_streams(src, torch.arange(5), par[:6])
    with pytest.raises(_lib.FgcnError, match="parents"):
        ops.clip_streams(src, torch.arange(5), [7] + par[1:])
    with pytest.raises(_lib.FgcnError, match="int32"):
        ops.clip_streams(src, torch.arange(5), par, valid=torch.ones(5, dtype=torch.int64, device=DEV))
    for bad in ((), ("joint",), ("bone", "bone"), ("speed",)):
        with pytest.raises(_lib.FgcnError, match="streams"):
            ops.clip_streams(src, torch.arange(5), par, streams=bad)
    with pytest.raises(_lib.FgcnError, match="alias src"):
        ops.clip_streams(src, torch.arange(5), par, out={"bone": src})
    with pytest.raises(_lib.FgcnError, match="for a batch of"):
        ops.clip_streams(src, torch.arange(4), par, out={"bone": torch.zeros(5, 2, 13, 7, 3, device=DEV)})
    with pytest.raises(_lib.FgcnError, match="not among the streams"):
        ops.clip_streams(src, torch.arange(5), par, out={"motion": torch.zeros(5, 2, 13, 7, 3, device=DEV)})
    with pytest.raises(_lib.FgcnError, match="C=4"):
        ops.clip_streams(torch.zeros(2, 1, 3, 7, 4, device=DEV), torch.arange(2), par)


# ---- ClipBatches ----------------------------------------------------------------------------------------------------------------------
N, BS = 10, 4                                                                 # batches of 4, 4 and a ragged 2: both slots, twice
PAR7 = _parents(7)


def _dataset(root, shapes, seed=0):
    from fusion_gcn_amd.data import MultiModalDataset, NumpyDatasetLoader
    arrays, labels = write_split(str(root), "train", N, shapes, seed=seed)
    return MultiModalDataset([(str(root), NumpyDatasetLoader())], "train"), arrays, labels


def _epoch(ds, resident, **kw):
    """-> (the iterator, [(features as a dict of host arrays, labels, indices, last_streams)]) of one shuffled pass in epoch 2"""
    from fusion_gcn_amd.data import ClipBatches
    it = ClipBatches(ds, BS, shuffle=True, seed=5, device=DEV, resident=resident, **kw)
    it.set_epoch(2)
    out = []
    for feats, lab, idx in it:
        feats = feats if isinstance(feats, dict) else {it.out_keys[0]: feats}
        out.append(({k: v.cpu().numpy().copy() for k, v in feats.items()}, lab.cpu().clone(), idx.clone(), dict(it.last_streams)))
    torch.cuda.synchronize()
    assert it.resident == resident and [len(b[2]) for b in out] == [4, 4, 2]
    return it, out


def _check(ds, stages, streams, expect, valid=None):
    """Both paths with ``streams=`` deliver the same bits; every batch is the restatement applied to what the same ClipBatches without
    ``streams=`` yields for the same seed and epoch; labels and indices are untouched.  ``expect``: feature id -> {stream: output id} for
    the features the stage applies to.  -> the resident pass with the streams and the one without"""
    _, plain = _epoch(ds, True, **stages)
    (it, res), (_, stream) = _epoch(ds, True, **stages, streams=streams), _epoch(ds, False, **stages, streams=streams)
    untouched = [k for k in plain[0][0] if k not in expect]
    keys = [i for k in plain[0][0] for i in (expect[k].values() if k in expect else [k])]
    assert it.out_keys == keys and it.stages[-1] is streams and it.streams is streams
    for a, b, p in zip(res, stream, plain):
        assert torch.equal(a[2], b[2]) and torch.equal(a[2], p[2]) and torch.equal(a[1], b[1]) and torch.equal(a[1], p[1])
        assert list(a[0]) == list(b[0]) == keys
        assert a[3] == b[3] == {k: list(ids.values()) for k, ids in expect.items()}
        for k in keys:
            assert R.same_values(a[0][k], b[0][k]) and a[0][k].tobytes() == b[0][k].tobytes(), k
        for k in untouched:
            assert a[0][k].tobytes() == p[0][k].tobytes(), k
        for k, ids in expect.items():
            rows = None if valid is None else valid[k][a[2].numpy()]
            want = R.batch(p[0][k], range(len(a[2])), streams.parents, rows)
            for s, i in ids.items():
                assert R.same_values(a[0][i], want[s]), (k, s)
    return res, plain


def test_clip_batches_streams_alone(tmp_path):
    from fusion_gcn_amd.data import Streams
    ds, arrays, labels = _dataset(tmp_path, {"skeleton": (2, 13, 7, 3), "inertial": (11, 6)})
    res, _ = _check(ds, {}, Streams(PAR7), {"skeleton": {"bone": "skeleton"}})             # one stream: the id stays
    for feats, lab, idx, _ in res:                                           # and it is the bone of the stored rows
        assert R.same_bits(feats["skeleton"], R.batch(arrays["skeleton"], idx.numpy(), PAR7)["bone"])
        assert np.array_equal(feats["inertial"], arrays["inertial"][idx.numpy()])
        assert torch.equal(lab, torch.from_numpy(labels.astype(np.int64))[idx])
    valid = {"skeleton": np.random.default_rng(4).integers(1, 14, N)}
    all4 = {"joint": "skeleton", "bone": "skeleton_bone", "motion": "skeleton_motion", "bone_motion": "skeleton_bone_motion"}
    res, _ = _check(ds, {}, Streams(PAR7, streams=("bone", "motion", "joint", "bone_motion"), valid_frames=valid), {"skeleton": all4}, valid)
    for feats, _, idx, _ in res:
        want = R.batch(arrays["skeleton"], idx.numpy(), PAR7, valid["skeleton"])
        assert all(R.same_bits(feats[i], want[s]) for s, i in all4.items())
        assert list(feats) == ["inertial", "skeleton", "skeleton_bone", "skeleton_motion", "skeleton_bone_motion"]
    # one stream, whichever: the id stays, and only= leaves nothing else to derive
    from fusion_gcn_amd.data import ClipBatches
    it = ClipBatches(ds, BS, device=DEV, streams=Streams(PAR7, streams=("motion",), only=["skeleton"]))
    feats, _, idx = next(iter(it))
    assert isinstance(feats, dict) and list(feats) == ["inertial", "skeleton"] and it.last_streams == {"skeleton": ["skeleton"]}
    assert R.same_bits(feats["skeleton"].cpu().numpy(), R.batch(arrays["skeleton"], idx.numpy(), PAR7)["motion"])


def test_clip_batches_behind_normalize(tmp_path):
    from fusion_gcn_amd.data import Normalize, Streams
    ds, _, _ = _dataset(tmp_path, {"skeleton": (2, 13, 7, 3)})
    stages = dict(normalize=Normalize(1, z_axis_joints=(0, 1), x_axis_joints=(3, 4)))
    _check(ds, stages, Streams(PAR7, streams=("bone", "bone_motion")), {"skeleton": {"bone": "skeleton_bone", "bone_motion": "skeleton_bone_motion"}})


def test_clip_batches_behind_inertial_enhance(tmp_path):
    """the enhanced skeleton has two sensor joints behind UTD-MHAD's twenty: ``for_dataset(..., extra_joints=2)`` copies them through"""
    from fusion_gcn_amd.data import Inertial, Streams
    ds, _, _ = _dataset(tmp_path, {"skeleton": (1, 13, 20, 3), "inertial": (29, 6)})
    rng = np.random.default_rng(6)
    frames = {"skeleton": rng.integers(2, 14, N), "inertial": rng.integers(2, 30, N)}
    streams = Streams.for_dataset("utd_mhad", extra_joints=2, streams=("joint", "bone", "motion"), valid_frames={"skeleton": frames["skeleton"]})
    expect = {"skeleton": {"joint": "skeleton", "bone": "skeleton_bone", "motion": "skeleton_motion"}}
    res, plain = _check(ds, dict(inertial=Inertial(frames=frames, enhance=True)), streams, expect, {"skeleton": frames["skeleton"]})
    for (feats, _, idx, _), (before, _, _, _) in zip(res, plain):
        assert feats["skeleton"].shape == (len(idx), 1, 13, 22, 3) and list(feats) == ["inertial", "skeleton", "skeleton_bone", "skeleton_motion"]
        assert R.same_bits(feats["skeleton_bone"][:, :, :, 20:], before["skeleton"][:, :, :, 20:])      # sensor axes, not positions
        assert not R.same_bits(feats["skeleton_bone"][:, :, :, :20], before["skeleton"][:, :, :, :20])
        assert feats["inertial"].tobytes() == before["inertial"].tobytes()
        for j, i in enumerate(idx.tolist()):                                  # the appended joints are zero from frame Ls on, and so is their motion
            assert not feats["skeleton_motion"][j, :, frames["skeleton"][i] - 1:].any()


def test_clip_batches_behind_augment(tmp_path):
    from fusion_gcn_amd.data import Augment, ClipBatches, Streams
    ds, arrays, _ = _dataset(tmp_path, {"skeleton": (2, 13, 7, 3), "inertial": (11, 6)})
    all4 = {"joint": "skeleton", "bone": "skeleton_bone", "motion": "skeleton_motion", "bone_motion": "skeleton_bone_motion"}
    res, plain = _check(ds, dict(augment=Augment()), Streams(PAR7, streams=R.STREAMS), {"skeleton": all4})
    for (feats, _, idx, _), (before, _, _, _) in zip(res, plain):
        assert R.same_bits(feats["skeleton"], before["skeleton"])             # "joint" is the augmented clip itself
        assert not R.same_bits(before["skeleton"], arrays["skeleton"][idx.numpy()])
    with pytest.raises(ValueError, match="behind an Augment"):
        ClipBatches(ds, BS, device=DEV, augment=Augment(), streams=Streams(PAR7, valid_frames={"skeleton": [13] * N}))


def test_clip_batches_behind_an_augment_that_leaves_a_feature_out(tmp_path):
    """Two skeleton features of one shape with different values, shuffled: behind ``Augment(only=["skeleton"])`` the resident path reads
    "skeleton" through rows 0..m-1 of the augmented batch and "pose" through the shard's indices of the resident array.  Either feature
    read through the other's rows gives another clip's values, so the comparison with the restatement fails."""
    from fusion_gcn_amd.data import Augment, Streams
    ds, arrays, _ = _dataset(tmp_path, {"skeleton": (2, 13, 7, 3), "pose": (2, 13, 7, 3), "inertial": (11, 6)})
    assert not np.array_equal(arrays["skeleton"], arrays["pose"])
    valid = {"pose": np.random.default_rng(9).integers(1, 14, N)}             # allowed: the augmentation does not apply to "pose"
    expect = {k: {"bone": f"{k}_bone", "motion": f"{k}_motion"} for k in ("pose", "skeleton")}
    streams = Streams(PAR7, streams=("bone", "motion"), valid_frames=valid)
    res, plain = _check(ds, dict(augment=Augment(only=["skeleton"])), streams, expect, {**valid, "skeleton": np.full(N, 13)})
    for (feats, _, idx, _), (before, _, _, _) in zip(res, plain):
        assert list(feats) == ["inertial", "pose_bone", "pose_motion", "skeleton_bone", "skeleton_motion"]
        assert idx.tolist() != list(range(len(idx)))                          # shuffled: the two kinds of rows differ
        assert R.same_bits(before["pose"], arrays["pose"][idx.numpy()]) and not R.same_bits(before["skeleton"], arrays["skeleton"][idx.numpy()])
        assert R.same_bits(feats["pose_bone"], R.batch(arrays["pose"], idx.numpy(), PAR7)["bone"])
        assert R.same_bits(feats["pose_motion"], R.batch(arrays["pose"], idx.numpy(), PAR7, valid["pose"])["motion"])


def test_model_trains_on_the_bone_stream(tmp_path):
    """a two-block AGCN on UTD-MHAD's graph, 4 clips of 16 frames: one training step on the bone stream has a finite loss and a gradient
    for every parameter that has one in the same step on the joints"""
    from fusion_gcn_amd.data import ClipBatches, MultiModalDataset, NumpyDatasetLoader, Streams
    from fusion_gcn_amd.datasets.utd_mhad import constants as utd
    from fusion_gcn_amd.models.mmargcn.agcn import Model
    from fusion_gcn_amd.util import Graph
    from oracle import filler
    shape, classes = (1, 16, 20, 3), 5
    arrays, _ = write_split(str(tmp_path), "train", 4, {"skeleton": shape}, classes=classes, seed=9)
    ds = MultiModalDataset([(str(tmp_path), NumpyDatasetLoader())], "train")

    def step(streams):
        model = Model(shape, classes, Graph(utd.skeleton_edges, center_joint=utd.center_joint), num_layers=2)
        filler.fill_state_dict(model.state_dict())
        model = guarded.to(model, DEV).train()
        (x, y, idx), = list(ClipBatches(ds, 4, device=DEV, streams=streams))
        loss = F.cross_entropy(model(x), y)
        loss.backward()
        torch.cuda.synchronize()
        return x.cpu().numpy(), float(loss.detach()), {n for n, p in model.named_parameters() if p.grad is not None and bool(torch.isfinite(p.grad).all())}

    x_joint, loss_joint, grads_joint = step(None)
    x_bone, loss_bone, grads_bone = step(Streams.for_dataset("utd_mhad"))
    assert x_bone.shape == (4, *shape) and R.same_bits(x_joint, arrays["skeleton"])
    assert R.same_bits(x_bone, R.batch(arrays["skeleton"], range(4), Streams.for_dataset("utd_mhad").parents)["bone"])
    assert np.isfinite(loss_bone) and np.isfinite(loss_joint) and loss_bone != loss_joint
    assert grads_joint and grads_joint <= grads_bone
