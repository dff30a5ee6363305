"""All six stages of ``ClipBatches`` in one pipeline (fusion_gcn_amd/stages.py: Bodies, Normalize, Inertial, Window, Augment, Streams), on
guarded allocations.  Each stage has a module of its own against its restatement; this one pins what only the whole list shows: the
protocol ``stages.Stage`` writes down -- the shapes handed from stage to stage, the tables indexed by source row, and on the resident path
the per-feature ``rows`` hand-over between the three per-batch stages behind the three that ran at upload -- by comparing a resident pass,
a streaming pass and the six ``ops`` calls applied by hand, bit for bit.  Nine clips in shuffled global batches of four: the last batch
is a ragged one of a single clip."""
import os

import numpy as np
import pytest
import torch

import guarded
from guarded import guarded_allocations  # noqa: F401  (the fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_allocations")]
DEV = torch.device("cuda:0")

N, BS, SEED, EPOCH = 9, 4, 5, 2
MR, M, T, V, C, L, S, W = 3, 2, 13, 6, 3, 10, 6, 8
PARENTS = [1, 1, 1, 2, 0, 4, -1, -1]                   # six joints and the two sensor joints Inertial(enhance=True) appends
NORM = dict(origin_joint=1, z_axis_joints=(0, 1), x_axis_joints=(4, 5))


def _split(root):
    """-> (the data set, its arrays, the frame counts): skeletons of 5 to 13 valid frames with zeros behind them, in three bodies of
    different spread, and recordings of 2 to L frames"""
    from fusion_gcn_amd.data import MultiModalDataset, NumpyDatasetLoader, NumpyWriter
    rng = np.random.default_rng(11)
    frames = {"skeleton": rng.integers(5, T + 1, N), "inertial": rng.integers(2, L + 1, N)}
    frames["skeleton"][:2] = 5, T
    skeleton = (rng.standard_normal((N, MR, T, V, C)) * rng.uniform(0.5, 2.0, (N, MR, 1, 1, 1))).astype(np.float32)
    for i, v in enumerate(frames["skeleton"]):
        skeleton[i, :, v:] = 0.0
    arrays = {"skeleton": skeleton, "inertial": rng.standard_normal((N, L, S)).astype(np.float32)}
    for name, a in arrays.items():
        with NumpyWriter(os.path.join(root, f"{name}_train_features.npy"), np.float32, a.shape) as w:
            for s in a:
                w.collect_next(s)
    np.save(os.path.join(root, "train_labels.npy"), np.arange(N) % 4)
    return MultiModalDataset([(root, NumpyDatasetLoader())], "train"), arrays, frames


def _stages(frames):
    from fusion_gcn_amd.data import Augment, Bodies, Inertial, Normalize, Streams, Window
    return dict(bodies=Bodies(M, only=["skeleton"]), normalize=Normalize(**NORM, only=["skeleton"]), inertial=Inertial(frames=frames, enhance=True),
                window=Window(W, train=True, valid_frames={k: frames["skeleton"] for k in ("skeleton", "inertial")}), augment=Augment(joints=(0, V)),
                streams=Streams(PARENTS, streams=("joint", "bone", "motion")))


def _by_hand(arrays, frames, idx, st):
    """the six stages through ops for the batch rows ``idx``: the first three over the whole split, as a resident upload runs them"""
    from fusion_gcn_amd import ops
    rows, di, batch_rows = torch.arange(N, device=DEV), idx.to(DEV), torch.arange(len(idx), device=DEV)
    skel, imu = (guarded.to(torch.from_numpy(arrays[k]), DEV) for k in ("skeleton", "inertial"))
    src_len, dst_len = (torch.from_numpy(frames[k].astype(np.int32)).to(DEV) for k in ("inertial", "skeleton"))
    kept = ops.clip_bodies(skel, rows, bodies=M)[0]
    norm = ops.clip_normalize(kept, rows, **NORM)[0]
    feats = {"inertial": ops.signal_prepare(imu, rows, src_len, dst_len, T)[0], "skeleton": ops.imu_enhance(norm, rows, imu, rows, src_len, dst_len)}
    window, augment, streams = st["window"], st["augment"], st["streams"]
    out = {}
    for k, v in feats.items():
        v, _ = ops.clip_window(v, di, di, window=W, interval=window.interval, mode="random", seed=SEED, epoch=EPOCH, site=window.site, valid=dst_len)
        out[k], _ = ops.clip_augment(v, batch_rows, di, seed=SEED, epoch=EPOCH, site=augment.site, max_angle=augment.max_angle, scale=augment.scale,
                                     min_window=augment.min_window, joints=augment.joint_range(v.shape[1:]))
    got = ops.clip_streams(out.pop("skeleton"), batch_rows, PARENTS, streams=streams.streams)
    out.update({i: got[s] for s, i in streams.output_ids("skeleton").items()})
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def test_the_six_stages_resident_streaming_and_by_hand_are_the_same_bits(tmp_path):
    from fusion_gcn_amd.data import ClipBatches
    ds, arrays, frames = _split(str(tmp_path))
    passes, its = [], []
    for resident in (True, False):
        it = ClipBatches(ds, BS, shuffle=True, seed=SEED, device=DEV, resident=resident, **_stages(frames))
        it.set_epoch(EPOCH)
        passes.append([({k: v.cpu() for k, v in feats.items()}, lab.cpu(), idx.clone()) for feats, lab, idx in it])
        torch.cuda.synchronize()
        its.append(it)
    res, stream = its
    assert res.resident and not stream.resident
    assert [s.name for s in res.stages] == [s.name for s in stream.stages] == ["bodies", "normalize", "inertial", "window", "augment", "streams"]
    enhanced = (M, W, V + S // 3, C)
    assert res.shapes == stream.shapes == {"inertial": (W, S), "skeleton": enhanced, "skeleton_bone": enhanced, "skeleton_motion": enhanced}
    assert res.out_keys == stream.out_keys == ["inertial", "skeleton", "skeleton_bone", "skeleton_motion"]
    assert {k: tuple(v.shape) for k, v in res.dev_feat.items()} == {"inertial": (N, T, S), "skeleton": (N, M, T, V + S // 3, C)}      # taken at upload
    assert [len(b[2]) for b in passes[0]] == [4, 4, 1]
    assert sorted(int(i) for b in passes[0] for i in b[2]) == list(range(N)) and passes[0][0][2].tolist() != [0, 1, 2, 3]
    st = _stages(frames)
    for (a, lab, idx), (b, lab2, idx2) in zip(*passes):
        assert torch.equal(idx, idx2) and torch.equal(lab, lab2) and list(a) == list(b) == res.out_keys
        want = _by_hand(arrays, frames, idx, st)
        for k in a:
            assert a[k].shape == (len(idx), *res.shapes[k]) and not torch.isnan(a[k]).any(), k
            assert torch.equal(a[k], b[k]), f"{k}: the resident and the streaming pass differ"
            assert torch.equal(a[k], want[k]), f"{k}: ClipBatches and the six ops calls differ"
