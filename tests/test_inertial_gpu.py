"""fgcn_signal_prepare and fgcn_imu_enhance on the device against the golden vectors recorded from the reference
(tests/golden/inertial.npz) and the restatement of tests/inertial_ref.py.  Every comparison is exact -- the steps are integer arithmetic,
correctly rounded float32 arithmetic or copies -- so there is no tolerance to derive.  The shapes are the smallest at which the kernels
can go wrong: rows of 21 and 27 floats (no 16-byte alignment), 78 elements of a signal (more than a wavefront, less than the
workgroup), 768 elements (a lane owns several), one appended joint, two coordinates, two bodies; recordings whose row is longer than
the recording end in NaN, so a frame read behind the recording shows.  Then the promises of ClipBatches: the same bits on the resident
and the streaming path, preparation behind the normalisation and in front of the augmentation, and a model fed from raw recordings."""
import os

import numpy as np
import pytest
import torch

import inertial_ref as R
from test_inertial import CASES, IDS, normalised

import guarded
from guarded import guarded_allocations  # noqa: F401  (the fixture)

# every test runs on guarded allocations: NaN around each tensor the host layer creates, margins verified at teardown (tests/guarded.py)
pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_allocations")]
DEV = torch.device("cuda:0")


def _f(a):
    return guarded.to(torch.as_tensor(np.ascontiguousarray(a)), DEV)


def _i(a, dtype):
    return torch.as_tensor(np.asarray(a), dtype=dtype).to(DEV)


def _rows(recordings, L):
    """recordings of different lengths -> (rows, L, S) float32, NaN behind each recording (never to be read), and their lengths"""
    out = np.full((len(recordings), L, recordings[0].shape[1]), np.nan, dtype=np.float32)
    for r, x in enumerate(recordings):
        out[r, :len(x)] = x
    return out, [len(x) for x in recordings]


def _signal(src, idx, li, ls, T, **kw):
    from fusion_gcn_amd import ops
    out, stats = ops.signal_prepare(_f(src), torch.as_tensor(idx, dtype=torch.int64), _i(li, torch.int32), _i(ls, torch.int32), T, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy(), stats.cpu().numpy()


def _enhance(skel, skel_idx, imu, imu_idx, li, ls):
    from fusion_gcn_amd import ops
    out = ops.imu_enhance(_f(skel), torch.as_tensor(skel_idx, dtype=torch.int64), _f(imu), torch.as_tensor(imu_idx, dtype=torch.int64),
                          _i(li, torch.int32), _i(ls, torch.int32))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _same(a, b):
    """value for value (-0 == +0, as numpy's min may return either zero), NaN where NaN"""
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_golden_case(case):
    """every golden case as a one-row source, for both kernels: values, stats and dtypes"""
    Li, Ls, T = case["Li"], case["Ls"], case["T"]
    src, _ = _rows([case["imu"]], Li + 2)
    out, stats = _signal(src, [0], [Li], [Ls], T)
    assert out.dtype == np.float32 and stats.dtype == np.float32 and out.shape == (1, *case["signal"].shape) and stats.shape == (1, 2)
    assert _same(out[0], case["signal"])
    mn = case["padded"].min()
    assert stats[0].tolist() == [mn, (case["padded"] - mn).max()]
    raw, stats = _signal(src, [0], [Li], [Ls], T, minmax=False)
    assert _same(raw[0], case["padded"]) and stats[0].tolist() == [0.0, 1.0]
    enh = _enhance(normalised(case)[None], [0], src, [0], [Li], [Ls])
    assert enh.dtype == np.float32 and _same(enh[0], case["enhanced"])


@pytest.mark.parametrize("M,T,V,C,S,L", [(2, 13, 7, 3, 6, 29), (1, 13, 7, 2, 6, 29), (1, 128, 20, 3, 6, 326), (1, 13, 7, 3, 3, 29)])
def test_shapes_with_repeated_unsorted_rows(M, T, V, C, S, L):
    """five source rows, gathered as [4, 0, 4] (the signal) and [1, 3, 1] (the skeleton); two calls give the same bits"""
    rng = np.random.default_rng(M * 1000 + T + V + C + S)
    lengths = [(L, T), (T - 2, T - 2), (2, T), (L - 1, 2), (L, T - 3)]       # (Li, Ls): full, equal, upsampling from two, two frames, padded
    imu, li = _rows([rng.standard_normal((n, S)).astype(np.float32) for n, _ in lengths], L)
    ls = [n for _, n in lengths]
    skel = rng.standard_normal((5, M, T, V, C)).astype(np.float32)
    idx, sidx = [4, 0, 4], [1, 3, 1]
    out, stats = _signal(imu, idx, li, ls, T)
    raw, stats0 = _signal(imu, idx, li, ls, T, minmax=False)
    enh = _enhance(skel, sidx, imu, idx, li, ls)
    assert out.shape == (3, T, S) and enh.shape == (3, M, T, V + S // 3, 3)
    for k, (r, rs) in enumerate(zip(idx, sidx)):
        want, want_stats = R.signal(imu[r], li[r], ls[r], T)
        assert _same(out[k], want) and _same(stats[k], want_stats), (k, r)
        assert _same(raw[k], R.padded(imu[r], li[r], ls[r], T)) and stats0[k].tolist() == [0.0, 1.0]
        assert _same(enh[k], R.enhanced(skel[rs], imu[r], li[r], ls[r])), (k, r, rs)
    assert np.isfinite(out).all() and np.isfinite(enh).all()                 # nothing behind a recording was read
    again, again_stats = _signal(imu, idx, li, ls, T)
    assert np.array_equal(out.view(np.uint8), again.view(np.uint8)) and np.array_equal(stats.view(np.uint8), again_stats.view(np.uint8))
    assert np.array_equal(enh.view(np.uint8), _enhance(skel, sidx, imu, idx, li, ls).view(np.uint8))
    # every row once, in order: the remaining length pairs
    out, stats = _signal(imu, list(range(5)), li, ls, T)
    enh = _enhance(skel, list(range(5)), imu, list(range(5)), li, ls)
    for r in range(5):
        want, want_stats = R.signal(imu[r], li[r], ls[r], T)
        assert _same(out[r], want) and _same(stats[r], want_stats) and _same(enh[r], R.enhanced(skel[r], imu[r], li[r], ls[r])), r


def test_constant_and_single_frame_recordings():
    """a constant array gives 0 / 0 as in the reference; Ls == 1 == Li reads frame 0; lengths outside the contract are clamped"""
    imu = np.zeros((3, 5, 3), dtype=np.float32)
    imu[1] = 2.5
    imu[2] = np.arange(15, dtype=np.float32).reshape(5, 3) + 1
    out, stats = _signal(imu, [0, 1, 2], [5, 5, 1], [4, 4, 1], 4)
    assert np.isnan(out[0]).all() and stats[0].tolist() == [0.0, 0.0]        # all zero: 0 / 0
    assert np.isnan(out[1]).all() and stats[1].tolist() == [2.5, 0.0]        # constant with Ls == T
    want, want_stats = R.signal(imu[2], 1, 1, 4)
    assert _same(out[2], want) and _same(stats[2], want_stats) and out[2, 0, 2] == 1.0 and not out[2, 1:].any()
    one, _ = _signal(imu, [2], [5, 5, 99], [4, 4, 0], 4, minmax=False)        # row 2: clamped into [1, L] and [1, T]
    four, _ = _signal(imu, [2], [5, 5, 99], [4, 4, 99], 4, minmax=False)
    assert _same(one[0], R.padded(imu[2], 5, 1, 4)) and _same(four[0], R.padded(imu[2], 5, 4, 4))


def test_wrapper_refusals():
    from fusion_gcn_amd import _lib, ops
    imu, skel = torch.zeros(5, 29, 6, device=DEV), torch.zeros(5, 2, 13, 7, 3, device=DEV)
    lens = torch.ones(5, dtype=torch.int32, device=DEV)
    with pytest.raises(_lib.FgcnError, match="rows outside"):
        ops.signal_prepare(imu, torch.tensor([5]), lens, lens, 13)
    with pytest.raises(_lib.FgcnError, match="rows outside"):
        ops.imu_enhance(skel, torch.tensor([0]), imu, torch.tensor([-1]), lens, lens)
    with pytest.raises(_lib.FgcnError, match="int64"):
        ops.signal_prepare(imu, torch.arange(5, dtype=torch.int32), lens, lens, 13)
    with pytest.raises(_lib.FgcnError, match="int32"):
        ops.signal_prepare(imu, torch.arange(5), lens.long(), lens, 13)
    with pytest.raises(_lib.FgcnError, match="int32"):
        ops.imu_enhance(skel, torch.arange(5), imu, torch.arange(5), lens, lens[:4])
    same = torch.zeros(5, 13, 6, device=DEV)
    with pytest.raises(_lib.FgcnError, match="alias"):
        ops.signal_prepare(same, torch.arange(5), lens, lens, 13, out=same)
    with pytest.raises(_lib.FgcnError, match="signal rows"):
        ops.imu_enhance(skel, torch.arange(5), imu, torch.arange(4), lens, lens)
    with pytest.raises(_lib.FgcnError, match="joints of three"):
        ops.imu_enhance(skel, torch.arange(5), torch.zeros(5, 29, 4, device=DEV), torch.arange(5), lens, lens)
    with pytest.raises(_lib.FgcnError, match="for a batch of"):
        ops.imu_enhance(skel, torch.arange(5), imu, torch.arange(5), lens, lens, out=torch.zeros(5, 2, 13, 9, 2, device=DEV))


# ---- ClipBatches ----------------------------------------------------------------------------------------------------------------------
BS, N, L = 4, 10, 29
SEVEN = [c for c in CASES if c["skel"].shape == (1, 13, 7, 3) and c["imu"].shape[1] == 6]      # they share their shapes and joint numbers
KW7 = dict(origin_joint=SEVEN[0]["origin"], z_axis_joints=SEVEN[0]["z"], x_axis_joints=SEVEN[0]["x"])


@pytest.fixture(scope="module")
def raw_dataset(tmp_path_factory):
    """ten raw samples -- the (1, 13, 7, 3) golden cases, then drawn ones -- written with NumpyWriter: skeletons that are zero behind
    their Ls frames, recordings in rows of L = 29 frames that are zero behind their Li frames (as a raw export pads them)"""
    from fusion_gcn_amd.data import MultiModalDataset, NumpyDatasetLoader, NumpyWriter
    root = str(tmp_path_factory.mktemp("inertial"))
    rng = np.random.default_rng(11)
    assert len(SEVEN) >= 5
    skel = np.zeros((N, 1, 13, 7, 3), dtype=np.float32)
    imu = np.zeros((N, L, 6), dtype=np.float32)
    ls, li = np.zeros(N, dtype=np.int64), np.zeros(N, dtype=np.int64)
    for r in range(N):
        if r < len(SEVEN):
            c = SEVEN[r]
            skel[r], ls[r], li[r] = c["skel"], c["Ls"], c["Li"]
            imu[r, :li[r]] = c["imu"]
        else:
            ls[r], li[r] = rng.integers(2, 14), rng.integers(2, L + 1)
            skel[r, :, :ls[r]] = rng.uniform(0.5, 3.0, (1, ls[r], 7, 3))
            imu[r, :li[r]] = rng.standard_normal((li[r], 6))
    for name, a in (("skeleton", skel), ("inertial", imu)):
        with NumpyWriter(os.path.join(root, f"{name}_train_features.npy"), np.float32, a.shape) as w:
            for s in a:
                w.collect_next(s)
    np.save(os.path.join(root, "train_labels.npy"), np.arange(N) % 5)
    return MultiModalDataset([(root, NumpyDatasetLoader())], "train"), skel, imu, {"skeleton": ls, "inertial": li}


@pytest.fixture(scope="module")
def prepared(raw_dataset):
    """what the batches must hold: ops.clip_normalize on the raw skeletons, then the restatement -- computed once, left unchanged"""
    from fusion_gcn_amd import ops
    _, skel, imu, frames = raw_dataset
    norm, _, _ = ops.clip_normalize(torch.from_numpy(skel).to(DEV), torch.arange(N), **KW7)
    norm = norm.cpu().numpy()
    ls, li = frames["skeleton"], frames["inertial"]
    signal = np.stack([R.signal(imu[r], li[r], ls[r], 13)[0] for r in range(N)])
    enhanced = np.stack([R.enhanced(norm[r], imu[r], li[r], ls[r]) for r in range(N)])
    for r, c in enumerate(SEVEN):                            # and the golden arrays where the sample is a golden case
        assert _same(signal[r], c["signal"]) and _same(enhanced[r, :, :, 7:], c["enhanced"][:, :, 7:])
    return torch.from_numpy(norm), torch.from_numpy(signal), torch.from_numpy(enhanced)


def _batches(ds, frames, resident, **kw):
    from fusion_gcn_amd.data import ClipBatches, Inertial, Normalize
    aug = kw.pop("augment", None)
    it = ClipBatches(ds, BS, shuffle=True, seed=5, device=DEV, resident=resident, normalize=Normalize(**KW7, only=["skeleton"]),
                     inertial=Inertial(frames=frames, **kw), augment=aug)
    it.set_epoch(2)
    out = []
    for feats, lab, idx in it:
        feats = feats if isinstance(feats, dict) else {"_": feats}
        out.append(({k: v.cpu().clone() for k, v in feats.items()}, lab.cpu().clone(), idx.clone()))
    torch.cuda.synchronize()
    return it, out


def _bits(t):
    return t.contiguous().view(torch.int32)


def test_clip_batches_resident_and_streaming_deliver_the_prepared_rows(raw_dataset, prepared):
    ds, _, _, frames = raw_dataset
    norm, signal, enhanced = prepared
    (res_it, res), (str_it, stream) = _batches(ds, frames, True, enhance=True), _batches(ds, frames, False, enhance=True)
    assert res_it.resident and not str_it.resident and [len(b[2]) for b in res] == [4, 4, 2] and len(stream) == 3
    assert res_it.dev_feat["inertial"].shape == (N, 13, 6) and res_it.dev_feat["skeleton"].shape == (N, 1, 13, 9, 3)      # prepared at upload
    assert str_it.last_inertial.shape == (2, 2) and res_it.last_inertial.shape == (N, 2)
    for a, b in zip(res, stream):
        assert torch.equal(a[2], b[2]) and torch.equal(a[1], b[1]) and list(a[0]) == list(b[0]) == ["inertial", "skeleton"]
        for k, want in (("inertial", signal), ("skeleton", enhanced)):
            assert a[0][k].dtype == torch.float32
            assert torch.equal(_bits(a[0][k]), _bits(b[0][k])), k                              # the same bits on both paths
            assert torch.equal(a[0][k], want[a[2]]), k                                         # clip_normalize, then the restatement
    # without enhance the skeleton is the normalised one; without minmax the signal is resampled and padded only
    _, plain = _batches(ds, frames, False, minmax=False)
    for feats, _, idx in plain:
        assert torch.equal(_bits(feats["skeleton"]), _bits(norm[idx]))
        assert torch.equal(feats["inertial"], enhanced[idx][:, 0, :, 7:].reshape(len(idx), 13, 6))


@pytest.mark.parametrize("resident", [True, False])
def test_drop_signal_yields_a_tensor_and_identity_augmentation_the_prepared_batch(raw_dataset, prepared, resident):
    from fusion_gcn_amd.data import Augment
    ds, _, _, frames = raw_dataset
    _, signal, enhanced = prepared
    it, got = _batches(ds, frames, resident, enhance=True, drop_signal=True)
    assert it.out_keys == ["skeleton"] and it.last_inertial is None
    for feats, _, idx in got:
        assert list(feats) == ["_"] and torch.equal(feats["_"], enhanced[idx])                 # a tensor, not a dict
    # identity parameters: the augmentation sees the prepared shapes (joints (0, 7) of nine) and returns the prepared batch
    aug = Augment(max_angle=(0.0, 0.0, 0.0), scale=0.0, min_window=1.0, joints=(0, 7))
    it, got = _batches(ds, frames, resident, enhance=True, augment=aug)
    assert set(it.last_params) == {"skeleton", "inertial"} and it.shapes == {"inertial": (13, 6), "skeleton": (1, 13, 9, 3)}
    for feats, _, idx in got:
        assert torch.equal(feats["skeleton"], enhanced[idx]) and torch.equal(feats["inertial"], signal[idx])
    # and with magnitudes it moves the skeleton joints and leaves the appended ones to the temporal part alone
    it, got = _batches(ds, frames, resident, enhance=True, augment=Augment(joints=(0, 7), min_window=1.0))
    for feats, _, idx in got:
        assert not torch.equal(feats["skeleton"][:, :, :, :7], enhanced[idx][:, :, :, :7])
        assert torch.equal(feats["skeleton"][:, :, :, 7:], enhanced[idx][:, :, :, 7:])


def test_three_stages_compose_in_order_on_both_paths_and_across_ranks(raw_dataset):
    """all three stages with real magnitudes, shuffled, epoch 2, batches of 4, 4, 2 (two slots, a ragged tail, a key whose shape a stage
    changes): the resident and the streaming path deliver the same bits, two ranks (one resident, one streaming) concatenate to the
    one-rank batches, and every batch is the stages composed by hand through ops -- normalise, prepare, augment"""
    from fusion_gcn_amd import ops
    from fusion_gcn_amd.data import Augment, ClipBatches, Inertial, Normalize
    ds, skel, imu, frames = raw_dataset
    Ls = frames["skeleton"]
    aug = Augment(joints=(0, 7), valid_frames={"skeleton": Ls, "inertial": Ls})      # its default angles, scale and window

    def epoch(resident, rank=0, world=1):
        it = ClipBatches(ds, BS, shuffle=True, seed=5, rank=rank, world=world, device=DEV, resident=resident,
                         normalize=Normalize(**KW7, only=["skeleton"]), inertial=Inertial(frames=frames, enhance=True),
                         augment=aug)
        it.set_epoch(2)
        out = []
        for feats, lab, idx in it:
            assert list(feats) == ["inertial", "skeleton"] and set(it.last_params) == set(feats)
            out.append(({k: v.cpu().clone() for k, v in feats.items()}, lab.cpu().clone(), idx.clone(),
                        {k: v.cpu().clone() for k, v in it.last_params.items()}))
        torch.cuda.synchronize()
        assert it.resident == resident
        return it, out

    def same(a, b):
        return (torch.equal(a[2], b[2]) and torch.equal(a[1], b[1])
                and all(torch.equal(_bits(a[0][k]), _bits(b[0][k])) and torch.equal(_bits(a[3][k]), _bits(b[3][k])) for k in a[0]))

    (it, res), (_, stream) = epoch(True), epoch(False)
    assert [len(b[2]) for b in res] == [4, 4, 2] and len(stream) == 3
    assert all(same(a, b) for a, b in zip(res, stream))
    # 1. == 2.: the ranks' shards, one rank resident and one streaming, are the halves of the one-rank batches
    (_, r0), (_, r1) = epoch(True, 0, 2), epoch(False, 1, 2)
    assert len(r0) == len(r1) == 3
    for one, a, b in zip(res, r0, r1):
        both = ({k: torch.cat([a[0][k], b[0][k]]) for k in one[0]}, torch.cat([a[1], b[1]]), torch.cat([a[2], b[2]]),
                {k: torch.cat([a[3][k], b[3][k]]) for k in one[3]})
        assert same(one, both)
    # 3. the stages by hand, in order
    raw_skel, raw_imu = _f(skel), _f(imu)
    li, ls = _i(frames["inertial"], torch.int32), _i(Ls, torch.int32)
    assert it.shapes == {"inertial": (13, 6), "skeleton": (1, 13, 9, 3)}
    for feats, _, idx, params in res:
        b = len(idx)
        norm, _, _ = ops.clip_normalize(raw_skel, idx, **KW7)
        signal, _ = ops.signal_prepare(raw_imu, idx, li, ls, 13)
        enhanced = ops.imu_enhance(norm, torch.arange(b), raw_imu, idx, li, ls)
        valid = _i(Ls[idx.numpy()], torch.int32)
        for k, src, joints in (("skeleton", enhanced, (0, 7)), ("inertial", signal, None)):
            want, want_params = ops.clip_augment(src, torch.arange(b), idx, seed=5, epoch=2, site=0, max_angle=aug.max_angle, scale=aug.scale,
                                                 min_window=aug.min_window, joints=joints, valid=valid)
            assert torch.equal(_bits(feats[k]), _bits(want.cpu())), k
            assert torch.equal(_bits(params[k]), _bits(want_params.cpu())), k


def test_clip_batches_refuses_what_it_cannot_prepare(raw_dataset):
    from fusion_gcn_amd import _lib
    from fusion_gcn_amd.data import Augment, ClipBatches, Inertial
    ds, _, _, frames = raw_dataset
    with pytest.raises(ValueError, match="does not have"):
        ClipBatches(ds, BS, device=DEV, inertial=Inertial(frames={"pose": frames["skeleton"], "inertial": frames["inertial"]}, main="pose"))
    with pytest.raises(ValueError, match=r"in \[1, 13\]"):
        ClipBatches(ds, BS, device=DEV, inertial=Inertial(frames={**frames, "skeleton": frames["skeleton"] + 12}))
    with pytest.raises(ValueError, match="expected 10 frame counts"):
        ClipBatches(ds, BS, device=DEV, inertial=Inertial(frames={k: v[:9] for k, v in frames.items()}))
    with pytest.raises(ValueError, match="joints"):                          # nine joints after the preparation, not ten
        ClipBatches(ds, BS, device=DEV, inertial=Inertial(frames=frames, enhance=True), augment=Augment(joints=(0, 10)))
    with pytest.raises(_lib.FgcnError, match="expected"):
        ClipBatches(ds, BS, device=DEV, inertial=Inertial(frames=frames, main="inertial", signal="skeleton"))


def test_model_fed_from_raw_recordings():
    """mmargcn, mode skeleton_imu_spatial_fusion (UTD-MHAD graph, two IMU joints, N = 2, T = 16): the logits of a batch ClipBatches
    prepared from raw recordings are, bit for bit, those of the golden enhanced array.  The two clips are normalised without an axis
    pair: the centred values are exact in float32, where a rotation is held to 2^-23 (section 8g)."""
    import tempfile

    from fusion_gcn_amd.data import ClipBatches, Inertial, MultiModalDataset, Normalize, NumpyDatasetLoader, NumpyWriter
    from fusion_gcn_amd.datasets.utd_mhad import constants as utd
    from fusion_gcn_amd.util import Graph
    from fusion_gcn_amd.util.dynamic_import import import_model
    from oracle import filler
    two = [c for c in CASES if c["skel"].shape == (1, 16, 20, 3)]
    assert len(two) == 2 and all(c["z"] is None and c["x"] is None and c["origin"] == utd.skeleton_center_joint for c in two)
    imu, li = _rows([c["imu"] for c in two], 48)
    imu = np.nan_to_num(imu, nan=0.0)
    frames = {"skeleton": np.array([c["Ls"] for c in two]), "inertial": np.array(li)}
    with tempfile.TemporaryDirectory() as root:
        for name, a in (("skeleton", np.stack([c["skel"] for c in two])), ("inertial", imu)):
            with NumpyWriter(os.path.join(root, f"{name}_val_features.npy"), np.float32, a.shape) as w:
                for s in a:
                    w.collect_next(s)
        np.save(os.path.join(root, "val_labels.npy"), np.array([3, 7]))
        ds = MultiModalDataset([(root, NumpyDatasetLoader(in_memory=True))], "val")
        it = ClipBatches(ds, 2, device=DEV, normalize=Normalize(utd.skeleton_center_joint, only=["skeleton"]),
                         inertial=Inertial(frames=frames, enhance=True, drop_signal=True))
        (batch, labels, _), = list(it)
    gold = np.stack([c["enhanced"] for c in two])
    assert batch.shape == (2, 1, 16, 22, 3) and labels.tolist() == [3, 7]
    assert torch.equal(_bits(batch.cpu()), _bits(torch.from_numpy(gold)))
    g = Graph(utd.skeleton_edges, center_joint=utd.center_joint)
    model = import_model("mmargcn")({"skeleton": (1, 16, 22, 3)}, 27, g, mode="skeleton_imu_spatial_fusion", num_imu_joints=2,
                                    imu_enhanced_mode="append_center")
    filler.fill_state_dict(model.state_dict(), rename=lambda k: k.replace("_model.agcn.", ""))
    model = guarded.to(model, DEV).eval()
    with torch.no_grad():
        from_raw, from_gold = model(batch), model(_f(gold))
    assert from_raw.shape == (2, 27) and bool(torch.isfinite(from_raw).all())
    assert torch.equal(_bits(from_raw.cpu()), _bits(from_gold.cpu()))
