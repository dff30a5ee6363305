"""fgcn_clip_normalize on the device against the golden vectors recorded from the reference
(tests/golden/normalize.npz) and the restatement of tests/normalize_ref.py: the frame map and the flags exactly, R to 1e-12, the result
value for value where nothing is rotated and within 2^-23 max|gold64| where something is (one float32 rounding is 2^-24; the float64
parameter differences are of order 1e-15 at the golden angles; tests/test_normalize.py has the derivation).  The shapes are the smallest
at which the kernels can go wrong: a row of 21 floats (84 bytes, no 16-byte alignment), an odd frame count, a scan that crosses two
wavefront boundaries, clips long enough that a lane of the plan kernel owns several frames, 64 joints, two coordinates.  Then the
promises of ClipBatches: the same bits on the resident and the streaming path, and augmentation reads the normalised clips."""
import numpy as np
import pytest
import torch

import normalize_ref as N
from test_normalize import CASES

import guarded
from guarded import guarded_allocations  # noqa: F401  (the fixture)

# every test runs on guarded allocations: NaN around each tensor the host layer creates, margins verified at teardown (tests/guarded.py)
pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_allocations")]
DEV = torch.device("cuda:0")


def _kw(origin, zp, xp):
    return dict(origin_joint=origin, z_axis_joints=zp, x_axis_joints=xp)


def _run(src, idx, **kw):
    from fusion_gcn_amd import ops
    out, frame_map, params = ops.clip_normalize(guarded.to(torch.as_tensor(src), DEV), torch.as_tensor(idx, dtype=torch.int64), **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy(), frame_map.cpu().numpy(), params.cpu().numpy()


@pytest.fixture(scope="module")
def device_results():
    """every golden case once, as a one-row source: name -> (out, frame_map, params)"""
    return {name: _run(x[None], [0], **_kw(origin, zp, xp)) for name, x, origin, zp, xp, *_ in CASES}


def _check(name, got, x, origin, zp, xp, gold=None, centred=None):
    """one clip's (out, frame_map, params) against the restatement and, where given, the reference's arrays"""
    out, frame_map, params = got
    want = N.normalize(x, origin, zp, xp)
    assert out.dtype == np.float32 and frame_map.dtype == np.int32 and params.dtype == np.float64
    assert np.array_equal(frame_map, want["frame_map"]), name
    assert params[9:12].tolist() == want["params"][9:12].tolist(), name
    assert np.abs(params[:9] - want["params"][:9]).max() <= 1e-12, name
    if not params[9] and not params[10]:
        assert np.array_equal(params[:9].reshape(3, 3), np.eye(3))
        assert np.array_equal(out, want["centred"] if centred is None else centred), name        # value for value (-0 == +0)
        return
    ref64 = want["out64"] if gold is None else gold
    bound = N.U23 * np.abs(ref64).max()
    err = np.abs(out.astype(np.float64) - ref64).max()
    print(f"[normalize] {name}: max error {err:.3e}, bound {bound:.3e} ({err / bound:.3f} of it)")
    assert err <= bound, (name, err, bound)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_golden_case(device_results, case):
    name, x, origin, zp, xp, centred, gold, applied = case
    out, frame_map, params = device_results[name]
    assert out.shape == (1, *x.shape) and frame_map.shape == (1, *x.shape[:2]) and params.shape == (1, 12)
    assert params[0, 9:11].tolist() == applied
    _check(name, (out[0], frame_map[0], params[0]), x, origin, zp, xp, gold=gold, centred=centred)


SEVEN = [c for c in CASES if c[1].shape == (2, 13, 7, 3)]          # they share their joint numbers
KW7 = _kw(*SEVEN[0][2:5])


def test_gather_of_repeated_unsorted_rows(device_results):
    five = SEVEN[1:6]
    src = np.stack([c[1] for c in five])
    out, frame_map, params = _run(src, [4, 0, 4], **KW7)
    assert out.shape == (3, 2, 13, 7, 3)
    for k, row in enumerate((4, 0, 4)):
        single = device_results[five[row][0]]
        assert np.array_equal(out[k], single[0][0]) and np.array_equal(frame_map[k], single[1][0]) and np.array_equal(params[k], single[2][0])


def test_two_calls_give_the_same_bits():
    src = np.stack([c[1] for c in SEVEN])
    idx = list(range(len(SEVEN)))[::-1]
    a, b = _run(src, idx, **KW7), _run(src, idx, **KW7)
    assert all(np.array_equal(p.view(np.uint8), q.view(np.uint8)) for p, q in zip(a, b))


@pytest.mark.parametrize("T", [300, 1031])
def test_long_clips_where_a_lane_owns_several_frames(T):
    """T above the plan kernel's 256 lanes (2 and 5 frames per lane, the last lanes empty): compaction, a kept interior null, an invalid
    body, against the restatement"""
    rng = np.random.default_rng(T)
    x = rng.uniform(0.5, 3.0, (3, 3, T, 5, 3)).astype(np.float32)
    x[0, 0, :7] = 0                                                # clip 0, body 0: leading, scattered and trailing nulls
    x[0, 0, rng.choice(np.arange(7, T), T // 3, replace=False)] = 0
    x[0, 0, T - 40:] = 0
    x[0, 1, 100] = 0                                               # body 1: an interior null that stays, trailing nulls
    x[0, 1, T - 129:] = 0
    x[0, 2] = 0                                                    # body 2: invalid
    x[1, 0, 1:] = 0                                                # clip 1: one frame, replicated T - 1 times
    x[1, 1, :T - 1] = 0                                            # the last frame alone: compaction to f = 1
    x[1, 2, 255:257] = 0                                           # nulls across a lane / wavefront boundary
    out, frame_map, params = _run(x, [2, 1, 0], origin_joint=1, z_axis_joints=(0, 1), x_axis_joints=(2, 4))
    for k, row in enumerate((2, 1, 0)):
        _check(f"T={T} clip {row}", (out[k], frame_map[k], params[k]), x[row], 1, (0, 1), (2, 4))
    assert params[:, 11].tolist() == [3.0, 3.0, 2.0]


def test_wrapper_refusals():
    from fusion_gcn_amd import _lib, ops
    src = torch.zeros(5, 2, 13, 7, 3, device=DEV)
    with pytest.raises(_lib.FgcnError, match="rows outside"):
        ops.clip_normalize(src, torch.tensor([5]), **KW7)
    with pytest.raises(_lib.FgcnError, match="rows outside"):
        ops.clip_normalize(src, torch.tensor([0, -1]), **KW7)
    with pytest.raises(_lib.FgcnError, match="alias"):
        ops.clip_normalize(src, torch.arange(5), out=src, **KW7)
    with pytest.raises(_lib.FgcnError, match="axis joints"):
        ops.clip_normalize(src, torch.arange(5), origin_joint=1, z_axis_joints=(3, 7))
    with pytest.raises(_lib.FgcnError, match="int64"):
        ops.clip_normalize(src, torch.arange(5, dtype=torch.int32), **KW7)


def test_more_frames_than_the_limit_are_refused():
    from fusion_gcn_amd import _lib, ops
    src = torch.zeros(1, 1, _lib.NORMALIZE_MAX_T + 1, 1, 3, device=DEV)
    with pytest.raises(_lib.FgcnError, match="frames, at most"):
        ops.clip_normalize(src, torch.arange(1), origin_joint=0)
    ok = torch.ones(1, 1, _lib.NORMALIZE_MAX_T, 1, 3, device=DEV)            # the limit itself is taken
    out, frame_map, _ = ops.clip_normalize(ok, torch.arange(1), origin_joint=0)
    assert torch.equal(frame_map[0, 0].cpu(), torch.arange(_lib.NORMALIZE_MAX_T, dtype=torch.int32)) and not bool(out.any())


# ---- ClipBatches ----------------------------------------------------------------------------------------------------------------------
BS = 4


@pytest.fixture(scope="module")
def raw_dataset(tmp_path_factory):
    """ten raw clips (the first ten (2, 13, 7, 3) golden inputs) written with NumpyWriter, and an inertial signal beside them"""
    import os

    from fusion_gcn_amd.data import MultiModalDataset, NumpyDatasetLoader, NumpyWriter
    root = str(tmp_path_factory.mktemp("normalize"))
    clips = np.stack([c[1] for c in SEVEN[:10]])
    inertial = np.random.default_rng(3).standard_normal((10, 11, 6)).astype(np.float32)
    for name, a in (("skeleton", clips), ("inertial", inertial)):
        with NumpyWriter(os.path.join(root, f"{name}_train_features.npy"), np.float32, a.shape) as w:
            for s in a:
                w.collect_next(s)
    np.save(os.path.join(root, "train_labels.npy"), np.arange(10) % 5)
    return MultiModalDataset([(root, NumpyDatasetLoader())], "train"), clips, inertial


def _norm():
    from fusion_gcn_amd.data import Normalize
    return Normalize(**KW7, only=["skeleton"])


def _epoch(ds, **kw):
    from fusion_gcn_amd.data import ClipBatches
    it = ClipBatches(ds, BS, shuffle=True, seed=5, device=DEV, normalize=_norm(), **kw)
    it.set_epoch(2)
    out = []
    for feats, lab, idx in it:
        assert set(it.last_plan) == {"skeleton"}
        out.append(({k: v.cpu() for k, v in feats.items()}, lab.cpu(), idx.clone()))
    torch.cuda.synchronize()
    return it, out


def test_clip_batches_resident_and_streaming_deliver_the_normalised_rows(raw_dataset):
    from fusion_gcn_amd import ops
    from fusion_gcn_amd.data import Normalize
    ds, clips, inertial = raw_dataset
    want, _, _ = ops.clip_normalize(guarded.to(torch.from_numpy(clips), DEV), torch.arange(10), **KW7)
    want = want.cpu()
    (res_it, res), (str_it, stream) = _epoch(ds, resident=True), _epoch(ds, resident=False)
    assert res_it.resident and not str_it.resident and [len(b[2]) for b in res] == [4, 4, 2]
    assert torch.equal(res_it.dev_feat["skeleton"].cpu(), want)              # normalised once, at upload
    assert str_it.last_plan["skeleton"][0].shape == (2, 2, 13) and str_it.last_plan["skeleton"][1].shape == (2, 12)
    for a, b in zip(res, stream):
        assert torch.equal(a[2], b[2]) and torch.equal(a[1], b[1])
        assert torch.equal(a[0]["skeleton"].view(torch.int32), b[0]["skeleton"].view(torch.int32))
        assert torch.equal(a[0]["skeleton"].view(torch.int32), want[a[2]].view(torch.int32))
        assert torch.equal(a[0]["inertial"], torch.from_numpy(inertial)[a[2]]) and torch.equal(b[0]["inertial"], a[0]["inertial"])
    z = Normalize.for_dataset("utd_mhad")
    assert (z.origin_joint, z.z_axis_joints, z.x_axis_joints) == (2, (3, 2), (4, 8))


@pytest.mark.parametrize("resident", [True, False])
def test_augmentation_reads_the_normalised_clips(raw_dataset, resident):
    from fusion_gcn_amd import ops
    from fusion_gcn_amd.data import Augment, ClipBatches
    ds, clips, _ = raw_dataset
    normalised, _, _ = ops.clip_normalize(guarded.to(torch.from_numpy(clips), DEV), torch.arange(10), **KW7)
    aug = Augment(only=["skeleton"])
    it = ClipBatches(ds, BS, shuffle=True, seed=5, device=DEV, resident=resident, normalize=_norm(), augment=aug)
    it.set_epoch(2)
    seen = 0
    for feats, _, idx in it:
        want, table = ops.clip_augment(normalised, idx, idx, seed=5, epoch=2, site=aug.site, max_angle=aug.max_angle, scale=aug.scale,
                                       min_window=aug.min_window, joints=(0, 7))
        assert torch.equal(feats["skeleton"].view(torch.int32), want.view(torch.int32)) and torch.equal(it.last_params["skeleton"], table)
        assert not torch.equal(feats["skeleton"], normalised[guarded.to(idx, DEV)])
        seen += len(idx)
    assert seen == 10


def test_clip_batches_refuses_what_it_cannot_normalise(raw_dataset):
    from fusion_gcn_amd import _lib
    from fusion_gcn_amd.data import ClipBatches, Normalize
    ds = raw_dataset[0]
    with pytest.raises(_lib.FgcnError, match="expected \\(samples, M, T, V, C\\)"):
        ClipBatches(ds, BS, device=DEV, normalize=Normalize(**KW7))           # the inertial signal is no skeleton
    with pytest.raises(ValueError, match="does not have"):
        ClipBatches(ds, BS, device=DEV, normalize=Normalize(**KW7, only=["depth"]))
    with pytest.raises(_lib.FgcnError, match="joints"):
        ClipBatches(ds, BS, device=DEV, normalize=Normalize(2, (3, 2), (4, 8), only=["skeleton"]))      # joint 8 of 7
