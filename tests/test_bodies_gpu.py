"""fgcn_clip_bodies on the device against the golden vectors recorded from the reference (tests/golden/bodies.npz) and
the restatement of tests/bodies_ref.py: the ranking exactly, the selected bodies bit for bit, the scores within

    |scores - restatement| <= 4 n 2^-53 score,   n = |F| V, the number of terms of each of the body's sums.

Derivation: each float64 sum of n terms carries at most (n - 1) 2^-53 relative error in any order (the deviations' squares are non-negative,
and a two-pass variance is second-order insensitive to the mean's error: at the fixtures' |mean| / std < 100 that term is below 1e-20); the
factor 4 covers the square root, the division and the sum over the channels.  The shapes are the smallest at which the kernels can go
wrong: bodies of 273 floats (1092 bytes: three of four bodies of a clip have no 16-byte alignment, so both load paths run), an odd frame
count, two coordinates, sixteen bodies kept of sixteen, one value per channel, and one (4, 300, 25, 3) clip whose reduction spans every wave
with many elements per lane and whose gather takes two pieces a body.  Then the promises of ClipBatches."""
import numpy as np
import pytest
import torch

import bodies_ref as B
from test_bodies import CASES

import guarded
from guarded import guarded_allocations  # noqa: F401  (the fixture)

# every test runs on guarded allocations: NaN around each tensor the host layer creates, margins verified at teardown (tests/guarded.py)
pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_allocations")]
DEV = torch.device("cuda:0")
U53 = 2.0 ** -53


def _run(src, idx, M, out=None):
    from fusion_gcn_amd import ops
    got, order, scores = ops.clip_bodies(guarded.to(torch.as_tensor(src), DEV), torch.as_tensor(idx, dtype=torch.int64), bodies=M, out=out)
    torch.cuda.synchronize()
    return got.cpu().numpy(), order.cpu().numpy(), scores.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _check(name, got, x, M):
    """one clip's (out, order, scores) against the restatement"""
    out, order, scores = got
    want = B.scores(x)
    assert out.dtype == np.float32 and order.dtype == np.int32 and scores.dtype == np.float64
    assert out.shape == (M, *x.shape[1:]) and order.shape == (len(x),) and scores.shape == (len(x),)
    assert np.array_equal(np.isnan(scores), np.isnan(want)), name
    num = ~np.isnan(want)
    bound = 4 * B.frames_counted(x) * U53 * want
    err = np.abs(scores[num] - want[num])
    print(f"[bodies] {name}: max score error {err.max() if num.any() else 0.0:.3e}, bound {bound[num].max() if num.any() else 0.0:.3e}")
    assert np.all(err <= bound[num]), (name, scores, want)
    assert not np.signbit(scores[num]).any()
    assert np.array_equal(order, B.order(want)), (name, order, scores)
    assert np.array_equal(_bits(out), _bits(x[order[:M]])), name


@pytest.fixture(scope="module")
def device_results():
    """every golden case once, as a one-row source: name -> (out, order, scores)"""
    return {name: _run(x[None], [0], len(sel)) for name, x, _, _, sel, _ in CASES}


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_golden_case(device_results, case):
    name, x, ref_scores, ref_order, sel, tied = case
    out, order, scores = device_results[name]
    assert out.shape == (1, *sel.shape) and order.shape == (1, len(x)) and scores.shape == (1, len(x))
    _check(name, (out[0], order[0], scores[0]), x, len(sel))
    assert np.all(np.abs(scores[0] - ref_scores) <= 1e-5 * scores[0])          # the reference's float32-path values
    if not tied:
        assert np.array_equal(order[0], ref_order)
    assert np.array_equal(_bits(out[0]), _bits(sel))                           # the reference's selection, bit for bit


def _draw(rng, shape, lo=0.02, hi=0.2):
    """as the golden inputs are drawn: every body 3 + amplitude * uniform(0.5, 3), the amplitudes spread and permuted"""
    amp = rng.permutation(np.geomspace(lo, hi, shape[-4]))
    return (3.0 + amp[:, None, None, None] * rng.uniform(0.5, 3.0, shape)).astype(np.float32)


def test_large_clip_where_every_wave_reduces_and_a_lane_owns_many_elements():
    x = _draw(np.random.default_rng(20261020), (4, 300, 25, 3))
    x[1, 250:] = 0
    x[2, :3] = 0
    x[2, 100] = 0
    _check("(4, 300, 25, 3)", [a[0] for a in _run(x[None], [0], 2)], x, 2)


def test_one_value_per_channel_scores_exactly_zero():
    x = np.array([[[[1.5, -2.0, 3.25]]], [[[0.5, 0.0, -0.0]]]], dtype=np.float32)       # (2, 1, 1, 3): n = 1, every deviation is x - x
    out, order, scores = _run(x[None], [0], 2)
    assert _bits(scores).ravel().tolist() == [0] * 16 and order[0].tolist() == [1, 0] and np.array_equal(_bits(out[0]), _bits(x[[1, 0]]))
    x[0] = 0                                                                             # a null body: +0 too, the tie by the higher index
    out, order, scores = _run(x[None], [0], 1)
    assert _bits(scores).ravel().tolist() == [0] * 16 and order[0].tolist() == [1, 0] and np.array_equal(_bits(out[0]), _bits(x[[1]]))


@pytest.fixture(scope="module")
def rows67():
    """67 clips of (3, 13, 7, 3): a clip is 3276 bytes, so the rows' alignment to 16 bytes differs from row to row"""
    rng = np.random.default_rng(67)
    x = np.stack([_draw(rng, (3, 13, 7, 3)) for _ in range(67)])
    x[5, 1] = 0
    x[41, 0, :2] = 0
    x[41, 2, 6] = 0
    return x


def test_batches_of_one_and_of_67_with_repeated_unsorted_rows(rows67):
    idx = np.random.default_rng(1).permutation(67)
    idx[3] = idx[50] = idx[0]                                                            # repeated
    out, order, scores = _run(rows67, idx, 2)
    assert out.shape == (67, 2, 13, 7, 3)
    for k, row in enumerate(idx):
        _check(f"row {row} at {k}", (out[k], order[k], scores[k]), rows67[row], 2)
    one = _run(rows67, [41], 2)
    _check("b = 1", [a[0] for a in one], rows67[41], 2)
    k = idx.tolist().index(41)
    assert np.array_equal(_bits(one[2][0]), _bits(scores[k])) and np.array_equal(one[1][0], order[k])


def test_a_clip_has_the_same_score_bits_alone_and_in_a_batch_and_in_a_second_call(rows67):
    whole = _run(rows67, np.arange(67), 3)
    again = _run(rows67, np.arange(67), 3)
    assert all(np.array_equal(_bits(p), _bits(q)) for p, q in zip(whole, again))
    for row in (41, 1, 66):                                                              # (rows at three different alignments)
        alone = _run(rows67[row][None], [0], 3)
        assert np.array_equal(_bits(alone[2][0]), _bits(whole[2][row])), row
        assert np.array_equal(alone[1][0], whole[1][row]) and np.array_equal(_bits(alone[0][0]), _bits(whole[0][row]))


def test_nan_and_inf_bodies_rank_first_and_stay_visible():
    x = _draw(np.random.default_rng(9), (4, 13, 7, 3))
    x[0, 4, 2, 1] = np.nan
    x[2, 11, 6, 0] = np.inf
    out, order, scores = _run(x[None], [0], 3)
    assert np.isnan(scores[0, [0, 2]]).all() and not np.isnan(scores[0, [1, 3]]).any()
    assert order[0, :2].tolist() == [2, 0]                                               # the higher index first
    _check("nan, inf", (out[0], order[0], scores[0]), x, 3)
    x[3, 0, 0, 0] = -np.inf                                                              # inf and -inf in one channel of a third body
    x[3, 1, 0, 0] = np.inf
    out, order, scores = _run(x[None], [0], 4)
    assert order[0].tolist() == [3, 2, 0, 1]
    _check("nan, inf, -inf", (out[0], order[0], scores[0]), x, 4)


def test_minus_zero_frames_are_null():
    x = _draw(np.random.default_rng(10), (2, 13, 7, 3))
    y = x.copy()
    x[0, 3:6] = -0.0
    y[0, 3:6] = 0.0
    a, b = _run(x[None], [0], 2), _run(y[None], [0], 2)
    assert np.array_equal(_bits(a[2]), _bits(b[2])) and np.array_equal(a[1], b[1])
    _check("-0", [v[0] for v in a], x, 2)
    assert np.signbit(a[0][0][a[1][0].tolist().index(0), 3:6]).all()                     # and they are copied as they are


def test_out_is_written_in_place_and_the_wrapper_refuses():
    from fusion_gcn_amd import _lib, ops
    name, x, *_ = CASES[1]
    src = guarded.to(torch.from_numpy(np.stack([x, x[::-1]])), DEV)
    buf = torch.full((5, 2, 13, 7, 3), 7.0, device=DEV)
    out, order, scores = ops.clip_bodies(src, torch.tensor([1, 0]), bodies=2, out=buf[1:3])
    assert out.data_ptr() == buf[1:3].data_ptr()
    assert torch.equal(buf[2].cpu(), torch.from_numpy(B.select(x, 2))) and torch.equal(buf[1].cpu(), torch.from_numpy(B.select(x[::-1], 2)))
    assert bool((buf[0] == 7).all()) and bool((buf[3:] == 7).all())
    with pytest.raises(_lib.FgcnError, match="rows outside"):
        ops.clip_bodies(src, torch.tensor([2]), bodies=2)
    with pytest.raises(_lib.FgcnError, match="int64"):
        ops.clip_bodies(src, torch.arange(2, dtype=torch.int32), bodies=2)
    for bad in (0, 5, 1.0, True):
        with pytest.raises(_lib.FgcnError, match="bodies="):
            ops.clip_bodies(src, torch.arange(2), bodies=bad)
    with pytest.raises(_lib.FgcnError, match="for a batch of"):
        ops.clip_bodies(src, torch.arange(2), bodies=2, out=torch.empty(2, 1, 13, 7, 3, device=DEV))
    with pytest.raises(_lib.FgcnError, match="alias"):
        ops.clip_bodies(src, torch.arange(2), bodies=4, out=src)
    with pytest.raises(_lib.FgcnError, match="expected \\(rows, Mr, T, V, C\\)"):
        ops.clip_bodies(src[0], torch.arange(2), bodies=2)


# ---- ClipBatches ----------------------------------------------------------------------------------------------------------------------
BS = 4
KW7 = dict(origin_joint=2, z_axis_joints=(3, 2), x_axis_joints=(4, 6))
PARENTS7 = [1, 2, 2, 2, 3, 2, 5]


@pytest.fixture(scope="module")
def raw_dataset(tmp_path_factory):
    """ten raw clips (4, 13, 7, 3) written with NumpyWriter and an inertial signal beside them: the two bodies with the largest
    amplitudes (the actors) end at frame 6 + k % 5, the two others (noise) go on to the last frame in every second clip"""
    import os

    from fusion_gcn_amd.data import MultiModalDataset, NumpyDatasetLoader, NumpyWriter
    root = str(tmp_path_factory.mktemp("bodies"))
    rng = np.random.default_rng(4)
    clips = np.stack([_draw(rng, (4, 13, 7, 3), 0.02, 0.4) for _ in range(10)])
    for k, x in enumerate(clips):
        ranked = B.order(B.scores(x))
        x[ranked[:2], 6 + k % 5:] = 0
        if k % 2:
            x[ranked[2:], 9:] = 0
        assert B.order(B.scores(x))[:2].tolist() == ranked[:2].tolist()
    inertial = rng.standard_normal((10, 11, 6)).astype(np.float32)
    for name, a in (("skeleton", clips), ("inertial", inertial)):
        with NumpyWriter(os.path.join(root, f"{name}_train_features.npy"), np.float32, a.shape) as w:
            for s in a:
                w.collect_next(s)
    np.save(os.path.join(root, "train_labels.npy"), np.arange(10) % 5)
    return MultiModalDataset([(root, NumpyDatasetLoader())], "train"), clips, inertial


def _bodies():
    from fusion_gcn_amd.data import Bodies
    return Bodies(2, only=["skeleton"])


def _epoch(ds, **kw):
    from fusion_gcn_amd.data import ClipBatches
    it = ClipBatches(ds, BS, shuffle=True, seed=5, device=DEV, bodies=_bodies(), **kw)
    it.set_epoch(2)
    out = []
    for feats, lab, idx in it:
        assert set(it.last_bodies) == {"skeleton"}
        out.append(({k: v.cpu() for k, v in feats.items()}, lab.cpu(), idx.clone()))
    torch.cuda.synchronize()
    return it, out


def test_clip_batches_resident_and_streaming_deliver_the_selected_bodies(raw_dataset):
    ds, clips, inertial = raw_dataset
    want = torch.from_numpy(np.stack([B.select(x, 2) for x in clips]))
    (res_it, res), (str_it, stream) = _epoch(ds, resident=True), _epoch(ds, resident=False)
    assert res_it.resident and not str_it.resident and [len(b[2]) for b in res] == [4, 4, 2]      # shuffled, a ragged last batch
    assert res_it.shapes == str_it.shapes == {"skeleton": (2, 13, 7, 3), "inertial": (11, 6)}
    assert [s.name for s in res_it.stages] == ["bodies"] and res_it.bodies is res_it.stages[0]
    assert torch.equal(res_it.dev_feat["skeleton"].cpu().view(torch.int32), want.view(torch.int32))      # selected once, at upload: M / Mr
    order, scores = str_it.last_bodies["skeleton"]                             # the tables of the last call: the ragged batch
    assert order.shape == (2, 4) and order.dtype == torch.int32 and scores.shape == (2, 4) and scores.dtype == torch.float64
    last = stream[-1][2]
    assert order.cpu().tolist() == [B.order(B.scores(clips[i])).tolist() for i in last.tolist()]
    assert res_it.last_bodies["skeleton"][0].shape == (10, 4)                  # the resident split's one call
    for a, b in zip(res, stream):
        assert torch.equal(a[2], b[2]) and torch.equal(a[1], b[1])
        assert a[0]["skeleton"].shape[1:] == (2, 13, 7, 3)
        assert torch.equal(a[0]["skeleton"].view(torch.int32), b[0]["skeleton"].view(torch.int32))
        assert torch.equal(a[0]["skeleton"].view(torch.int32), want[a[2]].view(torch.int32))
        assert torch.equal(a[0]["inertial"], torch.from_numpy(inertial)[a[2]]) and torch.equal(b[0]["inertial"], a[0]["inertial"])


@pytest.mark.parametrize("resident", [True, False])
def test_world_2_shards_are_the_halves_of_the_world_1_batch(raw_dataset, resident):
    ds = raw_dataset[0]
    _, whole = _epoch(ds, resident=resident)
    halves = [_epoch(ds, resident=resident, rank=r, world=2)[1] for r in (0, 1)]
    assert len(whole) == len(halves[0]) == len(halves[1]) == 3
    for w, h0, h1 in zip(whole, *halves):
        assert torch.equal(torch.cat([h0[2], h1[2]]), w[2])
        assert torch.equal(torch.cat([h0[0]["skeleton"], h1[0]["skeleton"]]).view(torch.int32), w[0]["skeleton"].view(torch.int32))


@pytest.mark.parametrize("resident", [True, False])
def test_normalize_reads_the_selected_bodies(raw_dataset, resident):
    """Bodies, then Normalize = normalize_ref applied to bodies_ref.select, to test_normalize's bound"""
    from fusion_gcn_amd.data import ClipBatches, Normalize
    from test_normalize_gpu import _check as check_normalized
    ds, clips, _ = raw_dataset
    it = ClipBatches(ds, BS, shuffle=True, seed=5, device=DEV, resident=resident, bodies=_bodies(), normalize=Normalize(**KW7, only=["skeleton"]))
    assert [s.name for s in it.stages][:2] == ["bodies", "normalize"] and it.shapes["skeleton"] == (2, 13, 7, 3)
    seen = 0
    for feats, _, idx in it:
        frame_map, params = (t.cpu().numpy() for t in it.last_plan["skeleton"])
        if resident:                                                           # (the tables of the one call at upload, by source row)
            frame_map, params = frame_map[idx.numpy()], params[idx.numpy()]
        out = feats["skeleton"].cpu().numpy()
        assert out.shape == (len(idx), 2, 13, 7, 3)
        for k, i in enumerate(idx.tolist()):
            check_normalized(f"clip {i}", (out[k], frame_map[k], params[k]), B.select(clips[i], 2), 2, (3, 2), (4, 6))
        seen += len(idx)
    assert seen == 10


@pytest.mark.parametrize("resident", [True, False])
def test_window_augment_and_streams_run_behind_the_selection(raw_dataset, resident):
    from fusion_gcn_amd.data import Augment, ClipBatches, Streams, Window, valid_frames
    ds = raw_dataset[0]
    table = valid_frames(ds, "skeleton", device=DEV, bodies=_bodies())
    it = ClipBatches(ds, BS, shuffle=True, seed=5, device=DEV, resident=resident, bodies=_bodies(),
                     window=Window({"skeleton": 8}, valid_frames={"skeleton": table}), augment=Augment(only=["skeleton"]),
                     streams=Streams(PARENTS7, streams=("joint", "bone"), only=["skeleton"]))
    assert [s.name for s in it.stages] == ["bodies", "window", "augment", "streams"]
    assert it.shapes == {"skeleton": (2, 8, 7, 3), "skeleton_bone": (2, 8, 7, 3), "inertial": (11, 6)}
    seen = 0
    for feats, _, idx in it:
        for k in ("skeleton", "skeleton_bone"):
            assert feats[k].shape == (len(idx), 2, 8, 7, 3) and bool(torch.isfinite(feats[k]).all())
        assert bool((feats["skeleton"][:, :, :, 0] - feats["skeleton"][:, :, :, 1] == feats["skeleton_bone"][:, :, :, 0]).all())
        seen += len(idx)
    assert seen == 10


def test_valid_frames_counts_the_selected_bodies_only(raw_dataset):
    from fusion_gcn_amd.data import Bodies, valid_frames
    ds, clips, _ = raw_dataset
    last = lambda x: max(int(np.flatnonzero(B.non_null(b))[-1]) + 1 if B.non_null(b).any() else 1 for b in x)      # noqa: E731
    want = np.array([last(B.select(x, 2)) for x in clips], dtype=np.int32)
    stored = np.array([last(x) for x in clips], dtype=np.int32)
    assert want.tolist() == [6 + k % 5 for k in range(10)] and stored.tolist() == [13, 9, 13, 9, 13, 9, 13, 9, 13, 10]      # a fixture on which they must differ
    got = valid_frames(ds, "skeleton", device=DEV, bodies=_bodies(), chunk=3)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert np.array_equal(valid_frames(ds, "skeleton", device=DEV), stored)    # without the argument: what it was
    assert np.array_equal(valid_frames(ds, "skeleton", device=DEV, bodies=Bodies(4)), stored)
    with pytest.raises(ValueError, match="does not apply"):
        valid_frames(ds, "skeleton", device=DEV, bodies=Bodies(2, only=["inertial"]))


def test_clip_batches_refuses_what_it_cannot_select_from(raw_dataset):
    from fusion_gcn_amd import _lib
    from fusion_gcn_amd.data import Bodies, ClipBatches
    ds = raw_dataset[0]
    with pytest.raises(_lib.FgcnError, match="expected \\(samples, Mr, T, V, C\\)"):
        ClipBatches(ds, BS, device=DEV, bodies=Bodies(2))                      # the inertial signal holds no bodies
    with pytest.raises(ValueError, match="does not have"):
        ClipBatches(ds, BS, device=DEV, bodies=Bodies(2, only=["depth"]))
    with pytest.raises(_lib.FgcnError, match="holds 4 bodies"):
        ClipBatches(ds, BS, device=DEV, bodies=Bodies(5, only=["skeleton"]))
