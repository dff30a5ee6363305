"""fgcn_clip_window and fgcn_clip_valid_frames on the device at the smallest shapes at which they can go wrong:
rows of 75, 21, 18 and 6 floats (no 16-byte alignment), windows shorter and longer than the clip, a window of one frame, a clip of one
frame, 1650 elements in a body (more than one workgroup, no multiple of 256), repeated and unsorted source rows, clips of 1, 2, 5, 7, 12
and 13 valid frames and counts outside [1, T].  The transform is compared with tests/window_ref.py's float64 restatement evaluated FROM
THE DEVICE'S OWN parameter table; the table itself equals fgcn_window_params' bit for bit (no transcendental function, contraction off).
Every test runs on guarded allocations: a read of frame v, of frame T behind a row, or a store past W reaches NaN or a margin.  Then the
promises of ClipBatches: the same bits on the resident and the streaming path and on one and two ranks, an evaluation split windowed once
at upload, the five stages in a row equal to the stages composed by hand, and a model built from ``ClipBatches.shapes`` that trains."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import window_ref as R
from test_data import write_split

import guarded
from guarded import guarded_allocations  # noqa: F401  (the fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_allocations")]
DEV = torch.device("cuda:0")

IDX, IDS = [4, 0, 4], [40, 2 ** 31 + 7, 41]          # the samples the rows are drawn for: not the rows' own numbers, one above 2^31
KW = dict(seed=0x1234567887654321, epoch=3, site=2, interval=(0.5, 1.0))
MODES = ("random", "centre")


def _src(rows, *shape, seed=1):
    return torch.randn(rows, *shape, generator=torch.Generator().manual_seed(seed))


def _run(src, W, idx=IDX, ids=IDS, valid=None, mode="random", **kw):
    from fusion_gcn_amd import ops
    v = None if valid is None else torch.tensor(valid, dtype=torch.int32, device=DEV)
    out, table = ops.clip_window(guarded.to(src, DEV), torch.tensor(idx), None if ids is None else torch.tensor(ids), window=W, valid=v, mode=mode,
                                 **{**KW, **kw})
    torch.cuda.synchronize()
    return out.cpu(), table.cpu()


def _frames(src):
    return src.shape[2] if src.dim() == 5 else src.shape[1]


def _tolerance(src):
    """(32 + 8 T) 2^-24 max|x|: 8 T is the effect of 4 ulps of pos (at most T - 1) on the interpolation weight, the rest the roundings of one
    lerp -- the bound of tests/test_augment_gpu.py for the same temporal formula, without the rotation's factor"""
    return (32 + 8 * _frames(src)) * 2.0 ** -24 * float(src.abs().max())


def _compare(src, out, table, W, valid=None, idx=IDX, what=""):
    want = R.transform(src.numpy(), idx, table.numpy(), W, valid)
    assert out.shape == want.shape
    err, tol = float(np.abs(out.double().numpy() - want).max()), _tolerance(src)
    print(f"[window] {tuple(src.shape)} -> {W} {what}: max error {err:.3e}, bound {tol:.3e}")
    assert err <= tol, (err, tol)


def _check_table(table, ids, mode, **kw):
    """equal bits with the host copy of the function the kernel calls; in CENTRE mode every row is the same"""
    from fusion_gcn_amd import ops
    k = {**KW, **kw}
    want = torch.tensor([ops.window_params(i, k["site"], k["epoch"], k["seed"], k["interval"], mode) for i in ids], dtype=torch.float32)
    assert table.shape == want.shape and torch.equal(table.view(torch.int32), want.view(torch.int32)), (table, want)


CASES = [((2, 13, 25, 3), 8), ((1, 13, 7, 3), 20), ((2, 5, 9, 2), 1), ((1, 1, 7, 3), 4), ((1, 40, 25, 3), 33), ((11, 6), 7)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape,W", CASES, ids=["x".join(map(str, s)) + f"-{w}" for s, w in CASES])
def test_kernel_against_the_restatement(shape, W, mode):
    """five source rows gathered as [4, 0, 4]: all frames valid, then rows of T - 1 and T - 2 (at least 1) valid frames; two calls, the same bits"""
    src = _src(5, *shape, seed=sum(shape) + W)
    T = _frames(src)
    out, table = _run(src, W, mode=mode)
    _check_table(table, IDS, mode)
    _compare(src, out, table, W, what=mode)
    # source row 4 twice: drawn for two samples, or not drawn at all (a clip of one frame has one part only)
    assert torch.equal(out[0], out[2]) == (mode == "centre" or T == 1)
    valid = [max(T - 2, 1), 3, 3, 3, max(T - 1, 1)]
    short, table2 = _run(src, W, valid=valid, mode=mode)
    assert torch.equal(table2, table)                                         # o and r are fractions: they do not depend on the count
    _compare(src, short, table2, W, valid, what=f"{mode}, valid {valid[4]} and {valid[0]}")
    again, table3 = _run(src, W, valid=valid, mode=mode)
    assert torch.equal(again, short) and torch.equal(table3, table2)
    if mode == "centre":                                                      # no ids are read
        none, table4 = _run(src, W, ids=None, valid=valid, mode=mode)
        assert torch.equal(none, short) and torch.equal(table4, table2)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape,W", [((2, 13, 25, 3), 8), ((13, 6), 20)], ids=["skeleton", "signal"])
def test_valid_frames_bound_what_is_read(shape, W, mode):
    """valid in {1, 2, 5, 7, 12, 13} and the counts 0 and T + 5, which are clamped; the source is NaN at and behind the (clamped) count, so
    an output that read such a frame would be NaN"""
    src = _src(8, *shape, seed=7)
    valid = [1, 2, 5, 7, 12, 13, 0, 18]
    for r, v in enumerate(valid):
        if src.dim() == 5:
            src[r, :, R.clamp_valid(v, 13):] = np.nan
        else:
            src[r, R.clamp_valid(v, 13):] = np.nan
    idx = [6, 3, 0, 7, 5, 1, 4, 2, 0]
    ids = list(range(100, 109))
    out, table = _run(src, W, idx=idx, ids=ids, valid=valid, mode=mode)
    assert not torch.isnan(out).any()
    _check_table(table, ids, mode)
    finite = torch.nan_to_num(src, nan=0.0)
    want = R.transform(finite.numpy(), idx, table.numpy(), W, valid)
    err = float(np.abs(out.double().numpy() - want).max())
    print(f"[window] {tuple(src.shape)} -> {W} {mode}, valid {valid}: max error {err:.3e}, bound {_tolerance(finite):.3e}")
    assert err <= _tolerance(finite)
    for k in (0, 2, 8):                                                       # counts 0 and 1: every output frame is frame 0
        first = finite[idx[k]][:, :1] if src.dim() == 5 else finite[idx[k]][:1]
        assert torch.equal(out[k], first.expand_as(out[k])), k


def test_the_whole_recording_at_its_own_length_is_the_gathered_rows():
    for shape in ((2, 13, 25, 3), (2, 1, 25, 3), (11, 6), (1, 40, 25, 3)):
        src = _src(5, *shape, seed=5)
        T = _frames(src)
        for mode in MODES:
            for valid in (None, [T] * 5):
                out, table = _run(src, T, valid=valid, mode=mode, interval=(1.0, 1.0))
                assert torch.equal(out, src.index_select(0, torch.tensor(IDX))), (shape, mode)
                assert torch.equal(table, torch.tensor([0.0, 1.0]).expand(3, 2)), (shape, mode)


def test_rows_depend_on_seed_site_epoch_and_sample_alone():
    src = _src(5, 2, 13, 25, 3)
    out, table = _run(src, 8)
    for other in (dict(epoch=4), dict(site=3), dict(seed=KW["seed"] + 1)):
        o2, t2 = _run(src, 8, **other)
        assert all(not torch.equal(o2[k], out[k]) and not torch.equal(t2[k], table[k]) for k in range(3)), other
        oc, tc = _run(src, 8, mode="centre", **other)                         # the centred part ignores all three
        assert torch.equal(oc, _run(src, 8, mode="centre")[0]) and torch.equal(tc[0], torch.tensor([0.0, 1.0]))
    # a row's result depends neither on its position in the batch nor on the other rows
    perm = [2, 0, 1]
    o3, t3 = _run(src, 8, idx=[IDX[p] for p in perm], ids=[IDS[p] for p in perm])
    assert torch.equal(o3, out[perm]) and torch.equal(t3, table[perm])
    o4, t4 = _run(src, 8, idx=[IDX[2]], ids=[IDS[2]])
    assert torch.equal(o4[0], out[2]) and torch.equal(t4[0], table[2])
    # a skeleton and a signal with another T and another window take the same part of the recording
    _, sig_table = _run(_src(5, 11, 6, seed=4), 7)
    assert torch.equal(sig_table.view(torch.int32), table.view(torch.int32))
    # and the part is not the one the augmentation draws at the same seed, site, epoch and samples
    from fusion_gcn_amd import ops
    _, aug = ops.clip_augment(guarded.to(src, DEV), torch.tensor(IDX), torch.tensor(IDS), seed=KW["seed"], epoch=KW["epoch"], site=KW["site"],
                              min_window=0.5)
    assert all(aug.cpu()[k, 10] != table[k, 1] for k in range(3))


def test_a_nan_and_an_inf_reach_the_outputs_that_read_them():
    """rule 3 of include/fgcn.h: by class, at exactly the outputs whose f0 or f1 is the frame -- with weight zero too -- and nowhere else"""
    clean = _src(3, 2, 13, 7, 3, seed=9)
    src = clean.clone()
    src[2, 0, 5, 3, 1], src[2, 1, 9, 0, 0], src[0, 1, 0, 6, 2] = np.nan, np.inf, -np.inf
    idx, ids = [2, 0, 2], [1, 2, 3]
    for mode, W, interval in (("random", 8, (0.5, 1.0)), ("centre", 13, (1.0, 1.0)), ("centre", 20, (0.8, 0.8))):
        out, table = _run(src, W, idx=idx, ids=ids, mode=mode, interval=interval)
        ref, _ = _run(clean, W, idx=idx, ids=ids, mode=mode, interval=interval)
        reads, cls = R.classes(src.numpy(), idx, table.numpy(), W)
        got = R.classify(out.numpy())
        assert reads.any() and np.array_equal(got != 0, reads), (mode, W)
        assert np.array_equal(got, cls), (mode, W, np.argwhere(got != cls)[:5])
        assert torch.equal(out[torch.from_numpy(~reads)], ref[torch.from_numpy(~reads)])          # the others: what they are on finite data
    # the whole recording at its own length: frame t reads t and t + 1 (weight zero), so a NaN in frame 5 shows in frames 4 and 5
    out, _ = _run(src, 13, idx=[2], ids=[0], mode="centre", interval=(1.0, 1.0))
    assert torch.isnan(out[0, 0, :, 3, 1]).tolist() == [t in (4, 5) for t in range(13)]


def test_more_than_one_table_workgroup_and_wrapper_refusals():
    """600 rows of (1, 5, 3, 3) to 4 frames: 10 table workgroups; every row against the restatement"""
    from fusion_gcn_amd import _lib, ops
    g = torch.Generator().manual_seed(6)
    src = torch.randn(9, 1, 5, 3, 3, generator=g)
    idx = torch.randint(0, 9, (600,), generator=g)
    ids = torch.arange(600) * 7
    valid = torch.randint(1, 6, (9,), generator=g)
    on_dev = guarded.to(src, DEV)
    out, table = ops.clip_window(on_dev, idx, ids, window=4, valid=guarded.to(valid.to(torch.int32), DEV), **KW)
    _compare(src, out.cpu(), table.cpu(), 4, valid.numpy(), idx=idx.numpy(), what="600 rows")
    _check_table(table.cpu(), ids.tolist(), "random")
    with pytest.raises(_lib.FgcnError, match="rows outside"):
        ops.clip_window(on_dev, torch.tensor([9]), torch.tensor([0]), window=4, **KW)
    with pytest.raises(_lib.FgcnError, match="valid"):
        ops.clip_window(on_dev, idx, ids, window=4, valid=guarded.to(valid, DEV), **KW)            # int64 frame counts
    with pytest.raises(_lib.FgcnError, match="alias"):
        ops.clip_window(on_dev, torch.arange(9), torch.arange(9), window=5, out=on_dev, **KW)
    with pytest.raises(_lib.FgcnError, match="for a batch of"):
        ops.clip_window(on_dev, torch.arange(9), torch.arange(9), window=4, out=torch.empty(9, 1, 5, 3, 3, device=DEV), **KW)
    with pytest.raises(_lib.FgcnError, match="sample_ids"):
        ops.clip_window(on_dev, torch.arange(9), None, window=4, **KW)
    with pytest.raises(_lib.FgcnError, match="sample_ids"):
        ops.clip_window(on_dev, torch.arange(9), torch.arange(8), window=4, **KW)
    for bad in (dict(window=0), dict(window=4, mode="middle"), dict(window=4, interval=(0.0, 1.0)), dict(window=4, interval=(0.5,))):
        with pytest.raises(_lib.FgcnError):
            ops.clip_window(on_dev, torch.arange(9), torch.arange(9), **{**KW, **bad})
    with pytest.raises(_lib.FgcnError, match="expected"):
        ops.clip_window(torch.zeros(3, 5, device=DEV), torch.arange(3), torch.arange(3), window=4, **KW)
    with pytest.raises(_lib.FgcnError, match="rows outside"):
        ops.clip_valid_frames(on_dev, torch.tensor([9]))


# ---- the valid frames ---------------------------------------------------------------------------------------------------------------------
def _clips_with_known_counts(M=2, T=13, V=7, C=3):
    """-> (rows, M, T, V, C) float32 whose counts are [6, 10, 4, T, 9, 1, 1, T]"""
    x = np.zeros((8, M, T, V, C), dtype=np.float32)
    rng = np.random.default_rng(3)
    x[0, :, :6] = rng.standard_normal((M, 6, V, C))                           # trailing null frames
    x[1, 0, :3], x[1, 0, 9, V - 1, C - 1] = 1.0, 2.0                          # interior null frames do not end the clip; one value in frame 9
    x[2, 0, :4], x[2, :, 4:] = 1.0, -0.0                                      # -0 counts as zero
    x[3, 0, 0, 0, 0], x[3, M - 1, T - 1, 0, 0] = 1.0, np.nan                  # a frame that holds nothing but a NaN: a value
    x[4, 0, :2], x[4, M - 1, :9] = 1.0, 1.0                                   # the second body is longer than the first
    x[6, 0, 0, 2, 1] = 5.0                                                    # (row 5 holds nothing: 1) one value in frame 0: 1 too
    x[7] = rng.standard_normal((M, T, V, C))                                  # all frames
    return x


def test_valid_frames_are_the_restatements():
    from fusion_gcn_amd import ops
    for M, T, V, C in ((2, 13, 7, 3), (1, 13, 25, 3), (2, 40, 25, 3)):       # 273 and 975 floats per body, then 3000: twelve trips of 256 lanes
        x = _clips_with_known_counts(M, T, V, C)
        want = R.valid_frames(x)
        assert want.tolist() == [6, 10, 4, T, 9, 1, 1, T]
        on_dev = guarded.to(torch.from_numpy(x), DEV)
        got = ops.clip_valid_frames(on_dev)
        assert got.dtype == torch.int32 and got.shape == (8,) and got.cpu().tolist() == want.tolist(), (M, T, V, C)
        idx = [5, 0, 7, 0, 3, 1, 6, 2, 4, 5]                                  # repeated and unsorted
        assert ops.clip_valid_frames(on_dev, torch.tensor(idx)).cpu().tolist() == R.valid_frames(x, idx).tolist()
    sig = np.ascontiguousarray(_clips_with_known_counts()[:, 0, :, :, 0])     # a (rows, T, S) signal
    assert ops.clip_valid_frames(guarded.to(torch.from_numpy(sig), DEV)).cpu().tolist() == R.valid_frames(sig).tolist() == [6, 3, 4, 1, 2, 1, 1, 13]


def _write(root, arrays, labels, split="train"):
    import os

    from fusion_gcn_amd.data import MultiModalDataset, NumpyDatasetLoader, NumpyWriter
    for name, a in arrays.items():
        with NumpyWriter(os.path.join(root, f"{name}_{split}_features.npy"), np.float32, a.shape) as w:
            for s in a:
                w.collect_next(s)
    np.save(os.path.join(root, f"{split}_labels.npy"), labels)
    return MultiModalDataset([(root, NumpyDatasetLoader())], split)


def test_valid_frames_of_a_written_split(tmp_path):
    """one pass in chunks that do not divide the split; the table is what Window takes, and the window then reads no padding"""
    from fusion_gcn_amd import data
    x = _clips_with_known_counts()
    sig = np.ascontiguousarray(x[:, 0, :, :2, :].reshape(8, 13, 6))
    ds = _write(str(tmp_path), {"skeleton": x, "inertial": sig}, np.arange(8) % 3)
    for chunk in (3, 8, 2048):
        got = data.valid_frames(ds, "skeleton", device=DEV, chunk=chunk)
        assert got.dtype == np.int32 and got.tolist() == R.valid_frames(x).tolist()
    assert data.valid_frames(ds, "inertial", device=DEV, chunk=5).tolist() == R.valid_frames(sig).tolist()
    table = {"skeleton": data.valid_frames(ds, "skeleton", device=DEV)}
    it = data.ClipBatches(ds, 8, device=DEV, window=data.Window({"skeleton": 6}, interval=(1.0, 1.0), train=False, valid_frames=table))
    (feats, _, idx), = list(it)
    assert feats["skeleton"].shape == (8, 2, 6, 7, 3) and feats["inertial"].shape == (8, 13, 6)
    assert torch.equal(feats["skeleton"][0].cpu(), torch.from_numpy(x[0][:, :6]))      # six valid frames to six: the frames themselves
    assert bool((feats["skeleton"][0] != 0).all())


# ---- ClipBatches ----------------------------------------------------------------------------------------------------------------------
N, BS, SHAPES, FRAMES = 10, 4, {"skeleton": (2, 13, 7, 3), "inertial": (11, 6)}, {"skeleton": 8, "inertial": 16}
PAR7 = [2, 0, 2, 1, 6, -1, 3]


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    from fusion_gcn_amd.data import MultiModalDataset, NumpyDatasetLoader
    root = str(tmp_path_factory.mktemp("window"))
    arrays, labels = write_split(root, "train", N, SHAPES)
    return MultiModalDataset([(root, NumpyDatasetLoader())], "train"), arrays, labels


def _valid_frames():
    rng = np.random.default_rng(8)
    return {"skeleton": rng.integers(1, 14, N), "inertial": rng.integers(1, 12, N)}


def _epoch(ds, epoch=2, train=True, **kw):
    """-> (the iterator, [(features, labels, indices, tables)] of one shuffled pass, on the host)"""
    from fusion_gcn_amd.data import ClipBatches, Window
    it = ClipBatches(ds, BS, shuffle=True, seed=5, device=DEV, window=Window(FRAMES, train=train, valid_frames=_valid_frames()), **kw)
    it.set_epoch(epoch)
    out = []
    for feats, lab, idx in it:
        out.append(({k: v.cpu() for k, v in feats.items()}, lab.cpu(), idx.clone(), {k: v.cpu() for k, v in it.last_window.items()}))
    torch.cuda.synchronize()
    return it, out


def _same(a, b, tables=True):
    return len(a) == len(b) and all(torch.equal(x[2], y[2]) and torch.equal(x[1], y[1]) and all(torch.equal(x[0][k], y[0][k]) for k in SHAPES)
                                    and (not tables or all(torch.equal(x[3][k], y[3][k]) for k in SHAPES)) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def resident_epoch2(dataset):
    return _epoch(dataset[0], resident=True)


def test_clip_batches_resident_and_streaming_deliver_the_same_bits(dataset, resident_epoch2):
    ds, arrays, labels = dataset
    it, res = resident_epoch2
    assert [len(b[2]) for b in res] == [4, 4, 2] and it.resident and [s.name for s in it.stages] == ["window"]
    assert it.shapes == {"skeleton": (2, 8, 7, 3), "inertial": (16, 6)} and it.out_keys == sorted(SHAPES)
    it2, stream = _epoch(ds, resident=False)
    assert not it2.resident and _same(stream, res)
    valid = _valid_frames()
    for feats, lab, idx, tables in res:                                      # and they are the contract's transform of the stored rows
        assert torch.equal(lab, torch.from_numpy(labels.astype(np.int64))[idx])
        assert set(tables) == set(SHAPES) and torch.equal(tables["skeleton"], tables["inertial"])      # one part of the recording for both
        _check_table(tables["skeleton"], idx.tolist(), "random", seed=5, epoch=2, site=0)
        for k in SHAPES:
            assert feats[k].shape == (len(idx), *it.shapes[k])
            _compare(torch.from_numpy(arrays[k]), feats[k], tables[k], FRAMES[k], valid[k], idx=idx.numpy(), what=f"ClipBatches {k}")
    assert not _same(_epoch(ds, epoch=3, resident=True)[1], res, tables=False)      # another epoch, another draw


def test_clip_batches_two_ranks_concatenate_to_one(dataset, resident_epoch2):
    ds = dataset[0]
    ranks = [_epoch(ds, resident=r == 0, rank=r, world=2)[1] for r in range(2)]          # (one rank resident, one streaming)
    assert [len(b[2]) for b in ranks[0]] == [2, 2, 1] and [len(b[2]) for b in ranks[1]] == [2, 2, 1]
    for b, (r0, r1) in enumerate(zip(*ranks)):
        one = resident_epoch2[1][b]
        assert torch.equal(torch.cat([r0[2], r1[2]]), one[2])
        for k in SHAPES:
            assert torch.equal(torch.cat([r0[0][k], r1[0][k]]), one[0][k]), (b, k)
            assert torch.equal(torch.cat([r0[3][k], r1[3][k]]), one[3][k]), (b, k)


def test_an_evaluation_split_is_windowed_once_at_upload(dataset):
    from fusion_gcn_amd import ops
    ds, arrays, _ = dataset
    it, res = _epoch(ds, train=False, resident=True)
    assert it.window.at_upload and {k: tuple(v.shape) for k, v in it.dev_feat.items()} == {"skeleton": (N, 2, 8, 7, 3), "inertial": (N, 16, 6)}
    _, stream = _epoch(ds, train=False, resident=False)
    assert _same(stream, res, tables=False)
    valid = _valid_frames()
    for feats, _, idx, _ in res:
        for k in SHAPES:
            want, table = ops.clip_window(guarded.to(torch.from_numpy(arrays[k]), DEV), idx, None, window=FRAMES[k], interval=(0.5, 1.0), mode="centre",
                                          valid=torch.from_numpy(valid[k].astype(np.int32)).to(DEV))
            assert torch.equal(feats[k], want.cpu()) and torch.equal(table.cpu(), torch.tensor([0.0, 1.0]).expand(len(idx), 2)), k
    other = _epoch(ds, epoch=7, train=False, resident=True)[1]                # no random part: the epoch changes the order alone
    by_clip = {int(i): b[0]["skeleton"][j] for b in res for j, i in enumerate(b[2])}
    assert all(torch.equal(b[0]["skeleton"][j], by_clip[int(i)]) for b in other for j, i in enumerate(b[2]))


def _chain_by_hand(arrays, idx, frames, window, augment, streams, epoch, seed):
    """normalize -> inertial (enhance) -> window -> augment -> streams through ops, for the batch rows ``idx``"""
    from fusion_gcn_amd import ops
    n = len(arrays["skeleton"])
    rows, di = torch.arange(n, device=DEV), idx.to(DEV)
    skel, imu = (guarded.to(torch.from_numpy(arrays[k]), DEV) for k in ("skeleton", "inertial"))
    src_len, dst_len = (torch.from_numpy(frames[k].astype(np.int32)).to(DEV) for k in ("inertial", "skeleton"))
    norm, _, _ = ops.clip_normalize(skel, rows, origin_joint=1, z_axis_joints=(0, 1), x_axis_joints=(3, 4))
    feats = {"inertial": ops.signal_prepare(imu, rows, src_len, dst_len, skel.shape[2])[0], "skeleton": ops.imu_enhance(norm, rows, imu, rows, src_len, dst_len)}
    batch_rows = torch.arange(len(idx), device=DEV)
    out = {}
    for k, v in feats.items():
        v, _ = ops.clip_window(v, di, di, window=window.length(k), interval=window.interval, mode=window.mode, seed=seed, epoch=epoch, site=window.site)
        if augment.applies_to(k):
            v, _ = ops.clip_augment(v, batch_rows, di, seed=seed, epoch=epoch, site=augment.site, max_angle=augment.max_angle, scale=augment.scale,
                                    min_window=augment.min_window, joints=augment.joint_range(v.shape[1:]))
        out[k] = v
    got = ops.clip_streams(out.pop("skeleton"), batch_rows, streams.parents, streams=streams.streams)
    out.update({i: got[s] for s, i in streams.output_ids("skeleton").items()})
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


@pytest.mark.parametrize("only", [None, ["inertial"]], ids=["all", "augment-leaves-the-skeleton-out"])
def test_the_five_stages_in_a_row_are_the_stages_composed_by_hand(tmp_path, only):
    """With ``Augment(only=["inertial"])`` the resident path hands Streams the skeleton as the Window wrote it and Augment the signal through
    the same batch rows, while the ids that key both draws stay the shard's indices."""
    from fusion_gcn_amd.data import Augment, ClipBatches, Inertial, MultiModalDataset, Normalize, NumpyDatasetLoader, Streams, Window
    arrays, _ = write_split(str(tmp_path), "train", N, {"skeleton": (2, 13, 7, 3), "inertial": (29, 6)}, seed=4)
    ds = MultiModalDataset([(str(tmp_path), NumpyDatasetLoader())], "train")
    rng = np.random.default_rng(6)
    frames = {"skeleton": rng.integers(2, 14, N), "inertial": rng.integers(2, 30, N)}
    window, augment = Window({"skeleton": 8, "inertial": 8}, interval=(0.4, 0.9), site=1), Augment(joints=(0, 7), only=only)
    streams = Streams(PAR7 + [-1, -1], streams=("joint", "bone", "motion"))
    passes = []
    for resident in (True, False):
        it = ClipBatches(ds, BS, shuffle=True, seed=5, device=DEV, resident=resident, normalize=Normalize(1, z_axis_joints=(0, 1), x_axis_joints=(3, 4), only=["skeleton"]),
                         inertial=Inertial(frames=frames, enhance=True), window=window, augment=augment, streams=streams)
        it.set_epoch(2)
        assert [s.name for s in it.stages] == ["normalize", "inertial", "window", "augment", "streams"]
        assert it.shapes == {"inertial": (8, 6), "skeleton": (2, 8, 9, 3), "skeleton_bone": (2, 8, 9, 3), "skeleton_motion": (2, 8, 9, 3)}
        passes.append([({k: v.cpu() for k, v in feats.items()}, idx.clone()) for feats, _, idx in it])
        torch.cuda.synchronize()
    assert [len(b[1]) for b in passes[0]] == [4, 4, 2]
    for (a, idx), (b, idx2) in zip(*passes):
        assert torch.equal(idx, idx2) and list(a) == list(b) == ["inertial", "skeleton", "skeleton_bone", "skeleton_motion"]
        want = _chain_by_hand(arrays, idx, frames, window, augment, streams, epoch=2, seed=5)
        for k in a:
            assert a[k].shape == (len(idx), *it.shapes[k]) and torch.equal(a[k], b[k]) and torch.equal(a[k], want[k]), k


@pytest.mark.parametrize("augmented", ["pose", "skeleton"])
def test_two_features_read_through_different_rows(tmp_path, augmented):
    """Two skeleton features of one shape with different values, shuffled; the Window writes "skeleton" alone.  On the resident path, with
    ``Augment(only=["pose"])`` the Augment reads "pose" through the shard's indices of the resident array although it runs behind a per-batch
    stage; with ``Augment(only=["skeleton"])`` it reads what the Window wrote through the batch's rows, and Streams then reads "skeleton"
    through the batch's rows and "pose" through the shard's indices.  Either feature read through the other's rows gives another clip's values."""
    from fusion_gcn_amd import ops
    from fusion_gcn_amd.data import Augment, ClipBatches, MultiModalDataset, NumpyDatasetLoader, Streams, Window
    arrays, _ = write_split(str(tmp_path), "train", N, {"skeleton": (2, 13, 7, 3), "pose": (2, 13, 7, 3)}, seed=2)
    ds = MultiModalDataset([(str(tmp_path), NumpyDatasetLoader())], "train")
    valid = {"pose": np.random.default_rng(9).integers(1, 14, N)}             # allowed: the window does not apply to "pose"
    window, streams = Window({"skeleton": 8}), Streams(PAR7, only=["skeleton", "pose"])
    augment = Augment(only=[augmented], valid_frames=valid if augmented == "pose" else None)
    passes = []
    for resident in (True, False):
        it = ClipBatches(ds, BS, shuffle=True, seed=5, device=DEV, resident=resident, window=window, augment=augment, streams=streams)
        it.set_epoch(2)
        passes.append([({k: v.cpu() for k, v in feats.items()}, idx.clone()) for feats, _, idx in it])
        assert it.shapes == {"pose": (2, 13, 7, 3), "skeleton": (2, 8, 7, 3)} and set(it.last_window) == {"skeleton"} and set(it.last_params) == {augmented}
    dev = {k: guarded.to(torch.from_numpy(a), DEV) for k, a in arrays.items()}
    kw = dict(seed=5, epoch=2, max_angle=augment.max_angle, scale=augment.scale, min_window=augment.min_window, joints=(0, 7))
    for (a, idx), (b, _) in zip(*passes):
        assert idx.tolist() != list(range(len(idx)))                          # shuffled: the two kinds of rows differ
        rows = torch.arange(len(idx))
        skel, _ = ops.clip_window(dev["skeleton"], idx, idx, window=8, interval=(0.5, 1.0), seed=5, epoch=2)
        if augmented == "pose":
            pose, _ = ops.clip_augment(dev["pose"], idx, idx, valid=torch.from_numpy(valid["pose"].astype(np.int32)).to(DEV), **kw)
            pose_rows = rows
        else:
            skel, _ = ops.clip_augment(skel, rows, idx, **kw)
            pose, pose_rows = dev["pose"], idx
        want = {"skeleton": ops.clip_streams(skel, rows, PAR7)["bone"].cpu(), "pose": ops.clip_streams(pose, pose_rows, PAR7)["bone"].cpu()}
        for k in ("pose", "skeleton"):
            assert torch.equal(a[k], b[k]) and torch.equal(a[k], want[k]), k


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
def test_graph_step_training_on_windowed_batches_repeats_bit_for_bit(tmp_path):
    """Three GraphStep training steps of a two-block AGCN built from ``ClipBatches.shapes`` -- 16 frames of the stored 24 -- on windowed,
    augmented batches: the batch is the recorded graph's input, so the recording verifies, and the loop run a second time from the same
    seeds ends on the same loss and parameters, bit for bit."""
    from fusion_gcn_amd.data import Augment, ClipBatches, MultiModalDataset, NumpyDatasetLoader, Window
    from fusion_gcn_amd.datasets.utd_mhad import constants as utd
    from fusion_gcn_amd.models.mmargcn.agcn import Model
    from fusion_gcn_amd.optim import FlatOptimizer
    from fusion_gcn_amd.session.procedures import GraphStep
    from fusion_gcn_amd.util import Graph
    from oracle import filler
    stored, classes = (1, 24, 20, 3), 5
    write_split(str(tmp_path), "train", 12, {"skeleton": stored}, classes=classes, seed=9)
    ds = MultiModalDataset([(str(tmp_path), NumpyDatasetLoader())], "train")

    def run():
        batches = ClipBatches(ds, 4, shuffle=True, seed=3, device=DEV, resident=True, window=Window(16), augment=Augment())
        batches.set_epoch(1)
        shape = batches.shapes["skeleton"]
        assert shape == (1, 16, 20, 3)
        model = Model(shape, classes, Graph(utd.skeleton_edges, center_joint=utd.center_joint), num_layers=2)
        filler.fill_state_dict(model.state_dict())
        model = guarded.to(model, DEV).train()
        opt = FlatOptimizer(model.parameters(), "SGD", 0.01, momentum=0.9)
        step = GraphStep(verify=True)
        losses = []
        for x, y, _ in batches:
            assert x.shape == (4, *shape)
            opt.zero_grad()
            _, loss = step.forward(model, F.cross_entropy, x, y)
            step.backward(loss)
            step.run_optimizer_step(opt)
            losses.append(loss.detach().clone())
        torch.cuda.synchronize()
        assert step.replays == 3 and len(step._recorded) == 1
        return torch.stack(losses).cpu(), torch.cat([p.detach().reshape(-1) for p in model.parameters()]).cpu()

    (l1, p1), (l2, p2) = run(), run()
    assert bool(torch.isfinite(l1).all()) and len(set(l1.tolist())) == 3
    assert torch.equal(l1, l2) and torch.equal(p1, p2)
