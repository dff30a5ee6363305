"""fgcn_clip_augment on the device at the smallest shapes at which it can go wrong: a row of 75 floats (no
16-byte alignment), an odd frame count, repeated and unsorted source rows, clips of one and two valid frames.  The transform is compared
with tests/augment_ref.py's float64 restatement evaluated FROM THE DEVICE'S OWN parameter table (that separates the transform from the
trigonometric functions); the table itself is held to the bounds of the host test.  Then the promises of the design: identity
parameters give the gathered rows, a row's result depends on (seed, site, epoch, sample id) alone, ClipBatches hands out the same bits
on the resident and the streaming path and on one and two ranks, and a training loop over augmented batches repeats bit for bit."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import augment_ref as A
from test_data import write_split

import guarded
from guarded import guarded_allocations  # noqa: F401  (the fixture)

# every test runs on guarded allocations: NaN around each tensor the host layer creates, margins verified at teardown (tests/guarded.py)
pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_allocations")]
DEV = torch.device("cuda:0")

ROWS, IDX, VALID = 7, [5, 0, 5, 3], [13, 1, 2, 7, 13, 12, 5]
IDS = [40, 2 ** 31 + 7, 41, 3]                      # the samples the rows are drawn for: not the rows' own numbers, one above 2^31
KW = dict(seed=0x1234567887654321, epoch=3, site=2, max_angle=(0.3, 0.2, 0.5), scale=0.1, min_window=0.5)


def _src(*shape, seed=1):
    return torch.randn(ROWS, *shape, generator=torch.Generator().manual_seed(seed))


def _run(src, idx=IDX, ids=IDS, valid=VALID, joints=None, **kw):
    from fusion_gcn_amd import ops
    v = None if valid is None else torch.tensor(valid, dtype=torch.int32, device=DEV)
    out, table = ops.clip_augment(guarded.to(src, DEV), torch.tensor(idx), torch.tensor(ids), joints=joints, valid=v, **{**KW, **kw})
    torch.cuda.synchronize()
    return out.cpu(), table.cpu()


def _tolerance(T, src, scale=KW["scale"]):
    """(32 + 8 T) 2^-24 sqrt(3) (1 + scale) max|x|: 8 T is the effect of 4 ulps of pos on the interpolation weight, the rest the
    roundings of one lerp and one 3 x 3 product"""
    return (32 + 8 * T) * 2.0 ** -24 * np.sqrt(3.0) * (1.0 + scale) * float(src.abs().max())


def _check_table(table, ids=IDS, **kw):
    k = {**KW, **kw}
    want = np.stack([A.params(i, k["site"], k["epoch"], k["seed"], k["max_angle"], k["scale"], k["min_window"]) for i in ids])
    A.check_table(table.numpy(), want, k["scale"])


def _compare(src, out, table, joints, valid=VALID, idx=IDX):
    want = A.transform(src.numpy(), idx, table.numpy(), valid, joints)
    T = src.shape[2] if src.dim() == 5 else src.shape[1]
    err, tol = float(np.abs(out.double().numpy() - want).max()), _tolerance(T, src)
    print(f"[augment] {tuple(src.shape)} joints {joints}: max error {err:.3e}, bound {tol:.3e}")
    assert err <= tol, (err, tol)


@pytest.fixture(scope="module")
def skeleton():
    """the headline case, shared: source, output and table of (M, T, V, C) = (2, 13, 25, 3)"""
    src = _src(2, 13, 25, 3)
    out, table = _run(src, joints=(0, 25))
    return src, out, table


def test_skeleton_against_the_float64_restatement(skeleton):
    src, out, table = skeleton
    assert out.shape == (4, 2, 13, 25, 3) and table.shape == (4, 12)
    _check_table(table)
    _compare(src, out, table, (0, 25))
    assert not torch.equal(out[0], out[2])                                   # source row 5 twice, drawn for two samples


def test_clips_of_one_and_two_valid_frames_are_clamped():
    """the source rows the headline batch does not gather: valid = 1 (every output frame is frame 0, rotated), 2, 5 and 13"""
    src = _src(2, 13, 25, 3)
    idx, ids = [1, 2, 6, 4], [7, 8, 9, 10]
    out, table = _run(src, idx=idx, ids=ids, joints=(0, 25))
    _check_table(table, ids=ids)
    _compare(src, out, table, (0, 25), idx=idx)
    a = table[0, :9].reshape(3, 3).double()
    assert float((out[0].double() - (src[1, :, :1].double() @ a.T).expand(2, 13, 25, 3)).abs().max()) <= _tolerance(13, src)
    assert torch.equal(out[0][:, :1].expand(2, 13, 25, 3), out[0])


def test_one_frame_clips():
    src = _src(2, 1, 25, 3, seed=2)
    out, table = _run(src, valid=[1] * ROWS, joints=(0, 25))
    _check_table(table)
    _compare(src, out, table, (0, 25), valid=[1] * ROWS)
    out2, table2 = _run(src, valid=None, joints=(0, 25))                     # valid == NULL counts as T
    assert torch.equal(out2, out) and torch.equal(table2, table)


def test_joint_range_leaves_the_appended_joints_to_the_interpolation():
    src = _src(2, 13, 27, 3, seed=3)
    out, table = _run(src, joints=(0, 20))
    _check_table(table)
    _compare(src, out, table, (0, 20))
    plain, _ = _run(src, joints=None)                                        # the same draw without a spatial part
    assert torch.equal(out[..., 20:, :], plain[..., 20:, :]) and not torch.equal(out[..., :20, :], plain[..., :20, :])
    _compare(src, plain, table, None)


def test_inertial_signal_takes_the_same_part_of_the_recording(skeleton):
    _, _, sk_table = skeleton
    src = _src(11, 6, seed=4)
    valid = [11, 1, 2, 7, 11, 10, 5]
    out, table = _run(src, valid=valid)
    assert out.shape == (4, 11, 6)
    assert torch.equal(table[:, 9:], sk_table[:, 9:])                        # o, r: bit for bit the skeleton call's
    _compare(src, out, table, None, valid=valid)


def test_identity_parameters_give_the_gathered_rows():
    for shape, joints in (((2, 13, 25, 3), (0, 25)), ((2, 1, 25, 3), (0, 25)), ((11, 6), None), ((2, 13, 27, 3), (0, 20))):
        src = _src(*shape, seed=5)
        out, table = _run(src, valid=None, joints=joints, max_angle=(0.0, 0.0, 0.0), scale=0.0, min_window=1.0)
        assert torch.equal(out, src.index_select(0, torch.tensor(IDX))), shape
        assert torch.equal(table, torch.tensor([1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 1, 0]).expand(4, 12)), shape


def test_rows_depend_on_seed_site_epoch_and_sample_alone(skeleton):
    src, out, table = skeleton
    again, table2 = _run(src, joints=(0, 25))
    assert torch.equal(again, out) and torch.equal(table2, table)            # two calls from one state
    for other in (dict(epoch=4), dict(site=3), dict(seed=KW["seed"] + 1)):
        o2, t2 = _run(src, joints=(0, 25), **other)
        assert all(not torch.equal(o2[k], out[k]) and not torch.equal(t2[k], table[k]) for k in range(4)), other
    # a row's result depends neither on its position in the batch nor on the other rows
    perm = [2, 0, 3, 1]
    o3, t3 = _run(src, idx=[IDX[p] for p in perm], ids=[IDS[p] for p in perm], joints=(0, 25))
    assert torch.equal(o3, out[perm]) and torch.equal(t3, table[perm])
    o4, t4 = _run(src, idx=[IDX[2]], ids=[IDS[2]], joints=(0, 25))
    assert torch.equal(o4[0], out[2]) and torch.equal(t4[0], table[2])


def test_more_than_one_workgroup_and_wrapper_refusals():
    """600 rows of (1, 5, 3, 3): 9000 joint lanes, 10 table workgroups; every row against the restatement"""
    from fusion_gcn_amd import _lib, ops
    g = torch.Generator().manual_seed(6)
    src = torch.randn(9, 1, 5, 3, 3, generator=g)
    idx = torch.randint(0, 9, (600,), generator=g)
    ids = torch.arange(600) * 7
    valid = torch.randint(1, 6, (9,), generator=g)
    out, table = ops.clip_augment(guarded.to(src, DEV), idx, ids, joints=(1, 3), valid=guarded.to(valid.to(torch.int32), DEV), **KW)
    want = A.transform(src.numpy(), idx.numpy(), table.cpu().numpy(), valid.numpy(), (1, 3))
    assert float(np.abs(out.cpu().double().numpy() - want).max()) <= _tolerance(5, src)
    _check_table(table.cpu(), ids=ids.tolist())
    with pytest.raises(_lib.FgcnError, match="rows outside"):
        ops.clip_augment(guarded.to(src, DEV), torch.tensor([9]), torch.tensor([0]), **KW)
    with pytest.raises(_lib.FgcnError, match="valid"):
        ops.clip_augment(guarded.to(src, DEV), idx, ids, valid=guarded.to(valid, DEV), **KW)           # int64 frame counts
    on_dev = guarded.to(src, DEV)
    with pytest.raises(_lib.FgcnError, match="alias"):
        ops.clip_augment(on_dev, torch.arange(9), torch.arange(9), out=on_dev, **KW)


# ---- ClipBatches ----------------------------------------------------------------------------------------------------------------------
N, BS, SHAPES = 19, 8, {"skeleton": (2, 13, 25, 3), "inertial": (11, 6)}


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    from fusion_gcn_amd.data import MultiModalDataset, NumpyDatasetLoader
    root = str(tmp_path_factory.mktemp("augment"))
    arrays, labels = write_split(root, "train", N, SHAPES)
    return MultiModalDataset([(root, NumpyDatasetLoader())], "train"), arrays, labels


def _valid_frames():
    rng = np.random.default_rng(8)
    return {"skeleton": rng.integers(1, 14, N), "inertial": rng.integers(1, 12, N)}


def _epoch(ds, epoch, **kw):
    """-> [(features, labels, indices, tables)] of one pass, on the host"""
    from fusion_gcn_amd.data import Augment, ClipBatches
    it = ClipBatches(ds, BS, shuffle=True, seed=5, device=DEV, augment=Augment(valid_frames=_valid_frames()), **kw)
    it.set_epoch(epoch)
    out = []
    for feats, lab, idx in it:
        assert set(it.last_params) == set(SHAPES) and all(t.shape == (len(idx), 12) for t in it.last_params.values())
        out.append(({k: v.cpu() for k, v in feats.items()}, lab.cpu(), idx.clone(), {k: v.cpu() for k, v in it.last_params.items()}))
    torch.cuda.synchronize()
    return out


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x[2], y[2]) and torch.equal(x[1], y[1]) and all(torch.equal(x[0][k], y[0][k]) for k in SHAPES)
                                    and all(torch.equal(x[3][k], y[3][k]) for k in SHAPES) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def resident_epoch3(dataset):
    return _epoch(dataset[0], 3, resident=True)


def test_clip_batches_resident_and_streaming_deliver_the_same_bits(dataset, resident_epoch3):
    ds, arrays, labels = dataset
    res = resident_epoch3
    assert [len(b[2]) for b in res] == [8, 8, 3]
    assert _same(_epoch(ds, 3, resident=False), res)
    valid = _valid_frames()
    for feats, lab, idx, tables in res:                                      # and they are the contract's transform of the stored rows
        assert torch.equal(lab, torch.from_numpy(labels.astype(np.int64))[idx])
        assert torch.equal(tables["skeleton"][:, 9:], tables["inertial"][:, 9:]) and torch.equal(tables["skeleton"], tables["inertial"])
        _check_table(tables["skeleton"], ids=idx.tolist(), seed=5, epoch=3, site=0, max_angle=(0.3, 0.3, 0.3), scale=0.1, min_window=0.5)
        for k, joints in (("skeleton", (0, 25)), ("inertial", None)):
            want = A.transform(arrays[k], idx.numpy(), tables[k].numpy(), valid[k], joints)
            T = SHAPES[k][-2] if k == "inertial" else SHAPES[k][1]
            assert float(np.abs(feats[k].double().numpy() - want).max()) <= _tolerance(T, torch.from_numpy(arrays[k])), k


def test_clip_batches_two_ranks_concatenate_to_one(dataset, resident_epoch3):
    ds = dataset[0]
    ranks = [_epoch(ds, 3, resident=r == 0, rank=r, world=2) for r in range(2)]          # (one rank resident, one streaming)
    assert [len(b[2]) for b in ranks[0]] == [4, 4, 1] and [len(b[2]) for b in ranks[1]] == [4, 4, 1]
    for b, (r0, r1) in enumerate(zip(*ranks)):
        one = resident_epoch3[b]
        n = len(r0[2]) + len(r1[2])                                          # the ragged tail is trimmed to a multiple of the world size
        assert torch.equal(torch.cat([r0[2], r1[2]]), one[2][:n])
        for k in SHAPES:
            assert torch.equal(torch.cat([r0[0][k], r1[0][k]]), one[0][k][:n]), (b, k)
            assert torch.equal(torch.cat([r0[3][k], r1[3][k]]), one[3][k][:n]), (b, k)


def test_clip_batches_repeat_an_epoch_and_change_with_it(dataset, resident_epoch3):
    ds = dataset[0]
    assert _same(_epoch(ds, 3, resident=True), resident_epoch3)
    other = _epoch(ds, 4, resident=True)
    by_clip = {int(i): (b[0]["skeleton"][j], b[3]["skeleton"][j]) for b in resident_epoch3 for j, i in enumerate(b[2])}
    for feats, _, idx, tables in other:
        for j, i in enumerate(idx.tolist()):
            assert not torch.equal(tables["skeleton"][j], by_clip[i][1]) and not torch.equal(feats["skeleton"][j], by_clip[i][0]), i


def test_only_names_the_modalities_to_augment(dataset):
    from fusion_gcn_amd.data import Augment, ClipBatches
    ds, arrays, _ = dataset
    it = ClipBatches(ds, BS, shuffle=False, device=DEV, resident=True, augment=Augment(only=["skeleton"]))
    feats, _, idx = next(iter(it))
    assert set(it.last_params) == {"skeleton"}
    assert torch.equal(feats["inertial"].cpu(), torch.from_numpy(arrays["inertial"])[idx])
    assert not torch.equal(feats["skeleton"].cpu(), torch.from_numpy(arrays["skeleton"])[idx])


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
def test_graph_step_training_on_augmented_batches_repeats_bit_for_bit(tmp_path):
    """Three GraphStep training steps of a two-block AGCN on augmented batches (the streaming path): the batch is the recorded graph's
    input, so the recording verifies as it does without augmentation, and the loop run a second time from the same seeds ends on the
    same loss and parameters, bit for bit."""
    from fusion_gcn_amd.data import Augment, ClipBatches, MultiModalDataset, NumpyDatasetLoader
    from fusion_gcn_amd.datasets.utd_mhad import constants as utd
    from fusion_gcn_amd.models.mmargcn.agcn import Model
    from fusion_gcn_amd.optim import FlatOptimizer
    from fusion_gcn_amd.session.procedures import GraphStep
    from fusion_gcn_amd.util import Graph
    from oracle import filler
    shape, classes = (1, 16, 20, 3), 5
    write_split(str(tmp_path), "train", 12, {"skeleton": shape}, classes=classes, seed=9)
    ds = MultiModalDataset([(str(tmp_path), NumpyDatasetLoader())], "train")

    def run():
        model = Model(shape, classes, Graph(utd.skeleton_edges, center_joint=utd.center_joint), num_layers=2)
        filler.fill_state_dict(model.state_dict())
        model = guarded.to(model, DEV).train()
        opt = FlatOptimizer(model.parameters(), "SGD", 0.01, momentum=0.9)
        step = GraphStep(verify=True)
        batches = ClipBatches(ds, 4, shuffle=True, seed=3, device=DEV, resident=False, augment=Augment())
        batches.set_epoch(1)
        losses = []
        for x, y, _ in batches:
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
