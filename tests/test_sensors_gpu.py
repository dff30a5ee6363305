"""fgcn_clip_sensors on the device at the smallest shapes at which it can go wrong: rows of 6, 3 and 48 floats (no
16-byte alignment), one sensor and sixteen (the limit), a clip of one frame, repeated and unsorted source rows, clips of one and two valid
frames, sample ids above 2^31, two, four and eight knots, the sensor joints of a two-body skeleton, and a signal of 600 triples, which
every lane of the min-max workgroup walks more than once.  The transform is compared with tests/sensors_ref.py's float64 restatement
evaluated FROM THE DEVICE'S OWN parameter table (that separates the transform from the trigonometric functions) and the restatement's own
noise; the table itself is held to the bounds of the host test.  Then the promises of the design: what is not a sensor's valid frame is
copied bit for bit, a dropped sensor is +0, identity parameters give the gathered rows, the signal and the sensor joints of every body
receive the same values, min-max is the float32 formula applied to the same call's plain output, a row's result depends on (seed, site,
epoch, sample id) alone, ClipBatches hands out the same bits on the resident and the streaming path and on one and two ranks, and a
training loop over such batches repeats bit for bit."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sensors_ref as S

import guarded
from guarded import guarded_allocations  # noqa: F401  (the fixture)

# every test runs on guarded allocations: NaN around each tensor the host layer creates, margins verified at teardown (tests/guarded.py)
pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_allocations")]
DEV = torch.device("cuda:0")

ROWS, IDX, VALID = 7, [5, 0, 5, 3], [13, 1, 2, 7, 13, 12, 5]
IDS = [40, 2 ** 31 + 7, 41, 3]                      # the samples the rows are drawn for: not the rows' own numbers, one above 2^31
KW = dict(seed=0x1234567887654321, epoch=3, site=2, max_angle=(0.3, 0.2, 0.5), scale=0.1, warp=0.1, warp_knots=4, jitter=0.05, drop=0.0)
IDENTITY = dict(max_angle=(0.0, 0.0, 0.0), scale=0.0, warp=0.0, jitter=0.0, drop=0.0)
# (sample shape, joints, knots, jitter): the signal, one sensor, one frame, sixteen sensors, the sensor joints of a two-body skeleton
CASES = {"signal": ((13, 6), None, 4, (0.05, 0.002)), "one_sensor": ((13, 3), None, 2, 0.05), "one_frame": ((1, 6), None, 8, 0.05),
         "sixteen": ((5, 48), None, 8, tuple(0.01 * (g + 1) for g in range(16))), "skeleton": ((2, 13, 22, 3), (20, 22), 4, (0.05, 0.002))}


def _src(*shape, seed=1):
    return torch.randn(ROWS, *shape, generator=torch.Generator().manual_seed(seed))


def _frames(shape):
    return shape[0] if len(shape) == 2 else shape[1]


def _valid(shape, valid=VALID):
    return None if valid is None else [min(v, _frames(shape)) for v in valid]


def _run(src, idx=IDX, ids=IDS, valid=VALID, joints=None, minmax=False, **kw):
    from fusion_gcn_amd import ops
    valid = _valid(src.shape[1:], valid)
    v = None if valid is None else torch.tensor(valid, dtype=torch.int32, device=DEV)
    out, table, stats = ops.clip_sensors(guarded.to(src, DEV), torch.tensor(idx), torch.tensor(ids), joints=joints, valid=v, minmax=minmax,
                                         **{**KW, **kw})
    torch.cuda.synchronize()
    return out.cpu(), table.cpu(), stats.cpu()


def _tolerance(src, scale, warp, jitter):
    """2^-24 (sqrt(3) (8 + 134 warp) (1 + scale) max|x| + 48 max sigma), from the roundings the contract counts.  |R x|_c <= sqrt(3) max|x|.
    Step 1: one product, two fmas and the gain, 4 roundings; step 2's product, step 3's sum and the store of y itself: 8 with a margin of
    one.  The factor m = 1 + delta against the restatement's: f carries the two roundings of q <= 7, 14 * 2^-24, and the curve's slope is at
    most 3 warp (the sum of the magnitudes of the four basis derivatives is largest, 3, at f = 1 / 2), 42 warp; the Horner form's eleven
    operations act on magnitudes of at most 8, 12, 20 and 22 warp and are halved at the end, < 90 warp; the final sum, 2.  The noise: logf
    within 1 ulp and the correctly rounded sqrtf give rad to 2 * 2^-24 relative, cospif / sinpif within 2 ulp of a value <= 1, the product
    one more: 5 * 2^-24 * 5.77 (the largest radius, sqrt(-2 ln 2^-24)) = 29, the product with sigma 6 more: 48 with a margin.  The contract
    caps the bound at 64 * 2^-24 (max|x| (1 + scale) (1 + 2 warp) + 8 max sigma), which is four orders below what a wrong draw, knot or
    sensor index misses by."""
    x, sigma = float(src.abs().max()), float(np.max(jitter))
    tol = 2.0 ** -24 * (np.sqrt(3.0) * (8.0 + 134.0 * warp) * (1.0 + scale) * x + 48.0 * sigma)
    assert tol <= 64 * 2.0 ** -24 * (x * (1.0 + scale) * (1.0 + 2.0 * warp) + 8.0 * sigma)
    return tol


def _check_table(table, sensors, ids=IDS, **kw):
    k = {**KW, **kw}
    want = np.stack([S.params(i, k["site"], k["epoch"], k["seed"], sensors, k["max_angle"], k["scale"], k["warp"], k["warp_knots"], k["drop"])
                     for i in ids])
    S.check_table(table.numpy(), want, sensors)


def _compare(name, src, out, table, joints, idx=IDX, ids=IDS, valid=VALID, **kw):
    k = {**KW, **kw}
    want = S.transform(src.numpy(), idx, ids, table.numpy(), seed=k["seed"], epoch=k["epoch"], site=k["site"], knots=k["warp_knots"],
                       jitter=k["jitter"], valid=_valid(src.shape[1:], valid), joints=joints)
    err, tol = float(np.abs(out.double().numpy() - want).max()), _tolerance(src, k["scale"], k["warp"], k["jitter"])
    print(f"[sensors] {name} {tuple(src.shape)} joints {joints} knots {k['warp_knots']}: max error {err:.3e}, bound {tol:.3e}")
    assert err <= tol, (err, tol)


def _copied_through(src, out, joints, idx=IDX, valid=VALID):
    """frames at or behind the valid count, and joints outside [lo, hi), are the source's bits"""
    valid = _valid(src.shape[1:], valid)
    for k, s in enumerate(idx):
        v = _frames(src.shape[1:]) if valid is None else valid[s]
        if src.dim() == 3:
            assert torch.equal(out[k, v:].view(torch.int32), src[s, v:].view(torch.int32)), k
        else:
            lo, hi = joints
            assert torch.equal(out[k, :, v:].view(torch.int32), src[s, :, v:].view(torch.int32)), k
            for part in (slice(0, lo), slice(hi, None)):
                assert torch.equal(out[k, :, :, part].contiguous().view(torch.int32), src[s, :, :, part].contiguous().view(torch.int32)), k


@pytest.fixture(scope="module")
def runs():
    """every case once, shared: name -> (source, output, table, stats, its keywords)"""
    got = {}
    for i, (name, (shape, joints, knots, jitter)) in enumerate(CASES.items()):
        src = _src(*shape, seed=10 + i)
        kw = dict(warp_knots=knots, jitter=jitter)
        got[name] = (src, *_run(src, joints=joints, **kw), kw)
    return got


@pytest.mark.parametrize("name", list(CASES))
def test_against_the_float64_restatement(runs, name):
    shape, joints, knots, jitter = CASES[name]
    src, out, table, stats, kw = runs[name]
    sensors = shape[1] // 3 if joints is None else joints[1] - joints[0]
    assert out.shape == (4, *shape) and table.shape == (4, 12 + 12 * sensors) and stats.shape == (4, 2)
    assert torch.equal(stats, torch.tensor([0.0, 1.0]).expand(4, 2))
    _check_table(table, sensors, **kw)
    _compare(name, src, out, table, joints, **kw)
    _copied_through(src, out, joints)
    if _frames(shape) > 1:
        assert not torch.equal(out[0], out[2])                               # source row 5 twice, drawn for two samples


def test_clips_of_one_and_two_valid_frames():
    """the source rows the shared batch does not gather: valid = 1 (q = 0: the first knot), 2, 5 and 13"""
    src = _src(13, 6, seed=2)
    idx, ids = [1, 2, 6, 4], [7, 8, 9, 10]
    for knots in (2, 8):
        out, table, _ = _run(src, idx=idx, ids=ids, warp_knots=knots)
        _check_table(table, 2, ids=ids, warp_knots=knots)
        _compare("short", src, out, table, None, idx=idx, ids=ids, warp_knots=knots)
        _copied_through(src, out, None, idx=idx)
    out2, table2, _ = _run(src, idx=[4], ids=[10], valid=None, warp_knots=8)  # valid == NULL counts as T: row 4 holds 13 valid frames
    assert torch.equal(out2[0], out[3]) and torch.equal(table2[0], table[3])


def test_a_dropped_sensor_is_zero_in_its_valid_frames():
    ids = [40, 41, 42, 43]
    flags = np.stack([S.params(i, KW["site"], KW["epoch"], KW["seed"], 2, KW["max_angle"], KW["scale"], KW["warp"], 4, 0.5) for i in ids])
    flags = flags[:, 12:].reshape(4, 2, 12)[:, :, 1]
    assert flags.min() == 0 and flags.max() == 1                             # the restatement: these ids hold a dropped and a kept sensor
    sig, skel = _src(13, 6, seed=3), _src(2, 13, 22, 3, seed=4)
    for src, joints in ((sig, None), (skel, (20, 22))):
        out, table, _ = _run(src, ids=ids, joints=joints, drop=0.5, jitter=(0.05, 0.002))
        assert np.array_equal(table[:, 12:].reshape(4, 2, 12)[:, :, 1].numpy(), flags)
        _compare("drop", src, out, table, joints, ids=ids, drop=0.5, jitter=(0.05, 0.002))
        _copied_through(src, out, joints)
        units = out.reshape(4, 13, 2, 3) if joints is None else out[:, :, :, 20:22]
        for k, s in enumerate(IDX):
            for g in range(2):
                part = units[k, :VALID[s], g] if joints is None else units[k, :, :VALID[s], g]
                zero = bool((part.contiguous().view(torch.int32) == 0).all())            # +0: no bit set
                assert zero == bool(flags[k, g]), (k, g)


def test_identity_parameters_give_the_gathered_rows():
    for name, (shape, joints, knots, _) in CASES.items():
        src = _src(*shape, seed=5)
        sensors = shape[1] // 3 if joints is None else joints[1] - joints[0]
        for valid in (None, VALID):
            out, table, stats = _run(src, valid=valid, joints=joints, warp_knots=knots, **IDENTITY)
            assert torch.equal(out, src.index_select(0, torch.tensor(IDX))), name
            want = torch.tensor([1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0] + ([1.0] + [0.0] * 11) * sensors)
            assert torch.equal(table, want.expand(4, -1)) and torch.equal(stats, torch.tensor([0.0, 1.0]).expand(4, 2)), name


def test_signal_and_sensor_joints_of_every_body_receive_the_same_values():
    sig = _src(13, 6, seed=6)
    skel = _src(2, 13, 22, 3, seed=7)
    skel[:, :, :, 20:22] = sig.reshape(ROWS, 1, 13, 2, 3)                    # "joint V + j of EVERY body holds the recording"
    kw = dict(jitter=(0.05, 0.002), drop=0.3, warp_knots=8)
    a, ta, _ = _run(sig, **kw)
    b, tb, _ = _run(skel, joints=(20, 22), **kw)
    assert torch.equal(ta.view(torch.int32), tb.view(torch.int32))
    for body in range(2):
        assert torch.equal(b[:, body, :, 20:22].reshape(4, 13, 6).view(torch.int32), a.view(torch.int32)), body
    assert not torch.equal(a, sig[IDX])
    # and the min-max form of the signal is the float32 formula on what the sensor joints of either body hold, with its mn, mx
    norm, tn, stats = _run(sig, minmax=True, **kw)
    assert torch.equal(tn.view(torch.int32), tb.view(torch.int32))
    for body in range(2):
        want, want_stats = S.minmax32(b[:, body, :, 20:22].reshape(4, 13, 6).numpy())
        assert np.array_equal(norm.numpy().view(np.int32), want.view(np.int32)), body
        assert np.array_equal(stats.numpy().view(np.int32), want_stats.view(np.int32)), body


def test_minmax_is_the_float32_formula_on_the_plain_output():
    for shape, knots in (((13, 6), 4), ((1, 6), 2), ((5, 48), 8), ((300, 6), 8)):      # 600 triples: more than the workgroup's lanes
        src = _src(*shape, seed=8) * 3.0 + 1.0
        valid = [shape[0]] + VALID[1:]
        kw = dict(warp_knots=knots, drop=0.2, valid=valid)
        plain, table, _ = _run(src, **kw)
        out, table2, stats = _run(src, minmax=True, **kw)
        want, want_stats = S.minmax32(plain.numpy())
        assert torch.equal(table, table2)
        assert np.array_equal(stats.numpy().view(np.int32), want_stats.view(np.int32)), shape
        assert np.array_equal(out.numpy().view(np.int32), want.view(np.int32)), shape
        assert float(out.min()) == 0.0 and float(out.max()) == 1.0
        if shape == (300, 6):
            _compare("long", src, plain, table, None, **kw)
            _copied_through(src, plain, None, valid=valid)


def test_non_finite_inputs_stay_visible_and_contained():
    src = _src(13, 6, seed=9)
    clean, _, _ = _run(src, valid=None)
    for bad in (float("nan"), float("inf"), float("-inf")):
        dirty = src.clone()
        dirty[5, 4, 1] = bad                                                 # sensor 0 of frame 4 of source row 5: batch rows 0 and 2
        out, _, _ = _run(dirty, valid=None)
        hit = torch.zeros(4, 13, 6, dtype=torch.bool)
        hit[0, 4, :3] = hit[2, 4, :3] = True
        assert not torch.isfinite(out[hit]).any() and torch.equal(out[~hit], clean[~hit]), bad
        norm, _, stats = _run(dirty, valid=None, minmax=True)
        if bad != bad:
            assert torch.isnan(norm[0]).all() and torch.isnan(norm[2]).all() and torch.isnan(stats[[0, 2]]).all()
        assert torch.isfinite(norm[[1, 3]]).all() and torch.isfinite(stats[[1, 3]]).all()


def test_rows_depend_on_seed_site_epoch_and_sample_alone(runs):
    src, out, table, _, kw = runs["skeleton"]
    again, table2, _ = _run(src, joints=(20, 22), **kw)
    assert torch.equal(again, out) and torch.equal(table2, table)            # two calls from one state
    for other in (dict(epoch=4), dict(site=3), dict(seed=KW["seed"] + 1)):
        o2, t2, _ = _run(src, joints=(20, 22), **{**kw, **other})
        assert all(not torch.equal(o2[k], out[k]) and not torch.equal(t2[k], table[k]) for k in range(4)), other
    # a row's result depends neither on its position in the batch nor on the other rows -- with min-max too
    sig, plain, sig_table, _, skw = runs["signal"]
    norm, _, stats = _run(sig, minmax=True, **skw)
    perm = [2, 0, 3, 1]
    o3, t3, _ = _run(src, idx=[IDX[p] for p in perm], ids=[IDS[p] for p in perm], joints=(20, 22), **kw)
    assert torch.equal(o3, out[perm]) and torch.equal(t3, table[perm])
    o4, t4, _ = _run(src, idx=[IDX[2]], ids=[IDS[2]], joints=(20, 22), **kw)
    assert torch.equal(o4[0], out[2]) and torch.equal(t4[0], table[2])
    n3, _, s3 = _run(sig, idx=[IDX[p] for p in perm], ids=[IDS[p] for p in perm], minmax=True, **skw)
    assert torch.equal(n3, norm[perm]) and torch.equal(s3, stats[perm])
    n4, t4, s4 = _run(sig, idx=[IDX[2], 6, 1], ids=[IDS[2], 5, 6], minmax=True, **skw)
    assert torch.equal(n4[0], norm[2]) and torch.equal(s4[0], stats[2]) and torch.equal(t4[0], sig_table[2])


def test_wrapper_refusals():
    from fusion_gcn_amd import _lib, ops
    sig, skel = guarded.to(_src(13, 6), DEV), guarded.to(_src(2, 13, 22, 3), DEV)
    idx, ids, kw = torch.arange(4), torch.arange(4), dict(seed=1, epoch=0)
    with pytest.raises(_lib.FgcnError, match="rows outside"):
        ops.clip_sensors(sig, torch.tensor([7]), torch.tensor([0]), **kw)
    with pytest.raises(_lib.FgcnError, match="valid"):
        ops.clip_sensors(sig, idx, ids, valid=torch.ones(ROWS, dtype=torch.int64, device=DEV), **kw)
    with pytest.raises(_lib.FgcnError, match="alias"):
        ops.clip_sensors(sig, torch.arange(ROWS), torch.arange(ROWS), out=sig, **kw)
    with pytest.raises(_lib.FgcnError, match="jitter holds 3"):
        ops.clip_sensors(sig, idx, ids, jitter=(0.1, 0.2, 0.3), **kw)
    with pytest.raises(_lib.FgcnError, match="joints"):
        ops.clip_sensors(skel, idx, ids, **kw)                               # a skeleton without a sensor range
    with pytest.raises(_lib.FgcnError, match="joints"):
        ops.clip_sensors(sig, idx, ids, joints=(0, 2), **kw)
    with pytest.raises(_lib.FgcnError, match="minmax"):
        ops.clip_sensors(skel, idx, ids, joints=(20, 22), minmax=True, **kw)
    with pytest.raises(_lib.FgcnError, match="sensor range"):
        ops.clip_sensors(skel, idx, ids, joints=(20, 23), **kw)


# ---- ClipBatches ----------------------------------------------------------------------------------------------------------------------
N, BS, M, T, V, L = 10, 4, 2, 13, 6, 10
PARENTS = [1, 1, 1, 2, 0, 4, -1, -1]                   # six joints and the two sensor joints Inertial(enhance=True) appends


@pytest.fixture(scope="module")
def raw_dataset(tmp_path_factory):
    """-> (the data set, the frame counts): skeletons of 5 to 13 recorded frames, recordings of 2 to L frames in sensor-sized units"""
    from fusion_gcn_amd.data import MultiModalDataset, NumpyDatasetLoader, NumpyWriter
    root = str(tmp_path_factory.mktemp("sensors"))
    rng = np.random.default_rng(21)
    frames = {"skeleton": rng.integers(5, T + 1, N), "inertial": rng.integers(2, L + 1, N)}
    arrays = {"skeleton": rng.standard_normal((N, M, T, V, 3)).astype(np.float32),
              "inertial": (rng.standard_normal((N, L, 6)) * np.array([1.0, 1.0, 1.0, 50.0, 50.0, 50.0])).astype(np.float32)}
    for name, a in arrays.items():
        with NumpyWriter(os.path.join(root, f"{name}_train_features.npy"), np.float32, a.shape) as w:
            for s in a:
                w.collect_next(s)
    np.save(os.path.join(root, "train_labels.npy"), np.arange(N) % 4)
    return MultiModalDataset([(root, NumpyDatasetLoader())], "train"), frames


def _epoch(ds, frames, epoch, **kw):
    """-> (the iterator, [(features, labels, indices, tables)] of one pass, on the host)"""
    from fusion_gcn_amd.data import Augment, ClipBatches, Inertial, Sensors, Streams
    it = ClipBatches(ds, BS, shuffle=True, seed=5, device=DEV, inertial=Inertial(frames=frames, enhance=True, minmax=False),
                     augment=Augment(joints=(0, V)), sensors=Sensors(joints=(V, V + 2), minmax=True, warp=0.1, jitter=(0.05, 2.0), drop=0.3),
                     streams=Streams(PARENTS, streams=("joint", "bone")), **kw)
    it.set_epoch(epoch)
    out = []
    for feats, lab, idx in it:
        assert set(it.last_sensors) == {"skeleton", "inertial"}
        assert all(p.shape == (len(idx), 36) and s.shape == (len(idx), 2) for p, s in it.last_sensors.values())
        out.append(({k: v.cpu() for k, v in feats.items()}, lab.cpu(), idx.clone(), {k: (p.cpu(), s.cpu()) for k, (p, s) in it.last_sensors.items()}))
    torch.cuda.synchronize()
    return it, out


def _same(a, b):
    return len(a) == len(b) and all(
        torch.equal(x[2], y[2]) and torch.equal(x[1], y[1]) and list(x[0]) == list(y[0])
        and all(torch.equal(x[0][k].view(torch.int32), y[0][k].view(torch.int32)) for k in x[0])
        and all(torch.equal(x[3][k][j].view(torch.int32), y[3][k][j].view(torch.int32)) for k in x[3] for j in range(2)) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def resident_epoch3(raw_dataset):
    return _epoch(*raw_dataset, 3, resident=True)


def test_clip_batches_resident_and_streaming_deliver_the_same_bits(raw_dataset, resident_epoch3):
    it, res = resident_epoch3
    it2, stream = _epoch(*raw_dataset, 3, resident=False)
    assert it.resident and not it2.resident
    assert [s.name for s in it.stages] == [s.name for s in it2.stages] == ["inertial", "augment", "sensors", "streams"]
    assert it.out_keys == ["inertial", "skeleton", "skeleton_bone"] and it.shapes["skeleton"] == (M, T, V + 2, 3)
    assert [len(b[2]) for b in res] == [4, 4, 2]
    assert _same(stream, res)
    for feats, _, idx, tables in res:
        (ps, ss), (pi, si) = tables["skeleton"], tables["inertial"]
        assert torch.equal(ps, pi) and torch.equal(ss, torch.tensor([0.0, 1.0]).expand(len(idx), 2))      # one draw for both arrays of a sample
        # the signal is the float32 min-max of what the sensor joints of either body hold: both were resampled and augmented alike
        for body in range(M):
            want, stats = S.minmax32(feats["skeleton"][:, body, :, V:].reshape(len(idx), T, 6).numpy())
            assert np.array_equal(feats["inertial"].numpy().view(np.int32), want.view(np.int32)), body
            assert np.array_equal(si.numpy().view(np.int32), stats.view(np.int32))
        assert torch.equal(feats["skeleton_bone"][:, :, :, V:], feats["skeleton"][:, :, :, V:])        # sensor joints are copied through
        dropped = pi[:, 12:].reshape(len(idx), 2, 12)[:, :, 1]
        for k in range(len(idx)):
            for g in range(2):
                assert bool((feats["skeleton"][k, :, :, V + g] == 0).all()) == bool(dropped[k, g]), (k, g)


def test_clip_batches_two_ranks_concatenate_to_one(raw_dataset, resident_epoch3):
    ranks = [_epoch(*raw_dataset, 3, resident=r == 0, rank=r, world=2)[1] for r in range(2)]          # (one rank resident, one streaming)
    assert [len(b[2]) for b in ranks[0]] == [2, 2, 1] and [len(b[2]) for b in ranks[1]] == [2, 2, 1]
    for one, r0, r1 in zip(resident_epoch3[1], *ranks):
        both = ({k: torch.cat([r0[0][k], r1[0][k]]) for k in one[0]}, torch.cat([r0[1], r1[1]]), torch.cat([r0[2], r1[2]]),
                {k: tuple(torch.cat([r0[3][k][j], r1[3][k][j]]) for j in range(2)) for k in one[3]})
        assert _same([one], [both])


def test_clip_batches_repeat_an_epoch_and_change_with_it(raw_dataset, resident_epoch3):
    assert _same(_epoch(*raw_dataset, 3, resident=True)[1], resident_epoch3[1])
    other = _epoch(*raw_dataset, 4, resident=True)[1]
    by_clip = {int(i): b[3]["inertial"][0][j] for b in resident_epoch3[1] for j, i in enumerate(b[2])}
    for _, _, idx, tables in other:
        for j, i in enumerate(idx.tolist()):
            assert not torch.equal(tables["inertial"][0][j], by_clip[i]), i


def test_a_later_stage_reads_the_valid_frames_of_the_batch_s_clips(tmp_path):
    """``Sensors`` is the one per-batch stage that writes a feature without filling its frames, so the stage behind it may hold a
    ``valid_frames`` table of its own: on the resident path that stage reads rows 0..m-1 of what ``Sensors`` wrote, and its table must be
    the batch's entries, not the data set's first m.  No ``Augment``, shuffled batches, every clip another frame count and values in every
    frame: the motion of a clip ends at ITS count on both paths, bit for bit the same."""
    from fusion_gcn_amd.data import ClipBatches, MultiModalDataset, NumpyDatasetLoader, NumpyWriter, Sensors, Streams
    rng = np.random.default_rng(31)
    arrays = {"skeleton": rng.standard_normal((N, M, T, V + 2, 3)).astype(np.float32),
              "inertial": rng.standard_normal((N, T, 6)).astype(np.float32)}
    for name, a in arrays.items():
        with NumpyWriter(os.path.join(str(tmp_path), f"{name}_train_features.npy"), np.float32, a.shape) as w:
            for s in a:
                w.collect_next(s)
    np.save(os.path.join(str(tmp_path), "train_labels.npy"), np.arange(N) % 4)
    ds = MultiModalDataset([(str(tmp_path), NumpyDatasetLoader())], "train")
    vf = np.array([3, 13, 5, 11, 2, 9, 4, 12, 6, 8])

    def epoch(resident):
        it = ClipBatches(ds, BS, shuffle=True, seed=5, device=DEV, resident=resident,
                         sensors=Sensors(joints=(V, V + 2), warp=0.1, jitter=0.05, valid_frames={"skeleton": vf, "inertial": vf}),
                         streams=Streams(PARENTS, streams=("joint", "motion"), valid_frames={"skeleton": vf}))
        it.set_epoch(2)
        out = [({k: v.cpu() for k, v in feats.items()}, idx.clone()) for feats, _, idx in it]
        torch.cuda.synchronize()
        assert it.resident == resident and [s.name for s in it.stages] == ["sensors", "streams"]
        return out

    res, stream = epoch(True), epoch(False)
    assert [len(i) for _, i in res] == [4, 4, 2] and res[0][1].tolist() != [0, 1, 2, 3]
    for (a, idx), (b, idx2) in zip(res, stream):
        assert torch.equal(idx, idx2) and list(a) == list(b) == ["inertial", "skeleton", "skeleton_motion"]
        for k in a:
            assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
        for j, i in enumerate(idx.tolist()):
            v, motion, src = int(vf[i]), a["skeleton_motion"][j], torch.from_numpy(arrays["skeleton"][i])
            assert bool((motion[:, v - 1:].contiguous().view(torch.int32) == 0).all()), (i, v)       # +0 from the clip's last valid frame on
            assert bool((motion[:, :v - 1] != 0).all()), (i, v)
            assert torch.equal(a["skeleton"][j][:, v:], src[:, v:]) and torch.equal(a["skeleton"][j][:, :, :V], src[:, :, :V])
            assert not torch.equal(a["skeleton"][j][:, :v, V:], src[:, :v, V:])
            assert torch.equal(motion[:, :v - 1, :V], src[:, 1:v, :V] - src[:, :v - 1, :V])


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
def test_graph_step_training_on_sensor_augmented_batches_repeats_bit_for_bit(tmp_path):
    """Three GraphStep training steps of a two-block skeleton_imu_spatial_fusion model on batches prepared from raw recordings, augmented
    and sensor-augmented (the streaming path): the batch is the recorded graph's input, so the recording verifies as it does without the
    stage, and the loop run a second time from the same seeds ends on the same loss and parameters, bit for bit."""
    from fusion_gcn_amd.data import Augment, ClipBatches, Inertial, MultiModalDataset, NumpyDatasetLoader, NumpyWriter, Sensors
    from fusion_gcn_amd.datasets.utd_mhad import constants as utd
    from fusion_gcn_amd.optim import FlatOptimizer
    from fusion_gcn_amd.session.procedures import GraphStep
    from fusion_gcn_amd.util import Graph
    from fusion_gcn_amd.util.dynamic_import import import_model
    from oracle import filler
    n, frames_t, joints, classes = 12, 16, 20, 5
    rng = np.random.default_rng(9)
    frames = {"skeleton": rng.integers(8, frames_t + 1, n), "inertial": rng.integers(4, 21, n)}
    for name, a in (("skeleton", rng.standard_normal((n, 1, frames_t, joints, 3))), ("inertial", rng.standard_normal((n, 20, 6)))):
        with NumpyWriter(os.path.join(str(tmp_path), f"{name}_train_features.npy"), np.float32, a.shape) as w:
            for s in a.astype(np.float32):
                w.collect_next(s)
    np.save(os.path.join(str(tmp_path), "train_labels.npy"), np.arange(n) % classes)
    ds = MultiModalDataset([(str(tmp_path), NumpyDatasetLoader())], "train")

    def run():
        model = import_model("mmargcn")({"skeleton": (1, frames_t, joints + 2, 3)}, classes, Graph(utd.skeleton_edges, center_joint=utd.center_joint),
                                        mode="skeleton_imu_spatial_fusion", num_imu_joints=2, imu_enhanced_mode="append_center", num_layers=2)
        filler.fill_state_dict(model.state_dict(), rename=lambda k: k.replace("_model.agcn.", ""))
        model = guarded.to(model, DEV).train()
        opt = FlatOptimizer(model.parameters(), "SGD", 0.01, momentum=0.9)
        step = GraphStep(verify=True)
        batches = ClipBatches(ds, 4, shuffle=True, seed=3, device=DEV, resident=False, inertial=Inertial(frames=frames, enhance=True, minmax=False),
                              augment=Augment(joints=(0, joints)),
                              sensors=Sensors(joints=(joints, joints + 2), minmax=True, warp=0.1, jitter=0.05, drop=0.2))
        batches.set_epoch(1)
        losses = []
        for x, y, _ in batches:
            opt.zero_grad()
            _, loss = step.forward(model, F.cross_entropy, x["skeleton"], y)
            step.backward(loss)
            step.run_optimizer_step(opt)
            losses.append(loss.detach().clone())
        torch.cuda.synchronize()
        assert step.replays == 3 and len(step._recorded) == 1
        return torch.stack(losses).cpu(), torch.cat([p.detach().reshape(-1) for p in model.parameters()]).cpu()

    (l1, p1), (l2, p2) = run(), run()
    assert bool(torch.isfinite(l1).all()) and len(set(l1.tolist())) == 3
    assert torch.equal(l1, l2) and torch.equal(p1, p2)
