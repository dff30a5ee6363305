"""Augmentation of inertial recordings as ClipBatches gathers them, the part that needs no GPU: the parameter table
of fgcn_sensors_params -- the host copy of the functions the kernel calls -- against the float64 restatement of tests/sensors_ref.py, the
identity row, the counter words it reads, the host-side argument checks of fgcn_clip_sensors (they precede any launch) and of ``Sensors``,
and the two promises of the Python surface that hold without a device: no host fallback, and ``sensors=None`` delivers what it always
delivered."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import sensors_ref as S
from fusion_gcn_amd import _lib, build
from test_data import write_split

ANGLES, SCALE, WARP, KNOTS, DROP, G = (0.3, 0.2, 0.5), 0.1, 0.2, 8, 0.5, 3


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def _row(lib, sample, site, epoch, seed, sensors=G, max_angle=ANGLES, scale=SCALE, warp=WARP, knots=KNOTS, drop=DROP):
    out = (C.c_float * S.row_floats(sensors))()
    assert lib.fgcn_sensors_params(sample, site, epoch, seed, (C.c_float * 3)(*max_angle), scale, warp, knots, drop, sensors, out) == 0
    return np.array(list(out), dtype=np.float32)


def _tuples():
    """51 (sample, site, epoch, seed): the corners of the counter and of the key (a sample id above 2^31, a 64-bit seed), then random ones"""
    rng = np.random.default_rng(12)
    fixed = [(0, 0, 0, 0), (2 ** 32 - 1, 2 ** 32 - 1, 2 ** 32 - 1, 2 ** 64 - 1), (2 ** 31 + 7, 0, 49, 0x1234567887654321)]
    return fixed + [(int(rng.integers(0, 2 ** 32)), int(rng.integers(0, 8)), int(rng.integers(0, 200)), int(rng.integers(0, 2 ** 64, dtype=np.uint64)))
                    for _ in range(48)]


def test_parameter_table_matches_the_float64_restatement(lib):
    tuples = _tuples()
    got = np.stack([_row(lib, *t) for t in tuples])
    want = np.stack([S.params(*t, G, ANGLES, SCALE, WARP, KNOTS, DROP) for t in tuples])
    S.check_table(got, want, G)
    groups = got[:, 12:].reshape(len(tuples), G, 12)
    assert np.all(np.abs(groups[:, :, 0] - 1) <= SCALE * (1 + 2 ** -23)) and np.all(np.abs(groups[:, :, 4:]) <= WARP)
    assert 0.25 < groups[:, :, 1].mean() < 0.75                                 # drop = 0.5: both kinds occur
    assert len({tuple(r) for r in got.tolist()}) == len(tuples)                  # every tuple draws its own row
    assert len({tuple(g) for g in groups.reshape(-1, 12).tolist()}) == len(tuples) * G      # and every sensor its own group
    # each coordinate of the counter and both key words matter, to the rotation and to every group
    base = _row(lib, 5, 1, 2, 3)
    for other in ((6, 1, 2, 3), (5, 2, 2, 3), (5, 1, 3, 3), (5, 1, 2, 4), (5, 1, 2, 3 + 2 ** 32)):
        row = _row(lib, *other)
        assert all(not np.array_equal(row[lo:lo + 12], base[lo:lo + 12]) for lo in range(0, len(base), 12)), other
    # fewer knots: the same first knots, zeros behind them; K = 0: none.  A sensor's group does not depend on how many sensors there are
    for knots in (0, 2, 4, 5):
        fewer = _row(lib, 5, 1, 2, 3, knots=knots).reshape(-1, 12)
        assert np.array_equal(fewer[1:, 4:4 + knots], base.reshape(-1, 12)[1:, 4:4 + knots]) and np.all(fewer[1:, 4 + knots:] == 0)
        assert np.array_equal(fewer[:, :4], base.reshape(-1, 12)[:, :4])
    assert np.array_equal(_row(lib, 5, 1, 2, 3, sensors=16)[:len(base)], base) and np.array_equal(_row(lib, 5, 1, 2, 3, sensors=1), base[:24])
    # drop = 0 drops nothing, whatever the word
    assert np.all(np.stack([_row(lib, *t, drop=0.0) for t in tuples])[:, 12:].reshape(-1, 12)[:, 1] == 0)


def test_zero_magnitudes_give_the_identity_row_exactly(lib):
    want = np.concatenate([[1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]] + [[1] + [0] * 11] * G).astype(np.float32)
    for t in _tuples()[:12]:
        row = _row(lib, *t, max_angle=(0.0, 0.0, 0.0), scale=0.0, warp=0.0, drop=0.0)
        assert np.array_equal(row, want), (t, row)
    from fusion_gcn_amd import ops
    assert ops.sensors_params(3, 0, 1, 7, 2) == [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0] + ([1] + [0] * 11) * 2      # the wrapper's defaults are the identity too


def test_the_row_reads_none_of_the_counter_words_of_augment_and_window(lib):
    """Augment draws from blocks j = 0, 1 and Window from j = 2 of the same (sample, site, epoch, seed): the restatement, which reads blocks
    3 and 16 + 4g .. alone, reproduces the row (above), the row's uniforms are not those blocks', and no parameter of the two other stages
    is an argument of the entry point -- changing them moves their rows and leaves this one."""
    from fusion_gcn_amd import ops
    t = (77, 1, 4, 0xABCDEF0123456789)
    row = _row(lib, *t, max_angle=(1.0, 1.0, 1.0), scale=0.5, warp=0.5, knots=8)
    mine = np.concatenate([np.arcsin(-row[6:7]), row[12::12] - 1.0, row[16:24], row[28:36]]).astype(np.float64)
    for j in (0, 1, 2):
        u = 2.0 * S._uniform(S._block(*t[:3], t[3], j)) - 1.0
        assert not np.isclose(mine[:, None], np.concatenate([u, 0.5 * u])[None, :], rtol=0, atol=1e-6).any(), j
    before = _row(lib, *t)
    rows = [ops.augment_params(*t, max_angle=a, scale=s, min_window=w) for a, s, w in (((0.3, 0.3, 0.3), 0.1, 0.5), ((0.1, 0.2, 0.3), 0.3, 0.9))]
    wins = [ops.window_params(*t, interval=i) for i in ((0.5, 1.0), (0.2, 0.4))]
    assert rows[0] != rows[1] and wins[0] != wins[1]
    assert np.array_equal(_row(lib, *t), before)


def test_the_restatement_on_the_library_s_rows(lib):
    """the curve goes through its knots -- the library's own, of a drawn row -- and is flat for equal ones; the noise is standard normal; the
    transform from the library's identity row is the gather"""
    drawn = _row(lib, 9, 0, 1, 5, sensors=1, warp=0.2, knots=8)[16:24].astype(np.float64)
    assert np.abs(drawn).max() <= 0.2 and len(set(drawn.tolist())) == 8
    for K in (2, 4, 8):
        assert np.allclose([S.catmull_rom(drawn, K, 4 * k, 4 * (K - 1) + 1) for k in range(K)], drawn[:K], atol=1e-15)
    d = np.array([0.1, -0.2, 0.05, 0.15, -0.1, 0.0, 0.2, -0.05])
    for K in (2, 4, 8):
        v = 4 * (K - 1) + 1
        assert np.allclose([S.catmull_rom(d, K, 4 * k, v) for k in range(K)], d[:K], atol=1e-15)
        assert all(abs(S.catmull_rom(d, K, t, v)) <= 1.25 * 0.2 for t in range(v))
        assert np.allclose([S.catmull_rom(np.full(8, 0.07), K, t, v) for t in range(v)], 0.07)
    assert S.warp(d, 0, 3, 9) == 1.0 and S.warp(d, 4, 0, 1) == 1.0 + d[0]
    n = np.stack([S.noise(9, 0, 1, 5, t, g, 2) for t in range(400) for g in range(2)])
    assert abs(n.mean()) < 0.1 and abs(n.std() - 1.0) < 0.1 and abs(np.corrcoef(n.T)[0, 1]) < 0.15 and np.abs(n).max() < 5.8
    rng = np.random.default_rng(3)
    src = rng.standard_normal((4, 5, 6))
    ident = _row(lib, 0, 0, 0, 0, sensors=2, max_angle=(0.0, 0.0, 0.0), scale=0.0, warp=0.0, knots=4, drop=0.0)
    ident = np.tile(ident.astype(np.float64), (3, 1))
    kw = dict(seed=1, epoch=0, site=0, knots=4, jitter=0.0)
    assert np.array_equal(S.transform(src, [2, 0, 2], [0, 1, 2], ident, **kw), src[[2, 0, 2]])
    dropped = ident.copy()
    dropped[0, 12 + 12 + 1] = 1.0                                               # sensor 1 of row 0
    out = S.transform(src, [2, 0, 2], [0, 1, 2], dropped, valid=[5, 5, 3, 5], **kw)
    assert np.all(out[0, :3, 3:] == 0) and np.array_equal(out[0, 3:], src[2, 3:]) and np.array_equal(out[0, :, :3], src[2, :, :3])
    y, stats = S.minmax32(src.astype(np.float32))
    assert y.min() == 0 and y.max() == 1 and np.array_equal(stats[:, 0], src.astype(np.float32).reshape(4, -1).min(1))


def test_host_side_validation(lib):
    """include/fgcn.h's list: each refusal is FGCN_E_BADARG with a message, before any launch (no device is touched: this runs without one)."""
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    ang, jit = (C.c_float * 3)(0.3, 0.3, 0.3), (C.c_float * 16)(*[0.1] * 16)

    def call(src=p, idx=p + 64, ids=p + 96, valid=None, out=p + 128, params=p + 192, stats=p + 224, b=1, outer=2, T=4, inner=12, lo=2, hi=4,
             angles=ang, scale=0.1, warp=0.1, knots=4, jitter=jit, drop=0.1, minmax=0):
        return lib.fgcn_clip_sensors(src, idx, ids, valid, out, params, stats, b, outer, T, inner, lo, hi, angles, scale, warp, knots, jitter, drop,
                                     minmax, 7, 0, 0, None)

    def refused(text, **kw):
        assert call(**kw) == -1, kw
        assert text in lib.fgcn_last_error(), (kw, lib.fgcn_last_error())

    for name in ("src", "idx", "ids", "out", "params", "stats", "jitter", "angles"):
        refused(b"null pointer", **{name: None})
    for name in ("b", "outer", "T", "inner"):
        for bad in (0, -3):
            refused(b"bad b/outer/T/inner", **{name: bad})
    refused(b"not a number of triples", inner=13)
    for lo, hi in ((-1, 2), (0, 5), (2, 1), (3, 3)):
        refused(b"sensor range", lo=lo, hi=hi)
    refused(b"sensors outside", inner=3 * 17, lo=0, hi=17)
    for what in ("scale", "warp", "drop"):
        for bad in (-0.1, 1.0, 2.0, math.nan, math.inf):
            refused(what.encode(), **{what: bad})
    for bad in (-1, 1, 9, 100):
        refused(b"warp_knots", knots=bad)
    for e in range(3):
        for bad in (math.nan, math.inf, -math.inf):
            a = [0.3, 0.3, 0.3]
            a[e] = bad
            refused(b"not finite", angles=(C.c_float * 3)(*a))
    for bad in (-0.5, math.nan, math.inf):
        refused(b"jitter[1]", jitter=(C.c_float * 2)(0.1, bad))
    refused(b"minmax", minmax=1)                                                # outer = 2: no (T, S) signal
    refused(b"alias", out=p)
    refused(b"counter words", outer=1, T=2 ** 27, inner=48, lo=0, hi=16)
    refused(b"2^29", outer=1, T=2 ** 27, inner=6, lo=0, hi=1)
    refused(b"one grid", b=2 ** 17, outer=2 ** 15, T=2 ** 20, inner=3, lo=0, hi=1)
    # the host entry point refuses the same magnitudes
    out = (C.c_float * 36)()
    assert lib.fgcn_sensors_params(0, 0, 0, 0, None, 0.1, 0.1, 4, 0.1, 2, out) == -1 and b"null pointer" in lib.fgcn_last_error()
    assert lib.fgcn_sensors_params(0, 0, 0, 0, ang, 0.1, 0.1, 4, 0.1, 2, None) == -1 and b"null pointer" in lib.fgcn_last_error()
    assert lib.fgcn_sensors_params(0, 0, 0, 0, ang, 1.0, 0.1, 4, 0.1, 2, out) == -1 and b"scale" in lib.fgcn_last_error()
    assert lib.fgcn_sensors_params(0, 0, 0, 0, ang, 0.1, 1.0, 4, 0.1, 2, out) == -1 and b"warp" in lib.fgcn_last_error()
    assert lib.fgcn_sensors_params(0, 0, 0, 0, ang, 0.1, 0.1, 1, 0.1, 2, out) == -1 and b"warp_knots" in lib.fgcn_last_error()
    assert lib.fgcn_sensors_params(0, 0, 0, 0, ang, 0.1, 0.1, 4, 1.0, 2, out) == -1 and b"drop" in lib.fgcn_last_error()
    for bad in (0, 17, -1):
        assert lib.fgcn_sensors_params(0, 0, 0, 0, ang, 0.1, 0.1, 4, 0.1, bad, out) == -1 and b"sensors outside" in lib.fgcn_last_error()
    assert lib.fgcn_sensors_params(0, 0, 0, 0, (C.c_float * 3)(0, math.nan, 0), 0.1, 0.1, 4, 0.1, 2, out) == -1 and b"not finite" in lib.fgcn_last_error()


def test_sensors_object_validates_its_arguments():
    from fusion_gcn_amd.data import Sensors
    s = Sensors()
    assert (s.max_angle, s.scale, s.warp, s.warp_knots, s.jitter, s.drop, s.joints, s.minmax, s.site, s.only, s.valid_frames) == \
        ((0.3, 0.3, 0.3), 0.1, 0.0, 4, 0.0, 0.0, None, False, 0, None, {})
    assert (s.name, s.at_upload) == ("sensors", False) and not s.fills_frames("inertial")
    assert s.applies_to("inertial") and not Sensors(only=["inertial"]).applies_to("skeleton")
    assert s.sensor_range((11, 6)) == (0, 2) and s.sensor_range((11, 7)) is None and s.sensor_range((2, 13, 22, 3)) is None
    assert Sensors(joints=(20, 22)).sensor_range((2, 13, 22, 3)) == (20, 22) and Sensors(joints=(20, 22)).sensor_range((2, 13, 22, 2)) is None
    assert Sensors(jitter=(0.1, 0.2)).jitter == (0.1, 0.2)
    for kw in (dict(max_angle=(0.1, 0.2)), dict(max_angle=(0.1, math.nan, 0.0)), dict(scale=1.0), dict(scale=-0.1), dict(warp=1.0), dict(warp=-0.1),
               dict(drop=1.0), dict(drop=-0.5), dict(scale=math.nan), dict(warp_knots=1), dict(warp_knots=9), dict(warp_knots=2.5),
               dict(jitter=-0.1), dict(jitter=math.inf), dict(jitter=(0.1, math.nan)), dict(joints=(3, 3)), dict(joints=(-1, 2))):
        with pytest.raises(ValueError):
            Sensors(**kw)


def test_bind_writes_what_fits_and_refuses_the_rest():
    from fusion_gcn_amd.data import Sensors
    shapes = {"skeleton": (2, 13, 22, 3), "inertial": (13, 6), "odd": (13, 7), "flat": (2, 13, 22, 2)}
    keys, n = list(shapes), 5
    assert Sensors().bind(shapes, n, keys) == (shapes, ["inertial"])
    assert Sensors(joints=(20, 22)).bind(shapes, n, keys) == (shapes, ["skeleton", "inertial"])
    assert Sensors(joints=(20, 22), only=["skeleton"]).bind(shapes, n, keys)[1] == ["skeleton"]
    assert Sensors(jitter=(0.1, 0.2), joints=(20, 22)).bind(shapes, n, keys)[1] == ["skeleton", "inertial"]
    for only in (["odd"], ["flat"], ["skeleton"]):                               # 7 columns; two coordinates; a 4-d array without joints
        with pytest.raises(_lib.FgcnError, match="leave it out with Sensors"):
            Sensors(only=only).bind(shapes, n, keys)
    with pytest.raises(_lib.FgcnError, match="leave it out with Sensors"):
        Sensors(joints=(20, 22), only=["flat"]).bind(shapes, n, keys)
    with pytest.raises(_lib.FgcnError, match="at most 16"):
        Sensors().bind({"wide": (13, 51)}, n, ["wide"])
    with pytest.raises(ValueError, match="joints"):
        Sensors(joints=(20, 23)).bind(shapes, n, keys)
    with pytest.raises(ValueError, match="jitter holds 3"):
        Sensors(jitter=(0.1, 0.2, 0.3)).bind(shapes, n, keys)
    with pytest.raises(ValueError, match="does not have"):
        Sensors(only=["gyro"]).bind(shapes, n, keys)
    with pytest.raises(ValueError, match="not in the batch"):
        Sensors(only=["inertial"]).bind({"skeleton": shapes["skeleton"]}, n, keys)      # (an Inertial(drop_signal=True) in front)
    with pytest.raises(ValueError, match="valid_frames"):
        Sensors(valid_frames={"inertial": [14] * n}).bind(shapes, n, keys)      # more frames than T
    with pytest.raises(ValueError, match="does not apply"):
        Sensors(valid_frames={"skeleton": [3] * n}).bind(shapes, n, keys)       # no joints: the skeleton is not written
    s = Sensors(joints=(20, 22), valid_frames={"inertial": np.arange(1, 6), "skeleton": np.arange(2, 7)})
    s.bind(shapes, n, keys)
    tabs = s.tables(["skeleton", "inertial"], n)
    assert set(tabs) == {None, "skeleton", "inertial"} and tabs[None].tolist() == list(range(n)) and tabs["inertial"].dtype == np.int32


def test_no_host_fallback(tmp_path):
    from fusion_gcn_amd import ops
    from fusion_gcn_amd.data import ClipBatches, MultiModalDataset, NumpyDatasetLoader, Sensors
    write_split(str(tmp_path), "train", 9, {"skeleton": (2, 5, 22, 3), "inertial": (5, 6)})
    ds = MultiModalDataset([(str(tmp_path), NumpyDatasetLoader())], "train")
    for resident in (True, False):
        with pytest.raises(_lib.FgcnError, match="sensors"):
            ClipBatches(ds, 4, device="cpu", resident=resident, sensors=Sensors())
    with pytest.raises(_lib.FgcnError):
        ops.clip_sensors(torch.zeros(3, 5, 6), torch.arange(2), torch.arange(2), seed=1, epoch=0)


@pytest.mark.parametrize("resident", [True, False])
def test_without_sensors_the_batches_are_the_stored_rows(tmp_path, resident):
    from fusion_gcn_amd.data import ClipBatches, MultiModalDataset, NumpyDatasetLoader
    arrays, labels = write_split(str(tmp_path), "train", 19, {"skeleton": (2, 5, 22, 3), "inertial": (7, 6)})
    ds = MultiModalDataset([(str(tmp_path), NumpyDatasetLoader())], "train")
    it = ClipBatches(ds, 8, shuffle=True, seed=1, device="cpu", resident=resident, sensors=None)
    it.set_epoch(3)
    assert it.sensors is None and it.last_sensors == {} and it.stages == []
    seen = 0
    for feats, lab, idx in it:
        for k, a in arrays.items():
            assert torch.equal(feats[k], torch.from_numpy(a).index_select(0, idx)), k
        assert torch.equal(lab, torch.from_numpy(labels.astype(np.int64)).index_select(0, idx))
        seen += len(idx)
    assert seen == 19 and it.last_sensors == {}
