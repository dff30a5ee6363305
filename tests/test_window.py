"""The clip window ClipBatches applies as it gathers, the part that needs no GPU: the parameter table of
fgcn_window_params -- the host copy of the function the kernel calls -- against the float64 restatement of tests/window_ref.py, the
host-side argument checks of fgcn_clip_window and fgcn_clip_valid_frames (they precede any launch), the arguments of ``data.Window`` and
what ``ClipBatches`` refuses at construction, no host fallback, ``window=None`` against ``index_select``, and the sanity of the
restatement the GPU tests compare the kernels with."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import window_ref as R
from fusion_gcn_amd import _lib, build
from test_data import write_split

INTERVALS = [(0.5, 1.0), (0.3, 0.7), (0.25, 0.25), (0.9, 1.0), (1e-3, 0.6)]


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def _row(lib, sample, site, epoch, seed, lo, hi, mode=R.RANDOM):
    out = (C.c_float * 2)()
    assert lib.fgcn_window_params(sample, site, epoch, seed, lo, hi, mode, out) == 0
    return np.array(list(out), dtype=np.float32)


def _tuples():
    """51 (sample, site, epoch, seed, lo, hi): the corners of the counter and of the key, then random ones; the intervals in turn"""
    rng = np.random.default_rng(13)
    fixed = [(0, 0, 0, 0), (2 ** 32 - 1, 2 ** 32 - 1, 2 ** 32 - 1, 2 ** 64 - 1), (860, 0, 49, 1)]
    four = fixed + [(int(rng.integers(0, 2 ** 32)), int(rng.integers(0, 8)), int(rng.integers(0, 200)), int(rng.integers(0, 2 ** 64, dtype=np.uint64)))
                    for _ in range(48)]
    return [(*t, *INTERVALS[i % len(INTERVALS)]) for i, t in enumerate(four)]


def test_parameter_table_matches_the_float64_restatement(lib):
    tuples = _tuples()
    got = np.stack([_row(lib, *t) for t in tuples]).astype(np.float64)
    want = np.array([R.params(*t, R.RANDOM) for t in tuples])
    ulps = R.ulps32(got, want)
    print(f"[window] o, r against the restatement: at most {ulps.max():.2f} float32 ulps")
    assert np.all(ulps <= 4), (got, want)
    lo, hi = (np.array([np.float32(t[i]) for t in tuples], dtype=np.float64) for i in (4, 5))
    o, r = got[:, 0], got[:, 1]
    assert np.all((lo <= r) & (r <= hi)) and np.all(o >= 0) and np.all(o + r <= 1 + 2.0 ** -23)
    moving = [i for i, t in enumerate(tuples) if t[4] != t[5]]
    assert len({tuple(got[i]) for i in moving}) == len(moving)                 # every tuple draws its own row
    assert all(got[i][1] == np.float32(t[5]) for i, t in enumerate(tuples) if t[4] == t[5])      # lo == hi: the length is fixed
    # each coordinate of the counter and both key words matter
    base = _row(lib, 5, 1, 2, 3, 0.5, 1.0)
    for other in ((6, 1, 2, 3), (5, 2, 2, 3), (5, 1, 3, 3), (5, 1, 2, 4), (5, 1, 2, 3 + 2 ** 32)):
        assert not np.array_equal(_row(lib, *other, 0.5, 1.0), base), other


def test_centre_mode_draws_nothing(lib):
    for lo, hi in INTERVALS + [(1.0, 1.0)]:
        rows = [_row(lib, *t[:4], lo, hi, R.CENTRE) for t in _tuples()[:8]]
        assert all(np.array_equal(x, rows[0]) for x in rows)                   # whatever the sample, the epoch and the seed
        o, r = rows[0]
        assert r == np.float32(hi) and o == (np.float32(1) - r) / np.float32(2)
        assert R.ulps32(rows[0], R.params(0, 0, 0, 0, lo, hi, R.CENTRE)).max() <= 4
    from fusion_gcn_amd import ops
    assert ops.window_params(3, 0, 1, 7, (0.5, 0.75), "centre") == [0.125, 0.75]


def test_the_whole_recording_gives_offset_zero_and_length_one_exactly(lib):
    for t in _tuples()[:12]:
        for mode in (R.RANDOM, R.CENTRE):
            assert tuple(_row(lib, *t[:4], 1.0, 1.0, mode)) == (0.0, 1.0), (t, mode)
    from fusion_gcn_amd import ops
    assert ops.window_params(3, 0, 1, 7) == [0, 1]                             # the wrapper's defaults are the identity too


def test_counter_word_two_is_the_one_that_is_used(lib):
    """Augment draws its temporal part from word 0 of block j = 1 at the same (sample, site, epoch, seed): with (lo, hi) = (min_window, 1)
    both are r = lo + u (1 - lo), so equal words would give equal r.  They differ, and the window's r is the restatement's at j = 2."""
    for t in _tuples()[:20]:
        four = t[:4]
        r = float(_row(lib, *four, 0.5, 1.0)[1])
        table = (C.c_float * 12)()
        assert lib.fgcn_augment_params(*four, (C.c_float * 3)(0, 0, 0), 0.0, 0.5, table) == 0
        assert r != table[10], four
        u = {j: float(R.words(*four, j=j)[0] >> np.uint32(8)) * R.U24 for j in (0, 1, 2)}
        assert r == np.float32(0.5 + 0.5 * u[2]) and table[10] == np.float32(0.5 + 0.5 * u[1])      # (0.5 + 0.5 u has one rounding)
        assert u[2] != u[1] and u[2] != u[0]


def test_host_side_validation(lib):
    """include/fgcn.h's lists: each refusal is FGCN_E_BADARG with a message, before any launch (no device is touched: this runs without one)."""
    buf = (C.c_float * 64)()
    p = C.addressof(buf)

    def call(src=p, idx=p + 64, ids=p + 96, valid=None, out=p + 128, params=p + 192, b=1, outer=2, T=4, W=3, inner=6, lo=0.5, hi=1.0,
             mode=R.RANDOM):
        return lib.fgcn_clip_window(src, idx, ids, valid, out, params, b, outer, T, W, inner, lo, hi, mode, 7, 0, 0, None)

    def refused(text, **kw):
        assert call(**kw) == -1, kw
        assert text in lib.fgcn_last_error(), (kw, lib.fgcn_last_error())

    for name in ("src", "idx", "out", "params"):
        for mode in (R.RANDOM, R.CENTRE):
            refused(b"null pointer", mode=mode, **{name: None})
    refused(b"null pointer (sample_ids", ids=None)                            # RANDOM reads them; CENTRE does not: it gets past this check
    refused(b"bad b/outer/T/W/inner", ids=None, mode=R.CENTRE, b=0)
    for name in ("b", "outer", "T", "W", "inner"):
        for bad in (0, -3):
            refused(b"bad b/outer/T/W/inner", **{name: bad})
    for lo, hi in ((0.0, 1.0), (-0.5, 0.5), (0.6, 0.5), (0.5, 1.5), (1.5, 1.5)):
        refused(b"outside 0 < lo <= hi <= 1", lo=lo, hi=hi)
    for lo, hi in ((math.nan, 1.0), (0.5, math.nan), (0.5, math.inf), (-math.inf, 0.5)):
        refused(b"not finite", lo=lo, hi=hi)
    for bad in (2, -1, 7):
        refused(b"unknown mode", mode=bad)
    refused(b"alias", out=p)
    refused(b"more than a lane indexes", W=2 ** 20, inner=2 ** 9)
    refused(b"more than one grid holds", b=2 ** 31 - 1, outer=2 ** 31 - 1, W=2 ** 14, inner=2 ** 14)      # no intermediate overflows
    refused(b"more than one grid holds", b=2 ** 30, outer=2, W=1, inner=1)
    # the host entry point refuses the same interval and mode
    out = (C.c_float * 2)()
    assert lib.fgcn_window_params(0, 0, 0, 0, 0.5, 1.0, R.RANDOM, None) == -1 and b"null pointer" in lib.fgcn_last_error()
    assert lib.fgcn_window_params(0, 0, 0, 0, 0.0, 1.0, R.RANDOM, out) == -1 and b"outside 0 < lo" in lib.fgcn_last_error()
    assert lib.fgcn_window_params(0, 0, 0, 0, 0.5, math.nan, R.CENTRE, out) == -1 and b"not finite" in lib.fgcn_last_error()
    assert lib.fgcn_window_params(0, 0, 0, 0, 0.5, 1.0, 2, out) == -1 and b"unknown mode" in lib.fgcn_last_error()

    def count(src=p, idx=p + 64, out=p + 128, b=1, outer=2, T=4, inner=6):
        return lib.fgcn_clip_valid_frames(src, idx, out, b, outer, T, inner, None)

    for name in ("src", "idx", "out"):
        assert count(**{name: None}) == -1 and b"null pointer" in lib.fgcn_last_error(), name
    for name in ("b", "outer", "T", "inner"):
        for bad in (0, -3):
            assert count(**{name: bad}) == -1 and b"bad b/outer/T/inner" in lib.fgcn_last_error(), (name, bad)
    assert count(T=2 ** 20, inner=2 ** 9) == -1 and b"more than a lane indexes" in lib.fgcn_last_error()


def test_window_object_validates_its_arguments():
    from fusion_gcn_amd.data import Window
    w = Window(64)
    assert (w.frames, w.interval, w.train, w.mode, w.at_upload, w.valid_frames, w.only, w.site, w.name) == \
        (64, (0.5, 1.0), True, "random", False, {}, None, 0, "window")
    e = Window({"skeleton": 64, "inertial": 32}, interval=(0.25, 0.95), train=False, site=3)
    assert (e.mode, e.at_upload, e.site, e.length("inertial"), e.length("skeleton")) == ("centre", True, 3, 32, 64)
    assert e.applies_to("skeleton") and not e.applies_to("rgb") and w.applies_to("rgb") and not Window(8, only=["a"]).applies_to("b")
    for bad in (0, -4, 2.5, True, "64", {}, {"skeleton": 0}, {"skeleton": 1.5}):
        with pytest.raises(ValueError, match="frames"):
            Window(bad)
    for bad in ((0.0, 1.0), (0.6, 0.5), (0.5, 1.5), (0.5,), (0.2, 0.5, 0.9), (math.nan, 1.0), (0.5, math.inf)):
        with pytest.raises(ValueError, match="interval"):
            Window(8, interval=bad)
    with pytest.raises(ValueError, match="only"):
        Window({"skeleton": 8}, only=["inertial"])


def test_bind_gives_the_windowed_shapes_and_refuses_at_construction():
    from fusion_gcn_amd.data import Window
    shapes = {"skeleton": (2, 13, 7, 3), "inertial": (11, 6)}
    keys = list(shapes)
    after, writes = Window(8).bind(shapes, 9, keys)
    assert after == {"skeleton": (2, 8, 7, 3), "inertial": (8, 6)} and list(after) == keys and writes == keys
    after, writes = Window({"skeleton": 20, "inertial": 5}).bind(shapes, 9, keys)                 # larger than T too
    assert after == {"skeleton": (2, 20, 7, 3), "inertial": (5, 6)} and writes == keys
    after, writes = Window(8, only=["skeleton"]).bind(shapes, 9, keys)
    assert after == {"skeleton": (2, 8, 7, 3), "inertial": (11, 6)} and writes == ["skeleton"]
    assert Window({"inertial": 4}).bind(shapes, 9, keys) == ({"skeleton": (2, 13, 7, 3), "inertial": (4, 6)}, ["inertial"])
    for kw in (dict(only=["pose"]), dict(valid_frames={"pose": [5] * 9})):
        with pytest.raises(ValueError, match="does not have"):
            Window(8, **kw).bind(shapes, 9, keys)
    with pytest.raises(ValueError, match="does not have"):
        Window({"pose": 8}).bind(shapes, 9, keys)
    with pytest.raises(ValueError, match="not in the batch"):                  # a signal an Inertial(drop_signal=True) in front dropped
        Window({"inertial": 8}).bind({"skeleton": (2, 13, 7, 3)}, 9, keys)
    with pytest.raises(ValueError, match="does not apply to"):
        Window(8, only=["skeleton"], valid_frames={"inertial": [5] * 9}).bind(shapes, 9, keys)
    with pytest.raises(_lib.FgcnError, match="expected"):
        Window(8).bind({"rgb": (3, 13, 8, 8, 2)}, 9, ["rgb"])
    for bad in ([13] * 8, [13] * 8 + [0], [13] * 8 + [14], [13.0] * 9):
        with pytest.raises(ValueError, match=r"expected 9 frame counts in \[1, 13\]"):
            Window(8, valid_frames={"skeleton": bad}).bind(shapes, 9, keys)
    ok = Window(8, valid_frames={"inertial": [1] + [11] * 8})
    ok.bind(shapes, 9, keys)
    tables = ok.tables(keys, 9)
    assert list(tables) == [None, "inertial"] and tables["inertial"].dtype == np.int32 and tables[None].tolist() == list(range(9))
    assert list(Window(8, train=False, valid_frames={"inertial": [11] * 9}).tables(keys, 9)) == ["inertial"]      # the centred part has no ids


def _ds(tmp_path, shapes, n=9):
    from fusion_gcn_amd.data import MultiModalDataset, NumpyDatasetLoader
    arrays, labels = write_split(str(tmp_path), "train", n, shapes)
    return MultiModalDataset([(str(tmp_path), NumpyDatasetLoader())], "train"), arrays, labels


def test_no_host_fallback_and_construction_refusals(tmp_path):
    from fusion_gcn_amd import data, ops
    from fusion_gcn_amd.data import Augment, ClipBatches, Streams, Window
    ds, _, _ = _ds(tmp_path, {"skeleton": (2, 5, 7, 3), "inertial": (5, 6)})
    par = [0, 0, 1, 2, 3, 4, -1]
    for resident in (True, False):
        for train in (True, False):
            with pytest.raises(_lib.FgcnError, match="no host fallback"):
                ClipBatches(ds, 4, device="cpu", resident=resident, window=Window(4, train=train))
    with pytest.raises(_lib.FgcnError):
        ops.clip_window(torch.zeros(3, 2, 5, 7, 3), torch.arange(2), torch.arange(2), window=4)
    with pytest.raises(_lib.FgcnError):
        ops.clip_valid_frames(torch.zeros(3, 2, 5, 7, 3))
    with pytest.raises(_lib.FgcnError, match="no host fallback"):
        data.valid_frames(ds, "skeleton", device="cpu")
    with pytest.raises(ValueError, match="no feature"):
        data.valid_frames(ds, "pose", device="cpu")
    # the windowed clip fills all W frames: a valid_frames table of a stage behind it is refused, whatever the device
    valid = {"skeleton": [5] * 9}
    with pytest.raises(ValueError, match="augment: .*behind a Window"):
        ClipBatches(ds, 4, device="cpu", window=Window(4), augment=Augment(valid_frames=valid))
    with pytest.raises(ValueError, match="streams: .*behind a Window"):
        ClipBatches(ds, 4, device="cpu", window=Window(4, valid_frames=valid), streams=Streams(par, valid_frames=valid))
    with pytest.raises(ValueError, match="behind a Window"):
        ClipBatches(ds, 4, device="cpu", window=Window({"skeleton": 4}, train=False), streams=Streams(par, valid_frames=valid))
    # a Window that leaves the feature out: only the device is refused
    with pytest.raises(_lib.FgcnError, match="no host fallback"):
        ClipBatches(ds, 4, device="cpu", window=Window(4, only=["inertial"]), augment=Augment(valid_frames=valid))
    with pytest.raises(_lib.FgcnError, match="no host fallback"):
        ClipBatches(ds, 4, device="cpu", window=Window({"inertial": 4}), streams=Streams(par, valid_frames=valid))


@pytest.mark.parametrize("resident", [True, False])
def test_without_a_window_the_batches_are_the_stored_rows(tmp_path, resident):
    from fusion_gcn_amd.data import ClipBatches
    ds, arrays, labels = _ds(tmp_path, {"skeleton": (2, 5, 25, 3), "inertial": (7, 6)}, n=19)
    it = ClipBatches(ds, 8, shuffle=True, seed=1, device="cpu", resident=resident)
    it.set_epoch(3)
    assert it.window is None and it.stages == [] and it.last_window == {}
    assert it.shapes == {"skeleton": (2, 5, 25, 3), "inertial": (7, 6)}
    seen = 0
    for feats, lab, idx in it:
        for k, a in arrays.items():
            assert torch.equal(feats[k], torch.from_numpy(a).index_select(0, idx)), k
        assert torch.equal(lab, torch.from_numpy(labels.astype(np.int64)).index_select(0, idx))
        seen += len(idx)
    assert seen == 19 and it.last_window == {}


def test_restatement_sanity():
    rng = np.random.default_rng(2)
    src = rng.standard_normal((4, 2, 5, 3, 3))
    whole = np.tile([0.0, 1.0], (3, 1))
    assert np.array_equal(R.transform(src, [2, 0, 2], whole, 5), src[[2, 0, 2]])                   # W == T, the whole recording
    out = R.transform(src, [1, 3], whole[:2], 5, valid=[5, 1, 5, 2])
    assert np.array_equal(out[0], np.broadcast_to(src[1][:, :1], src[1].shape))                    # one valid frame: every output frame is it
    assert np.array_equal(out[1][:, 0], src[3][:, 0]) and np.allclose(out[1][:, 4], src[3][:, 1])  # two: frame 0 .. frame 1
    assert np.allclose(out[1][:, 2], 0.5 * (src[3][:, 0] + src[3][:, 1]))
    up = R.transform(src, [0], whole[:1], 9)                                                       # upsampling: every second frame is a stored one
    assert up.shape == (1, 2, 9, 3, 3) and np.allclose(up[0][:, ::2], src[0]) and np.allclose(up[0][:, 1], 0.5 * (src[0][:, 0] + src[0][:, 1]))
    half = R.transform(src, [0], [[0.25, 0.5]], 3)                                                 # frames 1 .. 3 of five, in three
    assert np.allclose(half[0], src[0][:, 1:4])
    sig = R.transform(rng.standard_normal((3, 7, 4)), [1, 2], whole[:2], 1)
    assert sig.shape == (2, 1, 4)
    assert [R.clamp_valid(v, 6) for v in (None, 0, 1, 6, 9, -4)] == [6, 1, 1, 6, 6, 1]
    # the float32 positions: the whole recording at W == T reads frame t itself with weight zero
    assert R.reads32(0.0, 1.0, 5, 5) == [(t, min(t + 1, 4), 0.0) for t in range(5)]
    assert [f[:2] for f in R.reads32(0.0, 1.0, 4, 1)] == [(0, 0)] * 4
    # a NaN reaches the outputs that read its frame -- also with weight zero -- and no other
    x = rng.standard_normal((1, 1, 5, 2, 3)).astype(np.float32)
    x[0, 0, 2, 1, 0] = np.nan
    x[0, 0, 4, 0, 2] = -np.inf
    reads, cls = R.classes(x, [0], np.float32([[0.0, 1.0]]), 5)
    assert reads[0, 0, :, 1, 0].tolist() == [False, True, True, False, False] and cls[0, 0, :, 1, 0].tolist() == [0, 1, 1, 0, 0]
    assert reads[0, 0, :, 0, 2].tolist() == [False, False, False, True, True] and cls[0, 0, 3:, 0, 2].tolist() == [1, 1]
    assert reads.sum() == 4 and (cls != 0).sum() == 4
    # the valid frames
    c = np.zeros((6, 2, 5, 3, 2), dtype=np.float32)
    c[0, 0, :3] = 1                                                            # trailing null frames
    c[1, 0, 0], c[1, 0, 3] = 1, 1                                              # an interior null frame does not end the clip
    c[2, 0, :2], c[2, 0, 2:] = 1, -0.0                                         # -0 is zero
    c[3, 0, 0], c[3, 0, 4, 2, 1] = 1, np.nan                                   # a NaN is a value
    c[4, 0, :2], c[4, 1, :4] = 1, 1                                            # the second body is longer
    assert R.valid_frames(c).tolist() == [3, 4, 2, 5, 4, 1] and R.valid_frames(c, [5, 0, 5, 3]).tolist() == [1, 3, 1, 5]
    assert R.valid_frames(c[:, 0, :, :, 0]).tolist() == [3, 4, 2, 1, 2, 1]                         # a (rows, T, S) signal
