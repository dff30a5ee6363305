"""Augmentation of clips as ClipBatches gathers them, the part that needs no GPU: the parameter table of
fgcn_augment_params -- the host copy of the function the kernel calls -- against the float64 restatement of tests/augment_ref.py, the
identity parameters, the host-side argument checks of fgcn_clip_augment (they precede any launch), and the two promises of the Python
surface that hold without a device: no host fallback, and ``augment=None`` delivers what it always delivered."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import augment_ref as A
from fusion_gcn_amd import _lib, build
from test_data import write_split

ANGLES, SCALE, MIN_WINDOW = (0.3, 0.2, 0.5), 0.1, 0.5


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def _row(lib, sample, site, epoch, seed, max_angle=ANGLES, scale=SCALE, min_window=MIN_WINDOW):
    out = (C.c_float * 12)()
    assert lib.fgcn_augment_params(sample, site, epoch, seed, (C.c_float * 3)(*max_angle), scale, min_window, out) == 0
    return np.array(list(out), dtype=np.float32)


def _tuples():
    """51 (sample, site, epoch, seed): the corners of the counter and of the key, then random ones"""
    rng = np.random.default_rng(11)
    fixed = [(0, 0, 0, 0), (2 ** 32 - 1, 2 ** 32 - 1, 2 ** 32 - 1, 2 ** 64 - 1), (860, 0, 49, 1)]
    return fixed + [(int(rng.integers(0, 2 ** 32)), int(rng.integers(0, 8)), int(rng.integers(0, 200)), int(rng.integers(0, 2 ** 64, dtype=np.uint64)))
                    for _ in range(48)]


def test_parameter_table_matches_the_float64_restatement(lib):
    tuples = _tuples()
    got = np.stack([_row(lib, *t) for t in tuples])
    want = np.stack([A.params(*t, ANGLES, SCALE, MIN_WINDOW) for t in tuples])
    A.check_table(got, want, SCALE)
    assert np.all((got[:, 10] >= MIN_WINDOW) & (got[:, 10] <= 1)) and np.all((got[:, 9] >= 0) & (got[:, 9] + got[:, 10] <= 1 + 2 ** -23))
    assert len({tuple(r) for r in got.tolist()}) == len(tuples)                  # every tuple draws its own row
    # each coordinate of the counter and both key words matter
    base = _row(lib, 5, 1, 2, 3)
    for other in ((6, 1, 2, 3), (5, 2, 2, 3), (5, 1, 3, 3), (5, 1, 2, 4), (5, 1, 2, 3 + 2 ** 32)):
        assert not np.array_equal(_row(lib, *other), base), other
    # an asymmetric case: only the z angle, only the window
    only_z = _row(lib, 9, 0, 0, 1, (0.0, 0.0, 0.4), 0.0, 1.0)
    assert only_z[8] == 1 and only_z[2] == 0 and only_z[5] == 0 and only_z[6] == 0 and only_z[7] == 0 and abs(only_z[1]) > 0
    assert tuple(only_z[9:]) == (0, 1, 0)


def test_uniforms_of_the_restatement_are_exact_float32_in_the_unit_interval():
    u = np.concatenate([A.uniforms(*t) for t in _tuples()])
    assert np.all((u >= 0) & (u < 1)) and np.array_equal(u.astype(np.float32).astype(np.float64), u)
    assert 0.35 < u.mean() < 0.65


def test_zero_magnitudes_give_the_identity_exactly(lib):
    for t in _tuples()[:12]:
        row = _row(lib, *t, (0.0, 0.0, 0.0), 0.0, 1.0)
        assert np.array_equal(row[:9].reshape(3, 3), np.eye(3, dtype=np.float32)) and tuple(row[9:]) == (0.0, 1.0, 0.0), (t, row)
    from fusion_gcn_amd import ops
    assert ops.augment_params(3, 0, 1, 7) == [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 1, 0]      # the wrapper's defaults are the identity too


def test_reference_transform_is_the_gather_at_the_identity_and_clamps_short_clips():
    rng = np.random.default_rng(2)
    src = rng.standard_normal((4, 2, 5, 3, 3))
    ident = np.tile(np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 1, 0], dtype=np.float64), (3, 1))
    assert np.array_equal(A.transform(src, [2, 0, 2], ident, None, (0, 3)), src[[2, 0, 2]])
    out = A.transform(src, [1, 3], ident[:2], valid=[5, 1, 5, 2], joints=None)
    assert np.array_equal(out[0], np.broadcast_to(src[1][:, :1], src[1].shape))         # one valid frame: every output frame is it
    assert np.array_equal(out[1][:, 0], src[3][:, 0]) and np.allclose(out[1][:, 4], src[3][:, 1])      # two: frame 0 .. frame 1
    assert np.allclose(out[1][:, 2], 0.5 * (src[3][:, 0] + src[3][:, 1]))
    # a rotation by 90 degrees about z: (x, y, z) -> (-y, x, z), joints outside the range untouched
    rot = ident[:1].copy()
    rot[0, :9] = [0, -1, 0, 1, 0, 0, 0, 0, 1]
    got = A.transform(src, [0], rot, None, (0, 2))[0]
    assert np.array_equal(got[..., :2, 0], -src[0][..., :2, 1]) and np.array_equal(got[..., :2, 1], src[0][..., :2, 0])
    assert np.array_equal(got[..., 2, :], src[0][..., 2, :])


def test_host_side_validation(lib):
    """include/fgcn.h's list: each refusal is FGCN_E_BADARG with a message, before any launch (no device is touched: this runs without one)."""
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    ang = (C.c_float * 3)(0.3, 0.3, 0.3)

    def call(src=p, idx=p + 64, ids=p + 96, valid=None, out=p + 128, params=p + 192, b=1, outer=2, T=4, inner=6, Cc=3, lo=0, hi=2,
             angles=ang, scale=0.1, window=0.5):
        return lib.fgcn_clip_augment(src, idx, ids, valid, out, params, b, outer, T, inner, Cc, lo, hi, angles, scale, window, 7, 0, 0, None)

    def refused(text, **kw):
        assert call(**kw) == -1, kw
        assert text in lib.fgcn_last_error(), (kw, lib.fgcn_last_error())

    for name in ("src", "idx", "ids", "out", "params", "angles"):
        refused(b"null pointer", **{name: None})
    for name in ("b", "outer", "T", "inner"):
        for bad in (0, -3):
            refused(b"bad b/outer/T/inner", **{name: bad})
    refused(b"does not divide", Cc=0)
    refused(b"does not divide", Cc=-3)
    refused(b"does not divide", Cc=4)
    refused(b"does not divide", inner=7)
    for lo, hi in ((-1, 2), (0, 3), (2, 1), (3, 3)):
        refused(b"joint range", lo=lo, hi=hi)
    refused(b"needs C == 3", Cc=2, hi=1)
    refused(b"needs C == 3", Cc=6, hi=1)
    for bad in (0.0, -0.5, 1.5, math.nan, math.inf):
        refused(b"min_window", window=bad)
    for bad in (-0.1, 1.0, 2.0, math.nan, math.inf):
        refused(b"scale", scale=bad)
    for e in range(3):
        for bad in (math.nan, math.inf, -math.inf):
            a = [0.3, 0.3, 0.3]
            a[e] = bad
            refused(b"not finite", angles=(C.c_float * 3)(*a))
    refused(b"alias", out=p)
    # the host entry point refuses the same magnitudes
    out = (C.c_float * 12)()
    assert lib.fgcn_augment_params(0, 0, 0, 0, None, 0.1, 0.5, out) == -1 and b"null pointer" in lib.fgcn_last_error()
    assert lib.fgcn_augment_params(0, 0, 0, 0, ang, 0.1, 0.5, None) == -1 and b"null pointer" in lib.fgcn_last_error()
    assert lib.fgcn_augment_params(0, 0, 0, 0, ang, 1.0, 0.5, out) == -1 and b"scale" in lib.fgcn_last_error()
    assert lib.fgcn_augment_params(0, 0, 0, 0, ang, 0.1, 0.0, out) == -1 and b"min_window" in lib.fgcn_last_error()
    assert lib.fgcn_augment_params(0, 0, 0, 0, (C.c_float * 3)(0, math.nan, 0), 0.1, 0.5, out) == -1 and b"not finite" in lib.fgcn_last_error()


def test_augment_object_validates_its_arguments():
    from fusion_gcn_amd.data import Augment
    a = Augment()
    assert (a.max_angle, a.scale, a.min_window, a.joints, a.site, a.only, a.valid_frames) == ((0.3, 0.3, 0.3), 0.1, 0.5, None, 0, None, {})
    assert a.applies_to("skeleton") and not Augment(only=["inertial"]).applies_to("skeleton")
    assert a.joint_range((2, 13, 25, 3)) == (0, 25) and a.joint_range((11, 6)) is None and a.joint_range((2, 13, 25, 2)) is None
    assert Augment(joints=(0, 20)).joint_range((1, 16, 27, 3)) == (0, 20) and Augment(joints=(4, 4)).joint_range((1, 16, 27, 3)) is None
    with pytest.raises(ValueError):
        Augment(joints=(0, 26)).joint_range((2, 13, 25, 3))
    for kw in (dict(max_angle=(0.1, 0.2)), dict(max_angle=(0.1, math.nan, 0.0)), dict(scale=1.0), dict(scale=-0.1), dict(min_window=0.0),
               dict(min_window=1.5), dict(joints=(3, 2))):
        with pytest.raises(ValueError):
            Augment(**kw)


def test_no_host_fallback(tmp_path):
    from fusion_gcn_amd import ops
    from fusion_gcn_amd.data import Augment, ClipBatches, MultiModalDataset, NumpyDatasetLoader
    write_split(str(tmp_path), "train", 9, {"skeleton": (2, 5, 25, 3)})
    ds = MultiModalDataset([(str(tmp_path), NumpyDatasetLoader())], "train")
    for resident in (True, False):
        with pytest.raises(_lib.FgcnError):
            ClipBatches(ds, 4, device="cpu", resident=resident, augment=Augment())
    with pytest.raises(_lib.FgcnError):
        ops.clip_augment(torch.zeros(3, 2, 5, 25, 3), torch.arange(2), torch.arange(2), seed=1, epoch=0)


@pytest.mark.parametrize("resident", [True, False])
def test_without_augment_the_batches_are_the_stored_rows(tmp_path, resident):
    from fusion_gcn_amd.data import ClipBatches, MultiModalDataset, NumpyDatasetLoader
    arrays, labels = write_split(str(tmp_path), "train", 19, {"skeleton": (2, 5, 25, 3), "inertial": (7, 6)})
    ds = MultiModalDataset([(str(tmp_path), NumpyDatasetLoader())], "train")
    it = ClipBatches(ds, 8, shuffle=True, seed=1, device="cpu", resident=resident, augment=None)
    it.set_epoch(3)
    assert it.augment is None and it.last_params == {}
    seen = 0
    for feats, lab, idx in it:
        for k, a in arrays.items():
            assert torch.equal(feats[k], torch.from_numpy(a).index_select(0, idx)), k
        assert torch.equal(lab, torch.from_numpy(labels.astype(np.int64)).index_select(0, idx))
        seen += len(idx)
    assert seen == 19 and it.last_params == {}
