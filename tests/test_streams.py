"""The bone / motion streams ClipBatches derives as it gathers, the part that needs no GPU: the host-side refusals
of fgcn_clip_streams (they precede any launch), the arguments of ``data.Streams`` and what its ``bind`` refuses at construction, the
parents ``Streams.for_dataset`` builds, the output ids and their order, no host fallback, and the sanity of the numpy restatement
(tests/streams_ref.py) that the GPU tests compare the kernel with."""
import ctypes as C
import importlib

import numpy as np
import pytest

import streams_ref as R
from fusion_gcn_amd import _lib, build
from test_data import write_split


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def test_host_side_validation(lib):
    """include/fgcn.h's list: each refusal is FGCN_E_BADARG and names the argument, before any launch (no device is touched)"""
    buf = (C.c_float * 64)()
    p = C.addressof(buf)

    def call(src=p, idx=p + 32, parents=p + 64, valid=None, joint=None, bone=p + 96, motion=None, bone_motion=None, b=1, M=1, T=2, V=2, Cc=3):
        return lib.fgcn_clip_streams(src, idx, parents, valid, joint, bone, motion, bone_motion, b, M, T, V, Cc, None)

    def refused(text, **kw):
        assert call(**kw) == -1, kw
        assert text in lib.fgcn_last_error(), (kw, lib.fgcn_last_error())

    for name in ("src", "idx", "parents"):
        refused(b"null pointer (" + name.encode() + b")", **{name: None})
    refused(b"no derived output", bone=None)
    refused(b"no derived output", bone=None, joint=p + 96)                    # the joints alone derive nothing
    for name in ("b", "M", "T", "V"):
        for bad in (0, -3):
            refused(b"bad b/M/T/V", **{name: bad})
    for bad in (0, 1, 4, -3):
        refused(b"C=%d" % bad, Cc=bad)
    for name in ("joint", "bone", "motion", "bone_motion"):
        refused(b"alias src", **{name: p})
    refused(b"more than one grid holds", b=2 ** 31 - 1, M=2 ** 31 - 1, T=2 ** 31 - 1, V=2 ** 31 - 1)      # no intermediate overflows
    refused(b"more than one grid holds", b=2 ** 20, M=2, T=2 ** 10, V=2 ** 9)                              # 2^40 lanes
    refused(b"more than one grid holds", b=2 ** 31 - 1, M=1, T=257, V=1)                                   # 2^31 - 1 workgroups hold 256 each


def test_streams_object_validates_its_arguments():
    from fusion_gcn_amd.data import Streams
    s = Streams([0, 0, 1, -1])
    assert (s.parents, s.streams, s.only, s.valid_frames, s.name, s.at_upload) == ((0, 0, 1, -1), ("bone",), None, {}, "streams", False)
    assert Streams([0, 0], streams="motion").streams == ("motion",)
    assert Streams([0, 0], streams=R.STREAMS).streams == R.STREAMS == Streams.STREAMS
    for bad in ((), ("bone", "bone"), ("bone", "velocity"), ("joint",)):      # empty, duplicate, unknown, nothing derived
        with pytest.raises(ValueError, match="streams"):
            Streams([0, 0], streams=bad)
    for bad in ([0, 2], [-2, 0], [], [0, 1.5], [True, 0]):                    # a parent outside [-1, V), no joint, no joint number
        with pytest.raises(ValueError, match="parents"):
            Streams(bad)


def _ds(tmp_path, shapes, n=9):
    from fusion_gcn_amd.data import MultiModalDataset, NumpyDatasetLoader
    write_split(str(tmp_path), "train", n, shapes)
    return MultiModalDataset([(str(tmp_path), NumpyDatasetLoader())], "train")


def test_bind_refuses_at_construction():
    from fusion_gcn_amd.data import Streams
    shapes = {"skeleton": (2, 5, 7, 3), "inertial": (5, 6)}
    keys, par = list(shapes), [0, 0, 1, 2, 3, 4, -1]
    after, writes = Streams(par).bind(shapes, 9, keys)
    assert after == shapes and list(after) == keys and writes == ["skeleton"]  # the default leaves the (T, S) signal alone
    with pytest.raises(ValueError, match="does not have"):
        Streams(par, only=["pose"]).bind(shapes, 9, keys)
    with pytest.raises(ValueError, match="does not have"):
        Streams(par, valid_frames={"pose": [5] * 9}).bind(shapes, 9, keys)
    with pytest.raises(ValueError, match="already features"):                 # "skeleton_bone" is taken
        Streams(par, streams=("joint", "bone"), only=["skeleton"]).bind({**shapes, "skeleton_bone": (2, 5, 7, 3)}, 9, [*keys, "skeleton_bone"])
    with pytest.raises(_lib.FgcnError, match="7 joints, parents has 6"):
        Streams(par[:6]).bind(shapes, 9, keys)
    with pytest.raises(_lib.FgcnError, match="C of 2 or 3"):
        Streams(par, only=["skeleton"]).bind({"skeleton": (2, 5, 7, 4)}, 9, ["skeleton"])
    with pytest.raises(_lib.FgcnError, match="C of 2 or 3"):                  # a signal named on purpose
        Streams(par, only=["inertial"]).bind(shapes, 9, keys)
    assert Streams(par).bind({"skeleton": (2, 5, 7, 4)}, 9, ["skeleton"]) == ({"skeleton": (2, 5, 7, 4)}, [])      # C = 4 is not a default
    with pytest.raises(ValueError, match=r"expected 9 frame counts in \[1, 5\]"):
        Streams(par, valid_frames={"skeleton": [5] * 8}).bind(shapes, 9, keys)
    for bad in (0, 6):
        with pytest.raises(ValueError, match=r"expected 9 frame counts in \[1, 5\]"):
            Streams(par, valid_frames={"skeleton": [5] * 8 + [bad]}).bind(shapes, 9, keys)
    ok = Streams(par, valid_frames={"skeleton": [1] + [5] * 8})
    ok.bind(shapes, 9, keys)
    assert ok.tables(["skeleton"], 9)["skeleton"].dtype == np.int32 and list(ok.tables(["skeleton"], 9)) == ["skeleton"]


def test_output_ids_and_their_order():
    from fusion_gcn_amd.data import Streams
    shapes = {"inertial": (5, 6), "skeleton": (2, 5, 7, 3), "zed": (1, 5, 7, 2)}
    par = [0, 0, 1, 2, 3, 4, -1]
    for one in ("bone", "motion", "bone_motion"):                             # one stream: the id and the shape stay
        after, writes = Streams(par, streams=[one]).bind(shapes, 9, list(shapes))
        assert after == shapes and list(after) == list(shapes) and writes == ["skeleton", "zed"]
    after, writes = Streams(par, streams=("bone", "joint", "bone_motion"), only=["skeleton"]).bind(shapes, 9, list(shapes))
    assert list(after) == ["inertial", "skeleton", "skeleton_bone", "skeleton_bone_motion", "zed"]      # "joint" keeps the id, the rest behind it
    assert writes == ["skeleton", "skeleton_bone", "skeleton_bone_motion"] and all(after[k] == (2, 5, 7, 3) for k in writes)
    after, writes = Streams(par, streams=("motion", "bone")).bind(shapes, 9, list(shapes))               # without "joint" the id is dropped
    assert list(after) == ["inertial", "skeleton_motion", "skeleton_bone", "zed_motion", "zed_bone"] == ["inertial", *writes]
    assert after["zed_bone"] == (1, 5, 7, 2)
    s = Streams(par, streams=("motion", "joint"))
    assert s.output_ids("a") == {"joint": "a", "motion": "a_motion"} and Streams(par).output_ids("a") == {"bone": "a"}


@pytest.mark.parametrize("name", ["ntu_rgb_d", "utd_mhad", "mmact"])
def test_for_dataset_builds_the_parents_of_the_constants_module(name):
    from fusion_gcn_amd.data import Streams
    const = importlib.import_module(f"fusion_gcn_amd.datasets.{name}.constants")
    want = {**const._parent, const.center_joint: const.center_joint}
    s = Streams.for_dataset(name)
    assert len(s.parents) == const.num_joints and dict(enumerate(s.parents)) == want and s.streams == ("bone",)
    two = Streams.for_dataset(name, extra_joints=2, streams=("bone", "motion"), only=["skeleton"])
    assert two.parents == s.parents + (-1, -1) and two.streams == ("bone", "motion") and two.only == frozenset(["skeleton"])
    with pytest.raises(ValueError):
        Streams.for_dataset(name, extra_joints=-1)


def test_for_dataset_refuses_a_joint_that_appears_in_no_edge(monkeypatch):
    from fusion_gcn_amd.data import Streams
    from fusion_gcn_amd.datasets.mmact import constants
    monkeypatch.setattr(constants, "skeleton_edges", constants.skeleton_edges[:-1])
    with pytest.raises(ValueError, match=r"joints \[17\] of 18 appear in no edge"):
        Streams.for_dataset("mmact")
    with pytest.raises(ValueError, match="streams"):                          # the keywords go to the constructor
        Streams.for_dataset("utd_mhad", streams=())


def test_no_host_fallback_and_construction_refusals(tmp_path):
    import torch

    from fusion_gcn_amd import ops
    from fusion_gcn_amd.data import Augment, ClipBatches, Streams
    ds = _ds(tmp_path, {"skeleton": (2, 5, 7, 3)})
    par = [0, 0, 1, 2, 3, 4, -1]
    for resident in (True, False):
        with pytest.raises(_lib.FgcnError, match="no host fallback"):
            ClipBatches(ds, 4, device="cpu", resident=resident, streams=Streams(par))
    with pytest.raises(_lib.FgcnError):
        ops.clip_streams(torch.zeros(3, 2, 5, 7, 3), torch.arange(2), par)
    # the augmented clip fills all T frames: a valid_frames table of the Streams behind it is refused, whatever the device
    valid = {"skeleton": [5] * 9}
    with pytest.raises(ValueError, match="behind an Augment"):
        ClipBatches(ds, 4, device="cpu", augment=Augment(), streams=Streams(par, valid_frames=valid))
    with pytest.raises(ValueError, match="behind an Augment"):
        ClipBatches(ds, 4, device="cpu", augment=Augment(valid_frames=valid), streams=Streams(par, valid_frames=valid))
    with pytest.raises(_lib.FgcnError, match="no host fallback"):              # an Augment that leaves the feature out: only the device is refused
        ClipBatches(ds, 4, device="cpu", augment=Augment(only=[]), streams=Streams(par, valid_frames=valid))
    it = ClipBatches(ds, 4, device="cpu")                                      # streams=None: nothing of the stage
    assert it.streams is None and it.stages == [] and it.last_streams == {} and it.out_keys == ["skeleton"]


def test_parent_table_is_checked_on_the_host():
    from fusion_gcn_amd import ops
    for bad in ([0, 2], [-2, 0], []):
        with pytest.raises(_lib.FgcnError, match="parents"):
            ops.stream_parents(bad, "cpu")
    t = ops.stream_parents([1, 1, -1], "cpu")
    assert t.dtype.is_floating_point is False and t.tolist() == [1, 1, -1] and t.element_size() == 4


def test_restatement_sanity():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((2, 6, 4, 3)).astype(np.float32)
    par = [2, 0, 2, -1]                                                       # joint 0's parent has the higher number; 2 is the root; 3 a sensor
    for L in (None, 1, 2, 5, 6, 0, 9):
        s = R.streams(x, par, L)
        n = R.clamp_valid(L, 6)
        assert all(s[k].dtype == np.float32 and s[k].shape == x.shape for k in R.STREAMS)
        assert R.same_bits(s["joint"], x)
        assert not s["bone"][:, :, 2].any() and not np.signbit(s["bone"][:, :, 2]).any()          # the bone of the root is +0
        assert R.same_bits(s["bone"][:, :, 3], x[:, :, 3])                                     # copied through
        assert R.same_bits(s["bone"][:, :, 1], x[:, :, 1] - x[:, :, 0]) and R.same_bits(s["bone"][:, :, 0], x[:, :, 0] - x[:, :, 2])
        for k in ("motion", "bone_motion"):                                                    # +0 from frame L-1 on
            assert not s[k][:, n - 1:].any() and not np.signbit(s[k][:, n - 1:]).any() and (n == 1 or s[k][:, :n - 1, :2].all())
        assert R.same_bits(s["motion"][:, :n - 1], x[:, 1:n] - x[:, :n - 1])
        assert R.same_bits(s["bone_motion"][:, :, 3], s["motion"][:, :, 3])                    # of a -1 joint: its motion
        assert R.same_bits(s["bone_motion"][:, :n - 1, 1], s["bone"][:, 1:n, 1] - s["bone"][:, :n - 1, 1])
    assert [R.clamp_valid(v, 6) for v in (None, 0, 1, 6, 9, -4)] == [6, 1, 1, 6, 6, 1]
    # frames at and behind L are never read for the motions: NaN there does not reach them, and reaches joint and bone exactly there
    y = x.copy()
    y[:, 3:] = np.nan
    s = R.streams(y, par, 3)
    assert not np.isnan(s["motion"]).any() and not np.isnan(s["bone_motion"]).any()
    assert np.isnan(s["bone"][:, 3:]).all() and not np.isnan(s["bone"][:, :3]).any() and R.same_values(s["joint"], y)
    got = R.batch(np.stack([x, y]), [1, 0, 1], par, valid=[6, 3])
    assert got["bone"].shape == (3, *x.shape) and R.same_values(got["motion"][0], s["motion"]) and R.same_bits(got["motion"][1], R.motion(x))
    assert not R.same_values(got["motion"][1], got["motion"][0]) and not R.same_bits(x, y)
