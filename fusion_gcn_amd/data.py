"""The step before the hot path: the reference's on-disk feature format, its dataset interface, and an MI355X-first batch
pipeline.

Format (reference: util/preprocessing/data_writer.py:11-38,71-83; file names datagroup.py:203, preprocess_data.py:57-67):
``<modality>_<split>_features.npy`` is a NumPy v1.0 file whose header occupies exactly 128 bytes (the writer memory-maps
the raw array at offset 128 first and writes the header over the gap afterwards) followed by the raw little-endian array
``(num_samples, M, T, V, C)``; ``<split>_labels.npy`` holds the integer labels.  ``np.load(path, mmap_mode="r")`` reads it.

Reader (reference: torch_src/loader.py:21-33, torch_src/dataset.py:11-58): ``NumpyDatasetLoader`` / ``MultiModalDataset`` with
the same names and semantics (feature id = file-name prefix before the first underscore; one modality -> array, several ->
dict).

Batches (reference: ``DataLoader(dataset, batch_size, shuffle, drop_last)`` + a synchronous unpinned
``features_batch.float().cuda()`` per step, session/training.py:21-26, session/session.py:168-174): ``ClipBatches`` yields
the same ``(features, labels, indices)`` triples, already on the device, in one of two ways
  * resident: the whole split is uploaded once (NTU-RGB-D cross-subject train: 7.2 GB of 288 GB) and a batch is a device-side
    row gather -- no PCIe traffic per step at all;
  * streaming: rows are gathered from the memory map into one of two pinned host buffers and copied on a side HIP stream
    while the previous step computes (double buffering; the consumer waits on an event, never on the host).
Data-parallel ranks take contiguous shards of every global batch (``dp.shard_batch``), all ranks shuffling with the same
seed.  torch is plumbing here (pinned memory, streams, index_select); without a stage (below) nothing on this path calls the HIP kernels.

Preparation on the device: ``ClipBatches`` runs the stages it is given, in this order, each a HIP kernel of libfgcn (no host fallback)
  * ``bodies=Bodies(...)`` (reference: datasets/ntu_rgb_d/io.py:SkeletonSample._filter_bodies, an offline per-clip loop): the tracker's
    bodies of a RAW skeleton clip scored by the spread of their joints, and the most energetic ones kept, in descending order, with
    ``fgcn_clip_bodies`` -- FIRST, since every later stage must see the selected bodies (``Normalize`` centres the clip by body 0):
    section 8o;
  * ``normalize=Normalize(...)`` (reference: util/preprocessing/skeleton.py:normalize_skeleton, an offline per-clip loop): RAW skeleton
    clips -- null frames padded, the centre joint of the first body at the origin, spine to z, shoulders to x -- with
    ``fgcn_clip_normalize``: DESIGN.md section 8g;
  * ``inertial=Inertial(frames=...)`` (reference: SkeletonProcessor("imu_enhanced") and InertialProcessor, util/preprocessing/processor):
    the RAW accelerometer / gyroscope recording -- resampled to the skeleton's frame count, zero-padded and min-max normalised
    (``fgcn_signal_prepare``), and with ``enhance=True`` appended as extra joints behind the normalised skeleton (``fgcn_imu_enhance``):
    section 8h;
  * ``window=Window(frames, ...)`` (ours; the recipe of the two-stream AGCN family's successors): one ``fgcn_clip_window`` call per modality -- a
    part of the clip's VALID frames, a random one when training and the centred one when evaluating, resized to ``frames`` frames, for
    which the model is then built (``ClipBatches.shapes``); ``valid_frames`` counts a stored split's valid frames on the device: section 8n;
  * ``augment=Augment(...)`` (ours; the reference has none): one ``fgcn_clip_augment`` call in place of the row gather of each modality --
    random rotation and scale of the joints, a random temporal window resampled to the clip's length -- whose random numbers are keyed
    by (seed, epoch, global sample index): section 8f;
  * ``streams=Streams(parents, ...)`` (the bone and motion inputs 2s-AGCN is trained on; the reference has none): one ``fgcn_clip_streams``
    call per skeleton feature -- joint minus parent joint, frame t+1 minus frame t inside the valid frames, and the motion of the bones,
    of the clip as the stages before left it: section 8j.
The first three run once at upload on the resident path -- and so does the window of an evaluation split, which has no random part -- the
training window, the augmentation and the streams on every batch; on the streaming path all run per batch, behind the copy.  What
``ClipBatches`` asks of a stage is listed above ``Augment``.
"""
from __future__ import annotations

import os
from typing import Dict, Iterable, Iterator, List, Mapping, Optional, Sequence, Tuple, Union

import numpy as np
import numpy.lib.format
import torch

from ._lib import FgcnError
from .dp import shard_batch

HEADER_BYTES = 128      # data_writer.py:19: np.memmap(out_path, dtype, "w+", 128, shape)


# ---- writer (util/preprocessing/data_writer.py) -------------------------------------------------------------------------
class MemoryMappedArray:
    """Raw array memory-mapped at byte 128 of ``out_path``; the v1.0 ``.npy`` header is written over the gap on close."""

    def __init__(self, out_path: str, dtype: type, shape: Sequence[int]):
        self.out_path = out_path
        self.dtype = dtype
        self.shape = tuple(shape)
        self.data = None

    def create_file(self):
        if self.out_path:
            self.data = np.memmap(self.out_path, self.dtype, "w+", HEADER_BYTES, self.shape)

    def close_file(self):
        if self.data is not None:
            self.data.flush()
            MemoryMappedArray._write_header(self.data, self.out_path)
        self.data = None

    def __enter__(self):
        self.create_file()
        return self.data

    def __exit__(self, exc_type, exc_val, exc_tb):
        self.close_file()

    @staticmethod
    def _write_header(data: np.ndarray, out_path: str):
        header = np.lib.format.header_data_from_array_1_0(data)
        with open(out_path, "r+b") as file:
            np.lib.format.write_array_header_1_0(file, header)
            if file.tell() != HEADER_BYTES:     # the reference silently corrupts the first samples in this case
                raise ValueError(f"{out_path}: the .npy header takes {file.tell()} bytes, the format reserves {HEADER_BYTES}")


class NumpyWriter:
    """``with NumpyWriter(path, np.float32, (num_samples, M, T, V, C)) as w: w.collect_next(sample)``."""

    def __init__(self, out_path: str, dtype: type, shape: Sequence[int]):
        self.out_path = out_path
        self.sample_index = 0
        self._data_store = MemoryMappedArray(out_path, dtype, shape)

    def start_collect(self):
        self._data_store.create_file()

    def end_collect(self):
        self._data_store.close_file()

    def collect_next(self, sequence, sample_index: int = None):
        sample_index = sample_index or self.sample_index       # (the reference's `or`: an explicit index 0 means "next")
        self._data_store.data[sample_index] = sequence
        self.sample_index += 1

    def __enter__(self):
        self.start_collect()
        return self

    def __exit__(self, exc_type, exc_val, exc_tb):
        self.end_collect()


# ---- reader (torch_src/loader.py, torch_src/dataset.py) ---------------------------------------------------------------------
class NumpyDatasetLoader:
    def __init__(self, **kwargs):
        self._mmap_mode = None if kwargs.get("in_memory", False) else "r"

    def load_data(self, path: str):
        return np.load(path, self._mmap_mode)

    def index_data_sample(self, data: np.ndarray, index: int) -> np.ndarray:
        return np.array(data[index])

    def get_sample_shape(self, data: np.ndarray) -> Sequence[int]:
        return data.shape[1:]


class MultiModalDataset(torch.utils.data.Dataset):
    """Load data from multiple paths each using their own loader (same interface as the reference's class)."""

    def __init__(self, input_data: Sequence[Tuple[str, NumpyDatasetLoader]], split: str, debug=False):
        assert len(input_data) > 0, "Must at least specify one data path"
        self.labels_data = np.load(os.path.join(input_data[0][0], f"{split}_labels.npy"))
        self.features_data: Dict[str, tuple] = {}
        for input_path, input_loader in input_data:
            for file in filter(lambda f: "features" in f.name and split in f.name and f.is_file(),
                               sorted(os.scandir(input_path), key=lambda f: f.name)):
                feature_id = file.name[:file.name.index("_")]
                self.features_data[feature_id] = (input_loader, input_loader.load_data(file.path))
        if debug:
            self.labels_data = self.labels_data[:100]

    def __len__(self):
        return len(self.labels_data)

    def __getitem__(self, index: int):
        if len(self.features_data) == 1:
            loader, data = next(iter(self.features_data.values()))
            features = loader.index_data_sample(data, index)
        else:
            features = {k: loader.index_data_sample(data, index) for k, (loader, data) in self.features_data.items()}
        return features, self.labels_data[index], index

    def get_input_shape(self) -> dict:
        return {k: loader.get_sample_shape(data) for k, (loader, data) in self.features_data.items()}

    def get_num_classes(self) -> int:
        return len(np.unique(self.labels_data))


# ---- batches ------------------------------------------------------------------------------------------------------------------
Features = Union[torch.Tensor, Dict[str, torch.Tensor]]
Shapes = Dict[str, tuple]       # feature id -> the shape of a sample
Feats = Dict[str, torch.Tensor]
Tables = Dict[Optional[str], torch.Tensor]

# A stage of ClipBatches' preparation on the device -- Bodies, Normalize, Inertial, Window, Augment, Streams, run in that order -- is a configuration object with
#   name        its keyword of ClipBatches, for the refusal of a device without HIP kernels
#   at_upload   True: a resident split takes it once, at construction; False: every batch does (a class attribute, or one of the instance:
#               Window(train=False) runs at upload, Window(train=True) per batch)
#   bind(shapes, n, keys) -> (shapes, writes)   at construction: refuses what the stage cannot take of ``n`` samples of ``shapes`` (as the
#               stage before left them) in a data set with the feature ids ``keys``; -> the shapes behind the stage and the feature ids
#               it writes, which are the ones that need an output buffer
#   tables(writes, n) -> {name: (n,) array}   what the kernels read beside the rows, indexed by the sample's index in the data set;
#               None names the sample ids themselves
#   run(batches, feats, rows, tables, out) -> feats   launches on the current stream: rows ``rows`` of the arrays ``feats`` into the buffers
#               ``out`` (feature id -> tensor, or None = a new one); ``tables[name][rows[j]]`` belongs to output row j, except the sample ids,
#               which are listed by output row; what the stage keeps for inspection goes to ``batches.last_*``.  A per-batch stage that
#               may run BEHIND another per-batch stage on the resident path (Augment behind Window, Streams behind both) takes ``rows`` per
#               feature too, {feature id: rows}: what the stage before wrote holds the batch's rows in order (rows 0..m-1), what it left out is still the resident array
#               (the shard's indices).  The rows are handed over per feature rather than the left-out features gathered first: a gather
#               would be one more pass over rows that the stage's own kernel gathers anyway.
# A further stage is one more such class and one more entry of ClipBatches' stage list: Streams was the fourth, Window is the fifth (it runs
# third: in front of the rotation, which then touches W frames instead of T, and of the streams, whose motion is the windowed clip's).
# Bodies is the sixth, it runs first: it decides what body 0 is, by which Normalize centres and rotates the clip, and how many body slots
# every later stage and the model see.


class Augment:
    """What ``ClipBatches(augment=...)`` does to every clip it hands out (include/fgcn.h).

    ``max_angle``: the largest rotation about x, y, z in radians (each angle uniform in +-max_angle); ``scale``: the size factor is
    uniform in 1 +- scale; ``min_window``: the shortest temporal window as a fraction of the recording (the window's length is uniform in
    [min_window, 1], its start uniform in what is left), resampled to the clip's T frames by linear interpolation.  The temporal part
    applies to every modality, and all modalities of a sample take the same part of the recording; the spatial part to the joints of
    ``(M, T, V, 3)`` arrays.  ``joints = (lo, hi)`` restricts it to joints ``[lo, hi)`` (the appended sensor joints of a
    skeleton_imu_enhanced array hold sensor axes, not positions); None = all joints of an array with three coordinates.
    ``valid_frames``: feature id -> the number of valid frames of each sample (the window is taken from those; default: all T).
    ``only``: the feature ids to augment (default: all); the others are gathered unchanged.  ``site`` separates two uses of one seed."""

    def __init__(self, max_angle: Sequence[float] = (0.3, 0.3, 0.3), scale: float = 0.1, min_window: float = 0.5,
                 joints: Optional[Tuple[int, int]] = None, valid_frames: Optional[Mapping[str, Sequence[int]]] = None, site: int = 0,
                 only: Optional[Iterable[str]] = None):
        self.max_angle = tuple(float(a) for a in max_angle)
        if len(self.max_angle) != 3 or not all(np.isfinite(self.max_angle)):
            raise ValueError(f"max_angle: three finite angles (x, y, z), got {max_angle!r}")
        if not 0.0 <= scale < 1.0:
            raise ValueError(f"scale={scale} outside [0, 1)")
        if not 0.0 < min_window <= 1.0:
            raise ValueError(f"min_window={min_window} outside (0, 1]")
        if joints is not None and not 0 <= joints[0] <= joints[1]:
            raise ValueError(f"joints={joints!r}: expected (lo, hi) with 0 <= lo <= hi")
        self.scale, self.min_window, self.site = float(scale), float(min_window), int(site)
        self.joints = None if joints is None else (int(joints[0]), int(joints[1]))
        self.valid_frames = dict(valid_frames or {})
        self.only = None if only is None else frozenset(only)

    name, at_upload = "augment", False

    def applies_to(self, feature_id: str) -> bool:
        return self.only is None or feature_id in self.only

    def joint_range(self, sample_shape: Sequence[int]) -> Optional[Tuple[int, int]]:
        """The joints of a sample of this shape that are rotated and scaled; None: the modality has no spatial part."""
        if len(sample_shape) != 4 or sample_shape[3] != 3:
            return None
        lo, hi = self.joints or (0, sample_shape[2])
        if hi > sample_shape[2]:
            raise ValueError(f"joints={self.joints!r} for an array of {sample_shape[2]} joints")
        return (lo, hi) if hi > lo else None

    def bind(self, shapes: Shapes, n: int, keys: Sequence[str]) -> Tuple[Shapes, List[str]]:
        writes = [k for k in shapes if self.applies_to(k)]
        for k in writes:
            if len(shapes[k]) not in (2, 4):
                raise FgcnError(f"augment: feature {k!r} has shape {(n, *shapes[k])}; expected (samples, M, T, V, C) or "
                                f"(samples, T, S) -- leave it out with Augment(only=...)")
            self.joint_range(shapes[k])                 # (a joint range the array does not have: refused here, not mid-epoch)
        unknown = (set(self.valid_frames) | set(self.only or ())) - set(keys)
        if unknown:
            raise ValueError(f"augment names features the data set does not have: {sorted(unknown)}")
        for k, v in self.tables(writes, n).items():
            if k is not None:
                T = shapes[k][-2] if len(shapes[k]) == 2 else shapes[k][1]
                if v.shape != (n,) or v.min() < 1 or v.max() > T:
                    raise ValueError(f"valid_frames[{k!r}]: expected {n} frame counts in [1, {T}]")
        return dict(shapes), writes

    def tables(self, writes: Sequence[str], n: int) -> Dict[Optional[str], np.ndarray]:
        """None: the clips' ids, which key the random numbers; feature id: the valid frames of its clips"""
        valid = {k: np.asarray(self.valid_frames[k]).astype(np.int32) for k in writes if k in self.valid_frames}
        return {None: np.arange(n, dtype=np.int64), **valid}

    def run(self, batches: "ClipBatches", feats: Feats, rows: Union[torch.Tensor, Dict[str, torch.Tensor]], tables: Tables,
            out: Dict[str, Optional[torch.Tensor]]) -> Feats:
        """``rows`` per feature where the stage before (a per-batch ``Window``) wrote some features and not others (see the protocol above)"""
        from . import ops
        feats = dict(feats)
        for k, o in out.items():
            src = feats[k]
            feats[k], batches.last_params[k] = ops.clip_augment(
                src, rows[k] if isinstance(rows, dict) else rows, tables[None], seed=batches.seed, epoch=batches.epoch, site=self.site,
                max_angle=self.max_angle, scale=self.scale, min_window=self.min_window, joints=self.joint_range(src.shape[1:]), valid=tables.get(k), out=o)
        return feats


class Bodies:
    """What ``ClipBatches(bodies=...)`` does to every raw skeleton clip (include/fgcn.h): the reference's
    ``SkeletonSample._filter_bodies`` -- of the ``Mr`` bodies the tracker lists, the ``bodies`` with the highest ``body_score`` (the sum
    over the channels of the standard deviation of the body's non-null frames), in descending order; a NaN score ranks first, equal
    scores by the higher source index.  The (samples, Mr, T, V, C) arrays it applies to come out as (bodies, T, V, C).  ``only``: the
    feature ids to select in (default: all); the others are handed out as stored."""

    def __init__(self, bodies: int = 2, only: Optional[Iterable[str]] = None):
        from ._lib import BODIES_MAX
        if isinstance(bodies, bool) or not isinstance(bodies, (int, np.integer)) or not 1 <= bodies <= BODIES_MAX:
            raise ValueError(f"bodies={bodies!r}: expected a number of bodies in [1, {BODIES_MAX}]")
        self.bodies = int(bodies)
        self.only = None if only is None else frozenset(only)

    @classmethod
    def for_dataset(cls, name: str, only: Optional[Iterable[str]] = None) -> "Bodies":
        """The reference's number of bodies for a data set (``max_body_true`` of its constants module: ``"ntu_rgb_d"`` has one)."""
        from .util.dynamic_import import import_dataset_constants
        got = import_dataset_constants(name, ["max_body_true"])
        if len(got) != 1:
            raise ValueError(f"data set {name!r} has no max_body_true constant")
        return cls(got[0], only=only)

    def applies_to(self, feature_id: str) -> bool:
        return self.only is None or feature_id in self.only

    name, at_upload = "bodies", True

    def bind(self, shapes: Shapes, n: int, keys: Sequence[str]) -> Tuple[Shapes, List[str]]:
        from ._lib import BODIES_MAX
        unknown = set(self.only or ()) - set(keys)
        if unknown:
            raise ValueError(f"bodies names features the data set does not have: {sorted(unknown)}")
        writes = [k for k in shapes if self.applies_to(k)]
        after = dict(shapes)
        for k in writes:
            shape = shapes[k]
            if len(shape) != 4:
                raise FgcnError(f"bodies: feature {k!r} has shape {(n, *shape)}; expected (samples, Mr, T, V, C) -- leave it out with "
                                f"Bodies(only=...)")
            if shape[0] < self.bodies:
                raise FgcnError(f"bodies: feature {k!r} holds {shape[0]} bodies, {self.bodies} are to be kept")
            if shape[0] > BODIES_MAX:
                raise FgcnError(f"bodies: feature {k!r} holds {shape[0]} bodies, at most {BODIES_MAX}")
            if shape[3] not in (2, 3):
                raise FgcnError(f"bodies: feature {k!r} has {shape[3]} coordinates; expected 2 or 3")
            after[k] = (self.bodies, *shape[1:])
        return after, writes

    def tables(self, writes: Sequence[str], n: int) -> Dict[Optional[str], np.ndarray]:
        return {}

    def run(self, batches: "ClipBatches", feats: Feats, rows: torch.Tensor, tables: Tables, out: Dict[str, Optional[torch.Tensor]]) -> Feats:
        from . import ops
        feats = dict(feats)
        for k, o in out.items():
            feats[k], order, scores = ops.clip_bodies(feats[k], rows, bodies=self.bodies, out=o)
            batches.last_bodies[k] = (order, scores)
        return feats


class Normalize:
    """What ``ClipBatches(normalize=...)`` does to every raw skeleton clip (include/fgcn.h): the reference's
    ``normalize_skeleton(skeleton, origin_joint, z_axis_joints, x_axis_joints)``.

    ``origin_joint``: the joint of the first body that is moved to the origin; ``z_axis_joints`` / ``x_axis_joints``: the pair of joints
    whose bone is turned to the z / x axis (None: no such pass; a pair needs three coordinates).  ``only``: the feature ids to normalise
    (default: all); the others are handed out as stored."""

    def __init__(self, origin_joint: int, z_axis_joints: Optional[Sequence[int]] = None, x_axis_joints: Optional[Sequence[int]] = None,
                 only: Optional[Iterable[str]] = None):
        if isinstance(origin_joint, bool) or not isinstance(origin_joint, (int, np.integer)) or origin_joint < 0:
            raise ValueError(f"origin_joint={origin_joint!r}: expected a joint number >= 0")
        self.origin_joint = int(origin_joint)
        self.z_axis_joints, self.x_axis_joints = self._pair(z_axis_joints, "z_axis_joints"), self._pair(x_axis_joints, "x_axis_joints")
        self.only = None if only is None else frozenset(only)

    @staticmethod
    def _pair(pair, name: str) -> Optional[Tuple[int, int]]:
        if pair is None:
            return None
        pair = tuple(pair)
        if len(pair) != 2 or any(isinstance(j, bool) or not isinstance(j, (int, np.integer)) or j < 0 for j in pair) or pair[0] == pair[1]:
            raise ValueError(f"{name}={pair!r}: expected two different joint numbers >= 0")
        return int(pair[0]), int(pair[1])

    @classmethod
    def for_dataset(cls, name: str, only: Optional[Iterable[str]] = None) -> "Normalize":
        """The reference's joint numbers for a data set (``"utd_mhad"``, ``"mmact"``, ``"ntu_rgb_d"``; its constants module holds them)."""
        from .util.dynamic_import import import_dataset_constants
        got = import_dataset_constants(name, ["skeleton_center_joint", "skeleton_z_joints", "skeleton_x_joints"])
        if len(got) != 3:
            raise ValueError(f"data set {name!r} has no skeleton normalisation constants")
        return cls(*got, only=only)

    def applies_to(self, feature_id: str) -> bool:
        return self.only is None or feature_id in self.only

    def check_shape(self, feature_id: str, shape: Sequence[int]) -> None:
        """Refuses an array (samples, M, T, V, C) this normalisation cannot take -- at construction, not mid-epoch."""
        if len(shape) != 5:
            raise FgcnError(f"normalize: feature {feature_id!r} has shape {tuple(shape)}; expected (samples, M, T, V, C) -- leave it out "
                            f"with Normalize(only=...)")
        V, C = shape[3], shape[4]
        pairs = [p for p in (self.z_axis_joints, self.x_axis_joints) if p is not None]
        if C not in (2, 3) or (pairs and C != 3):
            raise FgcnError(f"normalize: feature {feature_id!r} has {C} coordinates; expected 2 or 3, and 3 with an axis pair")
        if max([self.origin_joint] + [j for p in pairs for j in p]) >= V:
            raise FgcnError(f"normalize: feature {feature_id!r} has {V} joints; the joint numbers {self.origin_joint}, {pairs} need more")

    name, at_upload = "normalize", True

    def bind(self, shapes: Shapes, n: int, keys: Sequence[str]) -> Tuple[Shapes, List[str]]:
        unknown = set(self.only or ()) - set(keys)
        if unknown:
            raise ValueError(f"normalize names features the data set does not have: {sorted(unknown)}")
        writes = [k for k in shapes if self.applies_to(k)]
        for k in writes:
            self.check_shape(k, (n, *shapes[k]))
        return dict(shapes), writes

    def tables(self, writes: Sequence[str], n: int) -> Dict[Optional[str], np.ndarray]:
        return {}

    def run(self, batches: "ClipBatches", feats: Feats, rows: torch.Tensor, tables: Tables, out: Dict[str, Optional[torch.Tensor]]) -> Feats:
        from . import ops
        feats = dict(feats)
        for k, o in out.items():
            feats[k], frame_map, params = ops.clip_normalize(feats[k], rows, origin_joint=self.origin_joint, z_axis_joints=self.z_axis_joints,
                                                             x_axis_joints=self.x_axis_joints, out=o)
            batches.last_plan[k] = (frame_map, params)
        return feats


class Inertial:
    """What ``ClipBatches(inertial=...)`` does to every raw inertial recording (include/fgcn.h): the reference's
    offline preprocessing of the ``inertial`` and ``skeleton_imu_enhanced`` features.

    ``frames``: feature id -> the number of recorded frames of each sample, for the two features ``main`` (the skeleton, (samples, M, T,
    V, C), whose count Ls is the length the recording is resampled to) and ``signal`` (the recording, (samples, L, S), Li frames of it
    valid).  ``features[signal]`` becomes the (T, S) signal -- resampled by nearest neighbour, zero from frame Ls on, min-max normalised
    over the padded array unless ``minmax=False`` (a constant recording gives 0 / 0 = NaN, as in the reference) -- or is left out of
    the batch with ``drop_signal=True``.  ``enhance=True``: ``features[main]`` becomes (M, T, V + S / 3, 3), the skeleton with the
    resampled, padded recording (not min-max normalised) appended as S / 3 joints of every body."""

    def __init__(self, frames: Mapping[str, Sequence[int]], main: str = "skeleton", signal: str = "inertial", enhance: bool = False,
                 minmax: bool = True, drop_signal: bool = False):
        self.main, self.signal = str(main), str(signal)
        self.enhance, self.minmax, self.drop_signal = bool(enhance), bool(minmax), bool(drop_signal)
        if self.main == self.signal:
            raise ValueError(f"main and signal are both {main!r}")
        if set(frames) != {self.main, self.signal}:
            raise ValueError(f"frames: expected the frame counts of {self.main!r} and {self.signal!r}, got {sorted(frames)}")
        if not self.enhance and self.drop_signal:
            raise ValueError("enhance=False with drop_signal=True leaves nothing to prepare")
        self.frames = {}
        for k in (self.main, self.signal):
            v = np.asarray(frames[k])
            if v.ndim != 1 or v.dtype.kind not in "iu" or (len(v) and v.min() < 1):
                raise ValueError(f"frames[{k!r}]: expected one integer frame count >= 1 per sample")
            self.frames[k] = v.astype(np.int32)
        ls, li = self.frames[self.main], self.frames[self.signal]
        if ls.shape != li.shape:
            raise ValueError(f"frames: {len(ls)} counts for {self.main!r}, {len(li)} for {self.signal!r}")
        bad = np.flatnonzero((ls == 1) & (li != 1))
        if len(bad):                                        # the reference divides by Ls - 1
            raise ValueError(f"frames: sample {int(bad[0])} has one {self.main} frame and {int(li[bad[0]])} {self.signal} frames: a "
                             f"recording cannot be resampled to a single frame")

    def check_shapes(self, shapes: Mapping[str, Sequence[int]], n: int) -> None:
        """Refuses arrays (feature id -> shape with the sample axis) this preparation cannot take -- at construction, not mid-epoch."""
        unknown = {self.main, self.signal} - set(shapes)
        if unknown:
            raise ValueError(f"inertial names features the data set does not have: {sorted(unknown)}")
        main, sig = tuple(shapes[self.main]), tuple(shapes[self.signal])
        if len(main) != 5 or len(sig) != 3:
            raise FgcnError(f"inertial: expected {self.main!r} (samples, M, T, V, C) and {self.signal!r} (samples, L, S), got {main} and {sig}")
        for k, limit, what in ((self.main, main[2], "T"), (self.signal, sig[1], "L")):
            v = self.frames[k]
            if v.shape != (n,) or v.max() > limit:
                raise ValueError(f"frames[{k!r}]: expected {n} frame counts in [1, {limit}] ({what} of {k!r})")
        if self.enhance and (sig[2] % 3 or main[4] not in (2, 3)):
            raise FgcnError(f"inertial: enhance appends joints of three values to a skeleton of 2 or 3 coordinates; {self.signal!r} has "
                            f"{sig[2]} values per frame, {self.main!r} {main[4]} coordinates")

    def sample_shapes(self, shapes: Mapping[str, Sequence[int]]) -> Dict[str, tuple]:
        """feature id -> the shape of a sample as the batch holds it, in the data set's order (the dropped signal left out)."""
        out = {k: tuple(v[1:]) for k, v in shapes.items()}
        M, T, V, _ = out[self.main]
        S = out[self.signal][1]
        if self.enhance:
            out[self.main] = (M, T, V + S // 3, 3)
        if self.drop_signal:
            del out[self.signal]
        else:
            out[self.signal] = (T, S)
        return out

    name, at_upload = "inertial", True

    def bind(self, shapes: Shapes, n: int, keys: Sequence[str]) -> Tuple[Shapes, List[str]]:
        full = {k: (n, *v) for k, v in shapes.items()}
        self.check_shapes(full, n)
        after = self.sample_shapes(full)
        return after, [k for k in after if k == self.signal or (k == self.main and self.enhance)]

    def tables(self, writes: Sequence[str], n: int) -> Dict[Optional[str], np.ndarray]:
        return {k: self.frames[k] for k in (self.signal, self.main)}

    def run(self, batches: "ClipBatches", feats: Feats, rows: torch.Tensor, tables: Tables, out: Dict[str, Optional[torch.Tensor]]) -> Feats:
        """reads the raw recordings and the normalised skeletons in ``feats``"""
        from . import ops
        src_len, dst_len = tables[self.signal], tables[self.main]
        res = {}
        for k, v in feats.items():
            if k == self.main and self.enhance:
                res[k] = ops.imu_enhance(v, rows, feats[self.signal], rows, src_len, dst_len, out=out[k])
            elif k != self.signal:
                res[k] = v
            elif not self.drop_signal:
                res[k], batches.last_inertial = ops.signal_prepare(v, rows, src_len, dst_len, feats[self.main].shape[2], minmax=self.minmax,
                                                                   out=out[k])
        return res


class Streams:
    """What ``ClipBatches(streams=...)`` derives from every skeleton clip it hands out (include/fgcn.h): the input
    streams of the two-stream AGCN family, from the clip as every stage before left it (the motion of a clip is not the resampled motion).

    ``parents``: one entry per joint -- its parent joint, the joint itself for the root (whose bone is zero), or -1 for a joint that is
    copied through (the sensor joints ``Inertial(enhance=True)`` appends).  ``streams``: distinct names of ``STREAMS``, at least one of
    them derived: "joint" the clip itself, "bone" joint minus parent, "motion" frame t+1 minus frame t (zero from the last valid frame
    on), "bone_motion" the motion of the bones.  One name: the feature keeps its id and holds that stream.  Several: "joint" keeps the
    feature's id ``k``, every other comes out as ``f"{k}_{stream}"`` directly behind it, and ``k`` is left out of the batch unless "joint"
    is named.  ``only``: the feature ids to apply to (default: every (M, T, V, C) feature with C of 2 or 3).  ``valid_frames``: feature
    id -> the number of valid frames of each sample, as ``Augment.valid_frames`` (default: all T)."""

    STREAMS = ("joint", "bone", "motion", "bone_motion")

    def __init__(self, parents: Sequence[int], streams: Sequence[str] = ("bone",), only: Optional[Iterable[str]] = None,
                 valid_frames: Optional[Mapping[str, Sequence[int]]] = None):
        if isinstance(streams, str):
            streams = (streams,)
        self.streams = tuple(streams)
        if not self.streams or len(set(self.streams)) != len(self.streams) or not set(self.streams) <= set(self.STREAMS):
            raise ValueError(f"streams={streams!r}: expected distinct names of {self.STREAMS}, at least one")
        if self.streams == ("joint",):
            raise ValueError("streams=('joint',) derives nothing: name at least one of 'bone', 'motion', 'bone_motion'")
        if any(isinstance(p, bool) or not isinstance(p, (int, np.integer)) for p in parents):
            raise ValueError(f"parents={parents!r}: expected one joint number (or -1) per joint")
        self.parents = tuple(int(p) for p in parents)
        V = len(self.parents)
        bad = [v for v, p in enumerate(self.parents) if not -1 <= p < V]
        if V == 0 or bad:
            raise ValueError(f"parents: expected {V or 'at least one'} entries in [-1, {V}); joint(s) {bad} have {[self.parents[v] for v in bad]}")
        self.only = None if only is None else frozenset(only)
        self.valid_frames = dict(valid_frames or {})
        self._device_parents = {}       # device -> the (V) int32 table, built (and checked by ops) on the first batch there

    @classmethod
    def for_dataset(cls, name: str, extra_joints: int = 0, **kw) -> "Streams":
        """The parents of a data set's skeleton (``"utd_mhad"``, ``"mmact"``, ``"ntu_rgb_d"``): its constants module's ``skeleton_edges``
        are (child, parent) rows and its ``center_joint`` is the root; ``extra_joints`` entries of -1 follow for appended sensor joints."""
        from .util.dynamic_import import import_dataset_constants
        got = import_dataset_constants(name, ["skeleton_edges", "center_joint", "num_joints"])
        if len(got) != 3:
            raise ValueError(f"data set {name!r} has no skeleton graph constants")
        edges, center, V = got
        parents = {**{int(child): int(parent) for child, parent in np.asarray(edges).tolist()}, int(center): int(center)}
        missing = sorted(set(range(V)) - set(parents))
        if missing:
            raise ValueError(f"data set {name!r}: joints {missing} of {V} appear in no edge as the child, and are not the centre joint")
        if extra_joints < 0:
            raise ValueError(f"extra_joints={extra_joints}")
        return cls([parents[v] for v in range(V)] + [-1] * int(extra_joints), **kw)

    name, at_upload = "streams", False

    def applies_to(self, feature_id: str, sample_shape: Sequence[int]) -> bool:
        if self.only is not None:
            return feature_id in self.only
        return len(sample_shape) == 4 and sample_shape[3] in (2, 3)

    def output_ids(self, feature_id: str) -> Dict[str, str]:
        """stream -> the id it comes out under, in the batch's order: the feature's own id first where it is kept"""
        if len(self.streams) == 1:
            return {self.streams[0]: feature_id}
        ordered = [s for s in self.streams if s == "joint"] + [s for s in self.streams if s != "joint"]
        return {s: feature_id if s == "joint" else f"{feature_id}_{s}" for s in ordered}

    def bind(self, shapes: Shapes, n: int, keys: Sequence[str]) -> Tuple[Shapes, List[str]]:
        unknown = (set(self.valid_frames) | set(self.only or ())) - set(keys)
        if unknown:
            raise ValueError(f"streams names features the data set does not have: {sorted(unknown)}")
        applied = [k for k in shapes if self.applies_to(k, shapes[k])]
        missing = (set(self.valid_frames) | set(self.only or ())) - set(applied)
        if missing:
            raise ValueError(f"streams names features that are not in the batch at this stage or that it does not apply to: {sorted(missing)}")
        V = len(self.parents)
        after, writes = {}, []
        for k, shape in shapes.items():
            if k not in applied:
                after[k] = shape
                continue
            if len(shape) != 4 or shape[3] not in (2, 3):
                raise FgcnError(f"streams: feature {k!r} has shape {(n, *shape)}; expected (samples, M, T, V, C) with C of 2 or 3 -- leave it "
                                f"out with Streams(only=...)")
            if shape[2] != V:
                raise FgcnError(f"streams: feature {k!r} has {shape[2]} joints, parents has {V} entries")
            if k in self.valid_frames:
                v = np.asarray(self.valid_frames[k])
                if v.shape != (n,) or v.dtype.kind not in "iu" or v.min() < 1 or v.max() > shape[1]:
                    raise ValueError(f"valid_frames[{k!r}]: expected {n} frame counts in [1, {shape[1]}]")
            for out_id in self.output_ids(k).values():
                after[out_id] = shape
                writes.append(out_id)
        taken = [k for k in shapes if k not in applied] + writes
        clash = sorted({k for k in taken if taken.count(k) > 1})
        if clash:
            raise ValueError(f"streams: the output ids {clash} are already features of the batch -- rename them or use Streams(only=...)")
        return after, writes

    def tables(self, writes: Sequence[str], n: int) -> Dict[Optional[str], np.ndarray]:
        """feature id: the valid frames of its clips"""
        return {k: np.asarray(v).astype(np.int32) for k, v in self.valid_frames.items()}

    def run(self, batches: "ClipBatches", feats: Feats, rows: Union[torch.Tensor, Dict[str, torch.Tensor]], tables: Tables,
            out: Dict[str, Optional[torch.Tensor]]) -> Feats:
        """``rows`` per feature where the stage before wrote some features and not others (see the protocol above ``Augment``)"""
        from . import ops
        res, batches.last_streams = {}, {}
        for k, src in feats.items():
            if not self.applies_to(k, src.shape[1:]):
                res[k] = src
                continue
            if src.device not in self._device_parents:
                self._device_parents[src.device] = ops.stream_parents(self.parents, src.device)
            ids = self.output_ids(k)
            got = ops.clip_streams(src, rows[k] if isinstance(rows, dict) else rows, self._device_parents[src.device], streams=self.streams,
                                   valid=tables.get(k), out={s: out[i] for s, i in ids.items() if out[i] is not None})
            res.update({i: got[s] for s, i in ids.items()})
            batches.last_streams[k] = list(ids.values())
        return res


class Window:
    """What ``ClipBatches(window=...)`` does to every clip it hands out (include/fgcn.h): a part of the clip's VALID
    frames, linearly interpolated to a window of ``frames`` frames -- the model is built for the window (``ClipBatches.shapes``), not for the
    stored T.

    ``frames``: the window's length W, an int for every modality or a mapping feature id -> int for modalities with different T (the
    window then applies to the ids it names).  ``interval = (lo, hi)``, ``0 < lo <= hi <= 1``: the part's length as a fraction of the
    recording.  ``train=True``: the length is uniform in the interval and the start uniform in what is left, drawn per (seed, epoch, clip)
    as ``Augment`` draws -- from the counter word ``Augment`` leaves free, so the two are independent at one ``site`` -- on every batch.
    ``train=False``: the centred part of length ``hi``, no random numbers; a resident split is windowed ONCE, at construction, and then
    takes W / T of the memory.  All modalities of a sample take the same part of the recording.  ``valid_frames``: feature id -> the number
    of valid frames of each sample (``data.valid_frames`` counts them; default: all T).  ``only``: the feature ids to window (default: all,
    or the ids ``frames`` names); the others keep their T."""

    name = "window"

    def __init__(self, frames: Union[int, Mapping[str, int]], interval: Sequence[float] = (0.5, 1.0), train: bool = True,
                 valid_frames: Optional[Mapping[str, Sequence[int]]] = None, only: Optional[Iterable[str]] = None, site: int = 0):
        def count(w) -> int:
            if isinstance(w, bool) or not isinstance(w, (int, np.integer)) or w < 1:
                raise ValueError(f"frames={frames!r}: expected a frame count >= 1, or one per feature id")
            return int(w)
        self.frames = {str(k): count(w) for k, w in frames.items()} if isinstance(frames, Mapping) else count(frames)
        if isinstance(self.frames, dict) and not self.frames:
            raise ValueError("frames={}: the window applies to no feature")
        interval = tuple(float(x) for x in interval)
        if len(interval) != 2 or not all(np.isfinite(interval)) or not 0.0 < interval[0] <= interval[1] <= 1.0:
            raise ValueError(f"interval={interval!r}: expected (lo, hi) with 0 < lo <= hi <= 1")
        self.interval, self.train, self.site = interval, bool(train), int(site)
        self.mode = "random" if self.train else "centre"
        self.at_upload = not self.train                     # nothing random in the centred part: a resident split takes it once
        self.valid_frames = dict(valid_frames or {})
        self.only = None if only is None else frozenset(only)
        if self.only is not None and isinstance(self.frames, dict) and not self.only <= set(self.frames):
            raise ValueError(f"only={sorted(self.only)} names features that frames={self.frames!r} gives no length")

    def applies_to(self, feature_id: str) -> bool:
        return (self.only is None or feature_id in self.only) and (not isinstance(self.frames, dict) or feature_id in self.frames)

    def length(self, feature_id: str) -> int:
        return self.frames[feature_id] if isinstance(self.frames, dict) else self.frames

    def bind(self, shapes: Shapes, n: int, keys: Sequence[str]) -> Tuple[Shapes, List[str]]:
        named = set(self.valid_frames) | set(self.only or ()) | set(self.frames if isinstance(self.frames, dict) else ())
        if named - set(keys):
            raise ValueError(f"window names features the data set does not have: {sorted(named - set(keys))}")
        if named - set(shapes):
            raise ValueError(f"window names features that are not in the batch at this stage: {sorted(named - set(shapes))}")
        writes = [k for k in shapes if self.applies_to(k)]
        stale = sorted(set(self.valid_frames) - set(writes))
        if stale:
            raise ValueError(f"window: valid_frames{stale} for features the window does not apply to")
        after = dict(shapes)
        for k in writes:
            shape = shapes[k]
            if len(shape) not in (2, 4):
                raise FgcnError(f"window: feature {k!r} has shape {(n, *shape)}; expected (samples, M, T, V, C) or (samples, T, S) -- leave it "
                                f"out with Window(only=...)")
            t_axis = 0 if len(shape) == 2 else 1
            if k in self.valid_frames:
                v = np.asarray(self.valid_frames[k])
                if v.shape != (n,) or v.dtype.kind not in "iu" or v.min() < 1 or v.max() > shape[t_axis]:
                    raise ValueError(f"valid_frames[{k!r}]: expected {n} frame counts in [1, {shape[t_axis]}]")
            after[k] = (*shape[:t_axis], self.length(k), *shape[t_axis + 1:])
        return after, writes

    def tables(self, writes: Sequence[str], n: int) -> Dict[Optional[str], np.ndarray]:
        """None: the clips' ids, which key the random numbers (the centred part has none); feature id: the valid frames of its clips"""
        valid = {k: np.asarray(self.valid_frames[k]).astype(np.int32) for k in writes if k in self.valid_frames}
        return {None: np.arange(n, dtype=np.int64), **valid} if self.train else valid

    def run(self, batches: "ClipBatches", feats: Feats, rows: Union[torch.Tensor, Dict[str, torch.Tensor]], tables: Tables,
            out: Dict[str, Optional[torch.Tensor]]) -> Feats:
        from . import ops
        feats = dict(feats)
        for k, o in out.items():
            feats[k], batches.last_window[k] = ops.clip_window(
                feats[k], rows[k] if isinstance(rows, dict) else rows, tables[None] if self.train else None, window=self.length(k),
                interval=self.interval, mode=self.mode, seed=batches.seed, epoch=batches.epoch, site=self.site, valid=tables.get(k), out=o)
        return feats


NORMALIZE_CHUNK = 2048      # clips per call when a resident split is normalised, prepared and windowed at upload


def valid_frames(dataset: MultiModalDataset, feature_id: str, device: Union[str, torch.device] = "cuda",
                 chunk: int = NORMALIZE_CHUNK, bodies: Optional[Bodies] = None) -> np.ndarray:
    """-> (n,) int32: the valid frames of every sample of feature ``feature_id`` of ``dataset`` -- 1 + the last frame in which any body holds
    a value that is not zero, 1 for a clip that holds none (``fgcn_clip_valid_frames``, include/fgcn.h) -- the table ``Window``, ``Augment``
    and ``Streams`` take as ``valid_frames[feature_id]`` (the reference's feature files do not hold it).  One pass over the stored array
    in chunks of ``chunk`` clips: upload, count on the device, download; a memory-mapped split is read once, front to back, and never
    held in memory as a whole.  Count the STORED clips of a raw split: ``Normalize`` repeats the valid frames up to T.  ``bodies``: the
    ``Bodies`` that ``ClipBatches`` is given -- the count is then taken over the bodies it selects (``fgcn_clip_bodies``, then the count,
    chunk by chunk on the device): a dropped body that outlives the kept ones does not stretch the table."""
    from . import ops
    if feature_id not in dataset.features_data:
        raise ValueError(f"valid_frames: the data set has no feature {feature_id!r} (it has {sorted(dataset.features_data)})")
    device = torch.device(device)
    if device.type != "cuda":
        raise FgcnError("valid_frames runs a HIP kernel and needs a 'cuda' device: there is no host fallback")
    if chunk < 1:
        raise ValueError(f"chunk={chunk}")
    array, n = dataset.features_data[feature_id][1], len(dataset)
    if array.ndim not in (3, 5):
        raise FgcnError(f"valid_frames: feature {feature_id!r} has shape {tuple(array.shape)}; expected (samples, M, T, V, C) or (samples, T, S)")
    if bodies is not None:
        if not bodies.applies_to(feature_id):
            raise ValueError(f"valid_frames: bodies does not apply to feature {feature_id!r}")
        bodies.bind({feature_id: tuple(array.shape[1:])}, n, list(dataset.features_data))      # (refuses what the selection cannot take)
    out = np.empty(n, dtype=np.int32)
    for lo in range(0, n, chunk):
        clips = torch.from_numpy(np.array(array[lo:min(lo + chunk, n)], dtype=np.float32)).to(device)
        if bodies is not None:
            clips = ops.clip_bodies(clips, torch.arange(len(clips), dtype=torch.int64, device=device), bodies=bodies.bodies)[0]
        out[lo:lo + len(clips)] = ops.clip_valid_frames(clips).cpu().numpy()
    return out


class ClipBatches:
    """Iterate one epoch of ``(features, labels, indices)`` device batches over a ``MultiModalDataset``.

    ``batch_size`` is the global batch (the reference's config value); rank r of ``world`` receives clips
    ``[r*bs/world, (r+1)*bs/world)`` of each global batch.  ``shuffle`` permutes with ``seed + epoch`` (``set_epoch``), the
    same permutation on every rank.  ``resident``: True / False, or None = upload the split when it takes at most
    ``resident_budget`` bytes.  Features come out float32, labels int64 (session.py:171-174).

    ``bodies``, ``normalize``, ``inertial``, ``augment``: None = the stored clips as they are; otherwise the stages (``self.stages``) run on
    the device in that order, each on what the one before left: ``shapes`` holds the sample shapes behind the last, ``out_keys`` their ids.
    A ``Bodies`` = the FIRST stage: of the Mr bodies of the (samples, Mr, T, V, C) arrays it names, the M most energetic come out, in
    descending order -- ``shapes`` then holds M, and the model is built from ``shapes``; ``last_bodies`` (feature id -> (order, scores))
    keeps the tables of the last call.  A resident split is selected once, at construction (``dev_feat`` then holds M / Mr of the stored
    bytes; whether a split is resident is still decided on the STORED size, which is what the upload holds until the selection is done).
    A ``Normalize`` = the (samples, M, T, V, C) arrays it names hold RAW skeletons; ``last_plan`` (feature id -> (frame_map, params))
    keeps the tables of the last call.  An ``Inertial`` = the signal it names holds RAW recordings; ``last_inertial`` keeps the (clips, 2)
    minimum / maximum table of the last call.  Both take a resident split once, at construction (``dev_feat`` then holds the prepared
    arrays), and a streamed batch behind its copy.  An ``Augment`` = every clip of the modalities it names transformed as it is gathered,
    a pure function of (``seed``, the epoch ``set_epoch`` set, the clip's index in the data set) -- labels and ``indices`` are
    untouched; ``last_params`` (feature id -> (clips, 12) tensor) keeps the parameter tables of the last batch.  ``streams``: a
    ``Streams`` = the last stage, on every batch: the skeleton features it names come out as their bone / motion streams (under the ids its
    docstring lists); ``last_streams`` (feature id -> the ids it came out under) keeps the map of the last batch.  ``window``: a ``Window`` =
    the third stage, behind ``inertial`` and in front of ``augment``: every clip of the modalities it names comes out as a part of its valid
    frames resized to the window's W frames -- ``shapes`` then holds W, and the model is built from ``shapes``; with ``train=False`` a
    resident split is windowed once, at construction (``dev_feat`` holds W frames); ``last_window`` (feature id -> (clips, 2) tensor)
    keeps the ``(o, r)`` table of the last call.  None, the default: no such stage, and every call issued is what it was."""

    def __init__(self, dataset: MultiModalDataset, batch_size: int, *, shuffle: bool = False, drop_last: bool = False,
                 seed: int = 1, rank: int = 0, world: int = 1, device: Union[str, torch.device] = "cuda",
                 resident: Optional[bool] = None, resident_budget: int = 64 << 30, augment: Optional[Augment] = None,
                 normalize: Optional[Normalize] = None, inertial: Optional[Inertial] = None, streams: Optional[Streams] = None,
                 window: Optional[Window] = None, bodies: Optional[Bodies] = None):
        if batch_size % world:
            raise ValueError(f"global batch {batch_size} is not divisible by world size {world}")
        self.ds, self.bs, self.shuffle, self.drop_last = dataset, batch_size, shuffle, drop_last
        self.seed, self.rank, self.world, self.epoch = seed, rank, world, 0
        self.device = torch.device(device)
        self.keys = list(dataset.features_data)
        self.arrays = {k: dataset.features_data[k][1] for k in self.keys}
        n = len(dataset)
        for k, a in self.arrays.items():
            if not isinstance(a, np.ndarray) or len(a) < n:
                raise TypeError(f"ClipBatches needs array-backed features with >= {n} samples (feature {k!r})")
        nbytes = sum(int(np.prod(a.shape[1:])) * 4 * n for a in self.arrays.values())
        self.resident = nbytes <= resident_budget if resident is None else bool(resident)
        self.labels = torch.from_numpy(np.asarray(dataset.labels_data).astype(np.int64))
        on_gpu = self.device.type == "cuda"
        self.normalize, self.inertial, self.window, self.augment, self.streams = normalize, inertial, window, augment, streams
        self.bodies = bodies
        self.stages = [s for s in (bodies, normalize, inertial, window, augment, streams) if s is not None]      # in the order they run
        self.last_plan, self.last_inertial, self.last_params, self.last_streams, self.last_window = {}, None, {}, {}, {}
        self.last_bodies = {}
        for later in (augment, streams):
            stale = sorted(k for k in later.valid_frames if window.applies_to(k)) if window is not None and later is not None else []
            if stale:                                       # the windowed clip fills all W frames: the table no longer describes it
                raise ValueError(f"{later.name}: valid_frames{stale} behind a Window that resizes these features to frames that are all valid "
                                 f"-- give the table to the Window alone")
        if streams is not None and augment is not None:
            stale = sorted(k for k in streams.valid_frames if augment.applies_to(k))
            if stale:                                       # the augmented clip fills all T frames: the table no longer describes it
                raise ValueError(f"streams: valid_frames{stale} behind an Augment that resamples these features to all T frames -- give the "
                                 f"table to the Augment alone")
        self.shapes = {k: tuple(a.shape[1:]) for k, a in self.arrays.items()}      # of a sample, as the batch holds it
        self.writes, self.tables, after = {}, {}, {}        # per stage: the features it writes, its host tables, the shapes behind it
        for s in self.stages:
            if not on_gpu:
                raise FgcnError(f"ClipBatches({s.name}=...) runs a HIP kernel and needs device='cuda': there is no host fallback")
            self.shapes, self.writes[s.name] = s.bind(self.shapes, n, self.keys)
            after[s.name] = self.shapes
            self.tables[s.name] = {t: torch.from_numpy(a) for t, a in s.tables(self.writes[s.name], n).items()}
        self.out_keys = list(self.shapes)
        self.norm_keys = self.writes.get("normalize", [])
        if self.resident:
            self.dev_feat = {k: torch.from_numpy(np.array(a[:n], dtype=np.float32)).to(self.device)
                             for k, a in self.arrays.items()}
            self.dev_labels = self.labels.to(self.device)
            # the whole tables, indexed by source row; the sample ids (table None) are the row numbers themselves here
            self.dev_tab = {s.name: {t: v.to(self.device) for t, v in self.tables[s.name].items() if t is not None} for s in self.stages}
            if sum(not s.at_upload for s in self.stages) > 1:      # the rows of what one per-batch stage wrote, for the next
                self.batch_rows = torch.arange(batch_size // world, dtype=torch.int64, device=self.device)
            for s in self.stages:
                if s.at_upload:                             # once, in chunks: nothing is done per batch, and the next stage reads the result
                    done = {k: torch.empty((n, *after[s.name][k]), dtype=torch.float32, device=self.device) for k in self.writes[s.name]}
                    tabs = self.dev_tab.pop(s.name)
                    for lo in range(0, n, NORMALIZE_CHUNK):
                        rows = torch.arange(lo, min(lo + NORMALIZE_CHUNK, n), dtype=torch.int64, device=self.device)
                        s.run(self, self.dev_feat, rows, {**tabs, None: rows}, {k: v[lo:lo + len(rows)] for k, v in done.items()})
                    self.dev_feat = {k: done.get(k, self.dev_feat[k]) for k in after[s.name]}      # (what it replaced is released)
        else:
            per = batch_size // world
            mk = lambda shape, dt: torch.empty(shape, dtype=dt, pin_memory=on_gpu)      # noqa: E731
            self.host = [{k: mk((per, *a.shape[1:]), torch.float32) for k, a in self.arrays.items()} for _ in range(2)]
            self.host_lab = [mk((per,), torch.int64) for _ in range(2)]
            self.dev = [{k: torch.empty((per, *a.shape[1:]), dtype=torch.float32, device=self.device)
                         for k, a in self.arrays.items()} for _ in range(2)]
            self.dev_lab = [torch.empty((per,), dtype=torch.int64, device=self.device) for _ in range(2)]
            self.copy_stream = torch.cuda.Stream(self.device) if on_gpu else None
            self.copied = [torch.cuda.Event() if on_gpu else None for _ in range(2)]
            self.consumed = [torch.cuda.Event() if on_gpu else None for _ in range(2)]
            if self.stages:
                self.slot_rows = torch.arange(per, dtype=torch.int64, device=self.device)
            # per slot and stage: what the stage writes (the uploaded rows, or the stage before, are its source; the slot's `consumed`
            # event covers it) and the table rows of the slot's clips, staged and copied with the clips
            self.stage_out = [{s.name: {k: torch.empty((per, *after[s.name][k]), dtype=torch.float32, device=self.device)
                                        for k in self.writes[s.name]} for s in self.stages} for _ in range(2)]
            self.dev_tab = [{name: {t: torch.empty((per,), dtype=v.dtype, device=self.device) for t, v in tabs.items()}
                             for name, tabs in self.tables.items()} for _ in range(2)]
            # per slot, every table in the order it is staged and copied: (the table, the slot's pinned rows, the slot's device rows)
            self.slot_tabs = [[(v, mk((per,), v.dtype), dev[name][t]) for name, tabs in self.tables.items() for t, v in tabs.items()]
                              for dev in self.dev_tab]

    def set_epoch(self, epoch: int) -> None:
        self.epoch = epoch

    def __len__(self) -> int:
        """Batches per epoch, the same on every rank (a ragged tail shorter than the world size yields no batch)."""
        n = len(self.ds)
        full, tail = divmod(n, self.bs)
        return full + int(not self.drop_last and tail >= self.world)

    def _order(self) -> torch.Tensor:
        n = len(self.ds)
        if not self.shuffle:
            return torch.arange(n)
        return torch.randperm(n, generator=torch.Generator().manual_seed(self.seed + self.epoch))

    def _shards(self) -> Iterator[torch.Tensor]:
        order = self._order()
        for b in range((len(order) + self.bs - 1) // self.bs if not self.drop_last else len(order) // self.bs):
            glob = order[b * self.bs:(b + 1) * self.bs]
            if len(glob) != self.bs:
                # ragged last batch (drop_last=False).  Every rank must step the same number of times with the same shard
                # size: ranks average their gradients with equal weight in ONE collective, so an empty or shorter shard would
                # hang the all-reduce or skew the mean.  The tail is trimmed to a multiple of the world size (at most
                # world - 1 clips of the epoch are left out, none when world == 1) and skipped when nothing is left.
                glob = glob[:len(glob) // self.world * self.world]
                if len(glob) == 0:
                    continue
            yield glob[shard_batch(len(glob), self.rank, self.world)]

    def _out(self, feats: Dict[str, torch.Tensor]) -> Features:
        return feats[self.out_keys[0]] if len(self.out_keys) == 1 else feats

    def __iter__(self) -> Iterator[Tuple[Features, torch.Tensor, torch.Tensor]]:
        if self.resident:
            per_batch = [s for s in self.stages if not s.at_upload]
            written = {k for s in per_batch for k in self.writes[s.name]}
            for idx in self._shards():
                di = idx.to(self.device)
                feats, rows = self.dev_feat, di          # rows = ids = the shard's indices, for the first per-batch stage
                for s in per_batch:
                    feats = s.run(self, feats, rows, {**self.dev_tab[s.name], None: di}, dict.fromkeys(self.writes[s.name]))
                    if s is not per_batch[-1]:           # what it wrote holds the batch's rows in order, the rest is still the resident array
                        rows = {k: self.batch_rows[:len(idx)] if k in self.writes[s.name] else rows[k] if isinstance(rows, dict) else rows
                                for k in feats}
                feats = {k: v if k in written else v.index_select(0, di) for k, v in feats.items()}
                yield self._out(feats), self.dev_labels.index_select(0, di), idx
            return
        on_gpu = self.device.type == "cuda"

        def stage(slot: int, idx: torch.Tensor) -> int:
            """Gather rows ``idx`` into pinned slot ``slot`` and start their copy to the device on the copy stream."""
            m = len(idx)
            if on_gpu:
                self.copied[slot].synchronize()          # the slot's previous H2D copy has left the pinned buffer
            order = np.sort(idx.numpy())                 # ascending file offsets for the memory map; undone below
            back = np.argsort(np.argsort(idx.numpy()))
            for k, a in self.arrays.items():
                rows = np.asarray(a[order], dtype=np.float32)
                self.host[slot][k][:m].copy_(torch.from_numpy(rows[back]))
            self.host_lab[slot][:m].copy_(self.labels[idx])
            for table, host, _ in self.slot_tabs[slot]:
                host[:m].copy_(table[idx])
            if on_gpu:
                self.copy_stream.wait_event(self.consumed[slot])      # the consumer of the device slot's last batch is done
                with torch.cuda.stream(self.copy_stream):
                    for k in self.keys:
                        self.dev[slot][k][:m].copy_(self.host[slot][k][:m], non_blocking=True)
                    self.dev_lab[slot][:m].copy_(self.host_lab[slot][:m], non_blocking=True)
                    for _, host, dev in self.slot_tabs[slot]:
                        dev[:m].copy_(host[:m], non_blocking=True)
                    self.copied[slot].record(self.copy_stream)
            else:
                for k in self.keys:
                    self.dev[slot][k][:m].copy_(self.host[slot][k][:m])
                self.dev_lab[slot][:m].copy_(self.host_lab[slot][:m])
            return m

        shards = list(self._shards())
        if on_gpu:
            for e in self.copied + self.consumed:
                e.record(torch.cuda.current_stream(self.device))
        pending = stage(0, shards[0]) if shards else 0
        for i, idx in enumerate(shards):
            slot, m = i % 2, pending
            if i + 1 < len(shards):
                pending = stage((i + 1) % 2, shards[i + 1])           # overlaps the step that consumes batch i
            if on_gpu:
                torch.cuda.current_stream(self.device).wait_event(self.copied[slot])
            feats = {k: self.dev[slot][k][:m] for k in self.keys}
            for s in self.stages:
                # on the consumer's stream, behind the copy: the slot's rows (or the stage before) are the source, `consumed` below covers
                # kernels and consumer
                feats = s.run(self, feats, self.slot_rows[:m], {t: v[:m] for t, v in self.dev_tab[slot][s.name].items()},
                              {k: v[:m] for k, v in self.stage_out[slot][s.name].items()})
            yield self._out(feats), self.dev_lab[slot][:m], idx
            if on_gpu:
                self.consumed[slot].record(torch.cuda.current_stream(self.device))
