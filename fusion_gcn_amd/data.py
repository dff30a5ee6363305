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
  * ``sensors=Sensors(...)`` (ours; the reference has none): one ``fgcn_clip_sensors`` call per inertial feature -- the (T, S) signal and
    the sensor joints of an enhanced skeleton -- a random rotation of the sensor frame, a gain per sensor, a smooth magnitude warp, additive
    jitter and the drop of a whole sensor, keyed like the augmentation and by (frame, sensor), then (``minmax=True``) the min-max
    normalisation that ``Inertial(minmax=False)`` left out; behind ``augment``, whose resampling would smooth the jitter: section 8p;
  * ``streams=Streams(parents, ...)`` (the bone and motion inputs 2s-AGCN is trained on; the reference has none): one ``fgcn_clip_streams``
    call per skeleton feature -- joint minus parent joint, frame t+1 minus frame t inside the valid frames, and the motion of the bones,
    of the clip as the stages before left it: section 8j.
The first three run once at upload on the resident path -- and so does the window of an evaluation split, which has no random part -- the
training window, the two augmentations and the streams on every batch; on the streaming path all run per batch, behind the copy.  The seven
classes live in stages.py and are imported here; what ``ClipBatches`` asks of a stage is the docstring of their base, ``stages.Stage``.
"""
from __future__ import annotations

import os
from typing import Dict, Iterator, Optional, Sequence, Tuple, Union

import numpy as np
import numpy.lib.format
import torch

from ._lib import FgcnError
from .dp import shard_batch
from .stages import Augment, Bodies, Inertial, Normalize, Sensors, Stage, Streams, Window      # noqa: F401 (`from .data import Window` still works)

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
# The stages of the preparation on the device live in stages.py, under ``Stage``, whose docstring is what ClipBatches asks of one.  A further
# stage is one more class there and one more entry of the tuple that builds ``ClipBatches.stages``.

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
    keeps the ``(o, r)`` table of the last call.  ``sensors``: a ``Sensors`` = the stage behind ``augment`` and in front of ``streams``, on
    every batch: the sensors of the (T, S) signals and -- with ``Sensors(joints=...)`` -- the sensor joints of the (M, T, V, 3) arrays it
    applies to come out rotated, scaled, warped, jittered and dropped, a pure function of (``seed``, the epoch, the clip's index in the
    data set) as the augmentation is, every body and both arrays of a sample with the same values; ``last_sensors`` (feature id ->
    ((clips, 12 + 12 G) parameter table, (clips, 2) minimum / maximum table)) keeps the tables of the last batch.  None, the default: no such
    stage, and every call issued is what it was."""

    def __init__(self, dataset: MultiModalDataset, batch_size: int, *, shuffle: bool = False, drop_last: bool = False,
                 seed: int = 1, rank: int = 0, world: int = 1, device: Union[str, torch.device] = "cuda",
                 resident: Optional[bool] = None, resident_budget: int = 64 << 30, augment: Optional[Augment] = None,
                 normalize: Optional[Normalize] = None, inertial: Optional[Inertial] = None, streams: Optional[Streams] = None,
                 window: Optional[Window] = None, bodies: Optional[Bodies] = None, sensors: Optional[Sensors] = None):
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
        self.bodies, self.normalize, self.inertial, self.window, self.augment, self.streams = bodies, normalize, inertial, window, augment, streams
        self.sensors = sensors
        self.stages = [s for s in (bodies, normalize, inertial, window, augment, sensors, streams) if s is not None]      # THE order they run in
        self.last_bodies, self.last_plan, self.last_inertial, self.last_window, self.last_params, self.last_streams = {}, {}, None, {}, {}, {}
        self.last_sensors = {}
        for i, later in enumerate(self.stages):
            for earlier in self.stages[:i]:
                stale = sorted(k for k in later.valid_frames if earlier.fills_frames(k))
                if stale:                                   # the earlier stage's clip fills every frame: the table no longer describes it
                    raise ValueError(f"{later.name}: valid_frames{stale} behind {earlier.fills} -- give the table to the "
                                     f"{type(earlier).__name__} alone")
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
                    # a table is indexed by the rows of its feature: the whole table for a feature that is still the resident array, the
                    # batch's entries in order for one an earlier per-batch stage wrote (only a stage that does not fill the frames, a
                    # Sensors, leaves a later stage such a table)
                    tabs = {t: v.index_select(0, di) if isinstance(rows, dict) and rows.get(t, di) is not di else v
                            for t, v in self.dev_tab[s.name].items()}
                    feats = s.run(self, feats, rows, {**tabs, None: di}, dict.fromkeys(self.writes[s.name]))
                    if s is not per_batch[-1]:           # what it wrote holds the batch's rows in order, the rest is still the resident array
                        rows = {k: self.batch_rows[:len(idx)] if k in self.writes[s.name] else Stage.rows_of(rows, k) for k in feats}
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
