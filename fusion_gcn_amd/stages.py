"""The stages of ``ClipBatches``' preparation on the device: ``Stage``, what data.py asks of one and what they share, and the seven stages,
whose ``run`` calls the HIP wrappers of ops.py (no host fallback).  data.py's module docstring says what each does and in which order."""
from __future__ import annotations

from typing import Dict, Iterable, List, Mapping, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import ops
from ._lib import BODIES_MAX, SENSORS_MAX, SENSORS_MAX_KNOTS, FgcnError

Shapes = Dict[str, tuple]       # feature id -> the shape of a sample
Feats = Dict[str, torch.Tensor]
Tables = Dict[Optional[str], torch.Tensor]
Rows = Union[torch.Tensor, Dict[str, torch.Tensor]]

# A further stage is one more subclass of Stage here and one more entry of the tuple that builds ClipBatches.stages: Streams was the fourth,
# Window is the fifth (it runs third: in front of the rotation, which then touches W frames instead of T, and of the streams, whose motion is
# the windowed clip's).  Bodies is the sixth, it runs first: it decides what body 0 is, by which Normalize centres and rotates the clip, and
# how many body slots every later stage and the model see.  Sensors is the seventh, it runs sixth: behind Augment, whose resampling would smooth
# its jitter, and in front of Streams, which derive their streams from the clip the model sees.

class Stage:
    """A stage of ClipBatches' preparation on the device -- Bodies, Normalize, Inertial, Window, Augment, Sensors, Streams, run in that order --
    is a configuration object with
      name        its keyword of ClipBatches, for the refusal of a device without HIP kernels
      at_upload   True: a resident split takes it once, at construction; False: every batch does (a class attribute, or one of the instance:
                  Window(train=False) runs at upload, Window(train=True) per batch)
      bind(shapes, n, keys) -> (shapes, writes)   at construction: refuses what the stage cannot take of ``n`` samples of ``shapes`` (as the
                  stage before left them) in a data set with the feature ids ``keys``; -> the shapes behind the stage and the feature ids
                  it writes, which are the ones that need an output buffer
      tables(writes, n) -> {name: (n,) array}   what the kernels read beside the rows, indexed by the sample's index in the data set;
                  None names the sample ids themselves
      run(batches, feats, rows, tables, out) -> feats   launches on the current stream: rows ``rows`` of the arrays ``feats`` into the buffers
                  ``out`` (feature id -> tensor, or None = a new one); ``tables[name][rows[j]]`` belongs to output row j, except the sample ids,
                  which are listed by output row; what the stage keeps for inspection goes to ``batches.last_*``.  A per-batch stage that
                  may run BEHIND another per-batch stage on the resident path (Augment behind Window, Sensors behind both, Streams behind
                  all) takes ``rows`` per feature too, {feature id: rows} (``rows_of`` reads either): what the stage before wrote holds the
                  batch's rows in order (rows 0..m-1), what it left out is still the resident array (the shard's indices).  The rows are
                  handed over per feature rather than the left-out features gathered first: a gather would be one more pass over rows that
                  the stage's own kernel gathers anyway.  A table goes with its feature's rows: where the stage before wrote the feature
                  without filling its frames (Sensors), ``ClipBatches`` hands the next stage the batch's table entries in order.
      fills_frames(feature_id) -> bool   True: every frame of the feature is valid behind the stage, so that a ``valid_frames`` table of a
                  later stage no longer describes it (``ClipBatches`` refuses one); ``fills`` then says how, for that refusal
    The class holds what the stages share and nothing more."""

    name: str
    at_upload = True

    def __init__(self, only: Optional[Iterable[str]] = None, valid_frames: Optional[Mapping[str, Sequence[int]]] = None):
        self.only = None if only is None else frozenset(only)
        self.valid_frames = dict(valid_frames or {})
        self._frame_tables: Dict[str, np.ndarray] = {}      # feature id -> the table ``bind`` checked

    def applies_to(self, feature_id: str) -> bool:
        return self.only is None or feature_id in self.only

    def fills_frames(self, feature_id: str) -> bool:
        return False

    def tables(self, writes: Sequence[str], n: int) -> Dict[Optional[str], np.ndarray]:
        return {}

    @staticmethod
    def rows_of(rows: Rows, feature_id: str) -> torch.Tensor:
        return rows[feature_id] if isinstance(rows, dict) else rows

    def refuse_unknown(self, named: Iterable[str], keys: Iterable[str], batch: Optional[Iterable[str]] = None, or_what: str = "") -> None:
        """Refuses feature ids the data set (``keys``) does not have and, with ``batch``, ids that the batch does not hold at this stage"""
        unknown = set(named) - set(keys)
        if unknown:
            raise ValueError(f"{self.name} names features the data set does not have: {sorted(unknown)}")
        missing = set() if batch is None else set(named) - set(batch)
        if missing:
            raise ValueError(f"{self.name} names features that are not in the batch at this stage{or_what}: {sorted(missing)}")

    def frame_table(self, feature_id: str, n: int, T: int, table=None) -> np.ndarray:
        """-> ``valid_frames[feature_id]`` (or ``table``, what the stage made of it) as (n,) int32 for ``tables``; refused unless in [1, T]"""
        v = np.asarray(self.valid_frames[feature_id] if table is None else table)
        if v.shape != (n,) or v.dtype.kind not in "iu" or v.min() < 1 or v.max() > T:
            raise ValueError(f"valid_frames[{feature_id!r}]: expected {n} frame counts in [1, {T}]")
        self._frame_tables[feature_id] = v.astype(np.int32, copy=False)
        return self._frame_tables[feature_id]

    def frame_tables(self, feature_ids: Iterable[str]) -> Dict[str, np.ndarray]:
        """feature id -> its int32 table, for ``tables``: the one ``bind`` checked (a stage that was never bound: converted, unchecked)"""
        return {k: self._frame_tables[k] if k in self._frame_tables else np.asarray(self.valid_frames[k]).astype(np.int32)
                for k in feature_ids if k in self.valid_frames}

    @staticmethod
    def dataset_constants(name: str, constants: Sequence[str], what: str) -> list:
        """The named constants of a data set's constants module; ``what`` ends the refusal of a data set that lacks one"""
        from .util.dynamic_import import import_dataset_constants
        got = import_dataset_constants(name, list(constants))
        if len(got) != len(constants):
            raise ValueError(f"data set {name!r} has no {what}")
        return got


class Augment(Stage):
    """What ``ClipBatches(augment=...)`` does to every clip it hands out (include/fgcn.h).

    ``max_angle``: the largest rotation about x, y, z in radians (each angle uniform in +-max_angle); ``scale``: the size factor is
    uniform in 1 +- scale; ``min_window``: the shortest temporal window as a fraction of the recording (the window's length is uniform in
    [min_window, 1], its start uniform in what is left), resampled to the clip's T frames by linear interpolation.  The temporal part
    applies to every modality, and all modalities of a sample take the same part of the recording; the spatial part to the joints of
    ``(M, T, V, 3)`` arrays.  ``joints = (lo, hi)`` restricts it to joints ``[lo, hi)`` (the appended sensor joints of a
    skeleton_imu_enhanced array hold sensor axes, not positions); None = all joints of an array with three coordinates.
    ``valid_frames``: feature id -> the number of valid frames of each sample (the window is taken from those; default: all T).
    ``only``: the feature ids to augment (default: all); the others are gathered unchanged.  ``site`` separates two uses of one seed."""

    name, at_upload = "augment", False
    fills = "an Augment that resamples these features to all T frames"

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
        super().__init__(only, valid_frames)

    fills_frames = Stage.applies_to

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
        self.refuse_unknown(set(self.valid_frames) | set(self.only or ()), keys)
        for k in writes:
            if k in self.valid_frames:                  # (cast first: a table of whole-numbered floats is taken, as it always was)
                self.frame_table(k, n, shapes[k][-2] if len(shapes[k]) == 2 else shapes[k][1], np.asarray(self.valid_frames[k]).astype(np.int32))
        return dict(shapes), writes

    def tables(self, writes: Sequence[str], n: int) -> Dict[Optional[str], np.ndarray]:
        """None: the clips' ids, which key the random numbers; feature id: the valid frames of its clips"""
        return {None: np.arange(n, dtype=np.int64), **self.frame_tables(writes)}

    def run(self, batches, feats: Feats, rows: Rows, tables: Tables, out: Dict[str, Optional[torch.Tensor]]) -> Feats:
        """``rows`` per feature where the stage before (a per-batch ``Window``) wrote some features and not others (see ``Stage``)"""
        feats = dict(feats)
        for k, o in out.items():
            src = feats[k]
            feats[k], batches.last_params[k] = ops.clip_augment(
                src, self.rows_of(rows, k), tables[None], seed=batches.seed, epoch=batches.epoch, site=self.site, max_angle=self.max_angle,
                scale=self.scale, min_window=self.min_window, joints=self.joint_range(src.shape[1:]), valid=tables.get(k), out=o)
        return feats


class Sensors(Stage):
    """What ``ClipBatches(sensors=...)`` does to the inertial half of every clip it hands out (include/fgcn.h): the
    standard perturbations of wearable-sensor data, behind ``augment`` (whose resampling would smooth the jitter) and in front of
    ``streams`` (which must see the clip the model sees).

    A sensor is a triple of values: columns ``3g .. 3g+2`` of a ``(T, S)`` signal with ``S % 3 == 0``, and -- with ``joints = (lo, hi)`` --
    joint ``lo + g`` of every body of an ``(M, T, V, 3)`` array (the sensor joints ``Inertial(enhance=True)`` appends; the other joints
    are gathered unchanged).  ``max_angle``: the largest rotation of the sensor frame about x, y, z in radians, ONE rotation per sample,
    independent of ``Augment``'s; ``scale``: the gain of each sensor is uniform in 1 +- scale; ``warp``: a smooth factor 1 + delta(t) over
    the valid frames, the Catmull-Rom curve through ``warp_knots`` values uniform in +-warp per sensor (``warp_knots``: 0, or 2..8);
    ``jitter``: the standard deviation of the additive normal noise, a scalar or one value per sensor, in the STORED units (accelerometer
    and gyroscope units differ by orders of magnitude); ``drop``: the probability that a whole sensor comes out as zeros.  All bodies of
    an array, and the signal and the enhanced skeleton of one sample, receive the same values.

    The values are taken as physical ones, zero meaning no signal: data prepared on the device uses ``Inertial(minmax=False)`` and this
    stage's ``minmax=True``, which applies the reference's min-max normalisation AFTER the augmentation, to the ``(T, S)`` signals only,
    over the whole padded array by ``Inertial``'s float32 formula.  Stored features that were min-max normalised offline have their zero
    somewhere else: the rotation and the drop are not meaningful for them (gain, warp and jitter act on the shifted values).
    ``valid_frames``: feature id -> the number of valid frames of each sample (the frames behind them are copied, so the padding stays
    zero; default: all T).  ``only``: the feature ids to apply to (default: every feature of a shape above; features of other shapes are then left
    alone, except that a ``(T, S)`` feature with ``S % 3 == 0`` and more than 16 triples is refused rather than skipped: it looks like a
    recording the kernel cannot take, and ``only=`` says which features are meant); ``site`` separates two uses of one seed (``Augment``
    and ``Window`` at the same site draw from other counter words)."""

    name, at_upload = "sensors", False

    def __init__(self, max_angle: Sequence[float] = (0.3, 0.3, 0.3), scale: float = 0.1, warp: float = 0.0, warp_knots: int = 4,
                 jitter: Union[float, Sequence[float]] = 0.0, drop: float = 0.0, joints: Optional[Tuple[int, int]] = None,
                 minmax: bool = False, valid_frames: Optional[Mapping[str, Sequence[int]]] = None, site: int = 0,
                 only: Optional[Iterable[str]] = None):
        self.max_angle = tuple(float(a) for a in max_angle)
        if len(self.max_angle) != 3 or not all(np.isfinite(self.max_angle)):
            raise ValueError(f"max_angle: three finite angles (x, y, z), got {max_angle!r}")
        for what, value in (("scale", scale), ("warp", warp), ("drop", drop)):
            if not 0.0 <= value < 1.0:
                raise ValueError(f"{what}={value} outside [0, 1)")
        whole = not isinstance(warp_knots, bool) and isinstance(warp_knots, (int, np.integer))
        if not whole or not (warp_knots == 0 or 2 <= warp_knots <= SENSORS_MAX_KNOTS):
            raise ValueError(f"warp_knots={warp_knots!r}: expected 0 or a number of knots in [2, {SENSORS_MAX_KNOTS}]")
        self.jitter = float(jitter) if np.ndim(jitter) == 0 else tuple(float(j) for j in jitter)
        if not all(np.isfinite(j) and j >= 0.0 for j in np.atleast_1d(self.jitter)):
            raise ValueError(f"jitter={jitter!r}: expected finite values >= 0")
        if joints is not None and not 0 <= joints[0] < joints[1]:
            raise ValueError(f"joints={joints!r}: expected (lo, hi) with 0 <= lo < hi")
        self.scale, self.warp, self.warp_knots, self.drop = float(scale), float(warp), int(warp_knots), float(drop)
        self.joints = None if joints is None else (int(joints[0]), int(joints[1]))
        self.minmax, self.site = bool(minmax), int(site)
        super().__init__(only, valid_frames)

    def sensor_range(self, sample_shape: Sequence[int]) -> Optional[Tuple[int, int]]:
        """The units of three values of a sample of this shape that are sensors; None: the stage does not apply to the shape."""
        if len(sample_shape) == 2 and sample_shape[1] % 3 == 0 and sample_shape[1] > 0:
            return 0, sample_shape[1] // 3
        if len(sample_shape) == 4 and sample_shape[3] == 3 and self.joints is not None:
            return self.joints
        return None

    def bind(self, shapes: Shapes, n: int, keys: Sequence[str]) -> Tuple[Shapes, List[str]]:
        self.refuse_unknown(set(self.valid_frames) | set(self.only or ()), keys, shapes)
        writes = []
        for k in shapes:
            if not self.applies_to(k):
                continue
            span = self.sensor_range(shapes[k])
            if span is None:
                if self.only is None:
                    continue
                raise FgcnError(f"sensors: feature {k!r} has shape {(n, *shapes[k])}; expected (samples, T, S) with S % 3 == 0 or, with "
                                f"joints=(lo, hi), (samples, M, T, V, 3) -- leave it out with Sensors(only=...)")
            lo, hi = span
            if len(shapes[k]) == 4 and hi > shapes[k][2]:
                raise ValueError(f"joints={self.joints!r} for an array of {shapes[k][2]} joints (feature {k!r})")
            if hi - lo > SENSORS_MAX:
                raise FgcnError(f"sensors: feature {k!r} holds {hi - lo} sensors, at most {SENSORS_MAX} -- leave it out with Sensors(only=...)")
            if np.ndim(self.jitter) and len(self.jitter) != hi - lo:
                raise ValueError(f"jitter holds {len(self.jitter)} values, feature {k!r} has {hi - lo} sensors")
            writes.append(k)
        stale = sorted(set(self.valid_frames) - set(writes))
        if stale:
            raise ValueError(f"sensors: valid_frames{stale} for features the stage does not apply to")
        for k in writes:
            if k in self.valid_frames:
                self.frame_table(k, n, shapes[k][0] if len(shapes[k]) == 2 else shapes[k][1])
        return dict(shapes), writes

    def tables(self, writes: Sequence[str], n: int) -> Dict[Optional[str], np.ndarray]:
        """None: the clips' ids, which key the random numbers; feature id: the valid frames of its clips"""
        return {None: np.arange(n, dtype=np.int64), **self.frame_tables(writes)}

    def run(self, batches, feats: Feats, rows: Rows, tables: Tables, out: Dict[str, Optional[torch.Tensor]]) -> Feats:
        """``rows`` per feature where the stage before (a per-batch ``Window`` or ``Augment``) wrote some features and not others (see ``Stage``)"""
        feats = dict(feats)
        for k, o in out.items():
            src = feats[k]
            feats[k], params, stats = ops.clip_sensors(
                src, self.rows_of(rows, k), tables[None], seed=batches.seed, epoch=batches.epoch, site=self.site, max_angle=self.max_angle,
                scale=self.scale, warp=self.warp, warp_knots=self.warp_knots, jitter=self.jitter, drop=self.drop,
                joints=self.joints if src.dim() == 5 else None, minmax=self.minmax and src.dim() == 3, valid=tables.get(k), out=o)
            batches.last_sensors[k] = (params, stats)
        return feats


class Bodies(Stage):
    """What ``ClipBatches(bodies=...)`` does to every raw skeleton clip (include/fgcn.h): the reference's
    ``SkeletonSample._filter_bodies`` -- of the ``Mr`` bodies the tracker lists, the ``bodies`` with the highest ``body_score`` (the sum
    over the channels of the standard deviation of the body's non-null frames), in descending order; a NaN score ranks first, equal
    scores by the higher source index.  The (samples, Mr, T, V, C) arrays it applies to come out as (bodies, T, V, C).  ``only``: the
    feature ids to select in (default: all); the others are handed out as stored."""

    name = "bodies"

    def __init__(self, bodies: int = 2, only: Optional[Iterable[str]] = None):
        if isinstance(bodies, bool) or not isinstance(bodies, (int, np.integer)) or not 1 <= bodies <= BODIES_MAX:
            raise ValueError(f"bodies={bodies!r}: expected a number of bodies in [1, {BODIES_MAX}]")
        self.bodies = int(bodies)
        super().__init__(only)

    @classmethod
    def for_dataset(cls, name: str, only: Optional[Iterable[str]] = None) -> "Bodies":
        """The reference's number of bodies for a data set (``max_body_true`` of its constants module: ``"ntu_rgb_d"`` has one)."""
        return cls(*cls.dataset_constants(name, ["max_body_true"], "max_body_true constant"), only=only)

    def bind(self, shapes: Shapes, n: int, keys: Sequence[str]) -> Tuple[Shapes, List[str]]:
        self.refuse_unknown(self.only or (), keys)
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

    def run(self, batches, feats: Feats, rows: torch.Tensor, tables: Tables, out: Dict[str, Optional[torch.Tensor]]) -> Feats:
        feats = dict(feats)
        for k, o in out.items():
            feats[k], order, scores = ops.clip_bodies(feats[k], rows, bodies=self.bodies, out=o)
            batches.last_bodies[k] = (order, scores)
        return feats


class Normalize(Stage):
    """What ``ClipBatches(normalize=...)`` does to every raw skeleton clip (include/fgcn.h): the reference's
    ``normalize_skeleton(skeleton, origin_joint, z_axis_joints, x_axis_joints)``.

    ``origin_joint``: the joint of the first body that is moved to the origin; ``z_axis_joints`` / ``x_axis_joints``: the pair of joints
    whose bone is turned to the z / x axis (None: no such pass; a pair needs three coordinates).  ``only``: the feature ids to normalise
    (default: all); the others are handed out as stored."""

    name = "normalize"

    def __init__(self, origin_joint: int, z_axis_joints: Optional[Sequence[int]] = None, x_axis_joints: Optional[Sequence[int]] = None,
                 only: Optional[Iterable[str]] = None):
        if isinstance(origin_joint, bool) or not isinstance(origin_joint, (int, np.integer)) or origin_joint < 0:
            raise ValueError(f"origin_joint={origin_joint!r}: expected a joint number >= 0")
        self.origin_joint = int(origin_joint)
        self.z_axis_joints, self.x_axis_joints = self._pair(z_axis_joints, "z_axis_joints"), self._pair(x_axis_joints, "x_axis_joints")
        super().__init__(only)

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
        return cls(*cls.dataset_constants(name, ["skeleton_center_joint", "skeleton_z_joints", "skeleton_x_joints"],
                                          "skeleton normalisation constants"), only=only)

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

    def bind(self, shapes: Shapes, n: int, keys: Sequence[str]) -> Tuple[Shapes, List[str]]:
        self.refuse_unknown(self.only or (), keys)
        writes = [k for k in shapes if self.applies_to(k)]
        for k in writes:
            self.check_shape(k, (n, *shapes[k]))
        return dict(shapes), writes

    def run(self, batches, feats: Feats, rows: torch.Tensor, tables: Tables, out: Dict[str, Optional[torch.Tensor]]) -> Feats:
        feats = dict(feats)
        for k, o in out.items():
            feats[k], frame_map, params = ops.clip_normalize(feats[k], rows, origin_joint=self.origin_joint, z_axis_joints=self.z_axis_joints,
                                                             x_axis_joints=self.x_axis_joints, out=o)
            batches.last_plan[k] = (frame_map, params)
        return feats


class Inertial(Stage):
    """What ``ClipBatches(inertial=...)`` does to every raw inertial recording (include/fgcn.h): the reference's
    offline preprocessing of the ``inertial`` and ``skeleton_imu_enhanced`` features.

    ``frames``: feature id -> the number of recorded frames of each sample, for the two features ``main`` (the skeleton, (samples, M, T,
    V, C), whose count Ls is the length the recording is resampled to) and ``signal`` (the recording, (samples, L, S), Li frames of it
    valid).  ``features[signal]`` becomes the (T, S) signal -- resampled by nearest neighbour, zero from frame Ls on, min-max normalised
    over the padded array unless ``minmax=False`` (a constant recording gives 0 / 0 = NaN, as in the reference) -- or is left out of
    the batch with ``drop_signal=True``.  ``enhance=True``: ``features[main]`` becomes (M, T, V + S / 3, 3), the skeleton with the
    resampled, padded recording (not min-max normalised) appended as S / 3 joints of every body."""

    name = "inertial"

    def __init__(self, frames: Mapping[str, Sequence[int]], main: str = "skeleton", signal: str = "inertial", enhance: bool = False,
                 minmax: bool = True, drop_signal: bool = False):
        super().__init__()
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
        self.refuse_unknown({self.main, self.signal}, shapes)
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

    def bind(self, shapes: Shapes, n: int, keys: Sequence[str]) -> Tuple[Shapes, List[str]]:
        full = {k: (n, *v) for k, v in shapes.items()}
        self.check_shapes(full, n)
        after = self.sample_shapes(full)
        return after, [k for k in after if k == self.signal or (k == self.main and self.enhance)]

    def tables(self, writes: Sequence[str], n: int) -> Dict[Optional[str], np.ndarray]:
        return {k: self.frames[k] for k in (self.signal, self.main)}

    def run(self, batches, feats: Feats, rows: torch.Tensor, tables: Tables, out: Dict[str, Optional[torch.Tensor]]) -> Feats:
        """reads the raw recordings and the normalised skeletons in ``feats``"""
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


class Streams(Stage):
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
    name, at_upload = "streams", False

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
        super().__init__(only, valid_frames)
        self._device_parents = {}       # device -> the (V) int32 table, built (and checked by ops) on the first batch there

    @classmethod
    def for_dataset(cls, name: str, extra_joints: int = 0, **kw) -> "Streams":
        """The parents of a data set's skeleton (``"utd_mhad"``, ``"mmact"``, ``"ntu_rgb_d"``): its constants module's ``skeleton_edges``
        are (child, parent) rows and its ``center_joint`` is the root; ``extra_joints`` entries of -1 follow for appended sensor joints."""
        edges, center, V = cls.dataset_constants(name, ["skeleton_edges", "center_joint", "num_joints"], "skeleton graph constants")
        parents = {**{int(child): int(parent) for child, parent in np.asarray(edges).tolist()}, int(center): int(center)}
        missing = sorted(set(range(V)) - set(parents))
        if missing:
            raise ValueError(f"data set {name!r}: joints {missing} of {V} appear in no edge as the child, and are not the centre joint")
        if extra_joints < 0:
            raise ValueError(f"extra_joints={extra_joints}")
        return cls([parents[v] for v in range(V)] + [-1] * int(extra_joints), **kw)

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
        applied = [k for k in shapes if self.applies_to(k, shapes[k])]
        self.refuse_unknown(set(self.valid_frames) | set(self.only or ()), keys, applied, " or that it does not apply to")
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
                self.frame_table(k, n, shape[1])
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
        return self.frame_tables(self.valid_frames)

    def run(self, batches, feats: Feats, rows: Rows, tables: Tables, out: Dict[str, Optional[torch.Tensor]]) -> Feats:
        """``rows`` per feature where the stage before wrote some features and not others (see ``Stage``)"""
        res, batches.last_streams = {}, {}
        for k, src in feats.items():
            if not self.applies_to(k, src.shape[1:]):
                res[k] = src
                continue
            if src.device not in self._device_parents:
                self._device_parents[src.device] = ops.stream_parents(self.parents, src.device)
            ids = self.output_ids(k)
            got = ops.clip_streams(src, self.rows_of(rows, k), self._device_parents[src.device], streams=self.streams, valid=tables.get(k),
                                   out={s: out[i] for s, i in ids.items() if out[i] is not None})
            res.update({i: got[s] for s, i in ids.items()})
            batches.last_streams[k] = list(ids.values())
        return res


class Window(Stage):
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
    fills = "a Window that resizes these features to frames that are all valid"

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
        super().__init__(only, valid_frames)
        if self.only is not None and isinstance(self.frames, dict) and not self.only <= set(self.frames):
            raise ValueError(f"only={sorted(self.only)} names features that frames={self.frames!r} gives no length")

    def applies_to(self, feature_id: str) -> bool:
        return super().applies_to(feature_id) and (not isinstance(self.frames, dict) or feature_id in self.frames)

    fills_frames = applies_to

    def length(self, feature_id: str) -> int:
        return self.frames[feature_id] if isinstance(self.frames, dict) else self.frames

    def bind(self, shapes: Shapes, n: int, keys: Sequence[str]) -> Tuple[Shapes, List[str]]:
        named = set(self.valid_frames) | set(self.only or ()) | set(self.frames if isinstance(self.frames, dict) else ())
        self.refuse_unknown(named, keys, shapes)
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
                self.frame_table(k, n, shape[t_axis])
            after[k] = (*shape[:t_axis], self.length(k), *shape[t_axis + 1:])
        return after, writes

    def tables(self, writes: Sequence[str], n: int) -> Dict[Optional[str], np.ndarray]:
        """None: the clips' ids, which key the random numbers (the centred part has none); feature id: the valid frames of its clips"""
        valid = self.frame_tables(writes)
        return {None: np.arange(n, dtype=np.int64), **valid} if self.train else valid

    def run(self, batches, feats: Feats, rows: Rows, tables: Tables, out: Dict[str, Optional[torch.Tensor]]) -> Feats:
        feats = dict(feats)
        for k, o in out.items():
            feats[k], batches.last_window[k] = ops.clip_window(
                feats[k], self.rows_of(rows, k), tables[None] if self.train else None, window=self.length(k), interval=self.interval,
                mode=self.mode, seed=batches.seed, epoch=batches.epoch, site=self.site, valid=tables.get(k), out=o)
        return feats
