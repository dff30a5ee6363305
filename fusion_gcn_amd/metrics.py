"""The reference's metric classes (torch_src/metrics.py) on ONE device-side state per context.

The reference's ``Mean`` / ``MultiClassAccuracy`` / ``TopKAccuracy`` read a number back from the device on every batch (``.item()``:
metrics.py:85,107,131) -- two to three host waits per step, the only thing left between a ``GraphStep`` replay and a host that runs
ahead of the device.  Here every value the container reports derives from a confusion matrix, a top-k hit count, a loss sum and
the per-sample argmax; ``fgcn_classify_update`` (include/fgcn.h) adds all of them to a device buffer in ONE launch per
``update_training`` / ``update_validation`` call, however many metrics are registered.  The host reads the buffer when it wants a
value:

  * ``metric.value`` waits for the device if the newest update has not been copied yet and applies the reference's formulas
    (float64; ``sys.float_info.epsilon`` in precision / recall, ``1e-15`` in F1 and the confusion normalisations) -- an empty
    metric divides by zero exactly as the reference's does;
  * ``str(metric)`` / ``format_*`` NEVER wait: after an update (at most every ``snapshot_every`` updates) the container enqueues a
    non-blocking copy of the state into one of its pinned host buffers and records an event; formatting uses the newest copy whose
    event has completed and prints zeros before the first one arrives.  A buffer with a copy in flight is neither read nor reused.

Same names, constructor arguments and container behaviour as the reference (training / validation split by "train" / "val" /
"loss" in the metric's name, ``reset_all`` history, ``to_summary`` on a duck-typed writer); figures and TensorBoard itself are not
built: visual metrics keep their ``.value`` and write nothing.  Metrics that are not state-backed -- ``SimpleMetric``, any user
``Metric`` subclass such as the reference's adjacency visualisations -- get the reference's ``update(val, context=, model=,
indices=)`` call.  A state-backed metric has a value only inside a ``MetricsContainer``.
No fallback: an update raises ``FgcnError`` without libfgcn / off gfx950 / for host tensors.
"""
from __future__ import annotations

import abc
import sys
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib, ops

_WORDS = _lib.CLS_WORDS
_COUNTS = _lib.CLS_LOSS_SUM          # the integer words in front of the float64 one


def _zero_arrays(classes: int) -> dict:
    return {"counts": np.zeros(_COUNTS, np.int64), "loss_sum": np.float64(0.0), "confusion": np.zeros((classes, classes), np.int32)}


class _State:
    """One context's accumulators: the device buffer ``fgcn_classify_update`` adds to, the rotating pinned snapshots of it, the
    prediction store of a ``MisclassifiedSamplesList`` and the newest copy the host holds (``arrays``: counts int64[7] indexed by
    ``_lib.CLS_*``, loss_sum float64, confusion int32 (classes, classes))."""

    def __init__(self, snapshot_every: int = 1, buffers: int = 3):
        if snapshot_every < 1 or buffers < 2:
            raise ValueError("snapshot_every >= 1 and at least two snapshot buffers")
        self.snapshot_every, self.buffers = snapshot_every, buffers
        self.k = 1
        self.classes: Optional[int] = None
        self.capacity = 0                   # of the prediction store (0: no MisclassifiedSamplesList)
        self.dev: Optional[torch.Tensor] = None
        self.pred: Optional[torch.Tensor] = None
        self.stream = None
        self.seq = 0                        # bumped by every update / reset / load
        self.host_seq = 0                   # the seq `arrays` shows
        self.snap_seq = 0                   # the seq of the newest enqueued copy
        self.arrays: Optional[dict] = None
        self.slots: list = []               # [pinned int64 tensor, event or None, seq]
        self.offset = 0                     # rows handed to the prediction store so far
        self.kept: list = []                # (indices, labels) of every update, as handed over
        self.base = None                    # (indices, pred, labels) int64 arrays installed by load()

    # ---- layout -----------------------------------------------------------------------------------------------------------------
    def _set_classes(self, classes: int) -> None:
        if self.classes is None:
            if not 1 <= classes <= _lib.CLS_MAX_CLASSES:
                raise _lib.FgcnError(f"metrics: {classes} classes (1..{_lib.CLS_MAX_CLASSES})")
            self.classes = classes
            if self.arrays is None:
                self.arrays = _zero_arrays(classes)
        elif self.classes != classes:
            raise ValueError(f"metrics: {classes} classes, the state holds {self.classes}")

    def _words(self) -> int:
        return _WORDS + (self.classes * self.classes + 1) // 2          # fgcn_classify_state_bytes / 8

    def _parse(self, raw: np.ndarray) -> dict:
        c = self.classes
        return {"counts": raw[:_COUNTS].copy(), "loss_sum": np.float64(raw[_COUNTS:_WORDS].view(np.float64)[0]),
                "confusion": raw[_WORDS:].view(np.int32)[:c * c].reshape(c, c).copy()}

    def _raw(self, arrays: dict) -> np.ndarray:
        raw = np.zeros(self._words(), np.int64)
        raw[:_COUNTS] = arrays["counts"]
        raw[_COUNTS:_WORDS].view(np.float64)[0] = arrays["loss_sum"]
        raw[_WORDS:].view(np.int32)[:self.classes ** 2] = np.asarray(arrays["confusion"], np.int32).reshape(-1)
        return raw

    # ---- device side ------------------------------------------------------------------------------------------------------------
    def update(self, loss, logits: torch.Tensor, labels: torch.Tensor, indices=None) -> None:
        ops.ensure_device()
        if not (torch.is_tensor(logits) and logits.is_cuda and torch.is_tensor(labels) and labels.is_cuda):
            raise _lib.FgcnError("metrics: logits and labels must be on the HIP device (there is no host path)")
        self._set_classes(logits.shape[1])
        dev = logits.device
        if self.dev is None:
            if any(np.any(v) for v in self.arrays.values()):               # a loaded state continues on the device
                self.dev = torch.from_numpy(self._raw(self.arrays)).to(dev)
            else:
                self.dev = torch.zeros(self._words(), dtype=torch.int64, device=dev)
            assert self.dev.numel() * 8 == ops.classify_state_bytes(self.classes)
            self.slots = [[torch.empty(self._words(), dtype=torch.int64, pin_memory=True), None, 0] for _ in range(self.buffers)]
            if self.capacity:
                self.pred = torch.full((self.capacity,), -1, dtype=torch.int32, device=dev)
        if loss is not None:
            if not torch.is_tensor(loss):
                loss = torch.tensor(float(loss), dtype=torch.float32).to(dev, non_blocking=True)
            loss = loss.detach()
            if loss.dtype != torch.float32 or loss.device != dev:
                loss = loss.to(device=dev, dtype=torch.float32)
        ops.classify_update(logits.detach(), labels, self.dev, k=self.k, loss=loss, pred_out=self.pred, pred_offset=self.offset)
        self.stream = torch.cuda.current_stream(dev)
        self.seq += 1
        if self.pred is not None:
            self.offset += labels.shape[0]
            # copies: a loader may reuse the buffers it hands out (data.ClipBatches rotates its device batches)
            self.kept.append((indices.clone() if torch.is_tensor(indices) else indices, labels.clone()))
        if self.seq - self.snap_seq >= self.snapshot_every:
            self._enqueue_snapshot()

    def _enqueue_snapshot(self) -> None:
        self.poll()                                   # harvest what has arrived: a completed slot is free afterwards
        for slot in self.slots:
            if slot[1] is None or slot[1].query():
                slot[0].copy_(self.dev, non_blocking=True)
                slot[1] = torch.cuda.Event()
                slot[1].record(self.stream)
                slot[2] = self.snap_seq = self.seq
                return
        # every buffer has a copy in flight: this update is covered by a later snapshot

    def poll(self) -> Optional[dict]:
        """The newest arrays that have ARRIVED (never waits)."""
        best = None
        for slot in self.slots:
            if slot[1] is not None and slot[2] > self.host_seq and slot[1].query() and (best is None or slot[2] > best[2]):
                best = slot
        if best is not None:
            self.arrays, self.host_seq = self._parse(best[0].numpy()), best[2]
        return self.arrays

    def sync(self) -> Optional[dict]:
        """The arrays after the newest update (waits for the device when they have not been copied yet)."""
        if self.host_seq < self.seq:
            self.poll()
        if self.host_seq < self.seq:
            torch.cuda.current_stream(self.dev.device).wait_stream(self.stream)
            self.arrays, self.host_seq = self._parse(self.dev.cpu().numpy()), self.seq
        return self.arrays

    def reset(self) -> None:
        if self.dev is not None:
            self.dev.zero_()
        self.seq += 1
        self.host_seq = self.seq
        self.arrays = None if self.classes is None else _zero_arrays(self.classes)
        self.offset, self.kept, self.base = 0, [], None

    def load(self, arrays: dict) -> None:
        confusion = np.asarray(arrays["confusion"])
        if confusion.ndim != 2 or confusion.shape[0] != confusion.shape[1]:
            raise ValueError("load_state: confusion must be (classes, classes)")
        self._set_classes(confusion.shape[0])
        counts = np.asarray(arrays["counts"], np.int64)
        if counts.shape != (_COUNTS,):
            raise ValueError(f"load_state: counts must hold {_COUNTS} integers")
        self.arrays = {"counts": counts.copy(), "loss_sum": np.float64(arrays["loss_sum"]), "confusion": confusion.astype(np.int32)}
        self.seq += 1
        self.host_seq = self.seq
        if self.dev is not None:
            self.dev.copy_(torch.from_numpy(self._raw(self.arrays)))
        self.offset, self.kept, self.base = 0, [], None
        if arrays.get("pred") is not None:
            self.base = tuple(np.asarray(arrays[key], np.int64).reshape(-1) for key in ("indices", "pred", "labels"))

    def samples(self):
        """(indices, predictions, labels) of every stored row, int64 arrays (waits for the device)."""
        parts = [self.base] if self.base is not None else []
        if self.pred is not None and self.offset:
            stored = min(self.offset, self.capacity)
            torch.cuda.current_stream(self.pred.device).wait_stream(self.stream)
            pred = self.pred[:stored].cpu().numpy().astype(np.int64)
            as_array = lambda seq: np.concatenate([np.asarray(t.cpu() if torch.is_tensor(t) else t, np.int64).reshape(-1)   # noqa: E731
                                                   for t in seq])[:stored]
            if any(i is None for i, _ in self.kept):
                raise ValueError("MisclassifiedSamplesList: an update came without sample indices")
            parts.append((as_array([i for i, _ in self.kept]), pred, as_array([y for _, y in self.kept])))
        if not parts:
            return tuple(np.zeros(0, np.int64) for _ in range(3))
        return tuple(np.concatenate([p[j] for p in parts]) for j in range(3))


# ---- the metric classes ---------------------------------------------------------------------------------------------------------
class Metric(abc.ABC):
    def __init__(self, name: str):
        self.name = name
        self.write_to_summary_interval = 1

    @abc.abstractmethod
    def update(self, val=None, **kwargs):
        ...

    @property
    @abc.abstractmethod
    def value(self):
        ...

    @abc.abstractmethod
    def reset(self):
        ...

    def to_summary(self, summary, epoch: int):
        if self.write_to_summary_interval > 0 and epoch % self.write_to_summary_interval == 0:
            self._to_summary(summary, epoch)

    @abc.abstractmethod
    def _to_summary(self, summary, epoch: int):
        ...

    def __str__(self):
        return f"{self.name}: {self.value:.4f}"


class ScalarMetric(Metric, abc.ABC):
    def __init__(self, name: str):
        super().__init__(name)
        self.show_in_progress_log = True

    def _to_summary(self, summary, epoch: int):
        summary.add_scalar(self.name, self.value, epoch)


class SimpleMetric(ScalarMetric):
    """A value the caller sets (the learning rate)."""

    def __init__(self, name: str):
        super().__init__(name)
        self.val = 0.

    def update(self, val=None, **kwargs):
        self.val = val

    @property
    def value(self) -> float:
        return self.val

    def reset(self):
        self.val = 0.


class _StateBacked:
    """Mixin of the metrics whose value derives from a ``_State``: the shared one of their context in the ``MetricsContainer`` they
    are registered in, which alone updates and resets it (one launch per batch for all of them)."""
    _contexts = ("train", "val")

    def _init_state(self):
        self._states: Optional[Dict[str, _State]] = None         # the container's
        self._context: Optional[str] = None

    def _configure(self, state: _State) -> None:
        """What this metric needs from the state it is bound to (k, classes, prediction store)."""

    def _bind(self, states: Dict[str, _State], context: str) -> None:
        self._states, self._context = states, context
        self._configure(states[context])

    def _state(self) -> _State:
        if self._states is None:
            raise RuntimeError(f"{self.name} derives its value from its container's device state: register it in a MetricsContainer")
        return self._states[self._context]

    def _derive(self, arrays: Optional[dict], lenient: bool):
        raise NotImplementedError

    def update(self, val=None, **kwargs):
        raise RuntimeError(f"{self.name} shares its container's state: update it through MetricsContainer.update_*")

    @property
    def value(self):
        return self._derive(self._state().sync(), False)

    def reset(self):
        raise RuntimeError(f"{self.name} shares its container's state: reset it through MetricsContainer.reset_all")

    def __str__(self):
        return f"{self.name}: {self._derive(self._state().poll(), True):.4f}"


def _ratio(num, den, lenient: bool) -> float:
    """The reference's ``float / int`` (ZeroDivisionError for an empty metric); 0 for an empty metric in a progress line."""
    if lenient and not den:
        return 0.0
    return float(num) / int(den)


def _count(arrays: Optional[dict], word: int) -> int:
    return 0 if arrays is None else int(arrays["counts"][word])


def _confusion(arrays: Optional[dict], classes: int = 1) -> np.ndarray:
    return np.zeros((classes, classes), np.int32) if arrays is None else arrays["confusion"]


class Mean(_StateBacked, ScalarMetric):
    """Sample-weighted mean of the step's loss: ``sum(loss * rows) / sum(rows)`` over the container's updates (under gradient
    accumulation the loss arrives divided by the quotient, as in the reference)."""

    def __init__(self, name: str = "mean"):
        super().__init__(name)
        self._init_state()

    def _derive(self, arrays, lenient):
        return _ratio(0.0 if arrays is None else arrays["loss_sum"], _count(arrays, _lib.CLS_LOSS_ITEMS), lenient)


class MultiClassAccuracy(_StateBacked, ScalarMetric):
    def __init__(self, name: str = "accuracy"):
        super().__init__(name)
        self._init_state()

    def _derive(self, arrays, lenient):
        return _ratio(_count(arrays, _lib.CLS_TOP1), _count(arrays, _lib.CLS_EXAMPLES), lenient)


class TopKAccuracy(_StateBacked, ScalarMetric):
    """A row is a hit when fewer than k logits rank above its label's (ties towards the lower class index: include/fgcn.h)."""

    def __init__(self, name: str = "top-k-accuracy", k: int = 5):
        super().__init__(name)
        self._init_state()
        self._k = k

    def _configure(self, state):
        state.k = self._k

    def _derive(self, arrays, lenient):
        return _ratio(_count(arrays, _lib.CLS_TOPK), _count(arrays, _lib.CLS_EXAMPLES), lenient)


class PrecisionRecallBase(_StateBacked, ScalarMetric, abc.ABC):
    def __init__(self, name: str):
        super().__init__(name)
        self._init_state()

    @staticmethod
    def _per_class(confusion: np.ndarray, axis: int) -> np.ndarray:
        """true positives / (positives + eps) per class, float64; axis 0: predicted as the class, axis 1: labelled as it"""
        return np.diagonal(confusion).astype(np.float64) / (confusion.sum(axis=axis).astype(np.float64) + sys.float_info.epsilon)

    @abc.abstractmethod
    def _tensor(self, confusion: np.ndarray) -> np.ndarray:
        ...

    def get_tensor(self) -> torch.Tensor:
        return torch.from_numpy(self._tensor(_confusion(self._state().sync())))

    def _derive(self, arrays, lenient):
        return float(self._tensor(_confusion(arrays)).mean())


class Precision(PrecisionRecallBase):
    def __init__(self, name: str = "precision"):
        super().__init__(name)

    def _tensor(self, confusion):
        return self._per_class(confusion, 0)


class Recall(PrecisionRecallBase):
    def __init__(self, name: str = "recall"):
        super().__init__(name)

    def _tensor(self, confusion):
        return self._per_class(confusion, 1)


class F1MeasureMetric(_StateBacked, ScalarMetric):
    def __init__(self, name: str = "f-measure"):
        super().__init__(name)
        self._init_state()

    def _derive(self, arrays, lenient):
        confusion = _confusion(arrays)
        p, r = PrecisionRecallBase._per_class(confusion, 0), PrecisionRecallBase._per_class(confusion, 1)
        return float(((p * r * 2) / (p + r + 1e-15)).mean())


class VisualMetric(Metric):
    """A metric the reference draws as a figure.  Figures are not built here: ``.value`` is the data, ``to_summary`` writes nothing."""

    def _to_summary(self, summary, epoch: int):
        pass

    def __str__(self):
        return f"{self.name}: {self.value}"


class ConfusionMatrix(_StateBacked, VisualMetric):
    """``.value``: the int32 (label, prediction) count matrix, or, float64, that matrix over the number of samples ("samples"),
    over its row sums ("recall") or over its column sums ("precision"), as a CPU tensor."""

    def __init__(self, num_classes: int, name: str = "confusion-matrix", mode: Optional[str] = None,
                 class_labels: Optional[Sequence[str]] = None):
        super().__init__(name)
        self._init_state()
        assert class_labels is None or len(class_labels) == num_classes
        self.num_classes = num_classes
        self.mode = mode
        self.class_labels = class_labels

    def _configure(self, state):
        state._set_classes(self.num_classes)

    def _derive(self, arrays, lenient):
        confusion = _confusion(arrays, self.num_classes)
        with np.errstate(divide="ignore", invalid="ignore"):
            if self.mode == "samples":
                return torch.from_numpy(confusion.astype(np.float64) / np.float64(_count(arrays, _lib.CLS_EXAMPLES)))
            if self.mode == "recall":
                return torch.from_numpy(confusion.astype(np.float64) / (confusion.sum(axis=1, dtype=np.int64)[:, None] + 1e-15))
            if self.mode == "precision":
                return torch.from_numpy(confusion.astype(np.float64) / (confusion.sum(axis=0, dtype=np.int64) + 1e-15))
        return torch.from_numpy(confusion.copy())

    @property
    def confusion_matrix(self) -> torch.Tensor:
        return torch.from_numpy(_confusion(self._state().sync(), self.num_classes).copy())

    def __str__(self):
        return f"{self.name}: {self._derive(self._state().poll(), True)}"


class AccuracyBarChart(_StateBacked, VisualMetric):
    """``.value``: {"train": per-class accuracy, "val": ...} (diagonal over row sums, float64, NaN for a class without samples).
    Its name should hold both "train" and "val": the container then feeds it from both of its states."""

    def __init__(self, num_classes: int, name: str = "bar-chart", class_labels: Optional[Sequence[str]] = None):
        super().__init__(name)
        self._init_state()
        assert class_labels is None or len(class_labels) == num_classes
        self.num_classes = num_classes
        self.class_labels = class_labels

    def _configure(self, state):
        state._set_classes(self.num_classes)

    def _bind(self, states, context):
        self._states, self._context = states, context
        for c in self._contexts:
            self._configure(states[c])

    def _bars(self, wait: bool):
        self._state()                       # raises for a chart outside a container
        out = {}
        for c, s in self._states.items():
            confusion = _confusion(s.sync() if wait else s.poll(), self.num_classes)
            with np.errstate(divide="ignore", invalid="ignore"):
                out[c] = torch.from_numpy(np.diagonal(confusion).astype(np.float64) / confusion.sum(axis=1, dtype=np.int64))
        return out

    @property
    def value(self):
        return self._bars(True)

    def __str__(self):
        return f"{self.name}: {self._bars(False)}"


class MisclassifiedSamplesList(_StateBacked, Metric):
    """``.value``: the sorted list of ``(sample index, prediction, ground truth)`` of every misclassified sample, as ints.  The
    per-row argmax is stored on the device (``capacity`` rows per epoch; rows past it are counted in the state's DROPPED word,
    ``.dropped``, and left out); the sample indices and labels handed to the updates are kept as they came and joined at ``.value``
    time.  Rows whose label is ignored or invalid are left out."""

    def __init__(self, name: str = "SampleList", sample_labels: Optional[Sequence[str]] = None,
                 class_labels: Optional[Sequence[str]] = None, capacity: int = 1 << 16):
        super().__init__(name)
        self._init_state()
        if capacity < 1:
            raise ValueError("MisclassifiedSamplesList: capacity >= 1")
        self.sample_labels = sample_labels
        self.class_labels = class_labels
        self.capacity = capacity

    def _configure(self, state):
        if state.dev is not None and state.capacity != self.capacity:
            raise RuntimeError("MisclassifiedSamplesList: the state is already in use")
        state.capacity = max(state.capacity, self.capacity)

    @property
    def dropped(self) -> int:
        return _count(self._state().sync(), _lib.CLS_DROPPED)

    @property
    def value(self) -> List[tuple]:
        indices, pred, labels = self._state().samples()
        wrong = (pred != labels) & (pred >= 0)
        return sorted(zip(indices[wrong].tolist(), pred[wrong].tolist(), labels[wrong].tolist()), key=lambda x: x[0])

    def _to_summary(self, summary, epoch: int):
        def sample(i):
            if self.sample_labels is None:
                return str(i)
            return f"Index: {i}<br />" + "<br />".join(map(str, self.sample_labels[i]))

        def klass(c):
            return str(c) if self.class_labels is None else f"{self.class_labels[c]} ({c})"

        rows = "  \n".join(f"| {sample(i)} | {klass(p)} | {klass(y)} |" for i, p, y in self.value)
        summary.add_text(self.name, "| Sample | Prediction | Ground Truth |  \n| --- | --- | --- |  \n" + rows, epoch)

    def __str__(self):
        return f"{self.name}: {self._state().offset} samples seen"


class StreamScores(Metric):
    """The class scores of every sample of a split, kept on the device by sample index: what one trained stream model contributes to a
    score-fusion ensemble (``ensemble.ScoreStore``).  Not state-backed: hand it to ``build_metrics`` as one of the
    ``additional_metrics`` under a name that holds "val", run one validation pass per stream model, ``save`` each.

    ``update((y_pred, y_true), indices=...)`` writes the batch's rows and labels at ``indices`` (``index_copy_``: it does not wait; indices
    on the host are range-checked, indices on the device are trusted to be sample numbers below ``num_samples``); ``value`` is the host
    ``(scores float32 (N, classes), labels int64 (N,), filled bool (N,))``; ``to_summary`` writes nothing."""

    def __init__(self, name: str, num_samples: int, num_classes: int):
        super().__init__(name)
        if num_samples < 1 or not 1 <= num_classes <= _lib.CLS_MAX_CLASSES:
            raise ValueError(f"StreamScores: num_samples={num_samples} (>= 1), num_classes={num_classes} (1..{_lib.CLS_MAX_CLASSES})")
        self.num_samples, self.num_classes = int(num_samples), int(num_classes)
        self._store = None                  # (scores, labels, filled) on the device, from the first update on

    def update(self, val=None, indices=None, **kwargs):
        y_pred, y_true = val
        if not (torch.is_tensor(y_pred) and y_pred.is_cuda and torch.is_tensor(y_true) and y_true.is_cuda):
            raise _lib.FgcnError("StreamScores: scores and labels must be on the HIP device (there is no host path)")
        if indices is None:
            raise ValueError("StreamScores: an update came without sample indices")
        if y_pred.dim() != 2 or y_pred.shape[1] != self.num_classes or y_true.shape != y_pred.shape[:1]:
            raise ValueError(f"StreamScores: scores {tuple(y_pred.shape)} and labels {tuple(y_true.shape)}, expected (rows, {self.num_classes}) and (rows,)")
        if not (torch.is_tensor(indices) and indices.is_cuda):
            host = torch.as_tensor(indices, dtype=torch.int64).reshape(-1)
            if host.numel() and not (0 <= int(host.min()) and int(host.max()) < self.num_samples):
                raise ValueError(f"StreamScores: sample indices outside [0, {self.num_samples})")
            indices = host.to(y_pred.device, non_blocking=True)
        indices = indices.reshape(-1).to(torch.int64)
        if indices.numel() != y_pred.shape[0]:
            raise ValueError(f"StreamScores: {indices.numel()} indices for {y_pred.shape[0]} rows")
        if self._store is None:
            self._store = ops.score_store(self.num_samples, self.num_classes, y_pred.device)
        elif self._store[0].device != y_pred.device:            # arrays installed by _load_arrays continue on the device
            self._store = tuple(ops.device_copy(t, y_pred.device) for t in self._store)
        scores, labels, filled = self._store
        scores.index_copy_(0, indices, y_pred.detach().to(torch.float32))
        labels.index_copy_(0, indices, y_true.to(torch.int64))
        filled.index_fill_(0, indices, 1)

    @property
    def device_value(self):
        """(scores, labels, filled uint8) on the device, or None before the first update"""
        return self._store

    @property
    def value(self):
        if self._store is None:
            return (np.zeros((self.num_samples, self.num_classes), np.float32), np.full(self.num_samples, -1, np.int64),
                    np.zeros(self.num_samples, bool))
        scores, labels, filled = (t.cpu().numpy() for t in self._store)
        return scores, labels, filled.astype(bool)

    def reset(self):
        if self._store is not None:
            self._store[0].zero_()
            self._store[1].fill_(-1)
            self._store[2].zero_()

    def _to_summary(self, summary, epoch: int):
        pass

    def _load_arrays(self, scores, labels, filled) -> None:
        """Not part of the interface: installs host arrays shaped like ``value`` as the store, so that ``value`` / ``save`` / ``reset`` and
        ``ScoreStore.from_metrics`` can be exercised where no device is (the next update would move them to its device)."""
        scores, labels, filled = np.asarray(scores, np.float32), np.asarray(labels, np.int64), np.asarray(filled).astype(np.uint8)
        if scores.shape != (self.num_samples, self.num_classes) or labels.shape != (self.num_samples,) or filled.shape != (self.num_samples,):
            raise ValueError(f"StreamScores._load_arrays: expected scores {(self.num_samples, self.num_classes)}, labels and filled "
                             f"{(self.num_samples,)}; got {scores.shape}, {labels.shape}, {filled.shape}")
        self._store = tuple(torch.from_numpy(np.ascontiguousarray(a).copy()) for a in (scores, labels, filled))

    def save(self, path: str) -> None:
        """``.npz`` with ``scores`` float32 (N, classes), ``labels`` int64 (N,) and ``filled`` bool (N,) (waits for the device)"""
        scores, labels, filled = self.value
        np.savez(path, scores=scores, labels=labels, filled=filled)

    def __str__(self):
        return f"{self.name}: scores of {self.num_samples} samples"


# ---- the container --------------------------------------------------------------------------------------------------------------
class MetricsContainer:
    """Stores, updates and formats the metrics of a session.  A metric is a training metric when its name holds "train", a validation
    metric when it holds "val", and the context's loss when it also holds "loss" (the reference's rule).  State-backed metrics of a
    context share ONE device state and ``update_training`` / ``update_validation`` are ONE kernel launch each; every other metric
    receives ``update((y_pred, y_true), context=, model=, indices=)``.

    ``snapshot_every``: enqueue the non-blocking host copy that ``format_*`` reads at most every that many updates; ``buffers``:
    pinned host buffers the copies rotate through (>= 2: one can be in flight while another is read)."""

    def __init__(self, metrics: list, snapshot_every: int = 1, buffers: int = 3):
        self._metrics = metrics
        self.training_loss = next((m for m in metrics if "train" in m.name and "loss" in m.name), None)
        self.validation_loss = next((m for m in metrics if "val" in m.name and "loss" in m.name), None)
        self._training_metrics = [m for m in metrics if "train" in m.name and "loss" not in m.name]
        self._validation_metrics = [m for m in metrics if "val" in m.name and "loss" not in m.name]
        self._training_format_metrics = self._log_metrics(self.training_loss, *self._training_metrics)
        self._validation_format_metrics = self._log_metrics(self.validation_loss, *self._validation_metrics)
        self._progress_metrics = self._log_metrics(*self._metrics)
        self._metrics_dict = {m.name: m for m in self._metrics}
        self._history: Dict[str, list] = {}
        self._states = {"train": _State(snapshot_every, buffers), "val": _State(snapshot_every, buffers)}
        for context, members in (("train", [self.training_loss] + self._training_metrics),
                                 ("val", [self.validation_loss] + self._validation_metrics)):
            ks = {m._k for m in members if isinstance(m, TopKAccuracy)}
            if len(ks) > 1:
                raise ValueError(f"one k per context (one launch per update): {sorted(ks)} among the {context} metrics")
            for m in members:
                if not isinstance(m, _StateBacked):
                    continue
                if m._states is self._states and not isinstance(m, AccuracyBarChart):
                    raise ValueError(f"{m.name!r} names both contexts: a state-backed metric belongs to one")
                m._bind(self._states, context)
        for m in metrics:
            if isinstance(m, _StateBacked) and m._states is not self._states:
                raise ValueError(f"{m.name!r} names no context: a state-backed metric needs 'train' or 'val' in its name")

    @staticmethod
    def _log_metrics(*metrics) -> list:
        return [m for m in metrics if isinstance(m, ScalarMetric) and m.show_in_progress_log]

    def __getitem__(self, item):
        return self._metrics_dict[item]

    def get_value_history(self) -> Dict[str, list]:
        """The value of every metric at every ``reset_all(save_history=True)`` (one entry per epoch)."""
        return self._history

    def get_metrics(self) -> List[Metric]:
        return self._metrics

    def to_summary(self, summary, epoch: int):
        for metric in self._metrics:
            metric.to_summary(summary, epoch)

    def _save_metrics(self):
        for name, metric in self._metrics_dict.items():
            self._history.setdefault(name, []).append(metric.value)
        lengths = {len(v) for v in self._history.values()}
        assert len(lengths) <= 1, "Inconsistency in history length when creating metric history"

    def reset_all(self, save_history: bool = True):
        if save_history:
            self._save_metrics()
        for m in self._metrics:
            if not isinstance(m, _StateBacked):
                m.reset()
        for state in self._states.values():
            state.reset()

    # ---- updates: one launch per call ---------------------------------------------------------------------------------------------
    def _update(self, context, loss_metric, members, loss, output, model, indices):
        y_pred, y_true = output
        own_loss = isinstance(loss_metric, _StateBacked)
        if own_loss or any(isinstance(m, _StateBacked) for m in members):
            self._states[context].update(loss if own_loss else None, y_pred, y_true, indices)
        if loss_metric is not None and not own_loss:
            loss_metric.update(loss, num_items=len(y_true))
        for m in members:
            if not isinstance(m, _StateBacked):
                m.update(output, context=context, model=model, indices=indices)

    def update_training(self, loss, output, model=None, indices=None):
        """``loss``: the step's loss (one float32 on the device); ``output`` = (y_pred, y_true)."""
        self._update("train", self.training_loss, self._training_metrics, loss, output, model, indices)

    def update_validation(self, loss, output, model=None, indices=None):
        self._update("val", self.validation_loss, self._validation_metrics, loss, output, model, indices)

    # ---- formatting: never waits ----------------------------------------------------------------------------------------------------
    def format_training(self) -> str:
        return self.format(self._training_format_metrics)

    def format_validation(self) -> str:
        return self.format(self._validation_format_metrics)

    def format_all(self) -> str:
        return self.format(self._progress_metrics)

    @staticmethod
    def format(metrics: Sequence[Metric]) -> str:
        return ", ".join(map(str, metrics))

    # ---- snapshots ------------------------------------------------------------------------------------------------------------------
    def state_snapshot(self, context: str) -> Optional[dict]:
        """The context's state after its newest update, as host arrays (waits for the device): ``counts`` int64[7] indexed by
        ``_lib.CLS_EXAMPLES .. CLS_LOSS_ITEMS``, ``loss_sum`` float64, ``confusion`` int32 (classes, classes) and, with a
        ``MisclassifiedSamplesList``, ``indices`` / ``pred`` / ``labels`` of the stored rows.  None before the class count is known."""
        state = self._states[context]
        arrays = state.sync()
        if arrays is None:
            return None
        out = {"counts": arrays["counts"].copy(), "loss_sum": np.float64(arrays["loss_sum"]), "confusion": arrays["confusion"].copy()}
        if state.capacity:
            out["indices"], out["pred"], out["labels"] = state.samples()
        return out

    def load_state(self, context: str, arrays: dict) -> None:
        """Installs ``state_snapshot``-shaped arrays as the context's state (on the device too once it exists)."""
        self._states[context].load(arrays)

    def all_reduce(self, group=None) -> None:
        """Sums every rank's state, integers as integers and the loss sum as float64, and installs the sum on every rank: call it
        once at the epoch's end, before reading values, so that a data-parallel run reports the whole batch and not one rank's
        shard.  The misclassified-sample lists stay per rank.  A no-op without a process group of more than one rank."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1):
            return
        for context, state in self._states.items():
            arrays = state.sync()
            if arrays is None:
                raise RuntimeError(f"all_reduce: the {context} state has no class count yet (register a ConfusionMatrix or update first)")
            ints = torch.from_numpy(np.concatenate([arrays["counts"], arrays["confusion"].astype(np.int64).reshape(-1)]))
            loss_sum = torch.tensor([float(arrays["loss_sum"])], dtype=torch.float64)
            if dist.get_backend(group) == "nccl":
                ints, loss_sum = ints.to(state.dev.device), loss_sum.to(state.dev.device)
            dist.all_reduce(ints, group=group)
            dist.all_reduce(loss_sum, group=group)
            ints = ints.cpu().numpy()
            merged = {"counts": ints[:_COUNTS], "loss_sum": float(loss_sum.cpu()[0]),
                      "confusion": ints[_COUNTS:].reshape(state.classes, state.classes)}
            if state.capacity:
                merged["indices"], merged["pred"], merged["labels"] = state.samples()
            state.load(merged)


def build_metrics(num_classes: int, class_labels=None, k: int = 5, additional_metrics: Optional[list] = None, is_eval: bool = False,
                  **container_args) -> MetricsContainer:
    """The container the reference's ``Session.build_metrics`` builds (session/session.py:108-158): loss and accuracy per context,
    the two confusion matrices (written every 5th epoch in training), top-k accuracy when k > 1, ``additional_metrics``, and the
    learning rate; an evaluation session (``is_eval``) holds the validation metrics only."""
    metrics: list = []
    if not is_eval:
        metrics.append(Mean("training_loss"))
    metrics.append(Mean("validation_loss"))
    if not is_eval:
        metrics.append(MultiClassAccuracy("training_accuracy"))
    metrics.append(MultiClassAccuracy("validation_accuracy"))
    conf_val = ConfusionMatrix(num_classes, "validation_confusion", class_labels=class_labels)
    conf_train = ConfusionMatrix(num_classes, "training_confusion", class_labels=class_labels)
    conf_val.write_to_summary_interval = conf_train.write_to_summary_interval = 1 if is_eval else 5
    if not is_eval:
        metrics.append(conf_train)
    metrics.append(conf_val)
    if k > 1:
        if not is_eval:
            metrics.append(TopKAccuracy(f"training_top{k}_accuracy", k=k))
        metrics.append(TopKAccuracy(f"validation_top{k}_accuracy", k=k))
    if additional_metrics:
        metrics.extend(additional_metrics)
    if not is_eval:
        metrics.append(SimpleMetric("lr"))
    return MetricsContainer(metrics, **container_args)
