"""Score fusion of separately trained stream models: the last step of the 2s-AGCN family's workflow.

The family trains one model per input stream (joint, bone, motion, bone-motion: ``data.ClipBatches(streams=...)``) and reports the accuracy
of the weighted sum of their class scores.  Two ways to that sum, both on ``fgcn_score_fuse`` / ``fgcn_fuse_sweep`` (include/fgcn.h):

  * ``StreamEnsemble``: the models themselves behind one ``forward`` -- the ``model`` of ``Session.validate_epoch`` with an unchanged
    ``MetricsContainer``;
  * ``ScoreStore``: the scores of one validation pass per model (``metrics.StreamScores``, saved as ``.npz``), fused, evaluated and
    searched for the best stream weights without running a model again: ``search`` ranks every sample under every candidate weight
    vector in one call.

No fallback: fusing raises ``FgcnError`` without libfgcn / off gfx950 / for host tensors.  This module allocates nothing on the device
itself: its buffers come from ``ops``."""
from __future__ import annotations

from typing import Dict, Mapping, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib, ops

MemberInput = Union[str, Mapping[str, str]]


def _check_transform(transform: str) -> str:
    if transform not in _lib.FUSE_TRANSFORMS:
        raise ValueError(f"transform={transform!r}: expected one of {sorted(_lib.FUSE_TRANSFORMS)}")
    return transform


def _weight_list(names: Sequence[str], weights) -> list:
    """one float per member, in the members' order; None: 1 each; a mapping must name exactly the members"""
    if weights is None:
        return [1.0] * len(names)
    if isinstance(weights, Mapping):
        if set(weights) != set(names):
            raise ValueError(f"weights names {sorted(weights)}, the members are {sorted(names)}")
        return [float(weights[n]) for n in names]
    got = [float(w) for w in (weights.tolist() if hasattr(weights, "tolist") else weights)]
    if len(got) != len(names):
        raise ValueError(f"{len(got)} weights for the {len(names)} members {list(names)}")
    return got


def simplex_grid(S: int, steps: int) -> np.ndarray:
    """Every weight vector ``(i_1, .., i_S) / steps`` with non-negative integers that sum to ``steps``, in lexicographic order of the
    integers: float64 (C(steps + S - 1, S - 1), S).  ``simplex_grid(2, 4)``: (0, 1), (.25, .75), (.5, .5), (.75, .25), (1, 0)."""
    if not 1 <= S <= _lib.FUSE_MAX_STREAMS or steps < 1:
        raise ValueError(f"simplex_grid: S={S} (1..{_lib.FUSE_MAX_STREAMS}), steps={steps} (>= 1)")
    rows = []

    def fill(prefix: tuple, left: int) -> None:
        if len(prefix) == S - 1:
            rows.append(prefix + (left,))
            return
        for i in range(left + 1):
            fill(prefix + (i,), left - i)
    fill((), steps)
    return np.asarray(rows, np.float64) / steps


class StreamEnsemble(torch.nn.Module):
    """The stream models behind one ``forward``: ``members`` maps a name to ``(model, input)``; ``input`` is a feature id of the batch --
    the model gets that tensor -- or a dict from the model's own keys to the batch's, for a model that takes a dict.  ``forward(features)``
    runs every member in eval mode under ``torch.no_grad()`` (the blocks take their inference kernels) and returns ``ops.score_fuse`` of
    their outputs, in the members' order, under ``weights`` (a mapping by member name or a sequence; default 1 each).

    Evaluation only: joint fine-tuning through the fused score is not built, and ``forward`` in training mode raises."""

    def __init__(self, members: Mapping[str, Tuple[torch.nn.Module, MemberInput]], weights=None, transform: str = "none"):
        super().__init__()
        if not isinstance(members, Mapping) or not 1 <= len(members) <= _lib.FUSE_MAX_STREAMS:
            raise ValueError(f"members: expected a mapping of 1..{_lib.FUSE_MAX_STREAMS} names to (model, input)")
        self.names = tuple(members)
        models, self.inputs = [], []
        for name, member in members.items():
            if not (isinstance(member, (tuple, list)) and len(member) == 2 and isinstance(member[0], torch.nn.Module)):
                raise ValueError(f"members[{name!r}]: expected (model, input)")
            model, inp = member
            if isinstance(inp, Mapping):
                if not inp or not all(isinstance(a, str) and isinstance(b, str) for a, b in inp.items()):
                    raise ValueError(f"members[{name!r}]: an input mapping takes the model's keys to feature ids of the batch")
                inp = dict(inp)
            elif not isinstance(inp, str):
                raise ValueError(f"members[{name!r}]: input must be a feature id or a mapping of the model's keys to feature ids")
            models.append(model)
            self.inputs.append(inp)
        self.models = torch.nn.ModuleList(models)
        self.weights = _weight_list(self.names, weights)
        self.transform = _check_transform(transform)
        self.eval()

    def member_outputs(self, features) -> list:
        """every member's own scores for the batch, in the members' order"""
        if not isinstance(features, Mapping):
            raise ValueError("StreamEnsemble: the batch must be a dict of features (ClipBatches(streams=(...)) with several streams gives one)")
        outs = []
        with torch.no_grad():
            for name, model, inp in zip(self.names, self.models, self.inputs):
                missing = [k for k in ([inp] if isinstance(inp, str) else inp.values()) if k not in features]
                if missing:
                    raise KeyError(f"StreamEnsemble: member {name!r} reads {missing}, the batch has {sorted(features)}")
                if model.training:
                    model.eval()
                x = features[inp] if isinstance(inp, str) else {mk: features[bk] for mk, bk in inp.items()}
                outs.append(model(x))
        return outs

    def forward(self, features):
        if self.training:
            raise RuntimeError("StreamEnsemble is evaluation-only: joint fine-tuning through the fused score is not built")
        return ops.score_fuse(self.member_outputs(features), self.weights, self.transform)


class ScoreStore:
    """The saved scores of the stream models over one split, fused without running a model again.  Build it with ``load`` (name -> the
    ``.npz`` a ``metrics.StreamScores.save`` wrote) or ``from_metrics`` (name -> ``StreamScores``): both refuse streams that differ in the
    number of samples, in the number of classes or in a label, and streams with a row no update wrote.  The arrays stay on the host until
    the first ``fuse`` / ``evaluate`` / ``search``, which uploads them once to ``device``."""

    def __init__(self, scores: Mapping[str, np.ndarray], labels: np.ndarray, transform: str = "none", device=None):
        if not 1 <= len(scores) <= _lib.FUSE_MAX_STREAMS:
            raise ValueError(f"ScoreStore: expected 1..{_lib.FUSE_MAX_STREAMS} streams, got {len(scores)}")
        self.names = tuple(scores)
        self.scores = {n: np.ascontiguousarray(scores[n], np.float32) for n in self.names}
        self.labels = np.ascontiguousarray(labels, np.int64)
        shapes = {n: a.shape for n, a in self.scores.items()}
        first = shapes[self.names[0]]
        if len(first) != 2 or any(s != first for s in shapes.values()) or self.labels.shape != first[:1]:
            raise ValueError(f"ScoreStore: score arrays {shapes} and labels {self.labels.shape}: expected one (N, classes) per stream and (N,)")
        self.transform = _check_transform(transform)
        self.device = device
        self._dev = None                    # ([scores on the device, in the streams' order], labels on the device)

    @classmethod
    def _checked(cls, parts: Dict[str, tuple], transform: str, device) -> "ScoreStore":
        """parts: name -> (scores, labels, filled) host arrays"""
        if not parts:
            raise ValueError("ScoreStore: no stream")
        names = list(parts)
        ref_scores, ref_labels, _ = parts[names[0]]
        for n in names:
            scores, labels, filled = (np.asarray(a) for a in parts[n])
            if scores.ndim != 2 or labels.shape != scores.shape[:1] or filled.shape != scores.shape[:1]:
                raise ValueError(f"ScoreStore: stream {n!r} holds scores {scores.shape}, labels {labels.shape}, filled {filled.shape}")
            if scores.shape[0] != np.shape(ref_scores)[0]:
                raise ValueError(f"ScoreStore: stream {n!r} has {scores.shape[0]} samples, stream {names[0]!r} has {np.shape(ref_scores)[0]}")
            if scores.shape[1] != np.shape(ref_scores)[1]:
                raise ValueError(f"ScoreStore: stream {n!r} has {scores.shape[1]} classes, stream {names[0]!r} has {np.shape(ref_scores)[1]}")
            if not filled.astype(bool).all():
                raise ValueError(f"ScoreStore: stream {n!r} has {int((~filled.astype(bool)).sum())} unfilled rows (first: "
                                 f"{int(np.flatnonzero(~filled.astype(bool))[0])}): its validation pass did not cover the split")
            if not np.array_equal(labels, ref_labels):
                raise ValueError(f"ScoreStore: the labels of stream {n!r} differ from those of stream {names[0]!r}: not the same split")
        return cls({n: parts[n][0] for n in names}, ref_labels, transform, device)

    @classmethod
    def load(cls, paths: Mapping[str, str], transform: str = "none", device=None) -> "ScoreStore":
        parts = {}
        for name, path in paths.items():
            with np.load(path) as z:
                missing = {"scores", "labels", "filled"} - set(z.files)
                if missing:
                    raise ValueError(f"ScoreStore: {path} lacks {sorted(missing)}: not a file StreamScores.save wrote")
                parts[name] = (z["scores"], z["labels"], z["filled"])
        return cls._checked(parts, transform, device)

    @classmethod
    def from_metrics(cls, metrics: Mapping[str, object], transform: str = "none", device=None) -> "ScoreStore":
        """name -> ``metrics.StreamScores`` (waits for the device); ``device`` defaults to the one the first metric's store is on"""
        parts = {}
        for name, metric in metrics.items():
            if not (hasattr(metric, "value") and hasattr(metric, "device_value")):
                raise ValueError(f"ScoreStore: metrics[{name!r}] is no StreamScores")
            parts[name] = metric.value
            if device is None and metric.device_value is not None and metric.device_value[0].is_cuda:
                device = metric.device_value[0].device
        return cls._checked(parts, transform, device)

    # ---- device side ----------------------------------------------------------------------------------------------------------------
    @property
    def num_samples(self) -> int:
        return self.labels.shape[0]

    @property
    def num_classes(self) -> int:
        return self.scores[self.names[0]].shape[1]

    def _device(self):
        if self._dev is None:
            ops.ensure_device()
            device = torch.device(self.device if self.device is not None else "cuda")
            self._dev = ([ops.device_copy(self.scores[n], device) for n in self.names], ops.device_copy(self.labels, device))
        return self._dev

    def fuse(self, weights=None) -> torch.Tensor:
        """-> the fused scores (N, classes) float32 on the device (``ops.score_fuse``)"""
        w = _weight_list(self.names, weights)
        scores, _ = self._device()
        return ops.score_fuse(scores, w, self.transform)

    def evaluate(self, weights=None, k: int = 5) -> dict:
        """-> ``{"top1": hits, "topk": hits, "examples": rows with a label in [0, classes)}`` of the fused scores, integers, under the
        ranking rules of the metrics kernel (waits for the device)"""
        found = self.search([_weight_list(self.names, weights)], k=k)
        return {"top1": int(found["counts"][0, 0]), "topk": int(found["counts"][0, 1]), "examples": found["examples"]}

    def search(self, candidates, k: int = 5) -> dict:
        """Every candidate weight vector (G, S) in ONE ``ops.fuse_sweep`` call -> ``{"counts": int64 (G, 2) top-1 and top-k hits,
        "best": the row with the most top-1 hits, then the most top-k hits, then the lowest number, "weights": that row of the candidates as
        float32, "examples": ...}`` (waits for the device; the choice is made on the host from the small table)"""
        cand = np.asarray(candidates.detach().cpu() if torch.is_tensor(candidates) else candidates, np.float64).astype(np.float32)
        if cand.ndim != 2 or cand.shape[1] != len(self.names) or cand.shape[0] < 1:
            raise ValueError(f"search: candidates {cand.shape}, expected (G, {len(self.names)}) with G >= 1")
        if cand.shape[0] > _lib.FUSE_MAX_CANDIDATES:
            raise ValueError(f"search: {cand.shape[0]} candidates, at most {_lib.FUSE_MAX_CANDIDATES} per call")
        if not 1 <= k <= self.num_classes:
            raise ValueError(f"search: k={k} outside [1, {self.num_classes}]")
        scores, labels = self._device()
        hits, header = ops.fuse_sweep(scores, cand, labels, k, self.transform)
        counts, header = hits.cpu().numpy(), header.cpu().numpy()
        best = best_candidate(counts)
        return {"counts": counts, "best": best, "weights": cand[best].copy(), "examples": int(header[_lib.FUSE_EXAMPLES]),
                "ignored": int(header[_lib.FUSE_IGNORED]), "invalid": int(header[_lib.FUSE_INVALID])}


def best_candidate(counts: np.ndarray) -> int:
    """the row of an int (G, 2) table with the most top-1 hits, then the most top-k hits, then the lowest number"""
    counts = np.asarray(counts)
    order = np.lexsort((np.arange(counts.shape[0]), -counts[:, 1], -counts[:, 0]))
    return int(order[0])
