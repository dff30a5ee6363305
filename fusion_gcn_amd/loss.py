"""The step's loss on libfgcn.  The reference builds ``torch.nn.CrossEntropyLoss()`` once per session and hands it to every step
(torch_src/session/session.py:53, session/procedures/step.py:38-46); ``CrossEntropyLoss`` here is that object -- same call
signature, mean reduction, rows labelled -100 (torch's ignore_index) do not count, any other label outside [0, classes) turns the loss
and the gradients into NaN (torch raises a device assert there) -- computed by one fixed-order kernel each way
(``fgcn_cross_entropy_fwd`` / ``_bwd``, include/fgcn.h).  A step that uses THIS loss (bench.py, GraphStep / the session when the
config's loss is built from this module) has bitwise reproducible gradients throughout, ``data_bn`` being on libfgcn as well; a
session that is handed ``torch.nn.CrossEntropyLoss`` instead runs torch's kernels for the loss.  No fallback: raises without
libfgcn / off gfx950.

The constructor and ``cross_entropy`` take torch's arguments as well: ``weight`` (class weights, a registered buffer),
``ignore_index``, ``reduction`` ("mean", "sum", "none"), ``label_smoothing``, and a float32 ``(rows, classes)`` target of class
probabilities in place of int64 labels (the dispatch is on the target's dtype).  Anything but the defaults with int64 labels runs
``fgcn_ce_fwd`` / ``_bwd`` (the formulas, the summation order), fixed-order and bitwise repeatable like the
plain pair; the defaults with int64 labels ARE the plain pair, bit for bit.  ``size_average`` / ``reduce`` (deprecated in torch)
are not built.  ``Session._to_device`` casts every label to int64, so probability targets are for callers of the loss or of a
``Step`` directly, not for a session's data loader.  Data-parallel training with ``weight=`` and mean reduction: each rank divides by
its own weight sum before the equal-weight all-reduce, exactly as under torch's DDP.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import block

REDUCTIONS = ("mean", "sum", "none")


def _check_options(weight: Optional[torch.Tensor], reduction: str, label_smoothing: float) -> None:
    if not isinstance(reduction, str) or reduction not in REDUCTIONS:
        raise ValueError(f"reduction must be one of {', '.join(REDUCTIONS)}, got {reduction!r}")
    if not 0.0 <= float(label_smoothing) <= 1.0:                       # (a NaN fails both comparisons)
        raise ValueError(f"label_smoothing must be in [0, 1], got {label_smoothing!r}")
    if weight is not None and not (isinstance(weight, torch.Tensor) and weight.dim() == 1 and weight.is_floating_point()):
        raise ValueError("weight must be a 1-D floating tensor with one entry per class")


def cross_entropy(logits: torch.Tensor, target: torch.Tensor, weight: Optional[torch.Tensor] = None, ignore_index: int = -100,
                  reduction: str = "mean", label_smoothing: float = 0.0) -> torch.Tensor:
    """``torch.nn.functional.cross_entropy`` for logits (rows, classes): ``target`` int64 labels (rows,) or float32 class
    probabilities (rows, classes).  ValueError for arguments torch rejects too; FgcnError without libfgcn / off gfx950."""
    _check_options(weight, reduction, label_smoothing)
    if weight is not None and (logits.dim() != 2 or weight.numel() != logits.shape[1]):
        raise ValueError(f"weight has {weight.numel()} entries for logits of shape {tuple(logits.shape)} (rows, classes)")
    if target.is_floating_point() and ignore_index != -100:
        raise ValueError("ignore_index applies to class-index targets, not to class probabilities")
    if weight is None and ignore_index == -100 and reduction == "mean" and label_smoothing == 0.0 and not target.is_floating_point():
        return block.cross_entropy(logits, target)
    if weight is not None and (weight.dtype != torch.float32 or weight.device != logits.device or not weight.is_contiguous()):
        weight = weight.to(device=logits.device, dtype=torch.float32).contiguous()
    return block.cross_entropy_options(logits, target, weight, int(ignore_index), reduction, float(label_smoothing))


class CrossEntropyLoss(torch.nn.Module):
    """``torch.nn.CrossEntropyLoss(weight, ignore_index=, reduction=, label_smoothing=)``; ``weight`` is a buffer: it moves with
    ``.to()`` and is in the ``state_dict``."""

    def __init__(self, weight: Optional[torch.Tensor] = None, ignore_index: int = -100, reduction: str = "mean",
                 label_smoothing: float = 0.0) -> None:
        super().__init__()
        _check_options(weight, reduction, label_smoothing)
        self.register_buffer("weight", None if weight is None else weight.detach().to(torch.float32).contiguous())
        self.ignore_index, self.reduction, self.label_smoothing = int(ignore_index), reduction, float(label_smoothing)

    def forward(self, y_pred: torch.Tensor, label: torch.Tensor) -> torch.Tensor:
        return cross_entropy(y_pred, label, self.weight, self.ignore_index, self.reduction, self.label_smoothing)

    def extra_repr(self) -> str:
        return f"ignore_index={self.ignore_index}, reduction={self.reduction!r}, label_smoothing={self.label_smoothing}"


def balanced_class_weights(labels, num_classes: int) -> torch.Tensor:
    """Class weights ``n / (C * count_c)`` (0 for a class without samples) as a float32 tensor of ``num_classes`` entries, from the
    labels of a training set (``MultiModalDataset.labels_data``, any sequence or tensor of class indices): what ``weight=`` takes."""
    labels = torch.as_tensor(labels).reshape(-1).to(torch.int64)
    if num_classes <= 0 or (labels.numel() and (int(labels.min()) < 0 or int(labels.max()) >= num_classes)):
        raise ValueError(f"labels outside [0, {num_classes})")
    count = torch.bincount(labels, minlength=num_classes).to(torch.float64)
    weight = torch.where(count > 0, labels.numel() / (num_classes * count.clamp(min=1)), torch.zeros_like(count))
    return weight.to(torch.float32)


__all__ = ["CrossEntropyLoss", "cross_entropy", "balanced_class_weights"]
