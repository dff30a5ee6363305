#!/usr/bin/env python3
"""Writes tests/golden/metrics.npz from the REFERENCE's own metric classes (torch_src/metrics.py), CPU only, on a machine that has
the reference checked out (``FGCN_REFERENCE``, import recipe of SURVEY.md Appendix B).  Nothing of the reference is copied: the file
holds the inputs this script draws and the values the reference's classes report for them.

The reference module imports TensorBoard and its visualisation package at the top; neither is needed for a value, so both are
stubbed in ``sys.modules`` before ``import metrics``.

Three streams of batches, each fed to a container that holds the list ``Session.build_metrics`` builds (session/session.py:108-158)
plus Precision, Recall, F1MeasureMetric, the three normalised ConfusionMatrix modes and MisclassifiedSamplesList, for both contexts:

    a27   27 classes, k = 5, batches of 8, 8 and 5 rows (a ragged last batch)
    b60   60 classes, k = 5, 3 batches of 64 rows
    c5     5 classes, k = 5 (k == classes), 2 batches of 6 rows

Logits are stored as float16 (every value is exact in float32) and no row holds two equal logits (asserted), so the reference's
``torch.topk`` needs no tie rule.  Recorded after EVERY batch: each metric's value, the top-k hit count and the loss sum behind them,
and the three format strings; after the last batch: the ``reset_all`` history.
"""
import os
import sys
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("FGCN_REFERENCE", "/root/reference")
sys.dont_write_bytecode = True
sys.path[:0] = [REF, os.path.join(REF, "torch_src")]

_tb = types.ModuleType("torch.utils.tensorboard")
_tb.SummaryWriter = object
sys.modules["torch.utils.tensorboard"] = _tb
import util.visualization  # noqa: E402,F401  (reference package; the stub below replaces its matplotlib module)
sys.modules["util.visualization.model_visualization"] = types.ModuleType("util.visualization.model_visualization")
import metrics as ref  # noqa: E402  (reference)

STREAMS = {"a27": (27, 5, (8, 8, 5)), "b60": (60, 5, (64, 64, 64)), "c5": (5, 5, (6, 6))}
CONTEXTS = (("train", "training"), ("val", "validation"))


def draw(gen, classes, rows, first_index):
    """One batch: labels, logits that favour the label about two times in three, the batch's cross entropy, sample indices."""
    labels = torch.randint(0, classes, (rows,), generator=gen)
    boost = (torch.rand(rows, generator=gen) < 0.65).float() * 3.0
    logits = torch.empty(rows, classes)
    for r in range(rows):
        while True:                 # float16 has few values: a row with two equal logits is drawn again
            row = torch.randn(classes, generator=gen)
            row[labels[r]] += boost[r]
            row = row.half().float()
            if len(set(row.tolist())) == classes:
                break
        logits[r] = row
    for row in logits:
        assert len(set(row.tolist())) == classes, "two equal logits in a row"
    loss = torch.nn.functional.cross_entropy(logits, labels)
    indices = first_index + torch.randperm(rows, generator=gen)
    return logits, labels, loss, indices


def build_list(classes, k):
    """The list of Session.build_metrics (training session) with the extra metrics passed as ``additional_metrics``."""
    extra = []
    for _, long in CONTEXTS:
        extra += [ref.Precision(f"{long}_precision"), ref.Recall(f"{long}_recall"), ref.F1MeasureMetric(f"{long}_f1"),
                  ref.ConfusionMatrix(classes, f"{long}_confusion_samples", mode="samples"),
                  ref.ConfusionMatrix(classes, f"{long}_confusion_recall", mode="recall"),
                  ref.ConfusionMatrix(classes, f"{long}_confusion_precision", mode="precision"),
                  ref.MisclassifiedSamplesList(f"{long}_misclassified")]
    lst = [ref.Mean("training_loss"), ref.Mean("validation_loss"), ref.MultiClassAccuracy("training_accuracy"),
           ref.MultiClassAccuracy("validation_accuracy"), ref.ConfusionMatrix(classes, "training_confusion"),
           ref.ConfusionMatrix(classes, "validation_confusion")]
    if k > 1:
        lst += [ref.TopKAccuracy(f"training_top{k}_accuracy", k=k), ref.TopKAccuracy(f"validation_top{k}_accuracy", k=k)]
    return lst + extra + [ref.SimpleMetric("lr")]


def record(out, prefix, container, k):
    for m in container.get_metrics():
        v = m.value
        if isinstance(m, ref.MisclassifiedSamplesList):
            v = np.array([[int(a), int(b), int(c)] for a, b, c in v], dtype=np.int64).reshape(-1, 3)
        elif torch.is_tensor(v):
            v = v.numpy().copy()            # the reference hands out its own, later updated, tensor
        else:
            v = np.float64(v)
        out[f"{prefix}_{m.name}"] = v
    for _, long in CONTEXTS:
        out[f"{prefix}_{long}_topk_hits"] = np.int64(container[f"{long}_top{k}_accuracy"]._num_correct)
        out[f"{prefix}_{long}_loss_sum"] = np.float64(container[f"{long}_loss"]._sum)
        out[f"{prefix}_{long}_loss_items"] = np.int64(container[f"{long}_loss"]._steps)
    out[f"{prefix}_format_training"] = np.array(container.format_training())
    out[f"{prefix}_format_validation"] = np.array(container.format_validation())
    out[f"{prefix}_format_all"] = np.array(container.format_all())


def main():
    out = {"torch_version": np.array(torch.__version__)}
    for si, (name, (classes, k, rows)) in enumerate(STREAMS.items()):
        gen = torch.Generator().manual_seed(1234 + si)
        container = ref.MetricsContainer(build_list(classes, k))
        out[f"{name}_classes"], out[f"{name}_k"], out[f"{name}_rows"] = np.int64(classes), np.int64(k), np.array(rows, dtype=np.int64)
        data = {ctx: [] for ctx, _ in CONTEXTS}
        first = 0
        for i, n in enumerate(rows):
            for ctx, _ in CONTEXTS:
                batch = draw(gen, classes, n, first)
                data[ctx].append(batch)
                update = container.update_training if ctx == "train" else container.update_validation
                update(batch[2], (batch[0], batch[1]), None, batch[3])
            first += n
            record(out, f"{name}_step{i}", container, k)
        for ctx, _ in CONTEXTS:
            out[f"{name}_{ctx}_logits"] = torch.cat([b[0] for b in data[ctx]]).numpy().astype(np.float16)
            out[f"{name}_{ctx}_labels"] = torch.cat([b[1] for b in data[ctx]]).numpy()
            out[f"{name}_{ctx}_loss"] = torch.stack([b[2] for b in data[ctx]]).numpy()
            out[f"{name}_{ctx}_indices"] = torch.cat([b[3] for b in data[ctx]]).numpy()
        container.reset_all(save_history=True)
        for key, values in container.get_value_history().items():
            if isinstance(container[key], ref.ScalarMetric):
                out[f"{name}_history_{key}"] = np.array(values, dtype=np.float64)
    path = os.path.join(REPO, "tests", "golden", "metrics.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
