"""Shared by tests/test_metrics.py and tests/test_metrics_gpu.py: the golden streams of tests/golden/metrics.npz (written by
tools/gen_golden_metrics.py from the reference's own metric classes) and the metric list they were recorded for."""
import os

import numpy as np

from conftest import GOLDEN
from fusion_gcn_amd import _lib
from fusion_gcn_amd import metrics as M

STREAMS = ("a27", "b60", "c5")
CONTEXTS = (("train", "training"), ("val", "validation"))


def load():
    return np.load(os.path.join(GOLDEN, "metrics.npz"))


def spec(d, s):
    """(classes, k, rows per batch) of stream ``s``"""
    return int(d[f"{s}_classes"]), int(d[f"{s}_k"]), [int(r) for r in d[f"{s}_rows"]]


def build_container(classes, k, **kw):
    """The generator's list: build_metrics (training session) + the extra metrics as ``additional_metrics``."""
    extra = []
    lst = {"capacity": kw.pop("capacity")} if "capacity" in kw else {}
    for _, long in CONTEXTS:
        extra += [M.Precision(f"{long}_precision"), M.Recall(f"{long}_recall"), M.F1MeasureMetric(f"{long}_f1"),
                  M.ConfusionMatrix(classes, f"{long}_confusion_samples", mode="samples"),
                  M.ConfusionMatrix(classes, f"{long}_confusion_recall", mode="recall"),
                  M.ConfusionMatrix(classes, f"{long}_confusion_precision", mode="precision"),
                  M.MisclassifiedSamplesList(f"{long}_misclassified", **lst)]
    return M.build_metrics(classes, k=k, additional_metrics=extra, **kw)


def expected_state(d, s, step, long):
    """The integer state after batch ``step``, from the golden confusion matrix and the recorded hit count / loss sum."""
    cm = d[f"{s}_step{step}_{long}_confusion"]
    counts = np.zeros(_lib.CLS_LOSS_SUM, np.int64)
    counts[_lib.CLS_EXAMPLES] = cm.sum()
    counts[_lib.CLS_TOP1] = np.trace(cm)
    counts[_lib.CLS_TOPK] = d[f"{s}_step{step}_{long}_topk_hits"]
    counts[_lib.CLS_LOSS_ITEMS] = d[f"{s}_step{step}_{long}_loss_items"]
    return {"counts": counts, "loss_sum": np.float64(d[f"{s}_step{step}_{long}_loss_sum"]), "confusion": cm.astype(np.int32)}


def batches(d, s, ctx):
    """[(logits float32, labels int64, loss float32 scalar, indices int64)] of the stream's context, as numpy arrays"""
    _, _, rows = spec(d, s)
    out, lo = [], 0
    for i, n in enumerate(rows):
        out.append((d[f"{s}_{ctx}_logits"][lo:lo + n].astype(np.float32), d[f"{s}_{ctx}_labels"][lo:lo + n],
                    d[f"{s}_{ctx}_loss"][i], d[f"{s}_{ctx}_indices"][lo:lo + n]))
        lo += n
    return out


def reference_predictions(d, s, ctx, upto_rows):
    """(indices, argmax, labels) of the first rows, for load_state's sample arrays (no ties in the golden logits)"""
    z = d[f"{s}_{ctx}_logits"][:upto_rows].astype(np.float32)
    return d[f"{s}_{ctx}_indices"][:upto_rows], z.argmax(axis=1), d[f"{s}_{ctx}_labels"][:upto_rows]


def check_values(container, d, s, step, k, rel=1e-12):
    """Every derived value of both contexts against the golden ones: integers exact, float64 ratios to ``rel``.  The reference
    normalises its confusion matrices in float32; the float64 quotient rounded to float32 IS the float32 quotient (the operands
    are integers below 2^24, and rounding a 53-bit quotient of two 24-bit numbers to 24 bits is the correctly rounded result:
    53 >= 2 * 24 + 2), so those compare exactly after the cast, and to ``rel`` against the float64 quotient computed here."""
    for _, long in CONTEXTS:
        g = lambda name: d[f"{s}_step{step}_{long}_{name}"]      # noqa: E731
        for name in ("loss", "accuracy", f"top{k}_accuracy", "precision", "recall", "f1"):
            got, want = container[f"{long}_{name}"].value, float(g(name))
            assert isinstance(got, float) and abs(got - want) <= rel * abs(want), (s, step, long, name, got, want)
        cm = g("confusion")
        got = container[f"{long}_confusion"].value.numpy()
        assert got.dtype == np.int32 and (got == cm).all()
        n = np.float64(cm.sum())
        exact = {"samples": cm / n, "recall": cm / (cm.sum(axis=1, dtype=np.int64)[:, None] + 1e-15),
                 "precision": cm / (cm.sum(axis=0, dtype=np.int64) + 1e-15)}
        for mode, want64 in exact.items():
            got = container[f"{long}_confusion_{mode}"].value.numpy()
            assert got.dtype == np.float64
            assert (got.astype(np.float32) == g(f"confusion_{mode}")).all(), (s, step, long, mode)
            assert np.allclose(got, want64, rtol=rel, atol=0), (s, step, long, mode)
        want = [tuple(int(v) for v in row) for row in g("misclassified")]
        assert container[f"{long}_misclassified"].value == want, (s, step, long)
