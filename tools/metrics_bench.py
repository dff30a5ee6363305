#!/usr/bin/env python3
"""What the metrics hook costs per training step, measured three ways in ONE process, twice over (a / b / c / a / b / c):

  (a) none    ``Session.train_epoch`` with no metrics object
  (b) item    a plain-torch container that does what the reference's Mean / MultiClassAccuracy / TopKAccuracy do: three ``.item()``
              read-backs per batch (torch_src/metrics.py:85,107,131)
  (c) device  ``fusion_gcn_amd.metrics.build_metrics``: one ``fgcn_classify_update`` launch per batch, a non-blocking snapshot copy,
              a progress line formatted from the newest snapshot that has arrived

on a short-step model (the ``rgb_patch_features`` mode at batch 8, the shape of tools/patch_bench.py) and at the headline shape
(AGCN, 64 clips of 2 x 300 x 25 x 3, 60 classes).  The step is ``GraphStep`` + ``loss.CrossEntropyLoss`` + ``optim.FlatOptimizer``
(SGD, lr 0).  (b) and (c) format a progress line after every batch, as the epoch loop does for a progress logger.

Per variant: ``wall_ms`` (host clock over the epoch, device drained at the end, per step), ``gpu_ms`` (HIP events around the same
epoch, per step) and ``host_ms`` (host clock until the LAST batch was enqueued, per step: below ``gpu_ms`` the host runs ahead).
Beside them ``update_kernel_us`` and ``cross_entropy_fwd_us``: each kernel alone, HIP events around a run of back-to-back launches
on the step's tensors, per launch.  One JSON line.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402


class ItemContainer:
    """The reference's per-batch arithmetic and read-backs, in plain torch."""

    def __init__(self, k):
        self.k, self.loss, self.n, self.top1, self.topk = k, 0., 0, 0, 0

    def update_training(self, loss, output, model, indices):
        y_pred, y_true = output
        n = len(y_true)
        self.loss += loss.item() * n
        self.top1 += torch.sum(torch.eq(torch.argmax(y_pred, dim=1), y_true)).item()
        self.topk += torch.sum(torch.eq(torch.topk(y_pred, self.k, dim=1)[1], y_true.view(-1, 1))).item()
        self.n += n

    def format_training(self):
        return f"training_loss: {self.loss / self.n:.4f}, training_accuracy: {self.top1 / self.n:.4f}, " \
               f"training_top{self.k}_accuracy: {self.topk / self.n:.4f}"


class Progress:
    def __init__(self):
        self.line, self.done = None, 0.0

    def update_epoch_mode(self, mode, metrics=None):
        self.line, self.done = metrics, time.perf_counter()


def patch_model(dev, batch, T):
    from fusion_gcn_amd.datasets.utd_mhad import constants as utd
    from fusion_gcn_amd.models.mmargcn.mmargcn import Model
    from fusion_gcn_amd.util import Graph
    torch.manual_seed(1)
    model = Model({"rgb": (1, T, 20, 512)}, 27, Graph(utd.skeleton_edges, center_joint=utd.center_joint), mode="rgb_patch_features",
                  patch_feature_input_dim=512)._model.to(dev).train()
    return model, torch.randn(batch, 1, T, 20, 512, device=dev), torch.randint(0, 27, (batch,), device=dev), 27


def headline_model(dev, batch):
    from fusion_gcn_amd.datasets.ntu_rgb_d import constants as ntu
    from fusion_gcn_amd.models.mmargcn.agcn import Model
    from fusion_gcn_amd.util import Graph
    torch.manual_seed(1)
    model = Model((2, 300, 25, 3), 60, Graph(ntu.skeleton_edges, center_joint=ntu.center_joint)).to(dev).train()
    return model, torch.randn(batch, 2, 300, 25, 3, device=dev), torch.randint(0, 60, (batch,), device=dev), 60


def kernel_alone(fn, reps=200):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return round(1e3 * t0.elapsed_time(t1) / reps, 2)


def measure(name, model, x, y, classes, steps, warmup, rounds):
    from fusion_gcn_amd import metrics as M
    from fusion_gcn_amd import ops
    from fusion_gcn_amd.loss import CrossEntropyLoss
    from fusion_gcn_amd.optim import FlatOptimizer
    from fusion_gcn_amd.session.procedures import DefaultBatchProcessor, GraphStep
    from fusion_gcn_amd.session.session import Session
    k = 5
    opt = FlatOptimizer(model.parameters(), "SGD", 0.0)
    processor, loss_fn = DefaultBatchProcessor(GraphStep()), CrossEntropyLoss()
    indices = torch.arange(y.shape[0])
    make = {"none": lambda: None, "item": lambda: ItemContainer(k), "device": lambda: M.build_metrics(classes, k=k)}
    Session.train_epoch(processor, model, loss_fn, [(x, y, indices)] * warmup, opt, None, None)         # records the graph
    out = {"batch": y.shape[0], "classes": classes, "steps": steps, "variants": []}
    for rnd in range(rounds):
        for variant, build in make.items():
            metrics = build()
            progress = Progress() if metrics is not None else None
            Session.train_epoch(processor, model, loss_fn, [(x, y, indices)] * warmup, opt, progress, metrics)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            Session.train_epoch(processor, model, loss_fn, [(x, y, indices)] * steps, opt, progress, metrics)
            t_host = time.perf_counter()
            e1.record()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            rec = {"variant": variant, "round": rnd, "wall_ms": round(1e3 * (t1 - t0) / steps, 3),
                   "gpu_ms": round(e0.elapsed_time(e1) / steps, 3), "host_ms": round(1e3 * (t_host - t0) / steps, 3)}
            if variant == "device":
                rec["last_progress_line"] = progress.line
                rec["final"] = metrics.format_training()
            elif variant == "item":
                rec["final"] = metrics.format_training()
            out["variants"].append(rec)
    with torch.no_grad():
        logits = torch.randn(y.shape[0], classes, device=y.device)
        state = torch.zeros(ops.classify_state_bytes(classes) // 8, dtype=torch.int64, device=y.device)
        loss = torch.zeros((), device=y.device)
        out["update_kernel_us"] = kernel_alone(lambda: ops.classify_update(logits, y, state, k=k, loss=loss))
        out["cross_entropy_fwd_us"] = kernel_alone(lambda: ops.cross_entropy_fwd(logits, y))
    mean = lambda v, key: round(sum(r[key] for r in out["variants"] if r["variant"] == v) / rounds, 3)      # noqa: E731
    out["summary"] = {f"{v}_{key}": mean(v, key) for v in make for key in ("wall_ms", "gpu_ms", "host_ms")}
    out["summary"]["device_minus_none_wall_us"] = round(1e3 * (out["summary"]["device_wall_ms"] - out["summary"]["none_wall_ms"]), 1)
    out["summary"]["item_minus_none_wall_us"] = round(1e3 * (out["summary"]["item_wall_ms"] - out["summary"]["none_wall_ms"]), 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--math", default="bf16x3")
    ap.add_argument("--only", default="patch,headline")
    ap.add_argument("--frames", type=int, default=128, help="frames per clip of the patch-feature model")
    args = ap.parse_args()
    from fusion_gcn_amd import ops
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "math": args.math}
    with ops.math_mode(args.math):
        if "patch" in args.only:
            out["rgb_patch_features_batch8"] = measure("patch", *patch_model(dev, 8, args.frames), args.steps, args.warmup, args.rounds)
        if "headline" in args.only:
            out["agcn_headline_batch64"] = measure("headline", *headline_model(dev, 64), max(10, args.steps // 2), args.warmup, args.rounds)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
