#!/usr/bin/env python3
"""What the guard of the fused optimizer step costs (FlatOptimizer(max_grad_norm=, skip_nonfinite=), fgcn_optim_step_guarded).

  optimizer   ``opt.step()`` alone at the headline model (AGCN, 2 x 300 x 25 x 3, 60 classes: 274 tensors, about 3.5 M parameters,
              ADAM, weight_decay 0.01): unguarded (one launch) against guarded with both options on (three launches), two optimizers
              over two copies of the model, alternated in ONE process after warm-up, HIP events around ``--opt-steps`` steps each.
  step        the whole training step, ``Session.train_epoch`` with ``GraphStep`` + ``loss.CrossEntropyLoss`` + the optimizer at 64
              clips, as tools/metrics_bench.py takes it (no metrics object): the same two optimizers, alternated, wall clock with the
              device drained at the end and HIP events, per step.

One JSON line.  Needs an MI355X (no fallback)."""
import argparse
import copy
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402


def headline_model(dev):
    from fusion_gcn_amd.datasets.ntu_rgb_d import constants as ntu
    from fusion_gcn_amd.models.mmargcn.agcn import Model
    from fusion_gcn_amd.util import Graph
    torch.manual_seed(1)
    return Model((2, 300, 25, 3), 60, Graph(ntu.skeleton_edges, center_joint=ntu.center_joint)).to(dev).train()


def build_optimizers(base, dev, lr):
    from fusion_gcn_amd.optim import FlatOptimizer
    out = {}
    for variant, kw in (("unguarded", {}), ("guarded", dict(max_grad_norm=1.0, skip_nonfinite=True))):
        model = copy.deepcopy(base)
        out[variant] = (model, FlatOptimizer(model.parameters(), "ADAM", lr, weight_decay=0.01, **kw))
    return out


def optimizer_alone(opts, steps, warmup, rounds):
    g = torch.Generator().manual_seed(3)
    for model, opt in opts.values():
        for p in model.parameters():
            p.grad = (torch.randn(p.shape, generator=g) * 0.01).to(p.device)
        for _ in range(warmup):
            opt.step()
    torch.cuda.synchronize()
    rec = {"tensors": len(next(iter(opts.values()))[1].params), "floats": next(iter(opts.values()))[1].flat.numel(), "steps": steps,
           "rounds": []}
    for rnd in range(rounds):
        row = {}
        for variant, (_, opt) in opts.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            for _ in range(steps):
                opt.step()
            t_host = time.perf_counter()
            e1.record()
            torch.cuda.synchronize()
            row[variant] = {"gpu_us": round(1e3 * e0.elapsed_time(e1) / steps, 2), "host_us": round(1e6 * (t_host - t0) / steps, 2)}
        rec["rounds"].append(row)
    for variant in opts:
        rec[f"{variant}_gpu_us"] = round(sum(r[variant]["gpu_us"] for r in rec["rounds"]) / rounds, 2)
    rec["guarded_minus_unguarded_gpu_us"] = round(rec["guarded_gpu_us"] - rec["unguarded_gpu_us"], 2)
    g_opt = opts["guarded"][1]
    rec["guarded_counters"] = {"steps": g_opt.steps, "skipped": g_opt.skipped_steps, "clipped": g_opt.clipped_steps,
                               "grad_norm": float(g_opt.grad_norm), "clip_coef": float(g_opt.clip_coef)}
    return rec


def whole_step(opts, dev, batch, steps, warmup, rounds):
    from fusion_gcn_amd.loss import CrossEntropyLoss
    from fusion_gcn_amd.session.procedures import DefaultBatchProcessor, GraphStep
    from fusion_gcn_amd.session.session import Session
    x, y = torch.randn(batch, 2, 300, 25, 3, device=dev), torch.randint(0, 60, (batch,), device=dev)
    data, loss_fn = (x, y, torch.arange(batch)), CrossEntropyLoss()
    procs = {v: DefaultBatchProcessor(GraphStep()) for v in opts}
    for v, (model, opt) in opts.items():
        Session.train_epoch(procs[v], model, loss_fn, [data] * warmup, opt)          # records the graph
    torch.cuda.synchronize()
    rec = {"batch": batch, "steps": steps, "rounds": []}
    for rnd in range(rounds):
        row = {}
        for v, (model, opt) in opts.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            Session.train_epoch(procs[v], model, loss_fn, [data] * steps, opt)
            e1.record()
            torch.cuda.synchronize()
            row[v] = {"wall_ms": round(1e3 * (time.perf_counter() - t0) / steps, 3), "gpu_ms": round(e0.elapsed_time(e1) / steps, 3)}
        rec["rounds"].append(row)
    for v in opts:
        rec[f"{v}_gpu_ms"] = round(sum(r[v]["gpu_ms"] for r in rec["rounds"]) / rounds, 3)
    rec["guarded_minus_unguarded_gpu_us"] = round(1e3 * (rec["guarded_gpu_ms"] - rec["unguarded_gpu_ms"]), 1)
    g_opt = opts["guarded"][1]
    rec["guarded_counters"] = {"steps": g_opt.steps, "skipped": g_opt.skipped_steps, "clipped": g_opt.clipped_steps}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--opt-steps", type=int, default=200)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--math", default="bf16x3")
    ap.add_argument("--only", default="optimizer,step")
    args = ap.parse_args()
    from fusion_gcn_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("optim_guard_bench needs an MI355X")
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "math": args.math}
    with ops.math_mode(args.math):
        base = headline_model(dev)
        if "optimizer" in args.only:
            out["optimizer_alone"] = optimizer_alone(build_optimizers(base, dev, 1e-4), args.opt_steps, 20, args.rounds)
        if "step" in args.only:
            out["whole_step"] = whole_step(build_optimizers(base, dev, 1e-4), dev, args.batch, args.steps, args.warmup, args.rounds)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
