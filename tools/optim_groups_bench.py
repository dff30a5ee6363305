#!/usr/bin/env python3
"""What parameter groups cost in the fused optimizer step (FlatOptimizer over a list of groups, fgcn_optim_step_groups).

``opt.step()`` alone at the headline model (AGCN, 2 x 300 x 25 x 3, 60 classes: 274 tensors, about 3.5 M parameters, ADAM,
weight_decay 0.01): the single group (``fgcn_optim_step``, the yardstick) against three groups -- BatchNorm / bias / adj_b without
decay, fc with its own LR, the rest -- over the model-order gradient buffer that GraphStep and dp.py share, where the groups
interleave.  Unguarded and guarded (max_grad_norm + skip_nonfinite).  All optimizers live in ONE process over copies of the model
and are alternated after warm-up, HIP events around ``--opt-steps`` steps each, ``--rounds`` times; the margin a difference has to
clear is the spread (max - min) of the single-group figure across the rounds of that same run.  ``--tile4`` adds grouped variants
whose tile table is cut into rows of another length (the kernel takes any length up to FGCN_OPT_TILE4).

One JSON line.  Needs an MI355X (no fallback)."""
import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

RULES = [{"match": r"bn|bias$|adj_b$", "weight_decay": 0.0}, {"match": r"^fc\.", "lr": 1e-3}]


def build_optimizers(base, lr, tile4s):
    from fusion_gcn_amd.dp import FlatGradients
    from fusion_gcn_amd.optim import FlatOptimizer, groups_from_rules
    out = {}
    for guard_name, kw in (("unguarded", {}), ("guarded", dict(max_grad_norm=1.0, skip_nonfinite=True))):
        model = copy.deepcopy(base)
        out[f"single_{guard_name}"] = (model, FlatOptimizer(model.parameters(), "ADAM", lr, weight_decay=0.01,
                                                            grads=FlatGradients(model.parameters()), **kw))
        for tile4 in tile4s:
            model = copy.deepcopy(base)
            opt = FlatOptimizer(groups_from_rules(model, RULES), "ADAM", lr, weight_decay=0.01, grads=FlatGradients(model.parameters()), **kw)
            if tile4 is not None:
                opt._tiles = torch.tensor(opt.tile_table(tile4), dtype=torch.int32).to(opt.flat.device)
            out[f"groups3_{guard_name}" + (f"_tile{tile4}" if tile4 is not None else "")] = (model, opt)
    return out


def measure(opts, steps, warmup, rounds):
    g = torch.Generator().manual_seed(3)
    grads = None
    for model, opt in opts.values():
        if grads is None:
            grads = [(torch.randn(p.shape, generator=g) * 0.01) for p in model.parameters()]
        for p, grad in zip(model.parameters(), grads):
            p.grad = grad.to(p.device)
        for _ in range(warmup):
            opt.step()
    torch.cuda.synchronize()
    first = next(iter(opts.values()))[1]
    rec = {"tensors": len(first.params), "floats": first.flat.numel(), "steps": steps, "rounds": [],
           "tile_rows": {k: int(o._tiles.shape[0]) for k, (_, o) in opts.items() if o._tiles is not None},
           "group_sizes": [len(gr["params"]) for gr in next(o for _, o in opts.values() if o._tiles is not None).param_groups]}
    for _ in range(rounds):
        row = {}
        for name, (_, opt) in opts.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                opt.step()
            e1.record()
            torch.cuda.synchronize()
            row[name] = round(1e3 * e0.elapsed_time(e1) / steps, 2)
        rec["rounds"].append(row)
    for name in opts:
        vals = [r[name] for r in rec["rounds"]]
        rec[name] = {"gpu_us_mean": round(sum(vals) / rounds, 2), "gpu_us_min": min(vals), "gpu_us_max": max(vals)}
    for guard_name in ("unguarded", "guarded"):
        single = rec[f"single_{guard_name}"]
        rec[f"{guard_name}_single_spread_us"] = round(single["gpu_us_max"] - single["gpu_us_min"], 2)
        for name in opts:
            if name.startswith(f"groups3_{guard_name}"):
                rec[f"{name}_minus_single_us"] = round(rec[name]["gpu_us_mean"] - single["gpu_us_mean"], 2)
    rec["counters"] = {k: {"steps": o.steps, "skipped": o.skipped_steps, "clipped": o.clipped_steps}
                       for k, (_, o) in opts.items() if k.endswith("guarded") and not k.endswith("unguarded")}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--opt-steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--tile4", default="", help="comma-separated row lengths to time besides the default (e.g. 256,512)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optim_groups_bench needs an MI355X")
    from optim_guard_bench import headline_model
    dev = torch.device("cuda:0")
    tile4s = [None] + [int(t) for t in args.tile4.split(",") if t]
    out = {"device": torch.cuda.get_device_name(0)}
    out.update(measure(build_optimizers(headline_model(dev), 1e-4, tile4s), args.opt_steps, args.warmup, args.rounds))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
