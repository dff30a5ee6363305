#!/usr/bin/env python3
"""What the fused optimizer step costs (fgcn_optim_step; profiles/optim_fold_vs_parent.json is this script against the parent's).

The headline model's flat buffers (AGCN, 2 x 300 x 25 x 3, 60 classes: 274 tensors, 3 469 524 floats = 13.9 MB).  The library call
itself -- ADAM plain and guarded over one group and over the three RULES groups (which interleave in the model-order gradient buffer
that GraphStep and dp.py share), SGD with momentum, ASGD plain with averaging (mu < 1) and with the copy (mu == 1), ASGD guarded -- and
``opt.step()`` as a whole (its host side, 274 pointer checks and version bumps, is longer than the kernel) for ADAM, one group, plain
and guarded.  All variants live in ONE process over copies of the model and alternate inside every round: HIP events around K
back-to-back calls, the median over the rounds after a warm-up; [min .. max] is the spread a difference has to clear.
``--tile4 256`` cuts the one-group tile tables into rows of that length instead of FlatOptimizer's own.

``python tools/optim_bench.py [--tile4 N] [OUT.json]``: one JSON line, also written to OUT.json.  Needs an MI355X (no fallback)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from fusion_gcn_amd import _lib  # noqa: E402
from fusion_gcn_amd.dp import FlatGradients  # noqa: E402
from fusion_gcn_amd.optim import KINDS, FlatOptimizer, _group_scalars, groups_from_rules  # noqa: E402

RULES = [{"match": r"bn|bias$|adj_b$", "weight_decay": 0.0}, {"match": r"^fc\.", "lr": 1e-3}]
K, ROUNDS, WARM = 20, 40, 5
GUARD = dict(max_grad_norm=1e30, skip_nonfinite=True)      # all three launches, a clip that never bites
dev = torch.device("cuda:0")


def make(kind, rules=None, tile4=None, **kw):
    model = bench.build_model(dev)
    params = groups_from_rules(model, rules) if rules else model.parameters()
    opt = FlatOptimizer(params, kind, 1e-5, grads=FlatGradients(model.parameters()), **kw)
    if tile4 and not rules:
        opt._tiles = torch.tensor(opt.tile_table(tile4), dtype=torch.int32).to(dev)
    opt.grads.zero_in_place()          # every p.grad is its view of the flat buffer: step() copies nothing
    opt.grads.flat.normal_(generator=torch.Generator(device=dev).manual_seed(1))
    opt.grads.flat.mul_(1e-3)
    return model, opt


def library_call(lib, opt, eta_mu=None):
    """The fgcn_optim_step call ``opt.step()`` makes, without its host side.  ``eta_mu``: ASGD's pair of the plain path."""
    tiles = opt._tiles
    pairs = [eta_mu] * len(opt.param_groups)
    groups = (_lib.OptimGroup * len(pairs))(*[_group_scalars(g, em) for g, em in zip(opt.param_groups, pairs)])
    n, guard = opt.flat.numel(), None
    if opt._guarded:
        if opt.kind == "ASGD":
            opt._write_sched()
        guard = _lib.OptimGuard(opt.max_grad_norm, 1, lib.fgcn_grad_norm_tiles(n), opt._partials.data_ptr(), opt._guard.data_ptr(),
                                opt._sched.data_ptr())
    head = (opt.flat.data_ptr(), opt.grads.flat.data_ptr(), opt.state1.data_ptr(), opt.state2.data_ptr() if opt.state2 is not None else None,
            n, KINDS[opt.kind], groups, len(groups), tiles.data_ptr(), tiles.shape[0], 1.0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    state = {"step": 0, "keep": (tiles, groups, guard)}

    def call():
        state["step"] += 1
        _lib.check(lib.fgcn_optim_step(*head, 0 if guard else state["step"], guard, stream), "fgcn_optim_step")
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tile4", type=int, default=None, help="row length of the one-group tile tables instead of FlatOptimizer's own")
    ap.add_argument("out", nargs="?")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optim_bench needs an MI355X")
    lib = _lib.load()
    keep, variants = [], {}

    def add(name, kind, how=library_call, eta_mu=None, **kw):
        keep.append(make(kind, weight_decay=0.01, tile4=args.tile4, **kw))
        opt = keep[-1][1]
        variants[name] = opt.step if how is None else how(lib, opt, eta_mu)

    add("adam_plain", "ADAM")
    add("adam_guarded", "ADAM", **GUARD)
    add("adam_plain_groups3", "ADAM", rules=RULES)
    add("adam_guarded_groups3", "ADAM", rules=RULES, **GUARD)
    add("sgd_momentum", "SGD", momentum=0.9)
    add("asgd_plain_average(mu<1)", "ASGD", eta_mu=(1e-5, 0.25))
    add("asgd_plain_copy(mu=1)", "ASGD", eta_mu=(1e-5, 1.0))
    add("asgd_guarded_average(t0=0)", "ASGD", t0=0, **GUARD)
    add("opt_step_adam_plain", "ADAM", how=None)
    add("opt_step_adam_guarded", "ADAM", how=None, **GUARD)

    times = {k: [] for k in variants}
    for r in range(WARM + ROUNDS):
        for name, call in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(K):
                call()
            e1.record()
            e1.synchronize()
            if r >= WARM:
                times[name].append(e0.elapsed_time(e1) * 1e3 / K)
    for _, o in keep:
        assert bool(torch.isfinite(o.flat).all())
    first = keep[0][1]
    out = {"what": "microseconds per optimizer call (fused update; guarded: norm + decision + update; opt_step_*: FlatOptimizer.step() as "
                   "a whole), HIP events around %d back-to-back calls, %d rounds after %d warm-up rounds, variants alternating inside "
                   "every round" % (K, ROUNDS, WARM),
           "device": torch.cuda.get_device_name(0), "flat_floats": first.flat.numel(), "flat_MB": round(first.flat.numel() * 4 / 1e6, 2),
           "tensors": len(first.params), "one_group_tile_rows": int(first._tiles.shape[0]),
           "us": {k: {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2),
                      "p10": round(sorted(v)[len(v) // 10], 2), "p90": round(sorted(v)[len(v) * 9 // 10], 2)} for k, v in times.items()}}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
