#!/usr/bin/env python3
"""What the ASGD launch costs against the ADAM launch of the same tree (profiles/optim_asgd_vs_adam.json).

The headline model's flat buffers (AGCN, 2 x 300 x 25 x 3, 60 classes: 274 tensors, 13.9 MB).  The library calls themselves, not
``opt.step()`` (whose host side -- 274 pointer checks and version bumps -- is longer than the kernel): fgcn_optim_step for ADAM and for
ASGD with and without averaging (mu < 1 / mu == 1), fgcn_optim_step_guarded for ADAM and fgcn_optim_step_groups_guarded with one group
for ASGD.  All variants live in ONE process over copies of the model and alternate inside every round: HIP events around K
back-to-back calls, the median over the rounds after a warm-up; min / max / p10 / p90 are the spread a difference has to clear.

``python tools/optim_asgd_bench.py [OUT.json]``: one JSON line, also written to OUT.json.  Needs an MI355X (no fallback)."""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from fusion_gcn_amd import _lib  # noqa: E402
from fusion_gcn_amd.optim import KINDS, FlatOptimizer, _group_scalars  # noqa: E402

dev = torch.device("cuda:0")
lib = _lib.load()
K, ROUNDS, WARM = 20, 40, 5


def make(kind, **kw):
    model = bench.build_model(dev)
    opt = FlatOptimizer(model.parameters(), kind, 1e-5, **kw)
    opt.grads.flat.normal_(generator=torch.Generator(device=dev).manual_seed(1))
    opt.grads.flat.mul_(1e-3)
    return model, opt


def plain(opt, eta_mu=None):
    h = _group_scalars(opt.param_groups[0], eta_mu)
    s1 = opt.state1.data_ptr()
    s2 = opt.state2.data_ptr() if opt.state2 is not None else None
    n = opt.flat.numel()
    args = (opt.flat.data_ptr(), opt.grads.flat.data_ptr(), s1, s2, n, KINDS[opt.kind], h.lr, h.weight_decay, 1.0, h.beta1, h.beta2, h.eps,
            h.momentum, h.dampening, h.nesterov)
    stream = torch.cuda.current_stream(dev).cuda_stream
    state = {"step": 0}

    def call():
        state["step"] += 1
        _lib.check(lib.fgcn_optim_step(*args, state["step"], stream), "fgcn_optim_step")
    return call


def guarded(opt):
    n = opt.flat.numel()
    s1 = opt.state1.data_ptr()
    s2 = opt.state2.data_ptr() if opt.state2 is not None else None
    stream = torch.cuda.current_stream(dev).cuda_stream
    tail = (1e30, 1, opt._partials.data_ptr(), lib.fgcn_grad_norm_tiles(n), opt._guard.data_ptr())
    h = _group_scalars(opt.param_groups[0])
    if opt.kind == "ASGD":
        opt._write_sched()
        groups = (_lib.OptimGroup * 1)(h)
        args = (opt.flat.data_ptr(), opt.grads.flat.data_ptr(), s1, s2, n, 3, groups, 1, opt._tiles.data_ptr(), opt._tiles.shape[0], 1.0,
                *tail, opt._sched.data_ptr(), stream)
        return lambda: _lib.check(lib.fgcn_optim_step_groups_guarded(*args), "groups_guarded")
    args = (opt.flat.data_ptr(), opt.grads.flat.data_ptr(), s1, s2, n, KINDS[opt.kind], h.lr, h.weight_decay, 1.0, h.beta1, h.beta2, h.eps,
            h.momentum, h.dampening, h.nesterov, *tail, stream)
    return lambda: _lib.check(lib.fgcn_optim_step_guarded(*args), "guarded")


keep = []
variants = {}
m, o = make("ADAM", weight_decay=0.01)
keep.append((m, o))
variants["adam_plain"] = plain(o)
m, o = make("ASGD", weight_decay=0.01)
keep.append((m, o))
variants["asgd_plain_average(mu<1)"] = plain(o, (1e-5, 0.25))
m, o = make("ASGD", weight_decay=0.01)
keep.append((m, o))
variants["asgd_plain_copy(mu=1)"] = plain(o, (1e-5, 1.0))
m, o = make("ADAM", weight_decay=0.01)
keep.append((m, o))
variants["adam_guarded"] = guarded(o)
m, o = make("ASGD", weight_decay=0.01, t0=0)
keep.append((m, o))
variants["asgd_guarded_average(t0=0)"] = guarded(o)
n_floats = keep[0][1].flat.numel()

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
for m, o in keep:
    assert bool(torch.isfinite(o.flat).all())
out = {"what": "microseconds per optimizer call (fused update; guarded: norm + decision + update), HIP events around %d back-to-back "
               "library calls, %d rounds after %d warm-up rounds, variants alternating inside every round" % (K, ROUNDS, WARM),
       "device": torch.cuda.get_device_name(0), "flat_floats": n_floats, "flat_MB": round(n_floats * 4 / 1e6, 2),
       "tensors": len(keep[0][1].params),
       "us": {k: {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2),
                  "p10": round(sorted(v)[len(v) // 10], 2), "p90": round(sorted(v)[len(v) * 9 // 10], 2)} for k, v in times.items()}}
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
print(json.dumps(out))
