#!/usr/bin/env python3
"""The sensor-augmented batch gather (ops.clip_sensors = fgcn_clip_sensors' two launches) against the plain row gather
it replaces in ClipBatches' resident path (``index_select``), at the headline batch: 64 rows of the (300, 6) signal and of the
(2, 300, 22, 3) enhanced skeleton (sensor joints 20 and 21) out of ``--samples`` resident ones.  The calls alternate in one process; every
round times ``--inner`` calls of each between device events after a warm-up, with a fresh random set of rows per round, and the result is
the median per call with the spread (min .. max over the rounds).  ``identity``: the same kernel with zero magnitudes and no jitter (the
cost of the pass without the noise's generator blocks); ``minmax``: the one-workgroup-per-clip form of the signal."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

FULL = dict(max_angle=(0.3, 0.3, 0.3), scale=0.1, warp=0.2, warp_knots=4, jitter=(0.05, 0.5), drop=0.1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--samples", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--inner", type=int, default=20)
    args = ap.parse_args()
    from fusion_gcn_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    state = {"idx": torch.randperm(args.samples, generator=g)[:args.batch].to(dev)}
    runs, moved = {}, {}
    for name, shape, joints in (("signal", (300, 6), None), ("skeleton", (2, 300, 22, 3), (20, 22))):
        src = torch.randn(args.samples, *shape, generator=g).to(dev)
        out = torch.empty(args.batch, *shape, device=dev)
        kw = dict(seed=1, epoch=0, joints=joints, out=out)
        moved[name] = 2 * out.numel() * 4                                      # read once, written once
        runs[f"{name}.index_select"] = lambda src=src, out=out: torch.index_select(src, 0, state["idx"], out=out)
        runs[f"{name}.sensors"] = lambda src=src, kw=kw: ops.clip_sensors(src, state["idx"], state["idx"], **FULL, **kw)
        runs[f"{name}.identity"] = lambda src=src, kw=kw: ops.clip_sensors(src, state["idx"], state["idx"], **kw)
        if joints is None:
            runs[f"{name}.minmax"] = lambda src=src, kw=kw: ops.clip_sensors(src, state["idx"], state["idx"], minmax=True, **FULL, **kw)

    def timed(fn) -> float:
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(args.inner):
            fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) * 1e3 / args.inner                    # us per call

    for _ in range(2):                                                        # warm-up: code objects, the allocator
        for fn in runs.values():
            timed(fn)
    t = {name: [] for name in runs}
    for _ in range(args.rounds):                                              # alternating: all see the same machine state
        state["idx"] = torch.randperm(args.samples, generator=g)[:args.batch].to(dev)
        for name, fn in runs.items():
            t[name].append(timed(fn))
    res = {"batch": args.batch, "samples": args.samples, "rounds": args.rounds, "inner": args.inner, "unit": "us per call",
           "mbytes_moved": {k: round(v / 1e6, 3) for k, v in moved.items()}}
    for name in runs:
        med = statistics.median(t[name])
        res[name] = {"median": round(med, 1), "min": round(min(t[name]), 1), "max": round(max(t[name]), 1),
                     "gb_per_s": round(moved[name.split(".")[0]] / med / 1e3, 1)}
    for name in moved:
        res[f"{name}.sensors_over_index_select"] = round(res[f"{name}.sensors"]["median"] / res[f"{name}.index_select"]["median"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
