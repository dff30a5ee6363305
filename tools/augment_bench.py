#!/usr/bin/env python3
"""The augmented batch gather (ops.clip_augment = fgcn_clip_augment's two launches) against the plain row gather
it replaces in ClipBatches' resident path (``index_select``), at the headline batch: 64 clips of (2, 300, 25, 3) out of ``--samples``
resident ones, 11.5 MB read and written per batch.  The two alternate in one process; every round times ``--inner`` calls of each between
device events after a warm-up, with a fresh random set of rows per round, and the result is the median per call with the spread
(min .. max over the rounds).  ``identity``: the same kernel with zero magnitudes (the cost of the pass without a rotation to apply)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--samples", type=int, default=512)
    ap.add_argument("--shape", type=int, nargs=4, default=(2, 300, 25, 3))
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--inner", type=int, default=20)
    args = ap.parse_args()
    from fusion_gcn_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    src = torch.randn(args.samples, *args.shape, generator=g).to(dev)
    out = torch.empty(args.batch, *args.shape, device=dev)
    state = {"idx": torch.randperm(args.samples, generator=g)[:args.batch].to(dev)}
    kw = dict(seed=1, epoch=0, joints=(0, args.shape[2]) if args.shape[3] == 3 else None)

    runs = {
        "index_select": lambda: torch.index_select(src, 0, state["idx"], out=out),
        "augment": lambda: ops.clip_augment(src, state["idx"], state["idx"], max_angle=(0.3, 0.3, 0.3), scale=0.1, min_window=0.5, out=out, **kw),
        "identity": lambda: ops.clip_augment(src, state["idx"], state["idx"], out=out, **kw),
    }

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
    nbytes = 2 * out.numel() * 4                                              # read once (f0 and f1 share cache lines), written once
    res = {"shape": [args.batch, *args.shape], "samples": args.samples, "rounds": args.rounds, "inner": args.inner, "unit": "us per call",
           "mbytes_moved": round(nbytes / 1e6, 2)}
    for name in runs:
        med = statistics.median(t[name])
        res[name] = {"median": round(med, 1), "min": round(min(t[name]), 1), "max": round(max(t[name]), 1), "gb_per_s": round(nbytes / med / 1e3, 1)}
    res["augment_over_index_select"] = round(res["augment"]["median"] / res["index_select"]["median"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
