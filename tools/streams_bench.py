#!/usr/bin/env python3
"""The bone / motion streams of a batch (ops.clip_streams = fgcn_clip_streams' one launch) against the torch
composition a user would write without it -- ``index_select`` of the rows, ``index_select`` of the parent joints and a subtraction, two
sliced subtractions padded with a zero frame -- at the headline batch: 64 clips of (2, 300, 25, 3) with NTU RGB+D's parents, all three
derived streams, 11.5 MB read and 34.6 MB written per batch.  Twice: ``resident`` gathers 64 random rows out of ``--samples`` resident
ones, ``streaming`` reads rows 0..63 of a batch-sized buffer, as behind the streaming copy.  The composition gives the same bits without
a valid-frame table (checked here before anything is timed).  The two alternate in one process on the same tensors; every round times
``--inner`` calls of each between device events after a warm-up, with a fresh random set of rows per round, and the result is the median
per call with the spread (min .. max over the rounds)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

DERIVED = ("bone", "motion", "bone_motion")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--samples", type=int, default=512)
    ap.add_argument("--shape", type=int, nargs=4, default=(2, 300, 25, 3))
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--inner", type=int, default=20)
    args = ap.parse_args()
    from fusion_gcn_amd import ops
    from fusion_gcn_amd.data import Streams
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    host_parents = list(Streams.for_dataset("ntu_rgb_d").parents) if args.shape[2] == 25 else [max(v - 1, 0) for v in range(args.shape[2])]
    parents = ops.stream_parents(host_parents, dev)
    parent_idx = parents.long()
    src = torch.randn(args.samples, *args.shape, generator=g).to(dev)
    slot = src[:args.batch].clone()
    out = {s: torch.empty(args.batch, *args.shape, device=dev) for s in DERIVED}
    state = {"idx": torch.randperm(args.samples, generator=g)[:args.batch].to(dev)}
    slot_rows = torch.arange(args.batch, device=dev)

    def composed(x, idx):
        x = x.index_select(0, idx)
        bone = x - x.index_select(3, parent_idx)
        return {"bone": bone, "motion": F.pad(x[:, :, 1:] - x[:, :, :-1], (0, 0, 0, 0, 0, 1)),
                "bone_motion": F.pad(bone[:, :, 1:] - bone[:, :, :-1], (0, 0, 0, 0, 0, 1))}

    runs = {
        "resident": lambda: ops.clip_streams(src, state["idx"], parents, streams=DERIVED, out=out),
        "resident_torch": lambda: composed(src, state["idx"]),
        "streaming": lambda: ops.clip_streams(slot, slot_rows, parents, streams=DERIVED, out=out),
        "streaming_torch": lambda: composed(slot, slot_rows),
    }
    for ours, theirs in (("resident", "resident_torch"), ("streaming", "streaming_torch")):      # the same bits, or the times compare nothing
        want = runs[theirs]()
        got = runs[ours]()
        torch.cuda.synchronize()
        for s in DERIVED:
            assert torch.equal(got[s].view(torch.int32), want[s].contiguous().view(torch.int32)), (ours, s)

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
    nbytes = (1 + len(DERIVED)) * out["bone"].numel() * 4                     # the rows read once, three streams written once
    res = {"shape": [args.batch, *args.shape], "samples": args.samples, "streams": list(DERIVED), "rounds": args.rounds, "inner": args.inner,
           "unit": "us per call", "mbytes_moved": round(nbytes / 1e6, 2)}
    for name in runs:
        med = statistics.median(t[name])
        res[name] = {"median": round(med, 1), "min": round(min(t[name]), 1), "max": round(max(t[name]), 1)}
        if not name.endswith("_torch"):
            res[name]["gb_per_s"] = round(nbytes / med / 1e3, 1)
    res["resident_torch_over_ours"] = round(res["resident_torch"]["median"] / res["resident"]["median"], 2)
    res["streaming_torch_over_ours"] = round(res["streaming_torch"]["median"] / res["streaming"]["median"], 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
