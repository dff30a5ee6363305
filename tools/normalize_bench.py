#!/usr/bin/env python3
"""The normalising batch gather (ops.clip_normalize = fgcn_clip_normalize's two launches) against the plain row
gather of the same rows (``index_select``), at the headline batch: 64 clips of (2, 300, 25, 3) out of ``--samples`` resident ones, 11.5 MB
read and written per batch by the copy.  The source looks like raw NTU RGB+D recordings: every clip ends in a random number of null
frames, and every second clip has no second body.  The two alternate in one process; every round times ``--inner`` calls of each between
device events after a warm-up, with a fresh random set of rows per round, and the result is the median per call with the spread
(min .. max over the rounds).  ``centre_only``: the same kernels without an axis pair (no rotation to form or to apply).  The rate
counts the bytes a gather has to move -- every row read once and written once -- for all three; the two-launch form reads the source a
second time in its plan kernel."""
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
    from fusion_gcn_amd.data import Normalize
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    M, T, V, C = args.shape
    src = torch.rand(args.samples, M, T, V, C, generator=g) * 2.5 + 0.5
    length = torch.randint(T // 4, T + 1, (args.samples,), generator=g)
    src *= (torch.arange(T)[None, :] < length[:, None]).float()[:, None, :, None, None]
    if M > 1:
        src[1::2, 1:] = 0
    src = src.to(dev)
    out = torch.empty(args.batch, *args.shape, device=dev)
    state = {"idx": torch.randperm(args.samples, generator=g)[:args.batch].to(dev)}
    z = Normalize.for_dataset("ntu_rgb_d")
    pairs = dict(z_axis_joints=z.z_axis_joints, x_axis_joints=z.x_axis_joints) if C == 3 and V > 8 else {}

    runs = {
        "index_select": lambda: torch.index_select(src, 0, state["idx"], out=out),
        "normalize": lambda: ops.clip_normalize(src, state["idx"], origin_joint=z.origin_joint, out=out, **pairs),
        "centre_only": lambda: ops.clip_normalize(src, state["idx"], origin_joint=z.origin_joint, out=out),
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
    nbytes = 2 * out.numel() * 4                                              # every row read once, written once
    res = {"shape": [args.batch, *args.shape], "samples": args.samples, "rounds": args.rounds, "inner": args.inner, "unit": "us per call",
           "mbytes_moved": round(nbytes / 1e6, 2)}
    for name in runs:
        med = statistics.median(t[name])
        res[name] = {"median": round(med, 1), "min": round(min(t[name]), 1), "max": round(max(t[name]), 1), "gb_per_s": round(nbytes / med / 1e3, 1)}
    res["normalize_over_index_select"] = round(res["normalize"]["median"] / res["index_select"]["median"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
