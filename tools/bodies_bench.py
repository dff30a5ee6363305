#!/usr/bin/env python3
"""The body selection (ops.clip_bodies = fgcn_clip_bodies's two launches) on 1024 clips of (4, 300, 25, 3), the two most
energetic bodies kept, beside ops.clip_normalize (an existing pair of kernels with the same access shape: one that reads every body to plan,
one that gathers) on the same rows in the same process.  The source looks like raw NTU RGB+D recordings: every clip ends in a random number
of null frames, the bodies of a clip differ in amplitude, and every second clip has no third and fourth body.  The two alternate; every
round times ``--inner`` calls of each between device events after a warm-up, and the result is the median per call with the spread (min ..
max over the rounds).  The effective bandwidth counts what the call has to move: ``src`` read once plus ``out`` written once (the selection
reads the source a second time in its score kernel, from L2 where it is lucky, and the kept bodies a third time in its gather).  The numpy
restatement (tests/bodies_ref.py) is timed on the host for the same clips.

The two kernels apart: device events cannot separate the launches of one call, so their times come from a run of their own,

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o bodies -- python3 tools/bodies_bench.py --rounds 3
    python3 tools/bodies_bench.py --kernel-stats DIR/.../bodies_kernel_stats.csv

The second command prints the average time per launch of the four kernels and the bandwidth each reaches on the bytes it has to read and
write once."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def kernel_stats(path: str, clips: int, shape, keep: int) -> dict:
    """the rows of a rocprofv3 kernel-stats file that belong to the two stages, with the bytes each kernel has to move once"""
    Mr, T, V, C = shape
    src = clips * Mr * T * V * C * 4
    moved = {"bodies_score_kernel": src, "bodies_gather_kernel": 2 * src * keep // Mr, "normalize_plan_kernel": src, "normalize_apply_kernel": 2 * src}
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            for name, nbytes in moved.items():
                if name in row["Name"]:
                    us = float(row["AverageNs"]) / 1e3
                    out[name] = {"calls": int(row["Calls"]), "average_us": round(us, 1), "min_us": round(float(row["MinNs"]) / 1e3, 1),
                                 "max_us": round(float(row["MaxNs"]) / 1e3, 1), "mbytes_moved": round(nbytes / 1e6, 1), "gb_per_s": round(nbytes / us / 1e3, 1)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--shape", type=int, nargs=4, default=(4, 300, 25, 3))
    ap.add_argument("--keep", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--no-host", action="store_true", help="skip the numpy restatement")
    ap.add_argument("--kernel-stats", help="a rocprofv3 *_kernel_stats.csv of a run of this tool: print the kernels' times and stop")
    args = ap.parse_args()
    if args.kernel_stats:
        print(json.dumps(kernel_stats(args.kernel_stats, args.clips, args.shape, args.keep)))
        return
    import torch
    from fusion_gcn_amd import ops
    from fusion_gcn_amd.data import Normalize
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    Mr, T, V, C = args.shape
    n = args.clips
    amp = torch.rand(n, Mr, generator=g) * 0.18 + 0.02
    host = 3.0 + amp[:, :, None, None, None] * (torch.rand(n, Mr, T, V, C, generator=g) * 2.5 + 0.5)
    length = torch.randint(T // 4, T + 1, (n,), generator=g)
    host *= (torch.arange(T)[None, :] < length[:, None]).float()[:, None, :, None, None]
    if Mr > 2:
        host[1::2, 2:] = 0
    src = host.to(dev)
    idx = torch.randperm(n, generator=g).to(dev)
    out_b = torch.empty(n, args.keep, T, V, C, device=dev)
    out_n = torch.empty(n, Mr, T, V, C, device=dev)
    z = Normalize.for_dataset("ntu_rgb_d")
    pairs = dict(z_axis_joints=z.z_axis_joints, x_axis_joints=z.x_axis_joints) if C == 3 and V > 8 else {}
    runs = {
        "bodies": (lambda: ops.clip_bodies(src, idx, bodies=args.keep, out=out_b), (src.numel() + out_b.numel()) * 4),
        "normalize": (lambda: ops.clip_normalize(src, idx, origin_joint=z.origin_joint if V > z.origin_joint else 0, out=out_n, **pairs),
                      (src.numel() + out_n.numel()) * 4),
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
        for fn, _ in runs.values():
            timed(fn)
    t = {name: [] for name in runs}
    for _ in range(args.rounds):                                              # alternating: both see the same machine state
        for name, (fn, _) in runs.items():
            t[name].append(timed(fn))
    res = {"clips": n, "shape": list(args.shape), "keep": args.keep, "rounds": args.rounds, "inner": args.inner, "unit": "us per call"}
    for name, (_, nbytes) in runs.items():
        med = statistics.median(t[name])
        res[name] = {"median": round(med, 1), "min": round(min(t[name]), 1), "max": round(max(t[name]), 1), "mbytes_moved": round(nbytes / 1e6, 1),
                     "gb_per_s": round(nbytes / med / 1e3, 1)}
    res["bodies_over_normalize_gb_per_s"] = round(res["bodies"]["gb_per_s"] / res["normalize"]["gb_per_s"], 3)
    if not args.no_host:
        import bodies_ref
        clips = host[idx.cpu()].numpy()
        t0 = time.perf_counter()
        want = [bodies_ref.order(bodies_ref.scores(x)) for x in clips]
        res["numpy_restatement_s"] = round(time.perf_counter() - t0, 3)
        order = ops.clip_bodies(src, idx, bodies=args.keep, out=out_b)[1].cpu().numpy()
        res["orders_equal"] = bool((order == want).all())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
