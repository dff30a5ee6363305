#!/usr/bin/env python3
"""The stream-weight search of a score-fusion ensemble (ops.fuse_sweep = fgcn_fuse_sweep) against the torch
composition a user would write without it: per candidate, the weighted sum of the stacked scores, then ``argmax`` / ``topk`` counts.
Headline: N = 16384 samples, 60 classes, S = 4 streams, ``simplex_grid(4, 20)`` = 1771 candidates, k = 5.

Before anything is timed the kernel's counts are asserted equal to a float64 torch composition that ranks by the header's own rule
(``#{fused > fused_y} + #{j < y: fused_j == fused_y}``), candidate by candidate.  The scores are built so that float64 is exact there: every
value is a multiple of 2^-16 below 16 (20 bits) and the values of a row are distinct, the weights are float32 -- each product has at most
44 bits and each sum of four at most 47, exact in float64 in any order, so that composition rounds the same number to float32 as the
kernel does.  The two TIMED compositions use ``argmax`` / ``topk``: ``torch_f64`` on the same float64 sum, ``torch_f32`` in float32, which
a user would more likely write.  Two distinct sums can round to one float32, and ``topk`` leaves the order of equal values open, so for
these two the number of candidates whose counts differ from the kernel's is reported, not asserted.
All three alternate in one process on the same tensors; every round times ``inner`` calls of each between device events after a
warm-up; the result is the median per call with the spread (min .. max over the rounds)."""
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
    ap.add_argument("--samples", type=int, default=16384)
    ap.add_argument("--classes", type=int, default=60)
    ap.add_argument("--streams", type=int, default=4)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    from fusion_gcn_amd import ops
    from fusion_gcn_amd.ensemble import best_candidate, simplex_grid
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    N, C, S, k = args.samples, args.classes, args.streams, args.k
    # distinct 20-bit values per row: the upper bits are a permutation of the classes (C <= 64), the lower 14 bits random
    assert C <= 64
    upper = torch.rand(S, N, C, generator=g).argsort(dim=-1)
    lower = torch.randint(0, 1 << 14, (S, N, C), generator=g)
    host = ((upper << 14) + lower).to(torch.float32) / 65536.0
    scores = [host[s].to(dev) for s in range(S)]
    labels = torch.randint(0, C, (N,), generator=g).to(dev)
    grid = torch.from_numpy(simplex_grid(S, args.steps)).to(torch.float32)
    cand = grid.to(dev)
    G = cand.shape[0]
    stack32 = torch.stack(scores)
    stack64 = stack32.double()
    cand64 = cand.double()

    def ours():
        return ops.fuse_sweep(scores, cand, labels, k)[0]

    def composed(stack, weights):
        hits = torch.zeros((G, 2), dtype=torch.int64, device=dev)
        for i in range(G):
            fused = (weights[i].view(S, 1, 1) * stack).sum(0).float()
            hits[i, 0] = (fused.argmax(1) == labels).sum()
            hits[i, 1] = (fused.topk(k, dim=1).indices == labels[:, None]).any(1).sum()
        return hits

    def by_the_rule():
        hits = torch.zeros((G, 2), dtype=torch.int64, device=dev)
        col, rows = torch.arange(C, device=dev)[None, :], torch.arange(N, device=dev)
        for i in range(G):
            fused = (cand64[i].view(S, 1, 1) * stack64).sum(0).float()
            fy = fused[rows, labels][:, None]
            rank = (fused > fy).sum(1) + ((fused == fy) & (col < labels[:, None])).sum(1)
            hits[i, 0], hits[i, 1] = (rank == 0).sum(), (rank < k).sum()
        return hits

    runs = {"fuse_sweep": ours, "torch_f64": lambda: composed(stack64, cand64), "torch_f32": lambda: composed(stack32, cand)}
    got = {name: fn().cpu() for name, fn in runs.items()}
    assert torch.equal(got["fuse_sweep"], by_the_rule().cpu()), "the kernel and the float64 composition by the header's rule count differently"
    differs = {name: int((got[name] != got["fuse_sweep"]).any(1).sum()) for name in ("torch_f64", "torch_f32")}

    def timed(fn, inner) -> float:
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(inner):
            fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) / inner                    # ms per call

    inner = {"fuse_sweep": args.inner, "torch_f64": 1, "torch_f32": 1}
    for name, fn in runs.items():                                  # warm-up: code objects, the allocator
        timed(fn, inner[name])
    t = {name: [] for name in runs}
    for _ in range(args.rounds):                                   # alternating: all see the same machine state
        for name, fn in runs.items():
            t[name].append(timed(fn, inner[name]))
    res = {"samples": N, "classes": C, "streams": S, "candidates": G, "k": k, "rounds": args.rounds, "inner": inner, "unit": "ms per call",
           "best_candidate": grid[best_candidate(got["fuse_sweep"].numpy())].tolist(), "candidates_whose_counts_differ": differs}
    for name in runs:
        res[name] = {"median": round(statistics.median(t[name]), 3), "min": round(min(t[name]), 3), "max": round(max(t[name]), 3)}
    res["torch_f64_over_fuse_sweep"] = round(res["torch_f64"]["median"] / res["fuse_sweep"]["median"], 1)
    res["torch_f32_over_fuse_sweep"] = round(res["torch_f32"]["median"] / res["fuse_sweep"]["median"], 1)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
