#!/usr/bin/env python3
"""The preparation of raw inertial recordings (ops.signal_prepare = fgcn_signal_prepare, ops.imu_enhance = fgcn_imu_enhance; DESIGN.md
section 8h) at the UTD-MHAD batch: 64 samples out of ``--samples`` resident ones, recordings of at most 326 frames of 6 values resampled to
skeleton recordings of at most 125 frames, skeletons (1, 125, 20, 3).  Beside each, the plain row gather (``index_select``) of an array of
the OUTPUT's shape, the copy the batch would cost without the preparation.  The three alternate in one process; every round times
``--inner`` calls of each between device events after a warm-up, with a fresh random set of rows per round, and the result is the median
per call with the spread (min .. max over the rounds).  The rate counts the bytes the call has to move: every output value written
once, and every input value it is made of read once (a recording's Ls resampled frames, the skeleton's rows)."""
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
    ap.add_argument("--shape", type=int, nargs=4, default=(1, 125, 20, 3), help="M T V C of the skeleton")
    ap.add_argument("--recording", type=int, nargs=2, default=(326, 6), help="L S of the recording")
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--inner", type=int, default=20)
    args = ap.parse_args()
    from fusion_gcn_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    (M, T, V, C), (L, S) = args.shape, args.recording
    n, b = args.samples, args.batch
    skel = torch.randn(n, M, T, V, C, generator=g).to(dev)
    imu = torch.randn(n, L, S, generator=g).to(dev)
    ls = torch.randint(max(2, T // 3), T + 1, (n,), generator=g, dtype=torch.int32)
    li = torch.randint(max(2, L // 3), L + 1, (n,), generator=g, dtype=torch.int32)
    ls_d, li_d = ls.to(dev), li.to(dev)
    signal_like, enhanced_like = torch.randn(n, T, S, generator=g).to(dev), torch.randn(n, M, T, V + S // 3, 3, generator=g).to(dev)
    out_s, out_e = torch.empty(b, T, S, device=dev), torch.empty(b, M, T, V + S // 3, 3, device=dev)
    state = {}

    def draw():
        rows = torch.randperm(n, generator=g)[:b]
        state["idx"], state["frames"] = rows.to(dev), int(ls[rows].sum())

    draw()
    runs = {
        "signal_prepare": lambda: ops.signal_prepare(imu, state["idx"], li_d, ls_d, T, out=out_s),
        "index_select_signal": lambda: torch.index_select(signal_like, 0, state["idx"], out=out_s),
        "imu_enhance": lambda: ops.imu_enhance(skel, state["idx"], imu, state["idx"], li_d, ls_d, out=out_e),
        "index_select_enhanced": lambda: torch.index_select(enhanced_like, 0, state["idx"], out=out_e),
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
    moved = {name: [] for name in runs}
    for _ in range(args.rounds):                                              # alternating: all see the same machine state
        draw()
        read = state["frames"] * S * 4                                        # the resampled frames of the batch's recordings
        nbytes = {"signal_prepare": out_s.numel() * 4 + read, "index_select_signal": 2 * out_s.numel() * 4,
                  "imu_enhance": out_e.numel() * 4 + b * M * T * V * C * 4 + M * read, "index_select_enhanced": 2 * out_e.numel() * 4}
        for name, fn in runs.items():
            t[name].append(timed(fn))
            moved[name].append(nbytes[name])
    res = {"batch": b, "skeleton": list(args.shape), "recording": list(args.recording), "samples": n, "rounds": args.rounds,
           "inner": args.inner, "unit": "us per call"}
    for name in runs:
        med, mb = statistics.median(t[name]), statistics.median(moved[name])
        res[name] = {"median": round(med, 1), "min": round(min(t[name]), 1), "max": round(max(t[name]), 1), "mbytes_moved": round(mb / 1e6, 3),
                     "gb_per_s": round(mb / med / 1e3, 1)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
