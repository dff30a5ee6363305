#!/usr/bin/env python3
"""The windowed batch gather (ops.clip_window = fgcn_clip_window's two launches) against the plain row gather it
replaces in ClipBatches' resident path (``index_select``), at the headline batch: 64 clips of (2, 300, 25, 3) out of ``--samples``
resident ones, resized to ``--window`` frames -- so the window writes ``window / 300`` of what the gather writes -- and the count of the
same rows' valid frames (ops.clip_valid_frames, one launch; the split is counted once, not per batch).  They alternate in one process;
every round times ``--inner`` calls of each between device events after a warm-up, with a fresh random set of rows per round, and the
result is the median per call with the spread (min .. max over the rounds).  ``centre``: the same kernel without random numbers (the
evaluation form).  The clips hold 60 to 120 valid frames, as NTU recordings do, and zeros behind them."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402


def step_times(args, dev):
    """``--step``: what the window buys.  The benchmark's training step (bench.py: the NTU two-stream AGCN, ``--batch`` clips, the library's
    default arithmetic, forward + backward with the packed weights rebuilt, captured once into a HIP graph and replayed) with the model built
    for each frame count of ``--frames``; the graphs alternate in one process, ``--rounds`` rounds of ``--inner`` replays between device events."""
    from fusion_gcn_amd import ops
    from fusion_gcn_amd.datasets.ntu_rgb_d import constants as ntu
    from fusion_gcn_amd.dp import FlatGradients
    from fusion_gcn_amd.loss import cross_entropy
    from fusion_gcn_amd.models.mmargcn.agcn import Model
    from fusion_gcn_amd.util import Graph
    ops.set_math_mode("bf16x3")
    M, _, V, C = args.shape
    graphs, keep = {}, []
    for T in args.frames:
        torch.manual_seed(1)
        model = Model((M, T, V, C), 60, Graph(ntu.skeleton_edges, center_joint=ntu.center_joint))
        with torch.no_grad():
            for n, p in model.named_parameters():
                if n.endswith("gcn1.bn.weight"):
                    p.fill_(1.0)
        model = model.to(dev).train()
        grads = FlatGradients(model.parameters())
        g = torch.Generator().manual_seed(1)
        x, y = torch.randn(args.batch, M, T, V, C, generator=g).to(dev), torch.randint(0, 60, (args.batch,), generator=g).to(dev)

        def fwd_bwd(model=model, x=x, y=y):
            for m in model.modules():
                if hasattr(m, "mark_packed_stale"):
                    m.mark_packed_stale()
            loss = cross_entropy(model(x), y)
            loss.backward()
            return loss

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                grads.zero()
                eager = fwd_bwd()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        eager = float(eager.detach())
        graph = torch.cuda.CUDAGraph()
        grads.zero()
        with torch.cuda.graph(graph):
            static_loss = fwd_bwd()
        graph.replay()
        torch.cuda.synchronize()
        if abs(float(static_loss.detach()) - eager) > 1e-4 * max(1.0, abs(eager)):
            raise SystemExit(f"T={T}: graph replay loss {float(static_loss.detach())} != eager loss {eager}")
        graphs[T] = graph
        keep.append((model, grads, x, y, static_loss))

    def timed(graph) -> float:
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(args.inner):
            graph.replay()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) / args.inner                          # ms per step

    for graph in graphs.values():
        timed(graph)
    t = {T: [] for T in graphs}
    for _ in range(args.rounds):
        for T, graph in graphs.items():
            t[T].append(timed(graph))
    res = {"step": "fwd+bwd, hipgraph, bf16x3", "clips": args.batch, "rounds": args.rounds, "inner": args.inner, "unit": "ms per step"}
    for T in graphs:
        med = statistics.median(t[T])
        res[f"T={T}"] = {"median": round(med, 2), "min": round(min(t[T]), 2), "max": round(max(t[T]), 2), "clips_per_s": round(args.batch / med * 1e3, 1)}
    first = res[f"T={args.frames[0]}"]["median"]
    res["speedup_over_first"] = {f"T={T}": round(first / res[f"T={T}"]["median"], 2) for T in graphs}
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--samples", type=int, default=512)
    ap.add_argument("--shape", type=int, nargs=4, default=(2, 300, 25, 3))
    ap.add_argument("--window", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--step", action="store_true", help="time the training step of models built for --frames instead of the kernels")
    ap.add_argument("--frames", type=int, nargs="+", default=(300, 100, 64))
    args = ap.parse_args()
    from fusion_gcn_amd import ops
    dev = torch.device("cuda:0")
    if args.step:
        return step_times(args, dev)
    g = torch.Generator().manual_seed(1)
    M, T, V, C = args.shape
    src = torch.randn(args.samples, *args.shape, generator=g)
    frames = torch.randint(min(60, T), min(120, T) + 1, (args.samples,), generator=g)
    src *= (torch.arange(T)[None, :] < frames[:, None]).to(src.dtype)[:, None, :, None, None]      # zero behind the recording
    src = src.to(dev)
    valid = ops.clip_valid_frames(src)
    assert valid.cpu().tolist() == frames.tolist()
    gathered = torch.empty(args.batch, *args.shape, device=dev)
    out = torch.empty(args.batch, M, args.window, V, C, device=dev)
    state = {"idx": torch.randperm(args.samples, generator=g)[:args.batch].to(dev)}
    kw = dict(window=args.window, interval=(0.5, 1.0), seed=1, epoch=0, valid=valid, out=out)

    runs = {
        "index_select": lambda: torch.index_select(src, 0, state["idx"], out=gathered),
        "window": lambda: ops.clip_window(src, state["idx"], state["idx"], mode="random", **kw),
        "centre": lambda: ops.clip_window(src, state["idx"], None, mode="centre", **kw),
        "valid_frames": lambda: ops.clip_valid_frames(src, state["idx"]),
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
    # bytes moved: the gather reads and writes the rows; the window reads at most the rows' valid frames and writes W frames; the count reads the rows
    moved = {"index_select": 2 * gathered.numel() * 4, "window": out.numel() * 4 * 2, "centre": out.numel() * 4 * 2, "valid_frames": gathered.numel() * 4}
    res = {"shape": [args.batch, *args.shape], "window_frames": args.window, "samples": args.samples, "rounds": args.rounds, "inner": args.inner,
           "unit": "us per call"}
    for name in runs:
        med = statistics.median(t[name])
        res[name] = {"median": round(med, 1), "min": round(min(t[name]), 1), "max": round(max(t[name]), 1),
                     "mbytes_moved": round(moved[name] / 1e6, 2), "gb_per_s": round(moved[name] / med / 1e3, 1)}
    res["window_over_index_select"] = round(res["window"]["median"] / res["index_select"]["median"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
