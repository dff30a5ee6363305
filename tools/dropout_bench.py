#!/usr/bin/env python3
"""fops.dropout (fgcn_dropout_fwd + fgcn_rng_advance, fgcn_dropout_bwd) against torch.nn.functional.dropout,
forward + backward, on the (B, V, O) tensor the IMU graph convolution drops in tools/imu_gcn_bench.py's default layer (batch 8,
326 x 6 = 1956 nodes, width 512): the two alternate in one process, every round times ``--inner`` forward + backward pairs of each
between device events after a warm-up -- enqueued from Python (``ours`` / ``torch``: the host's enqueue rate counts) and replayed from a
HIP graph of the same pairs (``*_graph``: device time) -- and the result is the median per pair with the spread (min .. max over the rounds).
Bytes per element: ours 4 + 4 + 1/8 forward and backward (the kept bits are an image), torch's 4 + 4 + 1 (a bool mask).

``--launches``: instead, the C-ABI calls of one training step of a small IMU graph model without dropout, by entry point -- the
launch record to compare between two trees (``dropout=0`` takes the calls it always took)."""
import argparse
import collections
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def count_calls(fn) -> dict:
    """{entry point: calls} of libfgcn while ``fn`` runs (every call of a launcher is one launch or a fixed few)."""
    from fusion_gcn_amd import _lib
    lib = _lib.load()
    counts = collections.Counter()
    saved = {}
    for name in _lib.SIGNATURES:
        orig = getattr(lib, name)
        saved[name] = orig

        def wrapper(*args, _orig=orig, _name=name):
            counts[_name] += 1
            return _orig(*args)
        setattr(lib, name, wrapper)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        for name, orig in saved.items():
            setattr(lib, name, orig)
    quiet = ("fgcn_last_error", "fgcn_get_math_mode", "fgcn_get_products", "fgcn_set_products", "fgcn_get_tuning", "fgcn_ctx_get_current")
    return {k: v for k, v in sorted(counts.items()) if k not in quiet}


def launches(args):
    from fusion_gcn_amd import ops
    from fusion_gcn_amd.models.mmargcn.mmargcn import Model
    dev = torch.device("cuda:0")
    out = {}
    for sparse in (False, True):
        torch.manual_seed(1)
        model = Model({"inertial": (40, 6)}, 27, None, mode="imu_gcn", gc_model="stgcn", graph_node_format="node_per_value",
                      inner_feature_dim=64, num_layers=5, sparse=sparse).to(dev).train()
        x, y = torch.randn(4, 40, 6, device=dev), torch.randint(0, 27, (4,), device=dev)

        def step():
            for p in model.parameters():
                p.grad = None
            F.cross_entropy(model(x), y).backward()
        with ops.math_mode("bf16x3"):
            step()                                                           # (lazily built forms)
            calls = count_calls(step)
        out["sparse" if sparse else "dense"] = {"total": sum(calls.values()), "calls": calls}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--nodes", type=int, default=326 * 6)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--p", type=float, default=0.3)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--launches", action="store_true")
    args = ap.parse_args()
    if args.launches:
        return launches(args)
    from fusion_gcn_amd import fops
    dev = torch.device("cuda:0")
    shape = (args.batch, args.nodes, args.width)
    x = torch.randn(shape, device=dev, requires_grad=True)
    g = torch.randn(shape, device=dev)
    drop = fops.FusedDropout(args.p).to(dev)
    drop.reseed(1)

    def ours():
        return torch.autograd.grad(fops.dropout(x, drop, args.p, True), x, g)[0]

    def torchs():
        return torch.autograd.grad(F.dropout(x, args.p, True), x, g)[0]

    def timed(run) -> float:
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        run()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) * 1e3 / args.inner                   # us per forward + backward

    def loop(fn):
        def run():
            for _ in range(args.inner):
                fn()
        return run

    def recorded(fn):
        """the same `inner` pairs as one HIP graph: device time, without the host's enqueue rate"""
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            loop(fn)()
        return graph.replay

    # "stream": enqueued pair by pair from Python (ours: three ctypes calls and an autograd Function per pair); "graph": replayed
    runs = {"ours": loop(ours), "torch": loop(torchs)}
    for name in ("ours", "torch", "ours", "torch"):                           # warm-up: code objects, allocator, autograd, the seed
        timed(runs[name])
    torch.cuda.synchronize()
    runs.update({"ours_graph": recorded(ours), "torch_graph": recorded(torchs)})
    for name in ("ours_graph", "torch_graph"):
        timed(runs[name])
    t = {name: [] for name in runs}
    for _ in range(args.rounds):                                              # alternating: all see the same machine state
        for name, run in runs.items():
            t[name].append(timed(run))
    n = x.numel()
    out = {"shape": list(shape), "p": args.p, "rounds": args.rounds, "inner": args.inner, "unit": "us per forward + backward"}
    for name in runs:
        med = statistics.median(t[name])
        bytes_per_elem = 2 * (8.125 if name.startswith("ours") else 9.0)
        out[name] = {"median": round(med, 1), "min": round(min(t[name]), 1), "max": round(max(t[name]), 1),
                     "gb_per_s": round(n * bytes_per_elem / med / 1e3, 1)}
    out["ours_over_torch"] = {"stream": round(out["ours"]["median"] / out["torch"]["median"], 3),
                              "graph": round(out["ours_graph"]["median"] / out["torch_graph"]["median"], 3)}
    out["steps_drawn"] = int(drop.step.view(torch.int64).item())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
