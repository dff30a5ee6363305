"""Times the loss kernels alone on one MI355X: ``fgcn_ce_fwd`` / ``fgcn_ce_bwd`` (torch's CrossEntropyLoss arguments; here weight +
label_smoothing 0.1, mean reduction, int64 labels) beside the plain ``fgcn_cross_entropy_fwd`` / ``_bwd`` at the same shapes, through
the C ABI on preallocated buffers (no allocation, no Python wrapper inside the timed window).

Per shape and call two figures in microseconds per call: ``stream`` = HIP events around 200 back-to-back launches on the current stream
after 20 warm-up launches (what a caller that enqueues them one by one sees; at these sizes it is bounded by the host's enqueue rate),
``graph`` = the same 200 launches recorded once into a HIP graph, events around one replay (the device time of the launches
themselves).  The fgcn_ce_fwd figures include its second, one-workgroup launch.  Prints one JSON line.

    python tools/loss_bench.py [--shapes 64x60,4096x1000] [--reps 200] [--warmup 20]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    stream_us = 1e3 * t0.elapsed_time(t1) / reps
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        for _ in range(reps):
            fn()
    graph.replay()
    torch.cuda.synchronize()
    t0.record()
    graph.replay()
    t1.record()
    torch.cuda.synchronize()
    return {"stream_us": round(stream_us, 2), "graph_us": round(1e3 * t0.elapsed_time(t1) / reps, 2)}


def measure(rows, classes, reps, warmup):
    from fusion_gcn_amd import _lib, ops
    from fusion_gcn_amd._lib import check
    ops.ensure_device()
    lib, dev = _lib.load(), torch.device("cuda:0")
    torch.manual_seed(rows + classes)
    f32 = dict(device=dev, dtype=torch.float32)
    z = torch.randn(rows, classes, **f32) * 3
    y = torch.randint(0, classes, (rows,), device=dev)
    w = torch.rand(classes, **f32) + 0.1
    probs, dl = torch.empty(rows, classes, **f32), torch.empty(rows, classes, **f32)
    row_loss, row_scale, loss, dloss = torch.empty(rows, **f32), torch.empty(rows, **f32), torch.empty(2, **f32), torch.ones(1, **f32)
    work = torch.empty(lib.fgcn_ce_workspace_bytes(rows) // 8, device=dev, dtype=torch.float64)
    p = lambda t: t.data_ptr()      # noqa: E731
    s = lambda: torch.cuda.current_stream().cuda_stream      # noqa: E731
    calls = {
        "cross_entropy_fwd": lambda: check(lib.fgcn_cross_entropy_fwd(p(z), p(y), p(probs), p(row_loss), p(loss), rows, classes, classes, s()),
                                           "fgcn_cross_entropy_fwd"),
        "cross_entropy_bwd": lambda: check(lib.fgcn_cross_entropy_bwd(p(probs), p(y), p(loss), p(dloss), p(dl), rows, classes, classes, s()),
                                           "fgcn_cross_entropy_bwd"),
        "ce_fwd": lambda: check(lib.fgcn_ce_fwd(p(z), p(y), None, p(w), p(probs), p(row_loss), p(row_scale), p(loss), p(work), rows, classes,
                                                classes, 0, -100, 0.1, 0, s()), "fgcn_ce_fwd"),
        "ce_bwd": lambda: check(lib.fgcn_ce_bwd(p(probs), p(y), None, p(w), p(row_scale), p(loss), p(dloss), p(dl), rows, classes, 0, classes,
                                                -100, 0.1, 0, s()), "fgcn_ce_bwd"),
    }
    return {"rows": rows, "classes": classes, **{name: timed(fn, reps, warmup) for name, fn in calls.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="64x60,4096x1000")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loss_bench: no GPU (a time is a GPU run or nothing)")
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup,
           "shapes": [measure(r, c, args.reps, args.warmup) for r, c in shapes]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
