#!/usr/bin/env python3
"""The STC attention module's kernels (fgcn_stc.hip) at the two ends of the headline step -- (128, 300, 25, 64), the
first four blocks' activation, and (128, 75, 25, 256), the last three's: the three forward passes over G (mean over frames, mean over joints,
the gated store), the three backward passes (q / r, the joint sums of dm G, the gradient store), and the five small launches between them as
one figure each way.  They alternate in one process; every round times ``--inner`` calls of each between device events after a warm-up,
and the result is the median per call with the spread and the bytes each pass moves to and from HBM.

``--step``: the benchmark's 64-clip training step (bench.py: the NTU AGCN, the library's default arithmetic, forward + backward with the
packed weights rebuilt, captured once into a HIP graph and replayed) with and without ``attention=True``, alternating in one process."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402


def timed(fn, inner: int) -> float:
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(inner):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / inner                                   # ms per call


def alternate(runs: dict, rounds: int, inner: int) -> dict:
    for _ in range(2):                                                        # warm-up: code objects, the allocator
        for fn in runs.values():
            timed(fn, inner)
    t = {name: [] for name in runs}
    for _ in range(rounds):                                                   # alternating: all see the same machine state
        for name, fn in runs.items():
            t[name].append(timed(fn, inner))
    return t


def step_times(args, dev):
    from fusion_gcn_amd import ops
    from fusion_gcn_amd.datasets.ntu_rgb_d import constants as ntu
    from fusion_gcn_amd.dp import FlatGradients
    from fusion_gcn_amd.loss import cross_entropy
    from fusion_gcn_amd.models.mmargcn.agcn import Model
    from fusion_gcn_amd.util import Graph
    ops.set_math_mode("bf16x3")
    M, T, V, C = 2, 300, 25, 3
    graphs, keep = {}, []
    for attention in (False, True):
        torch.manual_seed(1)
        model = Model((M, T, V, C), 60, Graph(ntu.skeleton_edges, center_joint=ntu.center_joint), attention=attention)
        with torch.no_grad():
            for n, p in model.named_parameters():
                if n.endswith("gcn1.bn.weight"):
                    p.fill_(1.0)
                if ".conv_ta." in n or ".fc2c." in n:                         # (zero at initialisation: a trained model's are not)
                    p.normal_(0, 0.05)
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
            raise SystemExit(f"attention={attention}: graph replay loss {float(static_loss.detach())} != eager loss {eager}")
        graphs["attention" if attention else "plain"] = graph
        keep.append((model, grads, x, y, static_loss))
    t = alternate({name: graph.replay for name, graph in graphs.items()}, args.rounds, args.inner)
    res = {"step": "fwd+bwd, hipgraph, bf16x3", "clips": args.batch, "rounds": args.rounds, "inner": args.inner, "unit": "ms per step"}
    for name in graphs:
        med = statistics.median(t[name])
        res[name] = {"median": round(med, 2), "min": round(min(t[name]), 2), "max": round(max(t[name]), 2), "clips_per_s": round(args.batch / med * 1e3, 1)}
    res["attention_adds_ms"] = round(res["attention"]["median"] - res["plain"]["median"], 2)
    print(json.dumps(res))


def kernel_times(args, dev, shape):
    from fusion_gcn_amd import _lib, ops
    B, T, V, C = shape
    gen = torch.Generator().manual_seed(1)
    g = torch.randn(shape, generator=gen).relu_().to(dev)
    dout = torch.randn(shape, generator=gen).to(dev)
    params = [(0.1 * torch.randn(s, generator=gen)).to(dev) for s in ops.stc_param_shapes(C, V)]
    w_sa, b_sa, w_ta, b_ta, w1, b1, w2, b2 = params
    out, S = ops.stc_forward(g, params)
    dg = torch.empty_like(g)
    ops.stc_backward(dout, g, S, params, out=dg)
    q, _ = ops.stc_bwd_qr(dout, g, S["s"], S["tg"])
    dm, dmt = torch.randn(B, T, C, generator=gen).to(dev), torch.randn(B, V, C, generator=gen).to(dev)
    lib, p, st = _lib.load(), ops._p, ops._stream
    new = lambda *s: torch.empty(s, device=dev)  # noqa: E731
    k = ops.stc_sa_kernel(V)
    ns = lib.fgcn_stc_splits(B, T)
    small = dict(dzc=new(B, C), dhpre=new(B, C // 2), dcm=new(B, C), dzt=new(B, T), dm=new(B, T, C), dwta=new(B, C, 9), dbta=new(B), dzs=new(B, V),
                 dmt=new(B, V, C), dwsa=new(B, C, k), dbsa=new(B), rpart=torch.zeros(B, ns, V, C, device=dev), dspart=torch.zeros(B, ns, V, device=dev))
    pgrads = [torch.empty_like(t) for t in params]

    def small_fwd():
        s = ops.stc_gate_s(S["mt"], w_sa, b_sa)
        ops.stc_gates_tc(S["m"], w_ta, b_ta, w1, b1, w2, b2)
        return s

    def small_bwd():
        d = small
        lib.fgcn_stc_bwd_tc(p(q), p(S["m"]), p(S["tg"]), p(S["cg"]), p(S["cm"]), p(S["h"]), p(w_ta), p(w1), p(w2), p(d["dzc"]), p(d["dhpre"]), p(d["dcm"]),
                            p(d["dzt"]), p(d["dm"]), p(d["dwta"]), p(d["dbta"]), B, T, C, st())
        lib.fgcn_stc_bwd_s(p(d["rpart"]), p(d["dspart"]), p(S["cg"]), p(S["s"]), p(S["mt"]), p(w_sa), p(d["dzs"]), p(d["dmt"]), p(d["dwsa"]), p(d["dbsa"]),
                           B, T, V, C, st())
        lib.fgcn_stc_param_grads(p(d["dzc"]), p(d["dhpre"]), p(S["cm"]), p(S["h"]), p(d["dwta"]), p(d["dbta"]), p(d["dwsa"]), p(d["dbsa"]),
                                 *(p(t) for t in pgrads), B, V, C, st())

    runs = {
        "fwd_a_mean_t": lambda: ops.stc_mean_t(g),
        "fwd_b_mean_v": lambda: ops.stc_mean_v(g, S["s"]),
        "fwd_c_apply": lambda: ops.stc_apply(g, S["s"], S["tg"], S["cg"], out),
        "fwd_small": small_fwd,
        "bwd_A_qr": lambda: ops.stc_bwd_qr(dout, g, S["s"], S["tg"]),
        "bwd_B_ds": lambda: ops.stc_bwd_ds(dm, g),
        "bwd_C_apply": lambda: ops.stc_bwd_apply(dout, S["s"], S["tg"], S["cg"], dm, dmt, dg),
        "bwd_small": small_bwd,
        "forward": lambda: ops.stc_forward(g, params),
        "backward": lambda: ops.stc_backward(dout, g, S, params, out=dg),
    }
    act = g.numel() * 4
    moved = {"fwd_a_mean_t": act, "fwd_b_mean_v": act, "fwd_c_apply": 2 * act, "bwd_A_qr": 2 * act, "bwd_B_ds": act, "bwd_C_apply": 2 * act,
             "forward": 4 * act, "backward": 5 * act}
    t = alternate(runs, args.rounds, args.inner)
    res = {"shape": list(shape), "activation_mbytes": round(act / 1e6, 1), "rounds": args.rounds, "inner": args.inner, "unit": "ms per call"}
    for name in runs:
        med = statistics.median(t[name])
        res[name] = {"median": round(med, 4), "min": round(min(t[name]), 4), "max": round(max(t[name]), 4)}
        if name in moved:
            res[name]["gb_per_s"] = round(moved[name] / med / 1e6, 1)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--step", action="store_true", help="time the 64-clip training step with and without attention=True instead of the kernels")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    if args.step:
        return step_times(args, dev)
    for shape in ((128, 300, 25, 64), (128, 75, 25, 256)):
        kernel_times(args, dev, shape)


if __name__ == "__main__":
    main()
