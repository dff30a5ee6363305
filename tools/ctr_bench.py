#!/usr/bin/env python3
"""CTR-GCN's graph convolution kernels (fgcn_ctr.hip) at the two ends of the 64-clip window step -- (128, 64, 25,
64 -> 64), the first blocks' shape, and (128, 16, 25, 256 -> 256), the last: each kernel, then the op forward and backward against the
stock-torch composition of the same op on the same device (which materialises A' and runs the einsum: the baseline, never the code under
test).  They alternate in one process; every round times ``--inner`` calls of each between device events after a warm-up, and the result
is the median per call with the spread.  A loop of identical calls finds its tensors in the Infinity Cache, so these are isolated figures.

``--step``: the 64-clip bf16x3 training step of ``model: ctrgcn`` at the window shape (2 bodies, 64 frames, 25 joints): forward + backward
with the packed weights rebuilt, eager and replayed from one HIP graph -- the in-step figure."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

K = 3


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


def summary(t: dict, digits: int = 4) -> dict:
    return {name: {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits)} for name, v in t.items()}


def torch_op(x3, x12, w4, b4, alpha, pa):
    """the stock-torch composition: A' (B, K, V, V, C) in memory, then the einsum"""
    B, T, V, KC = x3.shape
    C, R = KC // K, w4.shape[2]
    x1, x2 = x12[..., :K * R].view(B, V, K, R), x12[..., K * R:].view(B, V, K, R)
    th = torch.tanh(x1.permute(0, 2, 1, 3).unsqueeze(3) - x2.permute(0, 2, 1, 3).unsqueeze(2))        # (B, K, u, v, R)
    a = alpha * (torch.einsum("bkuvr,kcr->bkuvc", th, w4) + b4.view(1, K, 1, 1, C)) + pa.view(1, K, V, V, 1)
    return torch.einsum("bkuvc,btvkc->btuc", a, x3.view(B, T, V, K, C))


def kernel_times(args, dev, shape):
    from fusion_gcn_amd import fops, ops
    B, T, V, cin, C = shape
    R = ops.ctr_reduction(cin)
    gen = torch.Generator().manual_seed(1)
    rnd = lambda *s, scale=1.0: (scale * torch.randn(s, generator=gen)).to(dev)  # noqa: E731
    x, x3, x12, dy = rnd(B, T, V, cin), rnd(B, T, V, K * C), rnd(B, V, 2 * K * R), rnd(B, T, V, C)
    w4, b4, alpha, pa = rnd(K, C, R, scale=R ** -0.5), rnd(K, C, scale=0.1), torch.full((1,), 0.5, device=dev), rnd(K, V, V, scale=0.1)
    y, th = ops.ctr_forward(x3, x12, w4, b4, alpha, pa)
    ref = torch_op(x3, x12, w4, b4, alpha, pa)
    err = float((y - ref).norm() / ref.norm())
    if err > 1e-5:
        raise SystemExit(f"{shape}: the HIP op and the torch composition differ by {err:.2e}")
    lib, p, st = ops._lib.load(), ops._p, ops._stream
    new = lambda *s: torch.empty(s, device=dev)  # noqa: E731
    dx3, da, dz, dx12 = new(B, T, V, K * C), new(B, K, V, V, C), new(B, K, V, V, R), new(B, V, 2 * K * R)
    s2, s1, dpa_part, dal = new(B, K, C, R), new(B, K, C), new(B, K, V, V), new(B, K)
    d_w4, d_b4, d_pa, d_alpha = new(K, C, R), new(K, C), new(K, V, V), new(1)
    xm = ops.ctr_mean_t(x)
    leaves = [t.clone().requires_grad_(True) for t in (x3, x12, w4, b4, alpha, pa)]

    def torch_bwd():
        for t in leaves:
            t.grad = None
        torch_op(*leaves).backward(dy)

    def hip_fwd_bwd():
        for t in leaves:
            t.grad = None
        fops.ctr_aggregate(*leaves).backward(dy)

    runs = {
        "mean_t": lambda: ops.ctr_mean_t(x),
        "mean_t_bwd": lambda: ops.ctr_mean_t_bwd(xm, T),
        "tanh": lambda: ops.ctr_tanh(x12, R),
        "aggregate": lambda: lib.fgcn_ctr_aggregate(p(x3), p(th), p(w4), p(b4), p(alpha), p(pa), p(y), B, T, V, C, R, st()),
        "bwd_dx3": lambda: lib.fgcn_ctr_bwd_dx3(p(dy), p(th), p(w4), p(b4), p(alpha), p(pa), p(dx3), B, T, V, C, R, st()),
        "bwd_da": lambda: lib.fgcn_ctr_bwd_da(p(dy), p(x3), p(da), B, T, V, C, st()),
        "bwd_small": lambda: lib.fgcn_ctr_bwd_small(p(da), p(th), p(w4), p(b4), p(alpha), p(dz), p(dx12), p(s2), p(s1), p(dpa_part), p(dal), B, V, C, R, st()),
        "param_grads": lambda: lib.fgcn_ctr_param_grads(p(s2), p(s1), p(dpa_part), p(dal), p(alpha), p(d_w4), p(d_b4), p(d_pa), p(d_alpha), B, V, C, R, st()),
        "op_forward": lambda: ops.ctr_forward(x3, x12, w4, b4, alpha, pa),
        "op_forward_backward": hip_fwd_bwd,
        "torch_forward": lambda: torch_op(x3, x12, w4, b4, alpha, pa),
        "torch_forward_backward": torch_bwd,
    }
    res = {"shape": list(shape), "R": R, "x3_mbytes": round(x3.numel() * 4 / 1e6, 1), "dA_mbytes": round(da.numel() * 4 / 1e6, 1),
           "th_mbytes": round(th.numel() * 4 / 1e6, 1), "rounds": args.rounds, "inner": args.inner, "unit": "ms per call", "hip_vs_torch_rel_l2": err}
    res.update(summary(alternate(runs, args.rounds, args.inner)))
    print(json.dumps(res), flush=True)


def step_times(args, dev):
    from fusion_gcn_amd import ops
    from fusion_gcn_amd.datasets.ntu_rgb_d import constants as ntu
    from fusion_gcn_amd.dp import FlatGradients
    from fusion_gcn_amd.loss import cross_entropy
    from fusion_gcn_amd.models.ctrgcn.ctrgcn import Model
    from fusion_gcn_amd.util import Graph
    ops.set_math_mode("bf16x3")
    M, T, V, C = 2, 64, 25, 3
    torch.manual_seed(1)
    model = Model({"skeleton": (M, T, V, C)}, 60, Graph(ntu.skeleton_edges, center_joint=ntu.center_joint))
    with torch.no_grad():
        for n, p in model.named_parameters():                                 # (a trained model's: the initial values switch the refinement off)
            if n.endswith("gcn1.bn.weight"):
                p.fill_(1.0)
            if n.endswith("alpha"):
                p.fill_(0.5)
    model = model.to(dev).train()
    grads = FlatGradients(model.parameters())
    g = torch.Generator().manual_seed(1)
    x, y = torch.randn(args.batch, M, T, V, C, generator=g).to(dev), torch.randint(0, 60, (args.batch,), generator=g).to(dev)

    def fwd_bwd():
        model.mark_packed_stale()
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
    model.prepare_recording()
    graph = torch.cuda.CUDAGraph()
    grads.zero()
    with torch.cuda.graph(graph):
        static_loss = fwd_bwd()
    graph.replay()
    torch.cuda.synchronize()
    if abs(float(static_loss.detach()) - eager) > 1e-4 * max(1.0, abs(eager)):
        raise SystemExit(f"graph replay loss {float(static_loss.detach())} != eager loss {eager}")

    def eager_step():
        grads.zero()
        fwd_bwd()

    res = {"step": "ctrgcn fwd+bwd, bf16x3", "clips": args.batch, "window": [M, T, V, C], "rounds": args.rounds, "inner": args.inner, "unit": "ms per step"}
    res.update(summary(alternate({"eager": eager_step, "replayed": graph.replay}, args.rounds, args.inner), 2))
    res["clips_per_s_replayed"] = round(args.batch / res["replayed"]["median"] * 1e3, 1)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--step", action="store_true", help="time the 64-clip training step of model: ctrgcn instead of the kernels")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    if args.step:
        return step_times(args, dev)
    for shape in ((128, 64, 25, 64, 64), (128, 16, 25, 256, 256)):
        kernel_times(args, dev, shape)


if __name__ == "__main__":
    main()
