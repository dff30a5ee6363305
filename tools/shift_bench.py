#!/usr/bin/env python3
"""Shift-GCN's shift kernels (fgcn_shift.hip) at the two ends of the 64-clip window step -- (128, 64, 25, 64), the first
blocks' shape, and (128, 16, 25, 256), the last: each kernel form in ms and in effective TB/s (algorithmic bytes / time: every tensor the
definition reads or writes counted once) BESIDE ``fops.add_act`` on the same element count in the same run (three tensors of that size: the
yardstick of a memory pass), then each op forward and forward + backward against the stock-torch composition of the same op on the same
device (``index_select`` over the flattened (V C) axis times the gate; a gather and a lerp over the frames: the baseline, never the code
under test).  They alternate in one process; every round times ``--inner`` calls of each between device events after a warm-up, and the
result is the median per call with the spread.  The ``--inner`` calls are replayed from one HIP graph: a call of 20 us is shorter than its
Python enqueue, so an eager loop between device events times the host (``--eager`` does that).  A loop of identical calls finds its
tensors in the Infinity Cache, so these are isolated figures.

``--step``: the 64-clip bf16x3 training step of ``model: shiftgcn`` at the window shape (2 bodies, 64 frames, 25 joints): forward + backward
with the packed weights rebuilt, eager and replayed from one HIP graph -- the in-step figure."""
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


def recorded(fn, inner: int):
    """``inner`` calls of ``fn`` as one HIP graph: a call of 20 us is shorter than its Python enqueue, and between device events an eager loop
    of such calls times the host.  -> the replay, which ``timed(.., 1)`` times"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(inner):
            fn()
    return graph.replay


def alternate_recorded(runs: dict, rounds: int, inner: int) -> dict:
    t = alternate({name: recorded(fn, inner) for name, fn in runs.items()}, rounds, 1)
    return {name: [v / inner for v in times] for name, times in t.items()}


def summary(t: dict, digits: int = 4, tensors: dict = None, nbytes: int = 0) -> dict:
    out = {}
    for name, v in t.items():
        out[name] = {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits)}
        if tensors and name in tensors:                                       # effective TB/s at the median, and the element-sized tensors counted
            out[name]["tensors"] = tensors[name]
            out[name]["tb_per_s"] = round(tensors[name] * nbytes / (statistics.median(v) * 1e-3) / 1e12, 3)
    return out


def torch_joint_shift(x, mask, table):
    B, T, V, C = x.shape
    y = torch.index_select(x.view(B * T, V * C), 1, table).view(B, T, V, C)
    return y if mask is None else y * (torch.tanh(mask) + 1)


def torch_frame_shift(x, pos, stride, relu):
    B, T, V, C = x.shape
    T_out = (T - 1) // stride + 1
    k = torch.floor(pos.detach())
    f = (pos - k).view(1, 1, 1, C)
    phi = torch.relu(x) if relu else x
    t = (torch.arange(T_out, device=x.device).view(1, T_out, 1, 1) * stride + k.long().view(1, 1, 1, C)).expand(B, T_out, V, C)

    def tap(t):
        return torch.where((t >= 0) & (t < T), torch.gather(phi, 1, t.clamp(0, T - 1)), x.new_zeros(()))
    return (1 - f) * tap(t) + f * tap(t + 1)


def kernel_times(args, dev, shape):
    from fusion_gcn_amd import fops, ops
    B, T, V, C = shape
    gen = torch.Generator().manual_seed(1)
    rnd = lambda *s, scale=1.0: (scale * torch.randn(s, generator=gen)).to(dev)  # noqa: E731
    x, dy, other = rnd(B, T, V, C), rnd(B, T, V, C), rnd(B, T, V, C)
    mask, pos = rnd(V, C, scale=0.5), (2 * torch.rand(C, generator=gen) - 1).to(dev)
    table = torch.tensor([(i * C + j + j * C) % (V * C) for i in range(V) for j in range(C)], device=dev)
    dy2 = dy[:, :(T - 1) // 2 + 1].contiguous()
    errs = {"joint": float((ops.joint_shift_forward(x, mask, 1) - torch_joint_shift(x, mask, table)).norm() / x.norm()),
            "frame": float((ops.frame_shift_forward(x, pos, 1, True)[0] - torch_frame_shift(x, pos, 1, True)).norm() / x.norm()),
            "frame_s2": float((ops.frame_shift_forward(x, pos, 2, False)[0] - torch_frame_shift(x, pos, 2, False)).norm() / x.norm())}
    if max(errs.values()) > 1e-6:
        raise SystemExit(f"{shape}: the HIP ops and the torch compositions differ: {errs}")
    leaves = [t.clone().requires_grad_(True) for t in (x, mask, pos)]

    def fwd_bwd(fn, inputs, grad):
        def run():
            for t in inputs:
                t.grad = None
            fn(*inputs).backward(grad)
        return run

    runs = {
        "add_act": lambda: fops.add_act(x, other),
        "joint_fwd": lambda: ops.joint_shift_forward(x, None, -1),
        "joint_fwd_gate": lambda: ops.joint_shift_forward(x, mask, 1),
        "joint_dx": lambda: ops.joint_shift_backward(dy, None, None, -1),
        "joint_dx_gate_dmask": lambda: ops.joint_shift_backward(dy, x, mask, 1),
        "frame_fwd": lambda: ops.frame_shift_forward(x, pos, 1, False, False),
        "frame_fwd_relu_stats": lambda: ops.frame_shift_forward(x, pos, 1, True, True),
        "frame_fwd_relu_stats_s2": lambda: ops.frame_shift_forward(x, pos, 2, True, True),
        "frame_bwd": lambda: ops.frame_shift_backward(dy, x, pos, 1, False),
        "frame_bwd_relu": lambda: ops.frame_shift_backward(dy, x, pos, 1, True),
        "frame_bwd_relu_s2": lambda: ops.frame_shift_backward(dy2, x, pos, 2, True),
        "torch_joint_forward": lambda: torch_joint_shift(x, mask, table),
        "torch_frame_forward": lambda: torch_frame_shift(x, pos, 1, True),
        "op_joint_forward": lambda: fops.joint_shift(x, mask, 1),
        "op_frame_forward": lambda: fops.frame_shift(x, pos, 1, relu=True),
    }
    grad_runs = {
        "op_joint_forward_backward": fwd_bwd(lambda a, m, p: fops.joint_shift(a, m, 1), leaves, dy),
        "torch_joint_forward_backward": fwd_bwd(lambda a, m, p: torch_joint_shift(a, m, table), leaves, dy),
        "op_frame_forward_backward": fwd_bwd(lambda a, m, p: fops.frame_shift(a, p, 1, relu=True), leaves, dy),
        "torch_frame_forward_backward": fwd_bwd(lambda a, m, p: torch_frame_shift(a, p, 1, True), leaves, dy),
    }
    # element-sized tensors each kernel's definition reads or writes (stride 2: the output and its gradient are half-sized)
    tensors = {"add_act": 3, "joint_fwd": 2, "joint_fwd_gate": 2, "joint_dx": 2, "joint_dx_gate_dmask": 3, "frame_fwd": 2, "frame_fwd_relu_stats": 2,
               "frame_fwd_relu_stats_s2": 1.5, "frame_bwd": 3, "frame_bwd_relu": 3, "frame_bwd_relu_s2": 2.5}
    res = {"shape": list(shape), "tensor_mbytes": round(x.numel() * 4 / 1e6, 1), "rounds": args.rounds, "inner": args.inner, "unit": "ms per call",
           "hip_vs_torch_rel_l2": errs}

    def no_grad(fn):
        def run():
            with torch.no_grad():
                return fn()
        return run
    every = {**{k: no_grad(f) for k, f in runs.items()}, **grad_runs}
    t = alternate(every, args.rounds, args.inner) if args.eager else alternate_recorded(every, args.rounds, args.inner)
    res["timed"] = "eager loops" if args.eager else f"replays of one HIP graph of {args.inner} calls"
    res.update(summary(t, tensors=tensors, nbytes=x.numel() * 4))
    print(json.dumps(res), flush=True)


def step_times(args, dev):
    from fusion_gcn_amd import ops
    from fusion_gcn_amd.datasets.ntu_rgb_d import constants as ntu
    from fusion_gcn_amd.dp import FlatGradients
    from fusion_gcn_amd.loss import cross_entropy
    from fusion_gcn_amd.models.shiftgcn.shiftgcn import Model
    from fusion_gcn_amd.util import Graph
    ops.set_math_mode("bf16x3")
    M, T, V, C = 2, 64, 25, 3
    torch.manual_seed(1)
    model = Model({"skeleton": (M, T, V, C)}, 60, Graph(ntu.skeleton_edges, center_joint=ntu.center_joint))
    with torch.no_grad():
        for n, p in model.named_parameters():                                 # (a trained model's: the initial 1e-6 switches the graph unit off)
            if n.endswith("gcn1.bn.weight"):
                p.fill_(1.0)
            if n.endswith("Feature_Mask"):
                p.uniform_(-0.5, 0.5)
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

    res = {"step": "shiftgcn fwd+bwd, bf16x3", "clips": args.batch, "window": [M, T, V, C], "rounds": args.rounds, "inner": args.inner, "unit": "ms per step"}
    res.update(summary(alternate({"eager": eager_step, "replayed": graph.replay}, args.rounds, args.inner), 2))
    res["clips_per_s_replayed"] = round(args.batch / res["replayed"]["median"] * 1e3, 1)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--eager", action="store_true", help="time eager loops of the kernels and ops instead of HIP-graph replays (host enqueue included)")
    ap.add_argument("--step", action="store_true", help="time the 64-clip training step of model: shiftgcn instead of the kernels")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    if args.step:
        return step_times(args, dev)
    for shape in ((128, 64, 25, 64), (128, 16, 25, 256)):
        kernel_times(args, dev, shape)


if __name__ == "__main__":
    main()
