#!/usr/bin/env python3
"""Step time of agcn.Model against the joint count: V = 25 (NTU, the 32-joint kernels), 33 (a MediaPipe-sized random tree), 50 (the NTU
skeleton twice, a two-person graph) and 64 (a random tree) -- the last three on the wide route.  fwd+bwd
(train-mode BatchNorm, CrossEntropy) of ``--batch`` one-body clips of T frames on one MI355X, eager and replayed from a recorded HIP
graph (GraphStep), per math mode.  One JSON line; per_joint_us = graph ms per step / V (what a joint costs on each route)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402


def graph_for(V: int):
    from fusion_gcn_amd.datasets.ntu_rgb_d import constants as ntu
    from fusion_gcn_amd.util import Graph
    if V == 25:
        return Graph(ntu.skeleton_edges, center_joint=ntu.center_joint)
    if V == 50:
        edges = list(ntu.skeleton_edges)
        return Graph(edges + [(a + 25, b + 25) for a, b in edges], center_joint=ntu.center_joint)
    rng = np.random.default_rng(V)
    return Graph([(int(rng.integers(0, i)), i) for i in range(1, V)], center_joint=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("T", nargs="?", type=int, default=64, help="frames per clip")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--joints", default="25,33,50,64")
    ap.add_argument("--modes", default="bf16x3,f32,bf16")
    args = ap.parse_args()
    from fusion_gcn_amd import ops
    from fusion_gcn_amd.models.mmargcn.agcn import Model
    from steptime import time_step
    dev = torch.device("cuda:0")
    out = {"T": args.T, "batch": args.batch, "classes": 60, "device": torch.cuda.get_device_name(0)}
    for V in (int(v) for v in args.joints.split(",")):
        torch.manual_seed(1)
        model = Model((1, args.T, V, 3), 60, graph_for(V)).to(dev).train()
        x = torch.randn(args.batch, 1, args.T, V, 3, device=dev)
        y = torch.randint(0, 60, (args.batch,), device=dev)
        res = {"route": "wide" if ops.wide_graph(V) else "32-joint"}
        for math in args.modes.split(","):
            with ops.context(math):
                t = time_step(model, x, y, args.steps, graph=True)
            t["per_joint_us"] = round(1e3 * t["graph"]["ms_per_step"] / V, 2)
            res[math] = t
        out[f"V{V}"] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
