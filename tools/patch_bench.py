#!/usr/bin/env python3
"""Step time of the four RGB patch-feature modes at their configs' shapes (config/utd-mhad/rgb/openpose_patch_features_all.yaml,
openpose_patch_features_groups.yaml, skeleton+rgb/early_fusion/skeleton_rgb_patch_features_agcn_concat.yaml,
skeleton+rgb+imu/early_fusion/augment_v1_rgb_patch_features_concat.yaml): batch 8, one body, P = 512 features per joint, V = 20 joints
(5 body-part groups; 22 with the two IMU joints), reducer 512 -> 128 -> 6 with concatenation for the early-fusion modes.  fwd+bwd
(train-mode BatchNorm, CrossEntropy) on one MI355X in every math mode, eager and replayed from a recorded HIP graph (GraphStep), and
for the early-fusion modes with paths.patch_input_fused on and off (on / off / on, same process: the A/B of the input stage), plus the
input stage alone (forward + backward of block.patch_input, no blocks).  One JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

GROUP_EDGES = ["1, 0", "2, 0", "3, 0", "4, 0", "1, 2", "3, 4"]


def specs(T, P):
    red = dict(patch_feature_hidden_dim=128, patch_feature_output_dim=6)
    return {
        "rgb_patch_features": ({"rgb": (1, T, 20, P)}, dict(patch_feature_input_dim=P)),
        "rgb_patch_groups_features": ({"rgb": (1, T, 5, P)}, dict(rgb_patch_groups_edges=GROUP_EDGES)),
        "skeleton_rgb_patch_features_early_fusion": ({"skeleton": (1, T, 20, 3), "rgb": (1, T, 20, P)},
                                                     dict(fusion="concatenate", patch_feature_input_dim=P, **red)),
        "skeleton_imu_rgb_patch_features_early_fusion": ({"skeleton": (1, T, 22, 3), "rgb": (1, T, 20, P)},
                                                         dict(fusion="concatenate", patch_feature_input_dim=P, num_imu_joints=2,
                                                              imu_enhanced_mode="append_center", **red)),
    }


def time_input_stage(model, x, steps):
    from fusion_gcn_amd.block import patch_input
    w = [p for p in model.patch_feature_dim_reducer.parameters()]

    def one():
        for p in w:
            p.grad = None
        h = patch_input(x["skeleton"], x["rgb"], model.patch_feature_dim_reducer, model.agcn.data_bn, model.num_joints,
                        model.fusion_type)
        h.sum().backward()
    for _ in range(3):
        one()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps * 4):
        one()
    torch.cuda.synchronize()
    return round(1e3 * (time.perf_counter() - t0) / (steps * 4), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("T", nargs="?", type=int, default=128, help="frames per clip")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--features", type=int, default=512)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--modes", default="f32,bf16x3,f16x2,bf16")
    ap.add_argument("--no-graph", action="store_true")
    args = ap.parse_args()
    from fusion_gcn_amd import ops
    from fusion_gcn_amd.datasets.utd_mhad import constants as utd
    from fusion_gcn_amd.models.mmargcn.mmargcn import Model
    from fusion_gcn_amd.util import Graph
    from steptime import time_step
    dev = torch.device("cuda:0")
    out = {"T": args.T, "batch": args.batch, "P": args.features, "device": torch.cuda.get_device_name(0)}
    for mode, (shapes, kw) in specs(args.T, args.features).items():
        torch.manual_seed(1)
        model = Model(shapes, 27, Graph(utd.skeleton_edges, center_joint=utd.center_joint), mode=mode, **kw)._model.to(dev).train()
        x = {k: torch.randn(args.batch, *s, device=dev) for k, s in shapes.items()}
        feats = x if "skeleton" in x else x["rgb"]
        y = torch.randint(0, 27, (args.batch,), device=dev)
        res = {}
        fused_settings = (True, False, True) if "skeleton" in x else (True,)
        for math in args.modes.split(","):
            for i, fused in enumerate(fused_settings):
                with ops.context(math) as ctx:
                    ctx.paths.patch_input_fused = fused
                    t = time_step(model, feats, y, args.steps, graph=not args.no_graph)
                    if "skeleton" in x:
                        t["input_stage_ms"] = time_input_stage(model, x, args.steps)
                key = f"{math}" + ("" if len(fused_settings) == 1 else f"/fused={'on' if fused else 'off'}{'#2' if i == 2 else ''}")
                res[key] = t
        out[mode] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
