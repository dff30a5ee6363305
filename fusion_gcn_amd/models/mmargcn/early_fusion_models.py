"""Early skeleton + IMU fusion in front of one AGCN (reference torch_src/models/mmargcn/early_fusion_models.py:9-45).

``mode: skeleton_imu_spatial_fusion`` -- ``SkeletonImuSpatialFusionModel`` (:9-22): every IMU modality is an extra joint of the
skeleton graph (the preprocessing already appended their samples as joints V..V+n-1), so only the GRAPH changes.
``mode: skeleton_imu_channel_fusion`` -- ``SkeletonImuChannelFusionModel`` (:25-45): the IMU signals of a frame are broadcast to
every joint of every body as extra input CHANNELS, so only the input changes.
``mode: skeleton_rgb_patch_features_early_fusion`` -- ``SkeletonRgbPatchFeaturesEarlyFusion`` (:48-90) and
``mode: skeleton_imu_rgb_patch_features_early_fusion`` -- ``SkeletonImuRgbPatchFeaturesEarlyFusion`` (:163-210): precomputed RGB patch
features (one P-wide vector per joint), an optional reducer Linear(P, H) . Linear(H, Q) with no activation between, zero rows for the
joints without a patch (the IMU joints; inserted after the reducer), fusion with the skeleton rows, then the AGCN.  The input stage runs
in libfgcn (block.patch_input: one fgcn_patch_input_fwd pass in front of data_bn's apply).  Sub-module names and the order the initial
values are drawn in are the reference's: ``patch_feature_dim_reducer.0`` / ``.1`` (absent for the identity reducer) before ``agcn``.
The other RGB early-fusion variants of that file wrap image encoders and are out of scope.

Both are one AGCN (sub-module ``agcn``: the state-dict prefix the reference's checkpoints carry) behind a small adapter; what
differs is stated as two hooks instead of two constructors.
"""
from typing import Optional

import torch
import torch.nn as nn

from ... import ops
from ...block import patch_input
from . import agcn
from .fusion import get_skeleton_imu_fusion_graph
from .rgb_feature_models import agcn_kwargs

# model_args the reference forwards to agcn.Model (defaults are agcn.Model's own), plus this build's block switches
_FORWARDED = ("num_layers", "without_fc")
_BUILD_SWITCHES = ("static_adjacency", "fused_spatial", "attention")


class _AgcnBehindAdapter(nn.Module):
    forwarded = _FORWARDED

    def __init__(self, data_shape, num_classes: int, graph, **kwargs):
        super().__init__()
        shape, graph = self.network_shape_and_graph(data_shape, graph, kwargs)
        passed = {k: kwargs[k] for k in self.forwarded if k in kwargs}
        self.agcn = agcn.Model(tuple(shape), num_classes, graph, **passed)

    def network_shape_and_graph(self, data_shape, graph, kwargs):
        raise NotImplementedError

    def network_input(self, x):
        return x

    def forward(self, x):
        return self.agcn(self.network_input(x))


class SkeletonImuSpatialFusionModel(_AgcnBehindAdapter):
    forwarded = _FORWARDED + _BUILD_SWITCHES

    def network_shape_and_graph(self, data_shape, graph, kwargs):
        return data_shape["skeleton"], get_skeleton_imu_fusion_graph(graph, **kwargs)


class SkeletonImuChannelFusionModel(_AgcnBehindAdapter):
    def network_shape_and_graph(self, data_shape, graph, kwargs):
        *lead, channels = data_shape["skeleton"]
        return (*lead, channels + data_shape["inertial"][-1]), graph

    def network_input(self, x):
        skeleton, imu = x["skeleton"], x["inertial"]                  # (N, M, T, V, C) and (N, T, S): frames line up
        n, bodies, frames, joints, _ = skeleton.shape
        imu_on_joints = imu[:, None, :, None, :].expand(n, bodies, frames, joints, imu.shape[-1])
        return torch.cat((skeleton, imu_on_joints), dim=-1)


class _SkeletonPatchFeaturesEarlyFusion(nn.Module):
    """Shared body of the two early-fusion modes; subclasses pick the graph (skeleton, or skeleton + IMU joints)."""

    def __init__(self, data_shape, num_classes: int, graph, **kwargs):
        super().__init__()
        graph = self.fusion_graph(graph, kwargs)
        self.fusion_type = kwargs.get("fusion", "concatenate")
        if self.fusion_type not in ops.PATCH_FUSIONS:
            raise ValueError(f"Unsupported fusion for the patch-feature input: {self.fusion_type!r} (known: {', '.join(ops.PATCH_FUSIONS)})")
        p_in = kwargs.get("patch_feature_input_dim", 512)
        p_hidden = kwargs.get("patch_feature_hidden_dim", p_in)
        p_out = kwargs.get("patch_feature_output_dim", p_in)
        bodies, frames, _, skel_channels = data_shape["skeleton"]
        if self.fusion_type == "concatenate":
            channels = skel_channels + p_out
        else:
            if p_out != skel_channels:
                raise ValueError(f"fusion {self.fusion_type!r} combines channel by channel: patch_feature_output_dim ({p_out}) must equal "
                                 f"the skeleton's channel count ({skel_channels})")
            channels = skel_channels
        self.patch_feature_dim_reducer: Optional[nn.Sequential] = None
        if p_in != p_out:          # drawn before the AGCN, as in the reference
            self.patch_feature_dim_reducer = nn.Sequential(nn.Linear(p_in, p_hidden), nn.Linear(p_hidden, p_out))
            if p_in % 128 or p_in > 1024 or p_hidden % 32 or p_hidden > 1024 or p_out > 32:
                raise ValueError(f"patch-feature reducer {p_in} -> {p_hidden} -> {p_out}: the HIP input stage takes input dims that are "
                                 "multiples of 128 up to 1024, hidden dims that are multiples of 32 up to 1024 and up to 32 outputs")
        self.num_joints = graph.num_vertices
        self.agcn = agcn.Model((bodies, frames, graph.num_vertices, channels), num_classes, graph, **agcn_kwargs(kwargs))

    def fusion_graph(self, graph, kwargs):
        return graph

    def forward(self, x):
        skeleton, rgb = x["skeleton"], x["rgb"]                  # (N, M, T, V, Cs), (N, M, T, Vp, P)
        if rgb.shape[3] > self.num_joints or skeleton.shape[3] != self.num_joints:
            raise ValueError(f"patch rows {tuple(rgb.shape)} / skeleton rows {tuple(skeleton.shape)} do not fit a {self.num_joints}-joint graph")
        h = patch_input(skeleton, rgb, self.patch_feature_dim_reducer, self.agcn.data_bn, self.num_joints, self.fusion_type)
        return self.agcn.forward_blocks(h, skeleton.shape[0])


class SkeletonRgbPatchFeaturesEarlyFusion(_SkeletonPatchFeaturesEarlyFusion):
    """Skeleton rows fused with the (reduced) patch features of the same joints."""


class SkeletonImuRgbPatchFeaturesEarlyFusion(_SkeletonPatchFeaturesEarlyFusion):
    """The same on the skeleton + IMU graph: the IMU joints have no patch and get zero rows, inserted after the reducer."""

    def fusion_graph(self, graph, kwargs):
        return get_skeleton_imu_fusion_graph(graph, **kwargs)
