"""RGB patch-feature models (reference torch_src/models/mmargcn/rgb_feature_models.py:12-47, early_fusion_models.py:48-90, 163-210).

The reference's preprocessing turns every frame's patch around each joint into one CNN feature vector (512 floats for ResNet-18), so
these modes are the AGCN of this package on a wide per-joint input: no image model runs at training time and nothing here imports
torchvision.

``mode: rgb_patch_features`` -- ``RgbPatchFeaturesModel``: ``agcn.Model`` on the (M, T, V, P) features.
``mode: rgb_patch_groups_features`` -- ``RgbPatchGroupsFeaturesModel``: the same on a graph of body-part groups built from the
``rgb_patch_groups_edges`` strings ("a, b").
The two early-fusion modes on the same features are in early_fusion_models.py, as in the reference.
"""
import torch.nn as nn

from ...util.graph import Graph
from . import agcn


def agcn_kwargs(kwargs) -> dict:
    return dict(num_layers=kwargs.get("num_layers", 10), without_fc=kwargs.get("without_fc", False), attention=kwargs.get("attention", False))


def groups_graph(edges) -> Graph:
    """``rgb_patch_groups_edges`` entries "a, b" -> the body-part group graph (reference rgb_feature_models.py:38-40)."""
    return Graph([tuple(map(int, edge.split(", "))) for edge in edges])


class RgbPatchFeaturesModel(nn.Module):
    """AGCN on precomputed patch features: one P-wide feature vector per joint instead of (x, y, z)."""

    def __init__(self, data_shape, num_classes: int, graph, **kwargs):
        super().__init__()
        self.agcn = agcn.Model(tuple(data_shape["rgb"]), num_classes, self.patch_graph(graph, kwargs), **agcn_kwargs(kwargs))

    def patch_graph(self, graph, kwargs):
        return graph

    def forward(self, x):
        return self.agcn(x["rgb"] if isinstance(x, dict) else x)


class RgbPatchGroupsFeaturesModel(RgbPatchFeaturesModel):
    """The same on the graph of ``rgb_patch_groups_edges``: one feature vector per body-part group."""

    def patch_graph(self, graph, kwargs):
        return groups_graph(kwargs["rgb_patch_groups_edges"])
