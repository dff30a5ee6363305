"""CPU checks of the four RGB patch-feature modes (reference rgb_feature_models.py:12-47, early_fusion_models.py:48-90, 163-210):
construction through the mode dispatcher, state-dict names / order / shapes, initial values against the reference's construction order,
the body-part group graph, and the argument checks.  No GPU: nothing here runs a forward."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from fusion_gcn_amd.datasets.utd_mhad import constants as utd
from fusion_gcn_amd.models.mmargcn import agcn
from fusion_gcn_amd.models.mmargcn.fusion import get_skeleton_imu_fusion_graph
from fusion_gcn_amd.models.mmargcn.mmargcn import Model
from fusion_gcn_amd.util import Graph

GROUP_EDGES = ["1, 0", "2, 0", "3, 0", "4, 0", "1, 2", "3, 4"]       # config/utd-mhad/rgb/openpose_patch_features_groups.yaml
IMU_KW = dict(num_imu_joints=2, imu_enhanced_mode="append_center")


def _graph():
    return Graph(utd.skeleton_edges, center_joint=utd.center_joint)


def _build(mode, **kw):
    T = 32
    shapes = {"rgb_patch_features": {"rgb": (1, T, 20, 512)},
              "rgb_patch_groups_features": {"rgb": (1, T, 5, 512)},
              "skeleton_rgb_patch_features_early_fusion": {"skeleton": (1, T, 20, 3), "rgb": (1, T, 20, 512)},
              "skeleton_imu_rgb_patch_features_early_fusion": {"skeleton": (1, T, 22, 3), "rgb": (1, T, 20, 512)}}
    if mode == "rgb_patch_groups_features":
        kw.setdefault("rgb_patch_groups_edges", GROUP_EDGES)
    if mode.startswith("skeleton_imu"):
        kw = {**IMU_KW, **kw}
    return Model(shapes[mode], 27, _graph(), mode=mode, **kw)._model


PATCH_MODES = ["rgb_patch_features", "rgb_patch_groups_features", "skeleton_rgb_patch_features_early_fusion",
               "skeleton_imu_rgb_patch_features_early_fusion"]
OTHER_MODES = ["rgb_encoder_model", "rgb_r2p1d", "imu_signal_image", "skeleton_rgb_encoding_early_fusion",
               "skeleton_rgb_encoding_r2p1d_early_fusion", "skeleton_rgb_r2p1d_late_fusion", "skeleton_imu_rgb_cnn_encoder_early_fusion",
               "skeleton_imu_rgb_r2p1d_early_fusion"]


@pytest.mark.parametrize("mode", PATCH_MODES)
def test_patch_modes_construct(mode):
    m = _build(mode)
    assert isinstance(m.agcn, agcn.Model)
    first_cin = m.agcn.l0.cfg.cin
    assert first_cin == {"rgb_patch_features": 512, "rgb_patch_groups_features": 512}.get(mode, 3 + 512)


@pytest.mark.parametrize("mode", OTHER_MODES)
def test_other_modes_still_raise(mode):
    with pytest.raises(NotImplementedError):
        Model({"rgb": (1, 8, 20, 3), "skeleton": (1, 8, 20, 3), "inertial": (8, 6)}, 5, _graph(), mode=mode)


@pytest.mark.parametrize("mode", PATCH_MODES[2:])
@pytest.mark.parametrize("reducer", [None, (128, 6), (512, 6), (128, 3)])
def test_state_dict_keys_order_and_shapes(mode, reducer):
    kw = {} if reducer is None else dict(patch_feature_hidden_dim=reducer[0], patch_feature_output_dim=reducer[1])
    m = _build(mode, **kw)
    sd = m.state_dict()
    keys = list(sd)
    V = 22 if "imu" in mode else 20
    if reducer is None:
        assert not any(k.startswith("patch_feature_dim_reducer") for k in keys)
        assert m.patch_feature_dim_reducer is None
        cin = 3 + 512
    else:
        H, Q = reducer
        assert keys[:4] == ["patch_feature_dim_reducer.0.weight", "patch_feature_dim_reducer.0.bias",
                            "patch_feature_dim_reducer.1.weight", "patch_feature_dim_reducer.1.bias"]
        assert [tuple(sd[k].shape) for k in keys[:4]] == [(H, 512), (H,), (Q, H), (Q,)]
        cin = 3 + Q
    rest = [k for k in keys if not k.startswith("patch_feature_dim_reducer")]
    assert all(k.startswith("agcn.") for k in rest)
    ref = agcn.Model((1, 32, V, cin), 27, get_skeleton_imu_fusion_graph(_graph(), **IMU_KW) if "imu" in mode else _graph())
    assert rest == ["agcn." + k for k in ref.state_dict()]
    assert sd["agcn.data_bn.weight"].shape == (V * cin,)


@pytest.mark.parametrize("mode", PATCH_MODES[2:])
def test_initial_values_follow_the_reference_order(mode):
    torch.manual_seed(5)
    m = _build(mode, patch_feature_hidden_dim=128, patch_feature_output_dim=6)
    torch.manual_seed(5)
    reducer = nn.Sequential(nn.Linear(512, 128), nn.Linear(128, 6))
    V = 22 if "imu" in mode else 20
    g = get_skeleton_imu_fusion_graph(_graph(), **IMU_KW) if "imu" in mode else _graph()
    ref = agcn.Model((1, 32, V, 9), 27, g)
    for k, v in reducer.state_dict().items():
        assert torch.equal(m.state_dict()["patch_feature_dim_reducer." + k], v), k
    for k, v in ref.state_dict().items():
        assert torch.equal(m.state_dict()["agcn." + k], v), k


def test_identity_reducer_has_no_parameters():
    m = _build("skeleton_rgb_patch_features_early_fusion", patch_feature_hidden_dim=128)      # output dim defaults to the input's
    assert m.patch_feature_dim_reducer is None
    assert all(n.startswith("agcn.") for n, _ in m.named_parameters())


def test_groups_graph_from_edge_strings():
    m = _build("rgb_patch_groups_features")
    g = Graph([(1, 0), (2, 0), (3, 0), (4, 0), (1, 2), (3, 4)])
    assert g.num_vertices == 5
    np.testing.assert_array_equal(np.asarray(m.agcn.l0.gcn1.adj_a), np.asarray(agcn.Model((1, 8, 5, 512), 3, g).l0.gcn1.adj_a))
    assert m.agcn.l0.gcn1.adj_a.shape == (3, 5, 5)
    assert m.agcn.data_bn.num_features == 5 * 512


@pytest.mark.parametrize("fusion", ["sum", "product", "average"])
def test_channelwise_fusion_needs_matching_channels(fusion):
    with pytest.raises(ValueError, match="channel by channel"):
        _build("skeleton_rgb_patch_features_early_fusion", fusion=fusion, patch_feature_hidden_dim=128, patch_feature_output_dim=6)
    m = _build("skeleton_rgb_patch_features_early_fusion", fusion=fusion, patch_feature_hidden_dim=128, patch_feature_output_dim=3)
    assert m.agcn.l0.cfg.cin == 3


def test_unsupported_reducer_sizes_raise_at_construction():
    with pytest.raises(ValueError, match="HIP input stage"):
        _build("skeleton_rgb_patch_features_early_fusion", patch_feature_input_dim=500, patch_feature_hidden_dim=128,
               patch_feature_output_dim=6)
    with pytest.raises(ValueError, match="HIP input stage"):
        _build("skeleton_rgb_patch_features_early_fusion", patch_feature_hidden_dim=128, patch_feature_output_dim=64)
    with pytest.raises(ValueError, match="Unsupported fusion"):
        _build("skeleton_rgb_patch_features_early_fusion", fusion="weighted_average")


def test_no_torchvision_import():
    import sys
    import fusion_gcn_amd.models.mmargcn.early_fusion_models  # noqa: F401
    import fusion_gcn_amd.models.mmargcn.rgb_feature_models  # noqa: F401
    assert "torchvision" not in sys.modules
