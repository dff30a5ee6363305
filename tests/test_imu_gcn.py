"""SURVEY.md section 8 row f1 (static-adjacency half): the IMU graph model ``mode: imu_gcn`` with ``gc_model: stgcn``.

Chain of evidence: tests/golden/imu_gcn.npz is written by oracle/gen_golden_imu.py from the imported reference
(ImuGCN, build_imu_graph_adjacency); the CPU tests pin the oracle restatement and the product's graph builder / state-dict
surface to it; the GPU tests compare the HIP-backed model with the float64 oracle (forward 2e-5, gradients 5e-4 rel-L2,
exactly-zero gradients of the conv biases in front of a train-mode BatchNorm)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2
from oracle import filler
from oracle import imu_gcn_oracle as O

import guarded
from guarded import guarded_gpu_tests  # noqa: F401  (the fixture)

# the tests marked gpu run on guarded allocations, margins verified at teardown (tests/guarded.py); the host tests as they are
pytestmark = pytest.mark.usefixtures("guarded_gpu_tests")

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "imu_gcn.npz"))
CASES = {
    "value48": ((8, 6), 7, 3, dict(gc_model="stgcn", graph_node_format="node_per_value", num_layers=5, inner_feature_dim=16)),
    "sensor16": ((8, 6), 5, 4, dict(gc_model="stgcn", graph_node_format="node_per_sensor", num_signals=2, num_layers=4,
                                    inner_feature_dim=8, adjacency_normalization="row", num_temporal_back_connections=2,
                                    inter_signal_back_connections=True)),
    "agcn_sensor16": ((8, 6), 5, 3, dict(gc_model="agcn", graph_node_format="node_per_sensor", num_signals=2, num_layers=4,
                                         inner_feature_dim=16)),
    "agcn_value48": ((8, 6), 7, 2, dict(gc_model="agcn", graph_node_format="node_per_value", num_layers=3, inner_feature_dim=16,
                                        inter_signal_back_connections=True)),
}


def build(tag, shape=None, classes=None, kw=None, double=False):
    """-> (model with filler parameters, the same values as a float64 state dict under the reference's key names).
    ``double``: fill in float64 (the golden vectors' precision) instead of float32 (what the GPU model holds)."""
    from fusion_gcn_amd.models.mmargcn.mmargcn import Model
    if shape is None:
        shape, classes, _, kw = CASES[tag]
    model = Model({"inertial": shape}, classes, None, mode="imu_gcn", **kw)
    if double:
        model = model.double()
    filler.fill_state_dict(model.state_dict(), skip=("adj", "adj_a"), rename=lambda k: k.replace("_model.", ""))
    sd = {k.replace("_model.", ""): (v.detach().double().clone() if v.is_floating_point() else v.detach().clone())
          for k, v in model.state_dict().items()}
    return model, sd


def inputs(tag, shape, batch, classes):
    x = torch.from_numpy(filler.bellish(f"x.{tag}", (batch, *shape), scale=0.5)).double()
    y = torch.from_numpy(filler.uniform(f"y.{tag}", (batch,), 0, classes).astype(np.int64))
    return x, y


def fmt(kw):
    return dict(graph_node_format=kw["graph_node_format"],
                num_features=1 if kw["graph_node_format"] == "node_per_value" else 6 // kw["num_signals"])


def test_imu_graph_adjacency_matches_the_reference():
    from fusion_gcn_amd.models.mmargcn.imu_feature_models import build_imu_graph_adjacency
    for tag, (shape, sig, kw) in {"row_t1": ((5, 3), 0, dict(normalization="row")),
                                  "column_t2_inter": ((5, 3), 0, dict(normalization="column", temporal_back_connections=2,
                                                                       inter_signal_back_connections=True)),
                                  "symmetric_sensor": ((6, 4), 2, dict(normalization="symmetric"))}.items():
        want = GOLD[f"adj.{tag}"]
        got = build_imu_graph_adjacency(shape, sig, "stgcn", False, **kw).double().numpy()
        assert got.shape == want.shape and np.abs(got - want).max() < 1e-7          # (the reference stores float32)
        edges, n = O.imu_graph_edges(shape, sig, kw.get("temporal_back_connections", 1),
                                     kw.get("inter_signal_back_connections", False))
        mine = O.normalized_adjacency(edges, n, kw["normalization"], True)
        assert np.abs(mine - want).max() < 1e-7


@pytest.mark.parametrize("tag", list(CASES))
def test_oracle_and_state_dict_surface_match_the_reference(tag):
    shape, classes, batch, kw = CASES[tag]
    model, sd = build(tag, double=True)
    assert sorted(sd) == list(GOLD[f"{tag}.keys"])                                  # same keys as the reference's state dict
    assert np.abs(sd["gcn.gc1.adj" if "gcn.gc1.adj" in sd else "gcn.gc1.adj_a"].numpy() - GOLD[f"{tag}.adj"]).max() < 1e-7
    x, y = inputs(tag, shape, batch, classes)
    assert np.array_equal(y.numpy(), GOLD[f"{tag}.labels"])
    assert rel_l2(O.imu_gcn_forward(x, sd, train=False, **fmt(kw)).numpy(), GOLD[f"{tag}.eval.logits"]) < 1e-10
    logits, loss, grads = O.loss_and_grads(x, y, sd, **fmt(kw))
    assert rel_l2(logits.numpy(), GOLD[f"{tag}.train.logits"]) < 1e-10
    assert abs(float(loss) - float(GOLD[f"{tag}.train.loss"])) < 1e-10
    for k, g in grads.items():
        want = GOLD[f"{tag}.grad.{k}"]
        if np.abs(want).max() < 1e-12:
            assert g is None or float(g.abs().max()) < 1e-12
        else:
            assert rel_l2(g.numpy(), want) < 1e-9, k


def test_other_modes_fail_loudly():
    from fusion_gcn_amd.models.mmargcn.mmargcn import Model
    with pytest.raises(NotImplementedError):
        Model({"inertial": (8, 6)}, 5, None, mode="imu_signal_image")


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["value48", "sensor16", "value240", "value1956", "wide2048", "agcn_sensor16", "agcn_value48",
                                 "agcn_sensor652"])
def test_hip_imu_gcn_matches_the_oracle(tag):
    dev = torch.device("cuda:0")
    if tag in CASES:
        shape, classes, batch, kw = CASES[tag]
    elif tag == "value240":   # V = 240 nodes (not a multiple of 64: padded contraction), all three residual kinds, widths to 128
        shape, classes, batch = (40, 6), 27, 4
        kw = dict(gc_model="stgcn", graph_node_format="node_per_value", num_layers=5, inner_feature_dim=64)
    elif tag == "agcn_sensor652":   # the late-fusion configs' IMU branch: 326 x 2 sensor nodes, 3 features each, attention 652 x 652
        shape, classes, batch = (326, 6), 27, 2
        kw = dict(gc_model="agcn", graph_node_format="node_per_sensor", num_signals=2, num_layers=4, inner_feature_dim=64,
                  inter_signal_back_connections=True, include_additional_top_layer=True)
    elif tag == "wide2048":   # the config's widths: a Conv1d + BatchNorm residual into 2048 channels (1024-channel windows)
        shape, classes, batch = (8, 6), 27, 2
        kw = dict(gc_model="stgcn", graph_node_format="node_per_value", num_layers=4, inner_feature_dim=1024)
    else:                     # the UTD-MHAD config's node count (326 x 6 = 1956), narrow
        shape, classes, batch = (326, 6), 27, 2
        kw = dict(gc_model="stgcn", graph_node_format="node_per_value", num_layers=3, inner_feature_dim=32)
    model, sd = build(tag, shape, classes, kw)
    x, y = inputs(tag, shape, batch, classes)
    ref_eval = O.imu_gcn_forward(x, sd, train=False, **fmt(kw))
    ref_logits, ref_loss, ref_grads = O.loss_and_grads(x, y, sd, **fmt(kw))
    model = guarded.to(model, dev)
    model.eval()
    with torch.no_grad():
        got_eval = model(guarded.to(x.float(), dev)).cpu().double()
    assert rel_l2(got_eval.numpy(), ref_eval.numpy()) < 2e-5
    model.train()
    logits = model(guarded.to(x.float(), dev))
    loss = F.cross_entropy(logits, guarded.to(y, dev))
    loss.backward()
    assert rel_l2(logits.detach().cpu().double().numpy(), ref_logits.numpy()) < 2e-5
    assert abs(float(loss.detach()) - float(ref_loss)) < 2e-5 * max(1.0, abs(float(ref_loss)))
    scale = max(float(g.abs().max()) for g in ref_grads.values() if g is not None)
    for name, p in model.named_parameters():
        k = name.replace("_model.", "")
        want = ref_grads[k]
        got = p.grad.detach().cpu().double()
        if k.endswith(("residual.0.bias", "down.0.bias", "conv_d.0.bias", "conv_d.1.bias", "conv_d.2.bias")):
            # in front of a train-mode BatchNorm: exactly zero here, rounding noise in autograd
            assert float(got.abs().max()) == 0.0 and float(want.abs().max()) < 1e-9 * max(1.0, scale)
            continue
        if k.endswith(("conv_a.0.bias", "conv_a.1.bias", "conv_a.2.bias")):      # softmax shift invariance: analytically zero
            assert float(got.abs().max()) < 1e-5 * max(1.0, scale) and float(want.abs().max()) < 1e-9 * max(1.0, scale)
            continue
        # (a conv weight in front of a BatchNorm sums a mean-free gradient: cancellation leaves fp32 noise around 1e-3 there)
        tol = 2e-3 if k.endswith(("down.0.weight", "residual.0.weight")) else 5e-4
        assert rel_l2(got.numpy(), want.numpy()) < tol, (k, rel_l2(got.numpy(), want.numpy()))
    if tag in CASES:                                      # and against the reference's own numbers
        assert rel_l2(logits.detach().cpu().double().numpy(), GOLD[f"{tag}.train.logits"]) < 2e-5
        bn = dict(model.named_buffers())
        for k in GOLD.files:
            if k.startswith(f"{tag}.after."):
                name = "_model." + k[len(f"{tag}.after."):]
                assert rel_l2(bn[name].cpu().double().numpy(), GOLD[k]) < 1e-5, k


# ---- mode skeleton_imu_gcn_late_fusion: skeleton AGCN + IMU GCN (stgcn) + fusion + fc -----------------------------------------
LATE_KW = dict(gc_model="stgcn", graph_node_format="node_per_sensor", num_signals=2, num_layers=4, inner_feature_dim=64)
LATE_SHAPES = {"skeleton": (1, 16, 20, 3), "inertial": (8, 6)}


def late_build(double=False, gc_model="stgcn"):
    from fusion_gcn_amd.datasets.utd_mhad import constants as utd
    from fusion_gcn_amd.models.mmargcn.mmargcn import Model
    from fusion_gcn_amd.util import Graph
    model = Model(LATE_SHAPES, 27, Graph(utd.skeleton_edges, center_joint=utd.center_joint),
                  mode="skeleton_imu_gcn_late_fusion", **dict(LATE_KW, gc_model=gc_model))
    if double:
        model = model.double()
    filler.fill_state_dict(model.state_dict(), skip=("adj", "adj_a", "A"), rename=lambda k: k.replace("_model.", ""))
    sd = {k.replace("_model.", ""): (v.detach().double().clone() if v.is_floating_point() else v.detach().clone())
          for k, v in model.state_dict().items()}
    return model, sd


def late_inputs(batch=3):
    x = {"skeleton": torch.from_numpy(filler.skeleton_input("x.late.skeleton", (batch, *LATE_SHAPES["skeleton"]))).double(),
         "inertial": torch.from_numpy(filler.bellish("x.late.inertial", (batch, *LATE_SHAPES["inertial"]), scale=0.5)).double()}
    y = torch.from_numpy(filler.uniform("y.late", (batch,), 0, 27).astype(np.int64))
    return x, y


def late_oracle(x, sd, train=True):
    """late_fusion_models.py:67-75: both branches without fc, concatenate, fc."""
    from oracle import agcn_oracle as OA
    skel = OA.model_forward(x["skeleton"], {k[len("agcn."):]: v for k, v in sd.items() if k.startswith("agcn.")},
                            train=train, num_layers=LATE_KW["num_layers"])
    imu = O.imu_gcn_forward(x["inertial"], {k[len("imu_gcn."):]: v for k, v in sd.items() if k.startswith("imu_gcn.")},
                            graph_node_format="node_per_sensor", num_features=3, train=train)
    return F.linear(torch.cat([skel, imu], dim=-1), sd["fc.weight"], sd["fc.bias"])


def late_loss_and_grads(x, y, sd):
    params = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items()
              if v.is_floating_point() and not k.endswith(("running_mean", "running_var", ".adj", "adj_a"))}
    full = dict(sd)
    full.update(params)
    logits = late_oracle(x, full)
    loss = F.cross_entropy(logits, y)
    grads = torch.autograd.grad(loss, list(params.values()), allow_unused=True)
    return logits.detach(), loss.detach(), dict(zip(params.keys(), grads))


@pytest.mark.parametrize("gc_model", ["stgcn", "agcn"])
def test_late_fusion_oracle_matches_the_reference(gc_model):
    GOLD_ = GOLD
    tag = "late" if gc_model == "stgcn" else "late_agcn"
    model, sd = late_build(double=True, gc_model=gc_model)
    assert sorted(sd) == list(GOLD_[f"{tag}.keys"])
    x, y = late_inputs()
    assert np.array_equal(y.numpy(), GOLD[f"{tag}.labels"])
    assert rel_l2(late_oracle(x, sd, train=False).detach().numpy(), GOLD[f"{tag}.eval.logits"]) < 1e-10
    logits, loss, grads = late_loss_and_grads(x, y, sd)
    assert rel_l2(logits.numpy(), GOLD[f"{tag}.train.logits"]) < 1e-10
    assert abs(float(loss) - float(GOLD[f"{tag}.train.loss"])) < 1e-10
    for k, g in grads.items():
        want = float(GOLD[f"{tag}.gl2.{k}"])
        got = 0.0 if g is None else float(g.norm())
        assert abs(got - want) <= 1e-8 * max(1.0, want) + 1e-12, (k, got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("gc_model", ["stgcn", "agcn"])
def test_hip_late_fusion_matches_the_oracle(gc_model):
    dev = torch.device("cuda:0")
    tag = "late" if gc_model == "stgcn" else "late_agcn"
    model, sd = late_build(gc_model=gc_model)
    x, y = late_inputs()
    ref_logits, ref_loss, ref_grads = late_loss_and_grads(x, y, sd)
    ref_eval = late_oracle(x, sd, train=False).detach()
    model = guarded.to(model, dev)
    xg = {k: guarded.to(v.float(), dev) for k, v in x.items()}
    model.eval()
    with torch.no_grad():
        assert rel_l2(model(xg).cpu().double().numpy(), ref_eval.numpy()) < 5e-5
    model.train()
    logits = model(xg)
    loss = F.cross_entropy(logits, guarded.to(y, dev))
    loss.backward()
    assert rel_l2(logits.detach().cpu().double().numpy(), ref_logits.numpy()) < 5e-5
    assert abs(float(loss.detach()) - float(ref_loss)) < 1e-4
    assert rel_l2(logits.detach().cpu().double().numpy(), GOLD[f"{tag}.train.logits"]) < 5e-5
    for name, p in model.named_parameters():
        k = name.replace("_model.", "")
        want = ref_grads[k]
        got = p.grad.detach().cpu().double()
        wn = 0.0 if want is None else float(want.norm())
        if wn < 1e-9:                                    # analytically zero (biases in front of a train-mode BatchNorm, ...)
            assert float(got.norm()) < 1e-6, k
        else:
            assert abs(float(got.norm()) - wn) < 1e-2 * wn, (k, float(got.norm()), wn)   # as the cfg-3/4 fixtures: norms within 1 %


# ---- mode skeleton_imu_channel_fusion: IMU signals broadcast to every joint as extra input channels -----------------------------
def chan_build(double=False):
    from fusion_gcn_amd.datasets.utd_mhad import constants as utd
    from fusion_gcn_amd.models.mmargcn.mmargcn import Model
    from fusion_gcn_amd.util import Graph
    shapes = {"skeleton": (1, 16, 20, 3), "inertial": (16, 6)}
    model = Model(shapes, 27, Graph(utd.skeleton_edges, center_joint=utd.center_joint), mode="skeleton_imu_channel_fusion",
                  num_layers=4)
    if double:
        model = model.double()
    filler.fill_state_dict(model.state_dict(), skip=("adj_a", "A"), rename=lambda k: k.replace("_model.agcn.", ""))
    sd = {k.replace("_model.agcn.", ""): (v.detach().double().clone() if v.is_floating_point() else v.detach().clone())
          for k, v in model.state_dict().items()}
    x = {"skeleton": torch.from_numpy(filler.skeleton_input("x.chan.skeleton", (2, *shapes["skeleton"]))).double(),
         "inertial": torch.from_numpy(filler.bellish("x.chan.inertial", (2, *shapes["inertial"]), scale=0.5)).double()}
    return model, sd, x


def chan_oracle(x, sd, train):
    from oracle import agcn_oracle as OA
    imu = x["inertial"].unsqueeze(1).unsqueeze(3).expand(-1, x["skeleton"].shape[1], -1, x["skeleton"].shape[3], -1)
    return OA.model_forward(torch.cat([x["skeleton"], imu], dim=-1), sd, train=train, num_layers=4)


def test_channel_fusion_oracle_matches_the_reference():
    model, sd, x = chan_build(double=True)
    assert sorted(k.replace("_model.", "") for k in model.state_dict()) == list(GOLD["chan.keys"])
    assert rel_l2(chan_oracle(x, sd, False).detach().numpy(), GOLD["chan.eval.logits"]) < 1e-10
    assert rel_l2(chan_oracle(x, sd, True).detach().numpy(), GOLD["chan.train.logits"]) < 1e-10


@pytest.mark.gpu
def test_hip_channel_fusion_matches_the_reference():
    dev = torch.device("cuda:0")
    model, sd, x = chan_build()
    model = guarded.to(model, dev)
    xg = {k: guarded.to(v.float(), dev) for k, v in x.items()}
    model.eval()
    with torch.no_grad():
        assert rel_l2(model(xg).cpu().double().numpy(), chan_oracle(x, sd, False).detach().numpy()) < 5e-5
    model.train()
    logits = model(xg)
    assert rel_l2(logits.detach().cpu().double().numpy(), chan_oracle(x, sd, True).detach().numpy()) < 5e-5
    assert rel_l2(logits.detach().cpu().double().numpy(), GOLD["chan.train.logits"]) < 5e-5
    logits.square().sum().backward()                       # the 9-channel input block runs its backward
    assert all(torch.isfinite(p.grad).all() for p in model.parameters())
