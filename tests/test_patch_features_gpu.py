"""The RGB patch-feature input stage (fgcn_patch.hip, block.patch_input) and the four patch-feature modes on the GPU.

Kernel level: fgcn_patch_input_fwd (z and data_bn's statistics partials) and fgcn_patch_input_bwd (dW1, db1, dW2, db2) against float64
torch formulas in the four math modes -- f32-class modes at tests/test_kernels_gpu.py's tolerances, bf16 at SURVEY.md section 7's
contract.  Model level: each mode in train mode against a float64 CPU composition (torch reducer, zero pad, combine, then the AGCN
oracle), with the ReLU-flip accounting of tests/test_block_model_gpu.py; eval mode; fused against composed input stage; a verified
HIP-graph step; a FlatOptimizer Adam step; ClipBatches over a skeleton + rgb feature-file pair."""
import copy
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2
from fusion_gcn_amd import _lib, ops
from fusion_gcn_amd.datasets.utd_mhad import constants as utd
from fusion_gcn_amd.models.mmargcn.mmargcn import Model
from fusion_gcn_amd.util import Graph
from oracle import agcn_oracle as O
from oracle import relu_masks as RM

import guarded
from guarded import guarded_allocations  # noqa: F401  (the fixture)

# every test runs on guarded allocations: NaN around each tensor the host layer creates, margins verified at teardown (tests/guarded.py)
pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_allocations")]

FWD_TOL, RED_TOL = 3e-6, 2e-5          # tests/test_kernels_gpu.py
DEV = "cuda:0"
GROUP_EDGES = ["1, 0", "2, 0", "3, 0", "4, 0", "1, 2", "3, 4"]
IMU_KW = dict(num_imu_joints=2, imu_enhanced_mode="append_center")


def _rand(shape, gen, scale=1.0):
    return (torch.randn(shape, generator=gen, dtype=torch.float64) * scale)


def _reducer64(P, H, Q, gen):
    return (_rand((H, P), gen, 1 / math.sqrt(P)), _rand((H,), gen, 0.1), _rand((Q, H), gen, 1 / math.sqrt(H)), _rand((Q,), gen, 0.1))


def _combine(s, q, fusion):
    if s is None:
        return q
    return {"concatenate": lambda: torch.cat((s, q), -1), "sum": lambda: s + q, "product": lambda: s * q,
            "average": lambda: torch.stack((s, q), -1).mean(-1)}[fusion]()


def _ref_z(s, p, W, V, fusion):
    N, M, T, Vp, P = p.shape
    q = p if W is None else (p @ W[0].T + W[1]) @ W[2].T + W[3]
    q = F.pad(q, (0, 0, 0, V - Vp))
    return _combine(s, q, fusion)


def _ref_stats(z):
    N, M, T, V, C = z.shape
    tiles = []
    for n in range(N):
        for t0 in range(0, T, 32):
            blk = z[n, :, t0:t0 + 32].permute(1, 0, 2, 3).reshape(-1, M * V * C)
            tiles.append(torch.stack((blk.sum(0), (blk ** 2).sum(0))))
    return torch.stack(tiles)


def _dev(t):
    return None if t is None else guarded.put(t.float(), device=DEV)


MATH = ["f32", "bf16x3", "f16x2", "bf16"]
# (fusion, reducer (H, Q) or None, P, Vp, V, Cs)
CASES = [("concatenate", (128, 6), 512, 20, 20, 3), ("concatenate", (128, 6), 512, 20, 22, 3), ("concatenate", (512, 3), 512, 20, 22, 3),
         ("concatenate", (128, 6), 1024, 20, 20, 3), ("concatenate", None, 512, 20, 22, 3), ("sum", (128, 3), 512, 20, 22, 3),
         ("product", (512, 3), 512, 20, 20, 3), ("average", (128, 6), 1024, 20, 22, 6), ("product", None, 512, 18, 20, 512)]


def _case_ids():
    return [f"{f}-{'id' if r is None else f'{r[0]}x{r[1]}'}-P{P}-V{Vp}of{V}" for f, r, P, Vp, V, _ in CASES]


@pytest.mark.parametrize("mode", MATH)
@pytest.mark.parametrize("case", CASES, ids=_case_ids())
def test_patch_input_kernels(case, mode):
    fusion, red, P, Vp, V, Cs = case
    gen = torch.Generator().manual_seed(7)
    N, M, T = 2, 1, 40                                       # T = 40: a partial data_bn tile
    p = _rand((N, M, T, Vp, P), gen)
    s = _rand((N, M, T, V, Cs), gen)
    W = None if red is None else _reducer64(P, red[0], red[1], gen)
    z_ref = _ref_z(s, p, W, V, fusion)
    with ops.math_mode(mode):
        wd = (None,) * 4 if W is None else tuple(_dev(w) for w in W)
        z, part = ops.patch_input_fwd(_dev(s), _dev(p), *wd, V=V, fusion=fusion)
        torch.cuda.synchronize()
        assert z.shape == z_ref.shape
        # the statistics partials are fgcn_data_bn_stats over z itself: bitwise
        assert torch.equal(part, ops.data_bn_stats(z))
        bf = mode == "bf16" and W is not None
        assert rel_l2(z.cpu().numpy(), z_ref.numpy()) < (1e-2 if bf else FWD_TOL)
        assert rel_l2(part.cpu().numpy(), _ref_stats(z_ref).numpy()) < (1e-2 if bf else RED_TOL)
        if W is None:
            return
        dz = _rand(z_ref.shape, gen)
        Wr = [w.clone().requires_grad_(True) for w in W]
        zr = _ref_z(s, p, Wr, V, fusion)
        want = torch.autograd.grad((zr * dz).sum(), Wr)
        got = ops.patch_input_bwd(_dev(dz), _dev(s), _dev(p), wd[0], wd[1], wd[2], fusion=fusion)
        again = ops.patch_input_bwd(_dev(dz), _dev(s), _dev(p), wd[0], wd[1], wd[2], fusion=fusion)
        torch.cuda.synchronize()
        for a, b in zip(got, again):
            assert torch.equal(a, b)                          # fixed-order slab sums: bitwise reproducible
        for name, a, b in zip(("dW1", "db1", "dW2", "db2"), got, want):
            a = a.cpu().double()
            if bf:
                cos = float(torch.dot(a.flatten(), b.flatten()) / (a.norm() * b.norm()))
                assert cos > 0.98 and rel_l2(a.numpy(), b.numpy()) < 5e-2, (name, cos)
            else:
                assert rel_l2(a.numpy(), b.numpy()) < RED_TOL, name


def test_unsupported_sizes_raise():
    gen = torch.Generator().manual_seed(1)
    p, s = _dev(_rand((1, 1, 4, 20, 500), gen)), _dev(_rand((1, 1, 4, 20, 3), gen))
    W = [_dev(w) for w in _reducer64(500, 128, 6, gen)]
    with pytest.raises(_lib.FgcnError, match="unsupported reducer"):
        ops.patch_input_fwd(s, p, *W, V=20, fusion="concatenate")
    p = _dev(_rand((1, 1, 4, 20, 512), gen))
    W = [_dev(w) for w in _reducer64(512, 128, 40, gen)]
    with pytest.raises(_lib.FgcnError, match="unsupported reducer"):
        ops.patch_input_fwd(s, p, *W, V=20, fusion="concatenate")
    W = [_dev(w) for w in _reducer64(512, 128, 6, gen)]
    with pytest.raises(_lib.FgcnError, match="Q == Cs"):
        ops.patch_input_fwd(s, p, *W, V=20, fusion="sum")
    with pytest.raises(_lib.FgcnError, match="unsupported reducer"):
        ops.patch_input_bwd(_dev(_rand((1, 1, 4, 20, 9), gen)), s, p, W[0], W[1], _dev(_rand((40, 128), gen)), fusion="concatenate")


# ---- model level ----------------------------------------------------------------------------------------------------------------
MODES = {
    "rgb_patch_features": dict(shapes={"rgb": (1, 32, 20, 512)}, kw={}),
    "rgb_patch_groups_features": dict(shapes={"rgb": (1, 32, 5, 512)}, kw=dict(rgb_patch_groups_edges=GROUP_EDGES)),
    "skeleton_rgb_patch_features_early_fusion": dict(shapes={"skeleton": (1, 32, 20, 3), "rgb": (1, 32, 20, 512)},
                                                     kw=dict(patch_feature_hidden_dim=128, patch_feature_output_dim=6)),
    "skeleton_imu_rgb_patch_features_early_fusion": dict(shapes={"skeleton": (1, 32, 22, 3), "rgb": (1, 32, 20, 512)},
                                                         kw=dict(patch_feature_hidden_dim=128, patch_feature_output_dim=6, **IMU_KW)),
}
CLASSES = 27


def _model(mode, seed=3, **extra):
    torch.manual_seed(seed)
    spec = MODES[mode]
    return Model(spec["shapes"], CLASSES, Graph(utd.skeleton_edges, center_joint=utd.center_joint), mode=mode,
                 **{**spec["kw"], **extra})._model


def _inputs(mode, N=2, seed=11):
    gen = torch.Generator().manual_seed(seed)
    x = {k: _rand((N, *v), gen).float() for k, v in MODES[mode]["shapes"].items()}
    y = torch.randint(0, CLASSES, (N,), generator=gen)
    return x, y


def _oracle(model, x, y, train=True):
    """float64 CPU composition: torch reducer, zero pad, combine, then the AGCN oracle -> gradient_parity_report's oracle dict."""
    sd = {k: v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu().clone() for k, v in model.state_dict().items()}
    agcn_sd = {k[5:]: v for k, v in sd.items() if k.startswith("agcn.")}
    params = {k: v.clone().requires_grad_(True) for k, v in agcn_sd.items()
              if v.is_floating_point() and not k.endswith(("running_mean", "running_var", "adj_a"))}
    red = {k: v.clone().requires_grad_(True) for k, v in sd.items() if k.startswith("patch_feature_dim_reducer.")}
    full = dict(agcn_sd)
    full.update(params)
    if "skeleton" in x:
        p = x["rgb"].double()
        W = None if not red else [red[f"patch_feature_dim_reducer.{i}.{n}"] for i in (0, 1) for n in ("weight", "bias")]
        z = _ref_z(x["skeleton"].double(), p, W, model.num_joints, model.fusion_type)
    else:
        z = x["rgb"].double()
    cap = {}
    logits = O.model_forward(z, full, train=train, stats=O.Stats(), capture=cap)
    loss = F.cross_entropy(logits, y)
    names = [n for n, _ in model.named_parameters()]
    srcs = {**red, **{"agcn." + k: v for k, v in params.items()}}
    grads = dict(zip(srcs, torch.autograd.grad(loss, list(srcs.values()), allow_unused=True)))
    flat = torch.cat([grads[n].double().flatten() for n in names])
    nblocks = sum(1 for k in cap if k.endswith(".g"))
    return dict(logits=logits.detach(), loss=float(loss), flat=flat, images=RM.oracle_sign_images(cap, nblocks))


def _to_dev(x):
    return {k: guarded.to(v, DEV) for k, v in x.items()} if "skeleton" in x else guarded.to(x["rgb"], DEV)


# the patch-only modes have no reducer and no skeleton: data_bn is their input stage on either setting of patch_input_fused
PARITY = [(m, True) for m in MODES] + [(m, False) for m in MODES if m.startswith("skeleton")]


@pytest.mark.parametrize("math_mode", ["f32", "bf16x3"])
@pytest.mark.parametrize("mode,fused", PARITY)
def test_mode_matches_the_float64_composition(mode, fused, math_mode):
    _parity(mode, fused, math_mode, _model(mode))


@pytest.mark.parametrize("mode", ["skeleton_rgb_patch_features_early_fusion", "skeleton_imu_rgb_patch_features_early_fusion"])
def test_identity_reducer_mode_matches_the_float64_composition(mode):
    """no reducer (output dim = input dim): the first block takes 3 + 512 = 515 channels, padded to 516"""
    model = _model(mode, patch_feature_hidden_dim=512, patch_feature_output_dim=512)
    assert model.patch_feature_dim_reducer is None and model.agcn.l0.cfg.cx == 516
    _parity(mode, True, "f32", model)


def _parity(mode, fused, math_mode, model):
    x, y = _inputs(mode)
    ora = _oracle(model, x, y)
    model = guarded.to(model, DEV).train()
    with ops.context(math_mode) as ctx:
        ctx.paths.patch_input_fused = fused
        rep = RM.gradient_parity_report(model, _to_dev(x), guarded.to(y, DEV), oracle=ora)
    print(f"[{mode} fused={fused} {math_mode}] logits {rep['logits_err']:.2e} | flips {rep['flips']} of {rep['decisions']} | "
          f"grad {rep['err_plain']:.2e} / {rep['err_injected']:.2e}")
    assert rep["logits_err"] < 1e-5 and rep["loss_err"] < 1e-5, rep
    assert rep["err_injected"] < 1e-4, rep
    assert rep["err_plain"] <= 1e-4 + 2.0 * math.sqrt(rep["flips"] / (rep["decisions"] / 20)), rep


@pytest.mark.parametrize("mode", list(MODES))
def test_eval_mode_uses_running_statistics(mode):
    model = _model(mode)
    x, y = _inputs(mode)
    with torch.no_grad():
        for k, v in model.state_dict().items():
            if k.endswith("running_var"):
                v.uniform_(0.5, 2.0)
            elif k.endswith("running_mean"):
                v.uniform_(-0.3, 0.3)
    sd = {k: v.detach().double() if v.is_floating_point() else v.detach().clone() for k, v in model.state_dict().items()}
    agcn_sd = {k[5:]: v for k, v in sd.items() if k.startswith("agcn.")}
    if "skeleton" in x:
        W = None if model.patch_feature_dim_reducer is None else [sd[f"patch_feature_dim_reducer.{i}.{n}"] for i in (0, 1)
                                                                  for n in ("weight", "bias")]
        z = _ref_z(x["skeleton"].double(), x["rgb"].double(), W, model.num_joints, model.fusion_type)
    else:
        z = x["rgb"].double()
    want = O.model_forward(z, agcn_sd, train=False)
    model = guarded.to(model, DEV).eval()
    with torch.no_grad():
        got = model(_to_dev(x))
    assert rel_l2(got.cpu().numpy(), want.numpy()) < 1e-5


@pytest.mark.parametrize("mode", ["skeleton_rgb_patch_features_early_fusion", "skeleton_imu_rgb_patch_features_early_fusion"])
@pytest.mark.parametrize("train", [True, False])
def test_fused_and_composed_input_stage_agree(mode, train):
    """paths.patch_input_fused on and off: the same network input, running statistics and reducer gradients (the A/B routes).
    Compared at the input stage itself: past it, the blocks' ReLU decisions turn float32 rounding differences into flips."""
    from fusion_gcn_amd.block import patch_input
    base = guarded.to(_model(mode), DEV).train(train)
    x, _ = _inputs(mode)
    xd = _to_dev(x)
    gen = torch.Generator().manual_seed(2)
    out = {}
    for fused in (True, False):
        model = copy.deepcopy(base)
        with ops.context("f32") as ctx:
            ctx.paths.patch_input_fused = fused
            h = patch_input(xd["skeleton"], xd["rgb"], model.patch_feature_dim_reducer, model.agcn.data_bn, model.num_joints,
                            model.fusion_type)
            g = guarded.to(torch.randn(h.shape, generator=gen), DEV) if not out else out[True][3]
            (h * g).sum().backward()
        bn = model.agcn.data_bn
        out[fused] = (h.detach().cpu(), [p.grad.cpu() for p in model.patch_feature_dim_reducer.parameters()],
                      (bn.running_mean.cpu(), bn.running_var.cpu(), int(bn.num_batches_tracked)), g)
    (h1, g1, b1, _), (h0, g0, b0, _) = out[True], out[False]
    assert h1.shape == h0.shape and rel_l2(h1.numpy(), h0.numpy()) < 1e-5
    # (train mode: the bias gradients are zero up to rounding -- data_bn removes a per-channel constant -- so the four are compared as one)
    assert rel_l2(torch.cat([a.flatten() for a in g1]).numpy(), torch.cat([b.flatten() for b in g0]).numpy()) < 1e-4
    assert float((b1[0] - b0[0]).abs().max()) < 1e-6 and float((b1[1] - b0[1]).abs().max()) < 1e-6 and b1[2] == b0[2]


@pytest.mark.parametrize("mode", ["skeleton_rgb_patch_features_early_fusion", "rgb_patch_groups_features"])
def test_graph_step_replays_the_eager_step_and_adam_updates(mode):
    from fusion_gcn_amd.optim import FlatOptimizer
    from fusion_gcn_amd.session.procedures import GraphStep
    model = guarded.to(_model(mode), DEV).train()
    x, y = _inputs(mode)
    xd, yd = _to_dev(x), guarded.to(y, DEV)
    eager = copy.deepcopy(model)
    step = GraphStep(verify=True)
    opt = FlatOptimizer(model.parameters(), "ADAM", 1e-3, weight_decay=0.01, grads=None)
    for _ in range(2):
        opt.zero_grad()
        _, loss = step.forward(model, F.cross_entropy, xd, yd)
        step.backward(loss)
        opt.step()
    assert step.replays == 2
    eopt = torch.optim.Adam(eager.parameters(), 1e-3, weight_decay=0.01)
    for _ in range(2):
        eopt.zero_grad()
        eloss = F.cross_entropy(eager(xd), yd)
        eloss.backward()
        eopt.step()
    for (n, a), b in zip(model.named_parameters(), eager.parameters()):
        assert float((a - b).abs().max()) <= 1e-5 * max(1e-3, float(b.abs().max())) + 1e-6, n


def test_clip_batches_feed_skeleton_rgb_early_fusion(tmp_path):
    from fusion_gcn_amd.data import ClipBatches, MultiModalDataset, NumpyDatasetLoader, NumpyWriter
    import os
    rng = np.random.default_rng(0)
    n = 6
    arrays = {"skeleton": rng.standard_normal((n, 1, 32, 20, 3)).astype(np.float32),
              "rgb": rng.standard_normal((n, 1, 32, 20, 512)).astype(np.float32)}
    for name, a in arrays.items():
        with NumpyWriter(os.path.join(tmp_path, f"{name}_train_features.npy"), np.float32, a.shape) as w:
            for s in a:
                w.collect_next(s)
    np.save(os.path.join(tmp_path, "train_labels.npy"), rng.integers(0, CLASSES, n))
    ds = MultiModalDataset([(str(tmp_path), NumpyDatasetLoader())], "train")
    model = guarded.to(_model("skeleton_rgb_patch_features_early_fusion"), DEV).train()
    seen = 0
    for feats, labels, idx in ClipBatches(ds, 3, device=DEV):
        assert set(feats) == {"skeleton", "rgb"}
        loss = F.cross_entropy(model(feats), labels)
        loss.backward()
        assert torch.isfinite(loss)
        direct = {k: guarded.to(torch.from_numpy(arrays[k][idx.cpu().numpy()]), DEV) for k in arrays}
        assert torch.equal(feats["rgb"], direct["rgb"]) and torch.equal(feats["skeleton"], direct["skeleton"])
        seen += labels.numel()
    assert seen == n
    assert model.patch_feature_dim_reducer[0].weight.grad is not None
