"""Block- and model-level parity on the MI355X: the HIP-backed modules (fusion_gcn_amd.models) against the CPU
oracle (float64) on identical filler-generated parameters and inputs, and against the committed golden vectors
produced by the reference itself.

Tolerances (north star: <= 1e-3 relative, fp32): forward activations / logits <= 2e-5 rel-L2 per block, <= 1e-4
for the 10-block model; backward per block <= 2e-4 with the ReLU masks of the two implementations compared
(a flipped mask is reported, not hidden); end-to-end gradients <= 2e-3 (the fp32 noise floor of the reference
against itself is 3e-4..1.4e-3) with analytically-zero gradients checked absolutely."""
import numpy as np
import pytest
import torch

from conftest import rel_l2
from oracle import agcn_oracle as O
from oracle import filler, graph_oracle
from oracle import relu_masks as RM

import guarded
from guarded import guarded_allocations  # noqa: F401  (the fixture)

# every test runs on guarded allocations: NaN around each tensor the host layer creates, margins verified at teardown (tests/guarded.py)
pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_allocations")]


def dev():
    return torch.device("cuda:0")


def ntu_adj():
    from fusion_gcn_amd.datasets.ntu_rgb_d import constants as ntu
    return graph_oracle.spatial_partition_stack(ntu.skeleton_edges)


def adj_for(v):
    from fusion_gcn_amd.datasets.mmact import constants as mmact
    from fusion_gcn_amd.datasets.utd_mhad import constants as utd
    if v == 25:
        return ntu_adj()
    if v == 18:
        return graph_oracle.spatial_partition_stack(mmact.skeleton_edges)
    if v == 20:
        return graph_oracle.spatial_partition_stack(utd.skeleton_edges)
    if v == 22:
        return graph_oracle.spatial_partition_stack(
            graph_oracle.imu_fusion_edges(utd.skeleton_edges, 20, "append_center", 2, center_joint=1))
    if v == 27:
        from fusion_gcn_amd.datasets.ntu_rgb_d import constants as ntu
        return graph_oracle.spatial_partition_stack(
            graph_oracle.imu_fusion_edges(ntu.skeleton_edges, 25, "append_center", 2, center_joint=20))
    raise KeyError(v)


def fill_module(mod, prefix=""):
    filler.fill_state_dict(mod.state_dict(), prefix=prefix)


def oracle_sd(mod, prefix="", dtype=torch.float64):
    return {prefix + k: (v.detach().cpu().to(dtype) if v.is_floating_point() else v.detach().cpu().clone())
            for k, v in mod.state_dict().items()}


def check_gradients_with_flip_accounting(model, x_dev, labels_dev, x64, labels, sd64, ref, tag, strip=""):
    """The end-to-end gradient is a discontinuous function of the 20 ReLU sign patterns (oracle/relu_masks.py), so it is pinned in
    two parts: (a) with the ORACLE's ReLU decisions injected into the backward's sign images the difference is arithmetic only:
    flat gradient <= 1e-4 against the float64 oracle AND every parameter-gradient norm within 5e-3 of the REFERENCE's own -- the
    flat bound is the accuracy statement; the per-parameter one catches a wrong factor on a small parameter, which the flat norm
    would not see, and is as tight as float32 through a ten-block backward allows for the worst-conditioned ones (measured: 2.5e-3
    on l0.gcn1.conv_a.0.weight, a 9e-4-norm gradient behind the first block's attention softmax; 4.6e-4 on data_bn.bias; <= 2e-4
    elsewhere)
    (tests/golden, written by the imported reference -- whose float64 decisions are the oracle's); (b) as is, the error is bounded
    by what the counted flips explain.  Replaces the former 'flat gradient < 3e-3, norms within 1 %' bounds, which only said
    'somewhere near the flip noise'."""
    import math
    names = [n.replace(strip, "") if strip else n for n, _ in model.named_parameters()]
    oracle = RM.oracle_side(x64, labels, sd64, names)
    rep = RM.gradient_parity_report(model, x_dev, labels_dev, oracle=oracle, keep_grads=True)
    print(f"[{tag}] logits {rep['logits_err']:.2e} | ReLU flips {rep['flips']} of {rep['decisions']} | flat-grad rel-L2: as is "
          f"{rep['err_plain']:.2e}, with the oracle's decisions {rep['err_injected']:.2e}")
    assert rep["logits_err"] < 1e-5 and rep["loss_err"] < 1e-5, rep
    assert rep["err_injected"] < 1e-4, rep
    assert rep["err_plain"] <= 1e-4 + 2.0 * math.sqrt(rep["flips"] / (rep["decisions"] / 20)), rep
    for (n_, p), key in zip(model.named_parameters(), names):
        want = float(ref[f"{tag}.gl2.{key}"]) if f"{tag}.gl2.{key}" in ref else float(ref[f"{tag}.gl2.{n_}"])
        if key.endswith(ZERO_GRAD_SUFFIXES) or want < 1e-9:
            continue
        assert abs(float(p.grad.norm()) - want) <= 5e-3 * want, (n_, float(p.grad.norm()), want)
    model.zero_grad(set_to_none=True)
    return rep


ZERO_GRAD_SUFFIXES = ("conv_d.0.bias", "conv_d.1.bias", "conv_d.2.bias", "tcn1.conv.bias", "down.0.bias",
                      "residual.conv.bias", "conv_a.0.bias", "conv_a.1.bias", "conv_a.2.bias")


def compare_grads(got: dict, want: dict, tol: float, scale_ref: float):
    worst = ("", 0.0)
    for k, w in want.items():
        g = got[k]
        w = np.asarray(w, dtype=np.float64)
        g = np.asarray(g, dtype=np.float64).reshape(w.shape)
        if k.endswith(ZERO_GRAD_SUFFIXES):
            # analytically zero in train mode (bias in front of a BatchNorm / softmax shift invariance)
            assert np.abs(g).max() <= 1e-4 * scale_ref, (k, np.abs(g).max(), scale_ref)
            continue
        err = rel_l2(g, w)
        if err > worst[1]:
            worst = (k, err)
        assert err < tol, (k, err)
    return worst


@pytest.mark.parametrize("name,cin,cout,stride,residual,V,T,fused", [
    ("first", 3, 64, 1, False, 25, 12, True),
    ("identity64", 64, 64, 1, True, 25, 12, True),
    ("identity64_unfused", 64, 64, 1, True, 18, 9, False),
    ("down_s2", 64, 128, 2, True, 22, 13, True),
    ("identity128", 128, 128, 1, True, 25, 8, True),
    ("down_s2_256", 128, 256, 2, True, 27, 10, True),
    ("identity256", 256, 256, 1, True, 20, 6, True),
])
def test_block_forward_backward_vs_oracle(name, cin, cout, stride, residual, V, T, fused):
    from fusion_gcn_amd.models.mmargcn.agcn import SpatialTemporalConv
    B = 3
    adj = adj_for(V)
    blk = SpatialTemporalConv(cin, cout, adj, stride=stride, residual=residual, fused_spatial=fused)
    fill_module(blk, "l0.")
    sd = oracle_sd(blk, "l0.")
    blk = guarded.to(blk, dev())
    x = torch.from_numpy(filler.bellish(f"x.blk.{name}", (B, cin, T, V))).double()      # oracle layout (B, C, T, V)
    Tp = (T - 1) // stride + 1
    probe = torch.from_numpy(filler.uniform(f"probe.blk.{name}", (B, cout, Tp, V), -1, 1)).double()

    # ---- oracle (float64) ----------------------------------------------------------------------------------------
    params = {k: v.clone().requires_grad_(True) for k, v in sd.items()
              if v.is_floating_point() and not k.endswith(("running_mean", "running_var", "adj_a"))}
    live = dict(sd)
    live.update(params)
    xo = x.clone().requires_grad_(True)
    stats = O.Stats()
    out_o, adj_c = O.st_block(xo, live, "l0", stride, residual, True, stats)
    grads_o = torch.autograd.grad((out_o * probe).sum(), [xo] + list(params.values()), allow_unused=True)
    want = {k[3:]: g.numpy() for k, g in zip(params.keys(), grads_o[1:]) if g is not None}

    # ---- HIP path ------------------------------------------------------------------------------------------------
    blk.train()
    xg = guarded.to(x.float(), dev()).requires_grad_(True)
    out_g = blk.forward_nchw(xg)
    assert out_g.shape == out_o.shape
    fwd_err = rel_l2(out_g.detach().cpu().numpy(), out_o.detach().numpy())
    assert fwd_err < 2e-5, fwd_err
    c_err = rel_l2(torch.stack(blk.gcn1.adj_c, 1).cpu().numpy(), torch.stack(adj_c, 1).detach().numpy())
    assert c_err < 1e-5, c_err
    flips = int(((out_g.detach().cpu() > 0) != (out_o.detach() > 0)).sum())
    (out_g * guarded.to(probe.float(), dev())).sum().backward()
    tol = 2e-4 if flips == 0 else 5e-3
    dx_err = rel_l2(xg.grad.cpu().numpy(), grads_o[0].numpy())
    assert dx_err < tol, (dx_err, flips)
    got = {n: p.grad.detach().cpu().numpy() for n, p in blk.named_parameters()}
    scale_ref = max(float(np.abs(v).max()) for v in want.values())
    worst = compare_grads(got, want, tol, scale_ref)
    # BatchNorm running statistics after one training step
    for k, v in stats.updates.items():
        if k.endswith(("running_mean", "running_var")):
            assert rel_l2(blk.state_dict()[k[3:]].cpu().numpy(), v.numpy()) < 1e-5, k
        elif k.endswith("num_batches_tracked"):
            assert int(blk.state_dict()[k[3:]]) == int(v)
    print(f"[{name}] fwd {fwd_err:.2e} dx {dx_err:.2e} worst-param {worst} relu-flips {flips}")

    # ---- eval mode uses the running statistics ---------------------------------------------------------------------
    blk.eval()
    sd_eval = oracle_sd(blk, "l0.")
    with torch.no_grad():
        out_e = blk.forward_nchw(guarded.to(x.float(), dev()))
    want_e, _ = O.st_block(x, sd_eval, "l0", stride, residual, False)
    assert rel_l2(out_e.cpu().numpy(), want_e.numpy()) < 2e-5


def _random_tree_adjacency(V, seed):
    rng = np.random.default_rng(seed)
    edges = [(int(rng.integers(0, i)), i) for i in range(1, V)]          # a random tree over V joints, root 0
    return graph_oracle.spatial_partition_stack(edges)


@pytest.mark.parametrize("seed", range(12))
def test_block_random_shapes_vs_oracle(seed):
    """Seeded sweep over joint counts (5..32, random skeleton trees), frame counts (1..20), batch sizes and the block
    variants: forward, input gradient and every parameter gradient against the float64 oracle, train mode."""
    from fusion_gcn_amd.models.mmargcn.agcn import SpatialTemporalConv
    rng = np.random.default_rng(1000 + seed)
    V, T, B = int(rng.integers(5, 33)), int(rng.integers(1, 21)), int(rng.integers(1, 5))
    cin, cout, stride, residual = [(3, 64, 1, False), (64, 64, 1, True), (64, 128, 2, True), (128, 128, 1, True),
                                   (128, 256, 2, True), (256, 256, 1, True), (64, 64, 1, False), (64, 128, 1, True)][seed % 8]
    if T == 1 and stride == 2:
        T = 2
    adj = _random_tree_adjacency(V, seed)
    blk = SpatialTemporalConv(cin, cout, adj, stride=stride, residual=residual)
    fill_module(blk, "l0.")
    sd = oracle_sd(blk, "l0.")
    blk = guarded.to(blk, dev()).train()
    x = torch.from_numpy(filler.bellish(f"x.rnd.{seed}", (B, cin, T, V))).double()
    Tp = (T - 1) // stride + 1
    probe = torch.from_numpy(filler.uniform(f"probe.rnd.{seed}", (B, cout, Tp, V), -1, 1)).double()
    params = {k: v.clone().requires_grad_(True) for k, v in sd.items()
              if v.is_floating_point() and not k.endswith(("running_mean", "running_var", "adj_a"))}
    live = dict(sd)
    live.update(params)
    xo = x.clone().requires_grad_(True)
    out_o, _ = O.st_block(xo, live, "l0", stride, residual, True, O.Stats())
    grads_o = torch.autograd.grad((out_o * probe).sum(), [xo] + list(params.values()), allow_unused=True)
    want = {k[3:]: g.numpy() for k, g in zip(params.keys(), grads_o[1:]) if g is not None}
    xg = guarded.to(x.float(), dev()).requires_grad_(True)
    out_g = blk.forward_nchw(xg)
    fwd_err = rel_l2(out_g.detach().cpu().numpy(), out_o.detach().numpy())
    assert fwd_err < 2e-5, (fwd_err, V, T, B)
    flips = int(((out_g.detach().cpu() > 0) != (out_o.detach() > 0)).sum())
    (out_g * guarded.to(probe.float(), dev())).sum().backward()
    tol = 2e-4 if flips == 0 else 5e-3
    dx_err = rel_l2(xg.grad.cpu().numpy(), grads_o[0].numpy())
    assert dx_err < tol, (dx_err, flips, V, T, B)
    got = {n: p.grad.detach().cpu().numpy() for n, p in blk.named_parameters()}
    scale_ref = max(float(np.abs(v).max()) for v in want.values())
    worst = compare_grads(got, want, tol, scale_ref)
    print(f"[seed {seed}: V={V} T={T} B={B} {cin}->{cout} s{stride} res={residual}] fwd {fwd_err:.2e} dx {dx_err:.2e} "
          f"worst-param {worst} relu-flips {flips}")


@pytest.mark.parametrize("kt,stride,T", [(3, 2, 12), (7, 2, 9), (11, 2, 8), (3, 1, 6)])
def test_block_with_other_temporal_kernels_vs_oracle(kt, stride, T):
    """Temporal kernels the model never uses (kt = 3 / 7 / 11 with stride 2: odd padding): temporal_fwd / temporal_dgrad
    fall back to the row GEMM there, which records no operand maxima -- in math mode f16x2 the weight gradient must then run its
    bf16x3 form instead of scaling by a zero-initialised slot (block.py: g_amax / du_amax).  Forward and all gradients vs float64."""
    from fusion_gcn_amd.models.mmargcn.agcn import SpatialTemporalConv, TemporalConv
    V, B, cin, cout = 25, 2, 64, 128 if stride == 2 else 64
    blk = SpatialTemporalConv(cin, cout, ntu_adj(), stride=stride, residual=True)
    blk.tcn1 = TemporalConv(cout, cout, kernel_size=kt, stride=stride)
    fill_module(blk, "l0.")
    sd = oracle_sd(blk, "l0.")
    blk = guarded.to(blk, dev()).train()
    x = torch.from_numpy(filler.bellish(f"x.kt.{kt}.{stride}.{T}", (B, cin, T, V))).double()
    Tp = (T - 1) // stride + 1
    # gradients on a scale where an unscaled f16 split would lose them (2^-20) and one where it would overflow (2^18)
    for scale in (2.0 ** -20, 2.0 ** 18):
        probe = torch.from_numpy(filler.uniform(f"probe.kt.{kt}", (B, cout, Tp, V), -1, 1)).double() * scale
        params = {k: v.clone().requires_grad_(True) for k, v in sd.items()
                  if v.is_floating_point() and not k.endswith(("running_mean", "running_var", "adj_a"))}
        live = dict(sd)
        live.update(params)
        xo = x.clone().requires_grad_(True)
        out_o, _ = O.st_block(xo, live, "l0", stride, True, True, O.Stats())
        grads_o = torch.autograd.grad((out_o * probe).sum(), [xo] + list(params.values()), allow_unused=True)
        want = {k[3:]: g.numpy() for k, g in zip(params.keys(), grads_o[1:]) if g is not None}
        blk.zero_grad()
        xg = guarded.to(x.float(), dev()).requires_grad_(True)
        out_g = blk.forward_nchw(xg)
        assert rel_l2(out_g.detach().cpu().numpy(), out_o.detach().numpy()) < 2e-5
        flips = int(((out_g.detach().cpu() > 0) != (out_o.detach() > 0)).sum())
        (out_g * guarded.to(probe.float(), dev())).sum().backward()
        tol = 2e-4 if flips == 0 else 5e-3
        assert rel_l2(xg.grad.cpu().numpy(), grads_o[0].numpy()) < tol, (scale, flips)
        got = {n: p.grad.detach().cpu().numpy() for n, p in blk.named_parameters()}
        compare_grads(got, want, tol, max(float(np.abs(v).max()) for v in want.values()))


def test_static_adjacency_block_is_stgcn_special_case():
    """ST-GCN block = same kernels with the data-dependent C_k switched off."""
    from fusion_gcn_amd.models.mmargcn.agcn import SpatialTemporalConv
    adj = ntu_adj()
    blk = SpatialTemporalConv(64, 64, adj, static_adjacency=True)
    fill_module(blk, "l0.")
    sd = oracle_sd(blk, "l0.")
    blk = guarded.to(blk, dev()).train()
    x = torch.from_numpy(filler.bellish("x.stgcn", (2, 64, 10, 25))).double()
    params = {k: v.clone().requires_grad_(True) for k, v in sd.items() if k.endswith(("adj_b", "conv_d.1.weight"))}
    live = dict(sd)
    live.update(params)
    xo = x.clone().requires_grad_(True)
    out_o, _ = O.st_block(xo, live, "l0", 1, True, True, None, static_adjacency=True)
    g_o = torch.autograd.grad(out_o.square().sum(), [xo] + list(params.values()))
    xg = guarded.to(x.float(), dev()).requires_grad_(True)
    out_g = blk.forward_nchw(xg)
    assert rel_l2(out_g.detach().cpu().numpy(), out_o.detach().numpy()) < 2e-5
    out_g.square().sum().backward()
    assert rel_l2(xg.grad.cpu().numpy(), g_o[0].numpy()) < 5e-4
    assert rel_l2(blk.gcn1.adj_b.grad.cpu().numpy(), g_o[1].numpy()) < 5e-4
    assert rel_l2(blk.gcn1.conv_d[1].weight.grad.cpu().numpy(), g_o[2].numpy()) < 5e-4
    assert float(blk.gcn1.conv_a[0].weight.grad.abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------
def _model_case(tag, shape, classes, gname):
    from fusion_gcn_amd.datasets.ntu_rgb_d import constants as ntu
    from fusion_gcn_amd.datasets.utd_mhad import constants as utd
    from fusion_gcn_amd.models.mmargcn.agcn import Model
    from fusion_gcn_amd.util import Graph
    c = {"utd": utd, "ntu": ntu}[gname]
    n, m, t, v, ch = shape
    model = Model((m, t, v, ch), classes, Graph(c.skeleton_edges, center_joint=c.center_joint))
    fill_module(model)
    x = torch.from_numpy(filler.skeleton_input(f"x.{tag}", shape, empty_second_body=(m > 1)))
    labels = torch.from_numpy(filler.uniform(f"y.{tag}", (n,), 0, classes).astype(np.int64))
    return model, x, labels


@pytest.mark.parametrize("tag,shape,classes,gname", [("cfg1", (2, 1, 100, 20, 3), 27, "utd"),
                                                     ("cfg2_small", (2, 2, 32, 25, 3), 60, "ntu")])
def test_full_model_vs_golden_and_oracle(golden, tag, shape, classes, gname):
    """BASELINE configs[0] (cfg1) end to end: logits / loss against the REFERENCE's own outputs (golden), gradients
    and running statistics against the float64 oracle."""
    ref = golden("model.npz")
    model, x, labels = _model_case(tag, shape, classes, gname)
    sd = oracle_sd(model)
    model = guarded.to(model, dev())
    # eval-mode logits vs the reference
    model.eval()
    with torch.no_grad():
        lg = model(guarded.to(x.float(), dev()))
    e_eval = rel_l2(lg.cpu().numpy(), ref[f"{tag}.eval.logits"])
    assert e_eval < 1e-4, e_eval
    # train step
    model.train()
    logits = model(guarded.to(x.float(), dev()))
    loss = torch.nn.functional.cross_entropy(logits, guarded.to(labels, dev()))
    loss.backward()
    e_train = rel_l2(logits.detach().cpu().numpy(), ref[f"{tag}.train.logits"])
    assert e_train < 1e-4, e_train
    assert abs(float(loss) - float(ref[f"{tag}.train.loss"])) < 1e-4
    # running statistics of that ONE train step vs the oracle's (checked before any further forward moves them)
    _, _, _, stats = O.loss_and_grads(x.double(), labels, sd)
    for k, v in stats.updates.items():
        if k.endswith(("running_mean", "running_var")):
            assert rel_l2(model.state_dict()[k].cpu().numpy(), v.numpy()) < 1e-4, k
    # gradients: flip-accounted against the float64 oracle, per-parameter norms against the reference's own
    model.zero_grad(set_to_none=True)
    check_gradients_with_flip_accounting(model, guarded.to(x.float(), dev()), guarded.to(labels, dev()), x.double(), labels, sd, ref, tag)


def test_agcn_spelling_and_mmargcn_mode(golden):
    """`model: agcn` (l1..l10 / PA) and `model: mmargcn, mode: skeleton_imu_spatial_fusion` give the same numbers as
    the mmargcn.agcn spelling for the same filled parameters; the fused-graph V=22 logits match the reference."""
    from fusion_gcn_amd.datasets.utd_mhad import constants as utd
    from fusion_gcn_amd.util import Graph
    from fusion_gcn_amd.util.dynamic_import import import_model
    ref = golden("mmargcn.npz")
    g = Graph(utd.skeleton_edges, center_joint=utd.center_joint)
    mm = import_model("mmargcn")({"skeleton": (1, 20, 22, 3)}, 27, g, mode="skeleton_imu_spatial_fusion",
                                 num_imu_joints=2, imu_enhanced_mode="append_center")
    filler.fill_state_dict(mm.state_dict(), rename=lambda k: k.replace("_model.agcn.", ""))
    mm = guarded.to(mm, dev())
    x = guarded.to(torch.from_numpy(filler.skeleton_input("x.mm22", (2, 1, 20, 22, 3))).float(), dev())
    mm.eval()
    with torch.no_grad():
        assert rel_l2(mm(x).cpu().numpy(), ref["mm22.eval.logits"]) < 1e-4
    mm.train()
    assert rel_l2(mm(x).detach().cpu().numpy(), ref["mm22.train.logits"]) < 1e-4

    ref_m = golden("model.npz")
    agcn = import_model("agcn")({"skeleton": (1, 100, 20, 3)}, 27, g)
    inv = {O.agcn_key(k): k for k in O.new_state_dict((1, 100, 20, 3), 27, adj_for(20))}
    filler.fill_state_dict(agcn.state_dict(), rename=lambda k: inv[k])
    agcn = guarded.to(agcn, dev()).eval()
    xx = guarded.to(torch.from_numpy(filler.skeleton_input("x.cfg1", (2, 1, 100, 20, 3))).float(), dev())
    with torch.no_grad():
        assert rel_l2(agcn(xx).cpu().numpy(), ref_m["cfg1.eval.logits"]) < 1e-4


@pytest.mark.parametrize("tag,dataset,shape,classes,n_imu", [("ntu27", "ntu", (2, 2, 16, 27, 3), 60, 2),
                                                             ("mmact22", "mmact", (2, 2, 16, 22, 3), 35, 4),
                                                             ("mmact18", "mmact", (2, 2, 16, 18, 2), 35, 0)])
def test_other_baseline_shapes_vs_reference(golden, tag, dataset, shape, classes, n_imu):
    """BASELINE configs 3 and 4 at fixture size, through the reference's own entry points (`import_model("mmargcn")`,
    mode skeleton_imu_spatial_fusion with the IMU joints appended to the skeleton graph; plain AGCN for the
    skeleton-only MMAct case with 2 input channels): logits and loss against the reference's outputs, every
    parameter-gradient norm within the fp32 ReLU-flip floor."""
    from fusion_gcn_amd.datasets.mmact import constants as mmact
    from fusion_gcn_amd.datasets.ntu_rgb_d import constants as ntu
    from fusion_gcn_amd.models.mmargcn.agcn import Model
    from fusion_gcn_amd.util import Graph
    from fusion_gcn_amd.util.dynamic_import import import_model
    ref = golden("mmargcn.npz")
    c = {"ntu": ntu, "mmact": mmact}[dataset]
    g = Graph(c.skeleton_edges, center_joint=c.center_joint)
    if n_imu:
        model = import_model("mmargcn")({"skeleton": shape[1:]}, classes, g, mode="skeleton_imu_spatial_fusion",
                                        num_imu_joints=n_imu, imu_enhanced_mode="append_center")
        strip = "_model.agcn."
    else:
        model = Model(shape[1:], classes, g)
        strip = ""
    filler.fill_state_dict(model.state_dict(), rename=lambda k: k.replace(strip, "") if strip else k)
    model = guarded.to(model, dev())
    x = guarded.to(torch.from_numpy(filler.skeleton_input(f"x.{tag}", shape, empty_second_body=True)).float(), dev())
    labels = guarded.to(torch.from_numpy(ref[f"{tag}.labels"]), dev())
    model.eval()
    with torch.no_grad():
        assert rel_l2(model(x).cpu().numpy(), ref[f"{tag}.eval.logits"]) < 1e-4
    model.train()
    logits = model(x)
    loss = torch.nn.functional.cross_entropy(logits, labels)
    loss.backward()
    assert rel_l2(logits.detach().cpu().numpy(), ref[f"{tag}.train.logits"]) < 1e-4
    assert abs(float(loss.detach()) - float(ref[f"{tag}.train.loss"])) < 1e-4
    model.zero_grad(set_to_none=True)
    sd = {(k.replace(strip, "") if strip else k): (v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu().clone())
          for k, v in model.state_dict().items()}
    x64 = torch.from_numpy(filler.skeleton_input(f"x.{tag}", shape, empty_second_body=True)).double()
    check_gradients_with_flip_accounting(model, x, labels, x64, labels.cpu(), sd, ref, tag, strip=strip)


@pytest.mark.parametrize("joints", [25, 27, 22])
def test_size_independent_properties_at_headline_shape(joints):
    """BASELINE configs[1] shape (T=300, V=25, M=2) -- and configs 3 / 4 at their full T = 300 (V = 25 + 2 IMU joints on the NTU
    graph, V = 18 + 4 on the MMAct graph: the shapes whose 9x1 halo image is largest; the V = 27 LDS-tile cliff of round 1 was found
    by the benchmark, not by a test) -- at a batch the oracle cannot afford: properties that must hold at any size -- clip
    independence in eval mode (a clip's logits do not depend on its batch mates), permutation equivariance, determinism -- and a
    finite train step."""
    from fusion_gcn_amd.datasets.mmact import constants as mmact
    from fusion_gcn_amd.datasets.ntu_rgb_d import constants as ntu
    from fusion_gcn_amd.models.mmargcn.agcn import Model
    from fusion_gcn_amd.util import Graph
    from fusion_gcn_amd.util.dynamic_import import import_model
    torch.manual_seed(1)
    if joints == 25:
        model, classes = Model((2, 300, 25, 3), 60, Graph(ntu.skeleton_edges, center_joint=20)), 60
        fill_module(model)
    else:
        c, n_imu, classes = (ntu, 2, 60) if joints == 27 else (mmact, 4, 35)
        model = import_model("mmargcn")({"skeleton": (2, 300, joints, 3)}, classes, Graph(c.skeleton_edges, center_joint=c.center_joint),
                                        mode="skeleton_imu_spatial_fusion", num_imu_joints=n_imu, imu_enhanced_mode="append_center")
        filler.fill_state_dict(model.state_dict(), rename=lambda k: k.replace("_model.agcn.", ""))
    model = guarded.to(model, dev()).eval()
    x = torch.randn(8, 2, 300, joints, 3, device=dev())
    with torch.no_grad():
        full = model(x)
        again = model(x)
        half = model(x[:4])
        perm = model(x.flip(0))
    assert torch.equal(full, again)
    assert rel_l2(half.cpu().numpy(), full[:4].cpu().numpy()) < 1e-5
    assert rel_l2(perm.flip(0).cpu().numpy(), full.cpu().numpy()) < 1e-5
    assert torch.isfinite(full).all()
    # train step at this shape: finite loss / grads, batch statistics make the loss batch-dependent but bounded
    model.train()
    loss = torch.nn.functional.cross_entropy(model(x), torch.arange(8, device=dev()) % classes)
    loss.backward()
    assert torch.isfinite(loss)
    assert all(torch.isfinite(p.grad).all() for p in model.parameters())
    # and a second train step from the same state gives the same gradients bit for bit (fixed-order sums everywhere)
    first = [p.grad.clone() for p in model.parameters()]
    model.zero_grad(set_to_none=True)
    torch.nn.functional.cross_entropy(model(x), torch.arange(8, device=dev()) % classes).backward()
    assert all(torch.equal(a, p.grad) for a, p in zip(first, model.parameters()))


@pytest.mark.gpu
@pytest.mark.parametrize("fgcn_math_mode", ["bf16x3", "f16x2", "f32"])
def test_streamed_output_stores_change_no_bit(fgcn_math_mode):
    """Every kernel that writes an activation has two store forms -- plain, and non-temporal for tensors from 96 MiB on (fgcn_common.hpp
    stream_out; the launchers choose per call) -- that must be the same computation: one training step of the headline model with the
    streamed form forced everywhere (tuning key 10 = 2) against the step with it forbidden (= 1): loss and every gradient bit for bit."""
    from fusion_gcn_amd import _lib, ops
    from fusion_gcn_amd.datasets.ntu_rgb_d import constants as ntu
    from fusion_gcn_amd.models.mmargcn.agcn import Model
    from fusion_gcn_amd.util import Graph
    lib = _lib.load()
    torch.manual_seed(3)
    with ops.math_mode(fgcn_math_mode):
        model = Model((2, 64, 25, 3), 60, Graph(ntu.skeleton_edges, center_joint=20))
        fill_module(model)
        model = guarded.to(model, dev()).train()
        x = torch.randn(3, 2, 64, 25, 3, device=dev())
        labels = torch.arange(3, device=dev()) % 60
        runs = {}
        try:
            for key in (1, 2):
                lib.fgcn_set_tuning(10, key)
                model.zero_grad(set_to_none=True)
                loss = torch.nn.functional.cross_entropy(model(x), labels)
                loss.backward()
                runs[key] = (loss.detach().clone(), [p.grad.clone() for p in model.parameters()])
        finally:
            lib.fgcn_set_tuning(10, 0)
    assert torch.isfinite(runs[1][0]) and torch.equal(runs[1][0], runs[2][0])
    assert all(torch.equal(a, b) for a, b in zip(runs[1][1], runs[2][1]))


@pytest.mark.gpu
def test_pool_and_classifier_kernels_and_graph_replay():
    """Global average pooling and fc run on libfgcn (equal to torch.mean / nn.Linear incl. gradients), and a captured
    forward+backward of the 8-clip headline shard replays to the same logits every time (with torch's multi-block mean
    in the graph the pooled features were wrong from the second replay on)."""
    import torch.nn.functional as F
    from fusion_gcn_amd.block import LinearFunction
    dev = torch.device("cuda:0")
    torch.manual_seed(3)
    for n, k, classes in ((8, 256, 60), (3, 256, 27), (64, 128, 35)):
        h = torch.randn(n, k, device=dev, requires_grad=True)
        w = (torch.randn(classes, k, device=dev) * 0.1).requires_grad_(True)
        b = torch.randn(classes, device=dev, requires_grad=True)
        dy = torch.randn(n, classes, device=dev)
        want = F.linear(h.double(), w.double(), b.double())
        gh, gw, gb = torch.autograd.grad((want * dy.double()).sum(), (h, w, b))
        got = LinearFunction.apply(h, w, b)
        assert float((got.double() - want).norm() / want.norm()) < 3e-6
        dh, dw, db = torch.autograd.grad((got * dy).sum(), (h, w, b))
        for a_, b_ in ((dh, gh), (dw, gw), (db, gb)):
            assert float((a_.double() - b_).norm() / b_.norm()) < 3e-6
    from fusion_gcn_amd import ops
    for G, R, C in ((8, 3750, 256), (3, 77, 64), (64, 500, 128), (1, 1, 4)):
        xs = torch.randn(G, R, C, device=dev)
        got = ops.group_mean(xs)
        want = xs.double().mean(1)
        assert float((got.double() - want).norm() / want.norm()) < 3e-6
    from fusion_gcn_amd.datasets.ntu_rgb_d import constants as ntu
    from fusion_gcn_amd.models.mmargcn.agcn import Model
    from fusion_gcn_amd.util import Graph
    model = guarded.to(Model((2, 300, 25, 3), 60, Graph(ntu.skeleton_edges, center_joint=ntu.center_joint)), dev).train()
    x = torch.randn(8, 2, 300, 25, 3, device=dev)
    y = torch.randint(0, 60, (8,), device=dev)

    def fwd_bwd():
        for p in model.parameters():
            p.grad = None
        out = model(x)
        F.cross_entropy(out, y).backward()
        return out
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            ref = fwd_bwd().detach().clone()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_out = fwd_bwd()
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert float((static_out.detach() - ref).norm() / ref.norm()) < 1e-6


@pytest.mark.gpu
@pytest.mark.parametrize("G,R,C,res_mode", [(8, 3750, 256, 1), (3, 77, 64, 0), (64, 500, 128, 2), (2, 1, 8, 1), (5, 130, 320, 2)])
def test_last_blocks_epilogue_with_the_pooling_behind_it(G, R, C, res_mode):
    """fgcn_bn_act_pool = fgcn_bn_act (relu, sign image) + fgcn_group_mean without the activation between them: the pooled means to
    rounding, the sign image bit for bit, twice the same bits."""
    from fusion_gcn_amd import ops
    dev = torch.device("cuda:0")
    torch.manual_seed(11 + C)
    a = torch.randn(G * R, C, device=dev)
    b = torch.randn(G * R, C, device=dev) if res_mode else None
    mk = lambda: torch.stack([torch.randn(C, device=dev), torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev), torch.randn(C, device=dev)])   # noqa: E731
    va, vb = mk().contiguous(), (mk().contiguous() if res_mode == 2 else None)
    out, mask = ops.bn_act(a, va, b, vb, relu=True, sign_mask=True)
    pooled, pmask = ops.bn_act_pool(a, va, b, vb, G)
    again, amask = ops.bn_act_pool(a, va, b, vb, G)
    assert torch.equal(mask, pmask) and torch.equal(pooled, again) and torch.equal(pmask, amask)
    want = out.double().view(G, R, C).mean(1)
    assert float((pooled.double() - want).norm() / want.norm()) < 3e-6
    assert float((pooled - ops.group_mean(out.view(G, R, C))).abs().max()) < 1e-5 * float(want.abs().max())


@pytest.mark.gpu
@pytest.mark.parametrize("G,R,C,res_mode", [(4, 500, 64, 1), (3, 77, 128, 0), (2, 130, 256, 2), (5, 8, 8, 1)])
def test_batchnorm_backward_from_a_per_group_gradient(G, R, C, res_mode):
    """fgcn_bn_act_bwd_{reduce,apply}_g: the gradient of a pooled output as one row per group equals the two passes on its rows x C
    broadcast, bit for bit (the same values reach the same arithmetic)."""
    from fusion_gcn_amd import ops
    dev = torch.device("cuda:0")
    torch.manual_seed(3 + C)
    rows = G * R
    a = torch.randn(rows, C, device=dev)
    b = torch.randn(rows, C, device=dev) if res_mode else None
    mk = lambda: torch.stack([torch.randn(C, device=dev), torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev), torch.randn(C, device=dev)]).contiguous()   # noqa: E731
    va, vb = mk(), (mk() if res_mode == 2 else None)
    out, mask = ops.bn_act(a, va, b, vb, relu=True, sign_mask=True)
    dg = torch.randn(G, C, device=dev)
    full = dg.unsqueeze(1).expand(G, R, C).contiguous().view(rows, C)
    for train in (True, False):
        want = ops.bn_act_bwd(full, out, a, va, b, vb, res_mode=res_mode, train=train, sign_mask=mask)
        got = ops.bn_act_bwd(dg, out, a, va, b, vb, res_mode=res_mode, train=train, sign_mask=mask, grp_rows=R)
        for w, g_ in zip(want, got):
            assert (w is None) == (g_ is None) and (w is None or torch.equal(w, g_))
    with pytest.raises(Exception):
        ops.bn_act_bwd(dg, out, a, va, b, vb, res_mode=res_mode, train=True, sign_mask=mask, grp_rows=R + 1)


@pytest.mark.gpu
@pytest.mark.parametrize("B,T,V,C,group", [(4, 11, 25, 64, 2), (6, 7, 20, 128, 3), (2, 40, 25, 256, 1)])
def test_spatial_backward_tile_with_a_per_group_addend(B, T, V, C, group):
    """fgcn_spatial_bwd_tile with extra1_group > 0: the first gated addend as one row per group of samples = the launch with its (B, T, V, Cin) broadcast, bit for bit."""
    from fusion_gcn_amd import ops
    dev = torch.device("cuda:0")
    torch.manual_seed(7 + C)
    with ops.math_mode("bf16x3"):
        if not ops.spatial_bwd_tile_available(V, C, C):
            pytest.skip("tile backward not available for this shape")
        x, dy = torch.randn(B, T, V, C, device=dev), torch.randn(B, T, V, C, device=dev)
        a_hat = torch.randn(B, 3, V, V, device=dev) * 0.2
        w = torch.randn(1, C, 3 * C, device=dev) * 0.05
        w3 = ops.pack_split3(w)
        e2 = torch.randn(B, T, V, C, device=dev)
        m1 = torch.randint(0, 256, (B * T * V * C // 8,), device=dev, dtype=torch.uint8)
        m2 = torch.randint(0, 256, (B * T * V * C // 8,), device=dev, dtype=torch.uint8)
        eg = torch.randn(B // group, C, device=dev)
        full = eg.repeat_interleave(group, 0).view(B, 1, 1, C).expand(B, T, V, C).contiguous()
        dx0, dx1 = torch.empty(B, T, V, C, device=dev), torch.empty(B, T, V, C, device=dev)
        p0 = ops.spatial_bwd_tile(dy, x, a_hat, w3, dx0, accumulate=False, gated=[(full, m1), (e2, m2)])
        p1 = ops.spatial_bwd_tile(dy, x, a_hat, w3, dx1, accumulate=False, gated=[(eg, m1, group), (e2, m2)])
        assert torch.equal(dx0, dx1) and torch.equal(p0, p1)


@pytest.mark.gpu
def test_model_with_and_without_the_pooling_epilogue(fgcn_math):
    """The model's last block with the pooling in its epilogue against bn_act + group_mean: logits, loss and every gradient agree to
    rounding (the pooled sums run in another order); the backward is the same code on the same sign image."""
    import torch.nn.functional as F
    from fusion_gcn_amd import ops
    from fusion_gcn_amd.datasets.ntu_rgb_d import constants as ntu
    from fusion_gcn_amd.models.mmargcn.agcn import Model
    from fusion_gcn_amd.util import Graph
    dev = torch.device("cuda:0")
    torch.manual_seed(5)
    model = guarded.to(Model((2, 40, 25, 3), 60, Graph(ntu.skeleton_edges, center_joint=ntu.center_joint)), dev).train()
    with torch.no_grad():
        for m in model.modules():                       # (the reference's 1e-6 BatchNorm gain would silence the graph convolutions)
            if hasattr(m, "gcn1"):
                m.gcn1.bn.weight.fill_(1.0)
    x = torch.randn(3, 2, 40, 25, 3, device=dev)
    y = torch.randint(0, 60, (3,), device=dev)

    def run(flag, rows=True):
        with ops.context() as c:            # the kernel-form options are per context (fusion_gcn_amd/paths.py)
            c.paths.pool_epilogue, c.paths.pool_backward_rows = flag, rows
            for p in model.parameters():
                p.grad = None
            logits = model(x)
            loss = F.cross_entropy(logits, y)
            loss.backward()
            return logits.detach().clone(), float(loss), [p.grad.clone() for p in model.parameters()]
    lg0, l0, g0 = run(False)
    lg1, l1, g1 = run(True)
    assert float((lg1 - lg0).norm() / lg0.norm()) < 2e-6 and abs(l1 - l0) < 1e-5
    f0, f1 = torch.cat([g.flatten() for g in g0]).double(), torch.cat([g.flatten() for g in g1]).double()
    assert float((f1 - f0).norm() / f0.norm()) < 2e-5
    # the backward from the pooled gradient as one row per clip against its expansion: the same values reach the same arithmetic
    lg2, l2, g2 = run(True, rows=False)
    assert torch.equal(lg1, lg2) and l1 == l2
    for a_, b_ in zip(g1, g2):
        assert torch.equal(a_, b_)


@pytest.mark.gpu
def test_dropout_between_blocks_and_second_backward():
    """reference Model(dropout > 0) puts an in-place nn.Dropout after every block but the last (agcn.py:166-169): the block's output is
    overwritten in place after the block saved what its backward needs (the one-bit sign image, not the output itself), so a
    training step must run; in eval mode dropout is the identity, so the logits equal those of the dropout-free model with the
    same parameters; a second backward through the same graph raises a clear error instead of an opaque one."""
    from fusion_gcn_amd.datasets.utd_mhad import constants as utd
    from fusion_gcn_amd.models.mmargcn.agcn import Model
    from fusion_gcn_amd.util import Graph
    g = Graph(utd.skeleton_edges, center_joint=utd.center_joint)
    shape = (2, 1, 24, 20, 3)
    drop = Model(shape[1:], 27, g, dropout=0.25)
    fill_module(drop)
    plain = Model(shape[1:], 27, g)
    # the Dropout modules take l<i> slots of their own: block i of the plain model is slot 2i of the dropout model
    remap = {k: v for k, v in drop.state_dict().items()}
    plain.load_state_dict({k.replace(f"l{int(k.split('.')[0][1:])}.", f"l{int(k.split('.')[0][1:]) // 2}.", 1) if k.startswith("l") else k: v
                           for k, v in remap.items()})
    drop, plain = guarded.to(drop, dev()), guarded.to(plain, dev())
    x = guarded.to(torch.from_numpy(filler.skeleton_input("x.drop", shape)).float(), dev())
    drop.eval(), plain.eval()
    with torch.no_grad():
        assert torch.equal(drop(x), plain(x))
    drop.train()
    torch.manual_seed(0)
    out = drop(x)
    loss = out.square().mean()
    loss.backward(retain_graph=True)
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in drop.parameters())
    assert float(sum(p.grad.abs().sum() for p in drop.parameters())) > 0
    with pytest.raises(RuntimeError, match="backward ran twice"):
        loss.backward()


@pytest.mark.gpu
@pytest.mark.math_modes("bf16x3")
def test_inference_runs_the_fused_output_stages(fgcn_math):
    """Eval mode under torch.no_grad(): every block takes the inference forms of the two north-star kernels where they exist (BatchNorm
    + shortcut + ReLU in the epilogues: fgcn_spatial_fwd_tile_bn_relu, fgcn_tconv_halo_bn_relu) -- the logits equal those of the
    unfused eval path to rounding; with autograd on (a backward may follow) the unfused path runs and is bit-identical to before."""
    from fusion_gcn_amd import ops
    from fusion_gcn_amd.datasets.ntu_rgb_d import constants as ntu
    from fusion_gcn_amd.models.mmargcn.agcn import Model
    from fusion_gcn_amd.util import Graph
    dev = torch.device("cuda:0")
    torch.manual_seed(7)
    model = guarded.to(Model((2, 40, 25, 3), 60, Graph(ntu.skeleton_edges, center_joint=ntu.center_joint)), dev)
    with torch.no_grad():
        for m in model.modules():
            if hasattr(m, "gcn1"):
                m.gcn1.bn.weight.fill_(1.0)
            if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):      # non-trivial running statistics
                m.running_mean.normal_(0, 0.2)
                m.running_var.uniform_(0.5, 1.5)
    model.eval()
    x = torch.randn(3, 2, 40, 25, 3, device=dev)
    calls = {"conv": 0, "spatial": 0}
    conv, spatial = ops.tconv_halo_bn_relu, ops.spatial_fwd_tile_bn_relu

    def count(name, fn):
        def wrapped(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return wrapped
    ops.tconv_halo_bn_relu, ops.spatial_fwd_tile_bn_relu = count("conv", conv), count("spatial", spatial)
    try:
        with torch.no_grad():
            with ops.context() as c:
                c.paths.fused_inference = False
                ref = model(x)
            assert calls == {"conv": 0, "spatial": 0}
            fused = model(x)
        # the ten blocks: nine spatial stages (the first block has 3 input channels: no tile form), the seven stride-1 temporal stages
        # that are not the pooled last block
        assert calls == {"conv": 7, "spatial": 9}, calls
        with_grad = model(x)                         # autograd on: a backward may follow -> the unfused path, nothing fused is called
        assert calls == {"conv": 7, "spatial": 9}
    finally:
        ops.tconv_halo_bn_relu, ops.spatial_fwd_tile_bn_relu = conv, spatial
    assert torch.equal(with_grad.detach(), ref)
    err = float((fused - ref).norm() / ref.norm())
    assert err < 1e-5, err
