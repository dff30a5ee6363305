"""AGCN blocks on skeleton graphs of 33 .. 64 joints (the wide route: fgcn_joint_wide.hip, the joint-mix spatial form and the row-GEMM
temporal conv) on the MI355X.

Kernels against float64 formulas at V in {33, 48, 50, 64}; the block against the float64 oracle in all four math modes (the tolerances
of tests/test_block_model_gpu.py in f32 / bf16x3 / f16x2, the bf16 contract of tests/test_bf16_gpu.py in bf16); the model on a 50-joint
two-person graph against the oracle, its graph replay against the eager step; V = 65 fails with an error that names the limit."""
import numpy as np
import pytest
import torch

from conftest import rel_l2
from oracle import agcn_oracle as O
from oracle import filler, graph_oracle

import guarded
from guarded import guarded_allocations  # noqa: F401  (the fixture)

# every test runs on guarded allocations: NaN around each tensor the host layer creates, margins verified at teardown (tests/guarded.py)
pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_allocations")]
ALL_MODES = ["f32", "bf16x3", "f16x2", "bf16"]


def dev():
    return torch.device("cuda:0")


def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64)


def two_person_edges():
    from fusion_gcn_amd.datasets.ntu_rgb_d import constants as ntu
    edges = list(ntu.skeleton_edges)
    return edges + [(a + 25, b + 25) for a, b in edges]


def tree_adjacency(V, seed):
    rng = np.random.default_rng(seed)
    return graph_oracle.spatial_partition_stack([(int(rng.integers(0, i)), i) for i in range(1, V)])


# ---- kernels ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,T,B", [(33, 7, 3), (48, 5, 2), (50, 9, 2), (64, 3, 2)])
def test_joint_mix_wide(V, T, B):
    """out (+)= sum_terms M (or M^T) . in per frame, per-sample matrices, items of 4 / 20 / 32 channels, one to three terms."""
    from fusion_gcn_amd import ops
    C_in, C_out = 84, 56
    x, mats = rnd(B, T, V, C_in, seed=V), rnd(B, 3, V, V, seed=V + 1)
    spec = [dict(out_c=0, nch=32, terms=[(0, 1, 0)]),
            dict(out_c=32, nch=20, terms=[(1, 0, 40), (2, 1, 64)]),
            dict(out_c=52, nch=4, terms=[(0, 0, 80), (1, 1, 4), (2, 0, 8)])]

    def want(base):
        out = base.clone()
        for it in spec:
            o, n = it["out_c"], it["nch"]
            for m, tr, c in it["terms"]:
                M = mats[:, m].transpose(1, 2) if tr else mats[:, m]
                out[..., o:o + n] += torch.einsum("buv,btvc->btuc", M, x[..., c:c + n])
        return out
    for acc in (False, True):
        out0 = rnd(B, T, V, C_out, seed=7) if acc else torch.zeros(B, T, V, C_out, dtype=torch.float64)
        out = guarded.to(out0.float(), dev())
        ops.joint_mix_wide(guarded.to(x.float(), dev()), out, guarded.to(mats.float(), dev()), spec, accumulate=acc)
        assert rel_l2(out.cpu().numpy(), want(out0).numpy()) < 2e-6, acc
    # one shared set of matrices (static adjacency)
    out = torch.zeros(B, T, V, C_out, device=dev())
    ops.joint_mix_wide(guarded.to(x.float(), dev()), out, guarded.to(mats[:1].float(), dev()), spec[:1])
    ref = torch.einsum("vu,btvc->btuc", mats[0, 0], x[..., :32])
    assert rel_l2(out[..., :32].cpu().numpy(), ref.numpy()) < 2e-6
    assert float(out[..., 32:].abs().max()) == 0.0


@pytest.mark.parametrize("V,T,B,ic", [(33, 7, 3, 16), (48, 5, 2, 32), (50, 9, 2, 4), (64, 3, 2, 64)])
def test_joint_gram_and_column_softmax_wide(V, T, B, ic):
    """theta_k^T phi_k summed over frames -> S; C = softmax over dim -2 of S / (ic T); A^ = C + A + B; and the softmax backward."""
    from fusion_gcn_amd import ops
    emb = rnd(B, T, V, 6 * ic, seed=V + ic)
    items = [(2 * k * ic, (2 * k + 1) * ic, ic) for k in range(3)]
    part = ops.joint_gram(guarded.to(emb.float(), dev()), guarded.to(emb.float(), dev()), items)
    assert tuple(part.shape[2:]) == (3, 64, 64)
    S = torch.stack([torch.einsum("btvc,btwc->bvw", emb[..., a:a + w], emb[..., b:b + w]) for a, b, w in items], 1)
    got = part.double().sum(1).cpu()
    assert rel_l2(got[..., :V, :V].numpy(), S.numpy()) < 2e-6
    if V < 64:
        assert float(got[..., V:, :].abs().max()) == 0.0 and float(got[..., :, V:].abs().max()) == 0.0
    adj_a, adj_b = rnd(3, V, V, seed=1), rnd(3, V, V, seed=2)
    scale = 1.0 / (ic * T)
    c, a_hat = ops.adj_softmax_fwd(part, scale, guarded.to(adj_a.float(), dev()), B, adj_b=guarded.to(adj_b.float(), dev()))
    C = torch.softmax(S * scale, dim=-2)
    assert rel_l2(c.cpu().numpy(), C.numpy()) < 2e-6
    assert rel_l2(a_hat.cpu().numpy(), (C + adj_a + adj_b).numpy()) < 2e-6
    _, a_static = ops.adj_softmax_fwd(None, 1.0, guarded.to(adj_a.float(), dev()), 1, use_softmax=False, adj_b=guarded.to(adj_b.float(), dev()))
    assert rel_l2(a_static.cpu().numpy(), (adj_a + adj_b)[None].numpy()) < 1e-7
    # backward: the gram of x against dagg gives dA^; dS = scale C (dC - colsum(C dC))
    x, dagg = rnd(B, T, V, 8, seed=3), rnd(B, T, V, 24, seed=4)
    part_b = ops.joint_gram(guarded.to(x.float(), dev()), guarded.to(dagg.float(), dev()), [(0, 8 * k, 8) for k in range(3)])
    d_a_hat, d_s = ops.adj_softmax_bwd(part_b, scale, c, V)
    dC = torch.stack([torch.einsum("btvc,btwc->bvw", x, dagg[..., 8 * k:8 * k + 8]) for k in range(3)], 1)
    Cg = c.double().cpu()
    assert rel_l2(d_a_hat.cpu().numpy(), dC.numpy()) < 2e-6
    want_ds = scale * Cg * (dC - (Cg * dC).sum(-2, keepdim=True))
    assert rel_l2(d_s.cpu().numpy(), want_ds.numpy()) < 2e-5


@pytest.mark.parametrize("V,T,B,K,N,kt,s", [(33, 9, 2, 64, 64, 9, 1), (64, 7, 2, 64, 128, 9, 2)])
def test_row_kernels_do_not_depend_on_the_joint_count(V, T, B, K, N, kt, s):
    """The row kernels the wide route keeps (the temporal conv as a per-tap row GEMM, its data and weight gradient, BatchNorm +
    shortcut + ReLU) index rows: at 33 / 64 joints they give the float64 results."""
    import torch.nn.functional as F
    from fusion_gcn_amd import ops
    x, w = rnd(B, T, V, K, seed=11), rnd(N, K, kt, 1, seed=12) * 0.1
    Tp = (T - 1) // s + 1
    pad = (kt - 1) // 2
    ref = F.conv2d(x.permute(0, 3, 1, 2), w, stride=(s, 1), padding=(pad, 0)).permute(0, 2, 3, 1)
    wk = guarded.to(w[..., 0].permute(2, 1, 0).contiguous().float(), dev())            # (taps, K, N)
    u = torch.empty(B, Tp, V, N, device=dev())
    ops.rows_gemm(guarded.to(x.float(), dev()), wk, u, K=K, N=N, tmap=ops.conv_tmap(kt, s))
    assert rel_l2(u.cpu().numpy(), ref.numpy()) < 2e-6
    du = rnd(B, Tp, V, N, seed=13)
    xr = x.clone().requires_grad_(True)
    wr = w.clone().requires_grad_(True)
    (F.conv2d(xr.permute(0, 3, 1, 2), wr, stride=(s, 1), padding=(pad, 0)).permute(0, 2, 3, 1) * du).sum().backward()
    dg = torch.empty(B, T, V, K, device=dev())
    ops.rows_gemm(guarded.to(du.float(), dev()), guarded.to(w[..., 0].permute(2, 0, 1).contiguous().float(), dev()), dg, K=N, N=K,
                  tmap=ops.conv_dgrad_tmap(kt, s))
    assert rel_l2(dg.cpu().numpy(), xr.grad.numpy()) < 2e-6
    gw = ops.tconv_wgrad(guarded.to(x.float(), dev()), guarded.to(du.float(), dev()), taps=kt, stride=s, all_taps=False, conv_param=(1, K))
    assert rel_l2(gw.cpu().numpy(), wr.grad.numpy()) < 2e-6
    # BatchNorm (statistics, finalize) + identity shortcut + ReLU over V joints per frame
    a, r = rnd(B, Tp, V, N, seed=14), rnd(B, Tp, V, N, seed=15)
    part = torch.empty(B, Tp, V, N, device=dev())
    stats = ops.rows_gemm(guarded.to(a.float(), dev()), torch.eye(N, device=dev())[None].contiguous(), part, K=N, N=N, stats=True)
    gamma, beta = guarded.to(rnd(N, seed=16).float(), dev()), guarded.to(rnd(N, seed=17).float(), dev())
    vec = ops.bn_finalize(stats, B * Tp * V, gamma, beta)
    o, _ = ops.bn_act(part, vec, guarded.to(r.float(), dev()), None, relu=True, sign_mask=True)
    mean, var = a.mean((0, 1, 2)), a.var((0, 1, 2), unbiased=False)
    want = torch.relu((a - mean) / torch.sqrt(var + 1e-5) * gamma.double().cpu() + beta.double().cpu() + r)
    assert rel_l2(o.cpu().numpy(), want.numpy()) < 2e-5


# ---- block -------------------------------------------------------------------------------------------------------------
BLOCKS = [("first", 3, 64, 1, False, 33, 7, False), ("identity64", 64, 64, 1, True, 50, 5, False),
          ("down_s2", 64, 128, 2, True, 64, 7, False), ("identity256", 256, 256, 1, True, 33, 3, False),
          ("static64", 64, 64, 1, True, 64, 5, True)]


def _block_case(name, cin, cout, stride, residual, V, T, static, adj, B=2, seed_tag=""):
    from fusion_gcn_amd.models.mmargcn.agcn import SpatialTemporalConv
    blk = SpatialTemporalConv(cin, cout, adj, stride=stride, residual=residual, static_adjacency=static)
    filler.fill_state_dict(blk.state_dict(), prefix="l0.")
    sd = {"l0." + k: (v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu().clone()) for k, v in blk.state_dict().items()}
    x = torch.from_numpy(filler.bellish(f"x.wide.{name}{seed_tag}", (B, cin, T, V))).double()
    Tp = (T - 1) // stride + 1
    probe = torch.from_numpy(filler.uniform(f"probe.wide.{name}{seed_tag}", (B, cout, Tp, V), -1, 1)).double()
    params = {k: v.clone().requires_grad_(True) for k, v in sd.items()
              if v.is_floating_point() and not k.endswith(("running_mean", "running_var", "adj_a"))}
    live = dict(sd)
    live.update(params)
    xo = x.clone().requires_grad_(True)
    stats = O.Stats()
    out_o, adj_c = O.st_block(xo, live, "l0", stride, residual, True, stats, static_adjacency=static)
    grads_o = torch.autograd.grad((out_o * probe).sum(), [xo] + list(params.values()), allow_unused=True)
    want = {k[3:]: g.numpy() for k, g in zip(params.keys(), grads_o[1:]) if g is not None}
    blk = guarded.to(blk, dev()).train()
    xg = guarded.to(x.float(), dev()).requires_grad_(True)
    out_g = blk.forward_nchw(xg)
    (out_g * guarded.to(probe.float(), dev())).sum().backward()
    got = {n: p.grad.detach().cpu().numpy() for n, p in blk.named_parameters()}
    return blk, x, sd, stats, out_o, adj_c, grads_o[0], want, out_g, xg.grad, got


ZERO_GRAD = ("conv_d.0.bias", "conv_d.1.bias", "conv_d.2.bias", "down.0.bias", "tcn1.conv.bias", "residual.conv.bias",
             "conv_a.0.bias", "conv_a.1.bias", "conv_a.2.bias")


def _check_block(mode, out_o, adj_c, dx_o, want, out_g, dx, got, blk, static):
    flips = int(((out_g.detach().cpu() > 0) != (out_o.detach() > 0)).sum())
    fwd = rel_l2(out_g.detach().cpu().numpy(), out_o.detach().numpy())
    scale_ref = max(float(np.abs(v).max()) for v in want.values())
    if mode == "bf16":
        # the bf16 contract (tests/test_bf16_gpu.py): outputs within 1e-2, gradients at cosine >= 0.98
        assert fwd < 1e-2, fwd
        cos = lambda a, b: float(np.dot(a.ravel(), b.ravel()) / (np.linalg.norm(a) * np.linalg.norm(b) + 1e-300))   # noqa: E731
        assert cos(dx.cpu().numpy().astype(np.float64), dx_o.numpy()) > 0.98
        for k, w in want.items():
            if not k.endswith(ZERO_GRAD) and np.linalg.norm(w) > 1e-9 * scale_ref:
                assert cos(got[k].astype(np.float64).reshape(w.shape), w) > 0.98, k
        return fwd, flips
    assert fwd < 2e-5, fwd
    if not static:
        assert rel_l2(torch.stack(blk.gcn1.adj_c, 1).cpu().numpy(), torch.stack(adj_c, 1).detach().numpy()) < 1e-5
    tol = 2e-4 if flips == 0 else 5e-3
    assert rel_l2(dx.cpu().numpy(), dx_o.numpy()) < tol, flips
    for k, w in want.items():
        g = got[k].astype(np.float64).reshape(w.shape)
        if k.endswith(ZERO_GRAD):
            assert np.abs(g).max() <= 1e-4 * scale_ref, k
        else:
            assert rel_l2(g, w) < tol, (k, rel_l2(g, w), flips)
    return fwd, flips


@pytest.mark.parametrize("fgcn_math", ALL_MODES, indirect=True)
@pytest.mark.parametrize("case", BLOCKS, ids=[c[0] for c in BLOCKS])
def test_wide_block_vs_oracle(fgcn_math, case):
    """Forward, adj_c, dx, every parameter gradient, the BatchNorm running statistics and the eval-mode forward of one block."""
    name, cin, cout, stride, residual, V, T, static = case
    adj = graph_oracle.spatial_partition_stack(two_person_edges()) if V == 50 else tree_adjacency(V, V)
    blk, x, sd, stats, out_o, adj_c, dx_o, want, out_g, dx, got = _block_case(name, cin, cout, stride, residual, V, T, static, adj)
    fwd, flips = _check_block(fgcn_math, out_o, adj_c, dx_o, want, out_g, dx, got, blk, static)
    for k, v in stats.updates.items():
        if k.endswith(("running_mean", "running_var")):
            assert rel_l2(blk.state_dict()[k[3:]].cpu().numpy(), v.numpy()) < (1e-2 if fgcn_math == "bf16" else 1e-5), k
    blk.eval()
    sd_eval = {"l0." + k: (v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu().clone()) for k, v in blk.state_dict().items()}
    with torch.no_grad():
        out_e = blk.forward_nchw(guarded.to(x.float(), dev()))
    want_e, _ = O.st_block(x, sd_eval, "l0", stride, residual, False, static_adjacency=static)
    assert rel_l2(out_e.cpu().numpy(), want_e.numpy()) < (1e-2 if fgcn_math == "bf16" else 2e-5)
    print(f"[{fgcn_math} {name} V={V}] fwd {fwd:.2e} flips {flips}")


@pytest.mark.parametrize("fgcn_math", ["f32", "bf16x3"], indirect=True)
@pytest.mark.parametrize("seed", range(3))
def test_wide_block_random_trees_vs_oracle(fgcn_math, seed):
    """Seeded sweep over 33..64 joints (random skeleton trees), frame counts and block variants, train mode."""
    rng = np.random.default_rng(2000 + seed)
    V, T, B = int(rng.integers(33, 65)), int(rng.integers(1, 8)), int(rng.integers(1, 3))
    cin, cout, stride, residual = [(3, 64, 1, False), (64, 128, 2, True), (128, 128, 1, True)][seed % 3]
    if T == 1 and stride == 2:
        T = 2
    out = _block_case(f"rnd{seed}", cin, cout, stride, residual, V, T, False, tree_adjacency(V, seed), B=B)
    blk, x, sd, stats, out_o, adj_c, dx_o, want, out_g, dx, got = out
    _check_block(fgcn_math, out_o, adj_c, dx_o, want, out_g, dx, got, blk, False)


# ---- model ----------------------------------------------------------------------------------------------------------
def _two_person_model():
    from fusion_gcn_amd.datasets.ntu_rgb_d import constants as ntu
    from fusion_gcn_amd.models.mmargcn.agcn import Model
    from fusion_gcn_amd.util import Graph
    shape, classes = (2, 1, 12, 50, 3), 10
    model = Model(shape[1:], classes, Graph(two_person_edges(), center_joint=ntu.center_joint))
    filler.fill_state_dict(model.state_dict())
    x = torch.from_numpy(filler.skeleton_input("x.wide50", shape, empty_second_body=False))
    labels = torch.from_numpy(filler.uniform("y.wide50", (shape[0],), 0, classes).astype(np.int64))
    return model, x, labels


def test_two_person_model_vs_oracle():
    """agcn.Model on the 50-joint two-person NTU graph: logits and the flat gradient against the float64 oracle, with the ReLU
    decisions accounted as tests/test_block_model_gpu.py does."""
    import math
    from oracle import relu_masks as RM
    model, x, labels = _two_person_model()
    sd64 = {k: (v.detach().double() if v.is_floating_point() else v.detach().clone()) for k, v in model.state_dict().items()}
    names = [n for n, _ in model.named_parameters()]
    oracle = RM.oracle_side(x.double(), labels, sd64, names)
    model = guarded.to(model, dev()).train()
    rep = RM.gradient_parity_report(model, guarded.to(x.float(), dev()), guarded.to(labels, dev()), oracle=oracle)
    print(f"[wide50] logits {rep['logits_err']:.2e} flips {rep['flips']} of {rep['decisions']} grad {rep['err_plain']:.2e} / "
          f"{rep['err_injected']:.2e}")
    assert rep["logits_err"] < 1e-5 and rep["loss_err"] < 1e-5, rep
    assert rep["err_injected"] < 1e-4, rep
    assert rep["err_plain"] <= 1e-4 + 2.0 * math.sqrt(rep["flips"] / (rep["decisions"] / 20)), rep


def test_two_person_model_graph_replay():
    """GraphStep replays the 50-joint step: equal to the eager step, and two replays agree bit for bit."""
    import copy
    import torch.nn.functional as F
    from fusion_gcn_amd.session.procedures import GraphStep
    model, x, labels = _two_person_model()
    model = guarded.to(model, dev()).train()
    eager = copy.deepcopy(model)
    xd, yd = guarded.to(x.float(), dev()), guarded.to(labels, dev())
    step = GraphStep(verify=True)
    grads, losses = [], []
    for _ in range(3):
        model.zero_grad(set_to_none=False)
        _, loss = step.forward(model, F.cross_entropy, xd, yd)
        step.backward(loss)
        losses.append(float(loss))
        grads.append(torch.cat([p.grad.flatten() for p in model.parameters()]).clone())
    assert step.replays >= 2
    assert torch.equal(grads[1], grads[2]) and losses[1] == losses[2]
    eager.zero_grad()
    eloss = F.cross_entropy(eager(xd), yd)
    eloss.backward()
    ge = torch.cat([p.grad.flatten() for p in eager.parameters()])
    assert abs(float(eloss) - losses[-1]) < 1e-5
    assert rel_l2(grads[-1].cpu().numpy(), ge.cpu().numpy()) < 1e-4


# ---- limit ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("static", [False, True])
def test_more_than_64_joints_fail_at_the_first_forward(static):
    from fusion_gcn_amd import _lib
    from fusion_gcn_amd.models.mmargcn.agcn import SpatialTemporalConv
    blk = guarded.to(SpatialTemporalConv(64, 64, tree_adjacency(65, 0), static_adjacency=static), dev()).train()    # builds
    with pytest.raises(_lib.FgcnError, match="64"):
        blk.forward_nchw(torch.randn(1, 64, 4, 65, device=dev()))
