"""MS-G3D (reference torch_src/models/msg3d/*.py).

CPU: the oracle (oracle/msg3d_oracle.py) against tests/golden/msg3d.npz, written by importing the reference
(oracle/gen_golden_msg3d.py): logits, loss, every parameter-gradient norm, small gradients in full, running statistics, the
adjacency stacks; the build's module tree must have the reference's state-dict keys in the reference's order and, from the
same seed, the same initial values.  GPU: the HIP-backed model against the same golden vectors and the float64 oracle."""
import os

import numpy as np
import pytest
import torch

from conftest import rel_l2
from oracle import filler
from oracle import msg3d_oracle as O

import guarded
from guarded import guarded_gpu_tests  # noqa: F401  (the fixture)

# the tests marked gpu run on guarded allocations, margins verified at teardown (tests/guarded.py); the host tests as they are
pytestmark = pytest.mark.usefixtures("guarded_gpu_tests")

CASES = {"utd": ((2, 1, 16, 20, 3), 27), "ntu": ((2, 2, 12, 25, 3), 60)}
# conv biases in front of a train-mode BatchNorm: analytically zero gradient (compared absolutely)
ZERO_GRAD = (".0.bias", ".conv.bias", "out_conv.bias")


def _graph(tag):
    from fusion_gcn_amd.datasets.ntu_rgb_d import constants as ntu
    from fusion_gcn_amd.datasets.utd_mhad import constants as utd
    from fusion_gcn_amd.util import Graph
    c = {"utd": utd, "ntu": ntu}[tag]
    return Graph(c.skeleton_edges, center_joint=c.center_joint)


def _filled_state(ref, tag):
    """the reference's state dict (keys / shapes from the golden manifest) filled by the deterministic filler, float64"""
    from fusion_gcn_amd.models.msg3d.msg3d import Model
    shape, classes = CASES[tag]
    model = Model({"skeleton": shape[1:]}, classes, _graph(tag)).double()      # filled in float64, like the reference's model was
    filler.fill_state_dict(model.state_dict())
    return model, {k: v.detach().clone() for k, v in model.state_dict().items()}


def _inputs(ref, tag):
    shape, classes = CASES[tag]
    x = torch.from_numpy(filler.skeleton_input(f"x.msg3d.{tag}", shape, empty_second_body=(shape[1] > 1)))
    return x, torch.from_numpy(ref[f"{tag}.labels"])


@pytest.mark.parametrize("tag", list(CASES))
def test_adjacency_stacks_match_the_reference(golden, tag):
    ref = golden("msg3d.npz")
    a = ref[f"{tag}.a_binary"]
    assert np.array_equal(_graph(tag).get_adjacency_matrix().astype(np.float64), a)
    assert np.array_equal(O.multi_scale_adjacency(a, 13).astype(np.float64), ref[f"{tag}.A_powers.sgcn1"])
    for w in (3, 5):
        assert np.array_equal(O.multi_scale_adjacency(O.spatial_temporal_graph(a, w), 6).astype(np.float64), ref[f"{tag}.A_scales.w{w}"])


@pytest.mark.parametrize("tag", list(CASES))
def test_module_tree_has_the_references_keys_and_initial_values(golden, tag):
    from fusion_gcn_amd.models.msg3d.msg3d import Model
    ref = golden("msg3d.npz")
    shape, classes = CASES[tag]
    torch.manual_seed(1)
    sd = Model({"skeleton": shape[1:]}, classes, _graph(tag)).state_dict()
    assert list(sd.keys()) == [str(k) for k in ref[f"{tag}.keys"]]
    got = np.array([[float(p.double().sum()), float((p.double() ** 2).sum())] for p in sd.values()])
    assert np.allclose(got, ref[f"{tag}.init_fingerprint"], rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("tag", list(CASES))
def test_oracle_matches_the_reference(golden, tag):
    ref = golden("msg3d.npz")
    _, sd = _filled_state(ref, tag)
    x, labels = _inputs(ref, tag)
    a = ref[f"{tag}.a_binary"]
    with torch.no_grad():
        ev = O.model_forward(x.double(), sd, a, train=False)
    assert rel_l2(ev.numpy(), ref[f"{tag}.eval.logits"]) < 1e-10
    logits, loss, grads, stats = O.loss_and_grads(x.double(), labels, sd, a)
    assert rel_l2(logits.numpy(), ref[f"{tag}.train.logits"]) < 1e-10
    assert abs(float(loss) - float(ref[f"{tag}.train.loss"])) < 1e-10
    for k, g in grads.items():
        want = float(ref[f"{tag}.gl2.{k}"])
        assert abs(float(g.norm()) - want) <= 1e-8 * max(want, 1e-6), k
        if f"{tag}.grad.{k}" in ref.files and want > 1e-9:
            assert rel_l2(g.numpy(), ref[f"{tag}.grad.{k}"]) < 1e-8, k
    for k in ref.files:
        if k.startswith(f"{tag}.after."):
            assert rel_l2(stats.updates[k[len(tag) + 7:]].numpy(), ref[k]) < 1e-10, k


# ---- GPU -------------------------------------------------------------------------------------------------------------------------
def dev():
    return torch.device("cuda:0")


def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64)


@pytest.mark.gpu
@pytest.mark.parametrize("B,T,V,C,stride", [(2, 11, 5, 16, 1), (2, 12, 25, 32, 2), (1, 7, 20, 64, 2), (3, 1, 4, 8, 1)])
def test_temporal_max_pool_kernel(B, T, V, C, stride):
    """fgcn_tmaxpool3 forward / backward vs nn.MaxPool2d((3,1), (stride,1), (1,0)) (ms_tcn.py:76), including ties (post-ReLU
    zeros: torch routes the gradient to the first maximum)."""
    import torch.nn.functional as F
    from fusion_gcn_amd import fops
    x = torch.relu(rnd(B, T, V, C, seed=1)).float()                  # many exact ties at 0
    x_ref = x.double().permute(0, 3, 1, 2).clone().requires_grad_(True)          # (B, C, T, V)
    want = F.max_pool2d(x_ref, kernel_size=(3, 1), stride=(stride, 1), padding=(1, 0))
    probe = rnd(*want.shape, seed=2)
    (gx,) = torch.autograd.grad((want * probe).sum(), x_ref)
    xg = guarded.to(x, dev()).requires_grad_(True)
    got = fops.maxpool3(xg, stride)
    assert torch.equal(got.detach().cpu().double(), want.detach().permute(0, 2, 3, 1))
    (got * guarded.to(probe.permute(0, 2, 3, 1).float(), dev())).sum().backward()
    assert rel_l2(xg.grad.cpu().numpy(), gx.permute(0, 2, 3, 1).numpy()) < 1e-6


@pytest.mark.gpu
@pytest.mark.parametrize("B,T,V,C,window,stride,dilation", [(2, 10, 5, 8, 3, 1, 1), (2, 11, 25, 4, 5, 2, 1), (1, 9, 20, 16, 3, 2, 2),
                                                            (2, 4, 3, 4, 5, 1, 1)])
def test_unfold_windows_kernel(B, T, V, C, window, stride, dilation):
    from fusion_gcn_amd import fops
    x = rnd(B, T, V, C, seed=3)
    x_ref = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    want = O.unfold_windows(x_ref, window, stride, dilation)                      # (B, C, T', window * V)
    probe = rnd(*want.shape, seed=4)
    (gx,) = torch.autograd.grad((want * probe).sum(), x_ref)
    xg = guarded.to(x.float(), dev()).requires_grad_(True)
    got = fops.unfold_windows(xg, window, stride, dilation)
    assert torch.equal(got.detach().cpu().double(), want.detach().permute(0, 2, 3, 1).float().double())
    (got * guarded.to(probe.permute(0, 2, 3, 1).float(), dev())).sum().backward()
    assert rel_l2(xg.grad.cpu().numpy(), gx.permute(0, 2, 3, 1).numpy()) < 1e-6


@pytest.mark.gpu
@pytest.mark.parametrize("B,T,V,C,S", [(2, 6, 25, 4, 13), (2, 5, 75, 32, 6), (1, 3, 125, 16, 6), (2, 4, 20, 96, 13)])
def test_node_mix_aggregation(B, T, V, C, S, fgcn_math):
    """einsum('vu,nctu->nctv') over the stacked (S*V, V) matrix with the scales moved into the channel axis (ms_gcn.py:58-61,
    ms_gtcn.py:118-121), for V up to the 125 nodes of a 5-frame window of a 25-joint skeleton; gradients for x and the matrix."""
    from fusion_gcn_amd import fops
    x, a = rnd(B, T, V, C, seed=5), rnd(S * V, V, seed=6) * 0.2
    xr, ar = x.clone().requires_grad_(True), a.clone().requires_grad_(True)
    want = O.aggregate(xr.permute(0, 3, 1, 2), ar, S).permute(0, 2, 3, 1)         # (B, T, V, S*C)
    probe = rnd(*want.shape, seed=7)
    gx, ga = torch.autograd.grad((want * probe).sum(), (xr, ar))
    xg, ag = guarded.to(x.float(), dev()).requires_grad_(True), guarded.to(a.float(), dev()).requires_grad_(True)
    got = fops.node_mix(xg, fops.node_mix_matrix(ag, S), S)
    assert rel_l2(got.detach().cpu().numpy(), want.detach().numpy()) < 3e-6
    (got * guarded.to(probe.float(), dev())).sum().backward()
    assert rel_l2(xg.grad.cpu().numpy(), gx.numpy()) < 3e-6
    assert rel_l2(ag.grad.cpu().numpy(), ga.numpy()) < 2e-5


def _gpu_model(tag):
    from fusion_gcn_amd.models.msg3d.msg3d import Model
    shape, classes = CASES[tag]
    model = Model({"skeleton": shape[1:]}, classes, _graph(tag))
    filler.fill_state_dict(model.state_dict())
    sd = {k: (v.detach().double().clone() if v.is_floating_point() else v.detach().clone()) for k, v in model.state_dict().items()}
    return guarded.to(model, dev()), sd


@pytest.mark.gpu
@pytest.mark.parametrize("tag", list(CASES))
def test_hip_model_matches_the_reference_and_the_oracle(golden, tag, fgcn_math):
    """Logits (eval and train) and loss against the REFERENCE's outputs; every parameter gradient against the float64 oracle (norms
    within 1 %, the flat gradient within the ReLU-decision floor of float32); running statistics after one step."""
    import torch.nn.functional as F
    ref = golden("msg3d.npz")
    model, sd = _gpu_model(tag)
    x, labels = _inputs(ref, tag)
    a = ref[f"{tag}.a_binary"]
    model.eval()
    with torch.no_grad():
        e_eval = rel_l2(model(guarded.to(x.float(), dev())).cpu().numpy(), ref[f"{tag}.eval.logits"])
    model.train()
    logits = model(guarded.to(x.float(), dev()))
    loss = F.cross_entropy(logits, guarded.to(labels, dev()))
    loss.backward()
    e_train = rel_l2(logits.detach().cpu().numpy(), ref[f"{tag}.train.logits"])
    d_loss = abs(float(loss.detach()) - float(ref[f"{tag}.train.loss"]))
    _, _, grads_o, stats = O.loss_and_grads(x.double(), labels, sd, a)
    names = [n for n, _ in model.named_parameters()]
    flat_g = torch.cat([p.grad.detach().double().flatten().cpu() for _, p in model.named_parameters()])
    flat_o = torch.cat([grads_o[n].double().flatten() for n in names])
    e_grad = float((flat_g - flat_o).norm() / flat_o.norm())
    print(f"[msg3d {tag} {fgcn_math}] eval logits {e_eval:.2e}, train logits {e_train:.2e}, |loss diff| {d_loss:.2e}, flat gradient {e_grad:.2e}")
    assert e_eval < 1e-4 and e_train < 1e-4 and d_loss < 1e-4
    assert e_grad < 5e-3, e_grad
    scale = max(float(g.abs().max()) for g in grads_o.values())
    for n, p in model.named_parameters():
        want = float(grads_o[n].norm())
        if n.endswith(ZERO_GRAD) and not n.startswith("fc"):
            assert float(p.grad.abs().max()) <= 1e-4 * scale, n
        elif want > 1e-7 * scale:
            assert abs(float(p.grad.norm()) - want) <= 2e-2 * want, (n, float(p.grad.norm()), want)
    for k, v in stats.updates.items():
        assert rel_l2(model.state_dict()[k].cpu().numpy(), v.numpy()) < 1e-4, k


@pytest.mark.gpu
def test_msg3d_resolves_through_import_model_and_loads_reference_shaped_checkpoints():
    from fusion_gcn_amd.util.dynamic_import import import_model
    Model = import_model("msg3d")
    shape, classes = CASES["utd"]
    a, b = Model({"skeleton": shape[1:]}, classes, _graph("utd")), Model({"skeleton": shape[1:]}, classes, _graph("utd"))
    filler.fill_state_dict(a.state_dict())
    b.load_state_dict(a.state_dict())
    a, b = guarded.to(a, dev()).eval(), guarded.to(b, dev()).eval()
    x = guarded.to(torch.from_numpy(filler.skeleton_input("x.msg3d.utd", shape)).float(), dev())
    with torch.no_grad():
        assert torch.equal(a(x), b(x))


@pytest.mark.gpu
@pytest.mark.parametrize("B,T,V,K,N,kt,stride,dil", [(2, 12, 20, 16, 16, 3, 1, 1), (2, 13, 25, 32, 32, 3, 2, 3), (1, 9, 20, 64, 64, 3, 1, 4),
                                                     (2, 10, 5, 96, 16, 1, 2, 1), (2, 8, 100, 576, 96, 1, 1, 1)])
def test_conv_rows_matches_conv2d(B, T, V, K, N, kt, stride, dil, fgcn_math):
    """fops.conv_rows (the row GEMM with a temporal map: dilation, stride, 'same' padding -- TemporalConv of ms_tcn.py:15-34 and the
    1x1 convolutions) forward, input gradient, weight and bias gradients against torch's Conv2d in float64; V = 100 exercises the
    folded node axis of the 1x1 form."""
    import torch.nn.functional as F
    from fusion_gcn_amd import fops
    from fusion_gcn_amd.models.msg3d.ms_tcn import out_frames, temporal_map
    x, w, b = rnd(B, T, V, K, seed=11), rnd(N, K, kt, 1, seed=12) * (kt * K) ** -0.5, rnd(N, seed=13)
    xr, wr, br = x.permute(0, 3, 1, 2).clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    pad = (kt + (kt - 1) * (dil - 1) - 1) // 2
    want = F.conv2d(xr, wr, br, stride=(stride, 1), padding=(pad, 0), dilation=(dil, 1))
    probe = rnd(*want.shape, seed=14)
    gx, gw, gb = torch.autograd.grad((want * probe).sum(), (xr, wr, br))
    xg = guarded.to(x.float(), dev()).requires_grad_(True)
    wg, bg = guarded.to(w.float(), dev()).requires_grad_(True), guarded.to(b.float(), dev()).requires_grad_(True)
    got, part = fops.conv_rows(xg, wg[..., 0].permute(2, 1, 0), bg, tmap=temporal_map(kt, stride, dil), T_out=out_frames(T, stride), stats=True)
    assert rel_l2(got.detach().cpu().numpy(), want.detach().permute(0, 2, 3, 1).numpy()) < 3e-6
    flat = want.detach().permute(0, 2, 3, 1).reshape(-1, N)
    assert rel_l2(part.double().sum(0)[0].cpu().numpy(), flat.sum(0).numpy()) < 2e-5          # BatchNorm partial sums of the epilogue
    (got * guarded.to(probe.permute(0, 2, 3, 1).float(), dev())).sum().backward()
    assert rel_l2(xg.grad.cpu().numpy(), gx.permute(0, 2, 3, 1).numpy()) < 3e-6
    assert rel_l2(wg.grad.cpu().numpy(), gw.numpy()) < 2e-5
    assert rel_l2(bg.grad.cpu().numpy(), gb.numpy()) < 2e-5


@pytest.mark.gpu
@pytest.mark.parametrize("stride,cin,cout", [(1, 96, 96), (2, 96, 192)])
def test_multi_scale_temporal_block_matches_the_oracle(stride, cin, cout, fgcn_math):
    """One MultiScale_TemporalConv (ms_tcn.py:37-109: six branches, joined head BatchNorm, dilated convs, pooling, residual) forward,
    input gradient, every parameter gradient and the running statistics against the float64 oracle."""
    from fusion_gcn_amd.models.msg3d.ms_tcn import MultiScale_TemporalConv
    B, T, V = 2, 14, 20
    blk = MultiScale_TemporalConv(cin, cout, stride=stride)
    filler.fill_state_dict(blk.state_dict(), prefix="tcn1.")
    sd = {"tcn1." + k: (v.detach().double().clone() if v.is_floating_point() else v.detach().clone()) for k, v in blk.state_dict().items()}
    blk = guarded.to(blk, dev()).train()
    x = torch.from_numpy(filler.bellish("x.mstcn", (B, cin, T, V)))
    params = {k: v.clone().requires_grad_(True) for k, v in sd.items() if v.is_floating_point() and not k.endswith(("running_mean", "running_var"))}
    live = dict(sd)
    live.update(params)
    xo = x.clone().requires_grad_(True)
    stats = O.Stats()
    want = O.ms_tcn(xo, live, "tcn1", stride, True, stats)
    probe = rnd(*want.shape, seed=21)
    grads = torch.autograd.grad((want * probe).sum(), [xo] + list(params.values()), allow_unused=True)
    xg = guarded.to(x.float().permute(0, 2, 3, 1).contiguous(), dev()).requires_grad_(True)
    got = blk(xg)
    assert rel_l2(got.detach().cpu().numpy(), want.detach().permute(0, 2, 3, 1).numpy()) < 2e-5
    flips = int(((got.detach().cpu() > 0) != (want.detach().permute(0, 2, 3, 1) > 0)).sum())
    (got * guarded.to(probe.permute(0, 2, 3, 1).float(), dev())).sum().backward()
    tol = 2e-4 if flips == 0 else 5e-3
    assert rel_l2(xg.grad.cpu().numpy(), grads[0].permute(0, 2, 3, 1).numpy()) < tol, flips
    scale = max(float(g.abs().max()) for g in grads[1:] if g is not None)
    for (k, _), g in zip(params.items(), grads[1:]):
        mine = dict(blk.named_parameters())[k[5:]].grad
        if k.endswith(ZERO_GRAD):
            assert float(mine.abs().max()) <= 1e-4 * scale, k
        else:
            assert rel_l2(mine.cpu().numpy(), g.numpy()) < tol, (k, flips)
    for k, v in stats.updates.items():
        assert rel_l2(blk.state_dict()[k[5:]].cpu().numpy(), v.numpy()) < 1e-5, k


@pytest.mark.gpu
def test_standalone_module_repacks_its_weights_after_an_in_place_update(fgcn_math):
    """A MultiScale_TemporalConv used on its own (no Model.forward to run the batched refresh): after the parameters change in place
    (an optimizer step, load_state_dict) or move, the next forward must compute with the NEW values -- fops.ParamForms checks every
    form against its sources' addresses and version counters."""
    from fusion_gcn_amd.models.msg3d.ms_tcn import MultiScale_TemporalConv
    B, T, V, cin, cout = 2, 10, 20, 96, 96
    blk = MultiScale_TemporalConv(cin, cout, stride=1)
    filler.fill_state_dict(blk.state_dict(), prefix="tcn1.")
    blk = guarded.to(blk, dev()).train()
    x = torch.from_numpy(filler.bellish("x.mstcn.stale", (B, cin, T, V)))
    xg = guarded.to(x.float().permute(0, 2, 3, 1).contiguous(), dev())

    def oracle():
        sd = {"tcn1." + k: (v.detach().double().cpu().clone() if v.is_floating_point() else v.detach().cpu().clone())
              for k, v in blk.state_dict().items()}
        return O.ms_tcn(x.clone(), sd, "tcn1", 1, True, O.Stats()).permute(0, 2, 3, 1).numpy()

    want0 = oracle()
    got0 = blk(xg).detach().cpu().numpy()
    assert rel_l2(got0, want0) < 2e-5
    with torch.no_grad():                                    # in place: versions bump, addresses stay
        for n, p in blk.named_parameters():
            if n.endswith("weight") and p.dim() > 1:
                p.mul_(-0.7)
            elif n.endswith("bias"):
                p.add_(0.05)
    want1 = oracle()
    assert rel_l2(want1, want0) > 1e-2                       # the update matters
    got1 = blk(xg).detach().cpu().numpy()
    assert rel_l2(got1, want1) < 2e-5, "stale packed weights after an in-place parameter update"
    sd = {k: v.clone() for k, v in blk.state_dict().items()}
    for p in blk.parameters():                               # moved: new storage for every parameter
        p.data = p.data.clone() * 1.25
    want2 = oracle()
    got2 = blk(xg).detach().cpu().numpy()
    assert rel_l2(got2, want2) < 2e-5, "stale packed weights after the parameters moved"


# ---- the graph-conv and G3D pathway blocks, stand-alone, against the float64 oracle ------------------------------------------------
# Every block is built with no Model around it (its forms come from fops.ParamForms, not from the batched refresh_forms), filled by
# the deterministic filler under the key it has in the model, and compared with the oracle evaluated in float64 on the CPU: the
# forward output, the input gradient, EVERY parameter gradient element-wise (rel_l2, so direction as well as norm), and the
# running statistics.  The float64 references depend on the case only: they are computed once and shared by the three math modes.
FWD_TOL, GRAD_TOL, STAT_TOL = 2e-5, 2e-4, 1e-5              # the bounds of test_multi_scale_temporal_block_matches_the_oracle
FLIP_TOL, FLIP_CAP = 5e-3, 1e-4                              # gradients when float32 decided a ReLU differently; share of the hidden elements that may
MASK_EPS, MASK_CAP = 1e-3, 1e-2                              # |pre-activation| below which the probe is zero; largest share it may zero
# Blocks with the ReLU INSIDE: the oracle's smallest hidden |pre-activation| must be at least 20 x the error of a float32 evaluation of
# these unit-scale values (5e-7, torch in float32 on the CPU against the float64 oracle).  Among ~1e5 hidden elements one lies within
# 1e-6 of zero for about one input in ten, and no float32 implementation can be asked for that element's sign; the input is the first
# of the filler's salts whose ORACLE meets the condition (_off_the_kinks), so a kernel never decides which input is used.
KINK_EPS = 1e-5
GCN_SCALES, G3D_SCALES, BATCH = 13, 6, 2

GCN_CASES = [("utd", 3, 96), ("utd", 96, 96), ("utd", 12, 20), ("ntu", 96, 96)]                    # (graph, cin, cout); T = 11
G3D_CASES = [("utd", 3, 96, 3, 1, 11), ("utd", 3, 96, 5, 1, 4), ("utd", 96, 192, 3, 2, 11), ("utd", 96, 192, 5, 2, 12),
             ("utd", 12, 24, 5, 2, 11), ("ntu", 3, 96, 5, 1, 4), ("ntu", 96, 192, 5, 2, 12)]      # (graph, cin, cout, window, stride, T)


def _a_binary(tag):
    return _graph(tag).get_adjacency_matrix().astype(np.float64)


def _gcn_stack(tag):
    return torch.from_numpy(O.multi_scale_adjacency(_a_binary(tag), GCN_SCALES)).double()


def _g3d_stack(tag, window):
    return torch.from_numpy(O.multi_scale_adjacency(O.spatial_temporal_graph(_a_binary(tag), window), G3D_SCALES)).double()


def _state64(mod, prefix):
    """the module's state under the oracle's keys, float64 on the CPU"""
    return {prefix + k: (v.detach().double().cpu().clone() if v.is_floating_point() else v.detach().cpu().clone())
            for k, v in mod.state_dict().items()}


def _live(sd):
    params = {k: v.clone().requires_grad_(True) for k, v in sd.items()
              if v.is_floating_point() and not k.endswith(("running_mean", "running_var"))}
    live = dict(sd)
    live.update(params)
    return params, live


def _cl(t):
    """the oracle's (N, C, T, V) as channels-last (B, T, V, C)"""
    return t.permute(0, 2, 3, 1)


def _device_input(x):
    """(B, C, T, V) float64 -> the float32 channels-last leaf on the device; 3 channels travel as 4 with the 4th exactly zero (data_bn)"""
    xl = _cl(x).float()
    if x.shape[1] == 3:
        xl = torch.nn.functional.pad(xl, (0, 1))
    return guarded.put(xl, device=dev()).requires_grad_(True)


def _finish(ref, want, probe, xo, params, stats, **more):
    grads = torch.autograd.grad((want * probe).sum(), [xo] + list(params.values()))
    ref.update(want=want.detach(), probe=probe, gx=grads[0], grads=dict(zip(params, grads[1:])), stats=dict(stats.updates), **more)
    return ref


def _masked_probe(u, seed):
    """A probe that is zero wherever the oracle's pre-activation is within MASK_EPS of the ReLU's kink: an element whose sign float32 might
    decide differently carries no gradient on either side, so every gradient keeps the tight bound."""
    keep = u.detach().abs() >= MASK_EPS
    return rnd(*u.shape, seed=seed) * keep, 1.0 - float(keep.double().mean())


def _new_gcn(tag, cin, cout):
    from fusion_gcn_amd.models.msg3d.ms_gcn import MultiScale_GraphConv
    mod = MultiScale_GraphConv(GCN_SCALES, cin, cout, _a_binary(tag))
    filler.fill_state_dict(mod.state_dict(), prefix="sgcn1.0.")
    return mod


_references = {}


def _cached(fn):
    def wrapper(*key):
        if (fn.__name__, key) not in _references:
            _references[(fn.__name__, key)] = fn(*key)
        return _references[(fn.__name__, key)]
    return wrapper


@_cached
def _gcn_reference(tag, cin, cout, train=True):
    p = "sgcn1.0"
    params, live = _live(_state64(_new_gcn(tag, cin, cout), p + "."))
    V = len(_a_binary(tag))
    x = torch.from_numpy(filler.bellish(f"x.msgcn.{tag}.{cin}", (BATCH, cin, 11, V)))
    xo, a, stats = x.clone().requires_grad_(True), _gcn_stack(tag), O.Stats()
    want = O.ms_gcn(xo, live, p, a, GCN_SCALES, train, stats)
    with torch.no_grad():
        u = O.mlp(O.aggregate(x, a + live[f"{p}.A_res"], GCN_SCALES), live, f"{p}.mlp", train, None, relu=False)
    probe, masked = _masked_probe(u, seed=31)
    return _finish({"x": x, "prefix": p + "."}, want, probe, xo, params, stats, masked=masked)


def _new_g3d(tag, cin, cout, window, stride):
    from fusion_gcn_amd.models.msg3d.msg3d import MS_G3D
    mod = MS_G3D(cin, cout, _a_binary(tag), G3D_SCALES, window, stride, 1)
    filler.fill_state_dict(mod.state_dict(), prefix=_g3d_key(cin, window) + ".")
    return mod


def _g3d_key(cin, window):
    """the pathway's key in the model: stage 1 has the 3 input channels, the windows 3 and 5 are pathways 0 and 1"""
    return f"gcn3d{1 if cin == 3 else 2}.gcn3d.{(3, 5).index(window)}"


def _g3d_input(tag, cin, T, salt=0):
    return torch.from_numpy(filler.bellish(f"x.msg3d.block.{tag}.{cin}.{T}", (BATCH, cin, T, len(_a_binary(tag))), salt=salt))


def _off_the_kinks(make_input, hidden_of):
    """-> (x, the oracle's hidden pre-activations of x) for the first salt at which none of them is within KINK_EPS of zero"""
    for salt in range(16):
        x = make_input(salt)
        with torch.no_grad():
            hidden = hidden_of(x)
        if min(float(h.abs().min()) for h in hidden) >= KINK_EPS:
            return x, hidden
    raise AssertionError("no input among 16 salts keeps the oracle's hidden pre-activations off the ReLU's kink")


def _g3d_hidden(x, live, p, a_scales, window, stride, train, stats):
    """the first half of O.ms_g3d up to the pre-activation: (N, C_embed, T', window * V)"""
    q = f"{p}.gcn3d.1"
    a = a_scales + live[f"{q}.A_res"]
    return O.mlp(O.aggregate(O.unfold_windows(x, window, stride, 1), a, G3D_SCALES), live, f"{q}.mlp", train, stats, relu=False)


@_cached
def _stgcn_reference(tag, cin, cout, window, stride, T):
    """pathway.gcn3d of an MS_G3D: unfold -> SpatialTemporal_MS_GCN (aggregate, linear MLP, ReLU)"""
    p = _g3d_key(cin, window)
    sd = {k: v for k, v in _state64(_new_g3d(tag, cin, cout, window, stride), p + ".").items() if k.startswith(f"{p}.gcn3d.")}
    params, live = _live(sd)
    x = _g3d_input(tag, cin, T)
    xo, stats = x.clone().requires_grad_(True), O.Stats()
    u = _g3d_hidden(xo, live, p, _g3d_stack(tag, window), window, stride, True, stats)
    probe, masked = _masked_probe(u, seed=32)
    return _finish({"x": x, "prefix": f"{p}.gcn3d."}, torch.relu(u), probe, xo, params, stats, masked=masked)


@_cached
def _g3d_reference(tag, cin, cout, window, stride, T, train=True):
    p = _g3d_key(cin, window)
    params, live = _live(_state64(_new_g3d(tag, cin, cout, window, stride), p + "."))
    a, stats = _g3d_stack(tag, window), O.Stats()
    x, hidden = _off_the_kinks(lambda salt: _g3d_input(tag, cin, T, salt), lambda x: [_g3d_hidden(x, live, p, a, window, stride, train, None)])
    xo = x.clone().requires_grad_(True)
    want = O.ms_g3d(xo, live, p, a, G3D_SCALES, window, stride, 1, train, stats)
    return _finish({"x": x, "prefix": p + "."}, want, rnd(*want.shape, seed=33), xo, params, stats, hidden=hidden[0])


def _errors(mod, ref, got, xg, params=True):
    """(forward, input gradient, {parameter: gradient error}, largest |gradient| of the zero-gradient biases relative to the largest
    gradient entry, {buffer: running statistic error}) of a module after its backward; the 4th input channel's gradient must be 0"""
    prefix, cin = ref["prefix"], ref["x"].shape[1]
    e_fwd = rel_l2(got.detach().cpu().numpy(), _cl(ref["want"]).numpy())
    gx = xg.grad.cpu()
    e_dx = rel_l2(gx[..., :cin].numpy(), _cl(ref["gx"]).numpy())
    assert gx.shape[-1] == cin or not gx[..., cin:].any(), "the zero pad channel of the input received a gradient"
    e_par, e_zero = {}, 0.0
    if params:
        named = dict(mod.named_parameters())
        scale = max(float(g.abs().max()) for g in ref["grads"].values())
        for k, g in ref["grads"].items():
            mine = named[k[len(prefix):]].grad
            assert mine is not None and mine.shape == g.shape, k
            if k.endswith(ZERO_GRAD):
                e_zero = max(e_zero, float(mine.abs().max()) / scale)
            else:
                e_par[k] = rel_l2(mine.cpu().numpy(), g.numpy())
    state = mod.state_dict()
    e_stat = {k: rel_l2(state[k[len(prefix):]].cpu().numpy(), v.numpy()) for k, v in ref["stats"].items()}
    return e_fwd, e_dx, e_par, e_zero, e_stat


def _report_and_assert(label, errors, tol, note=""):
    e_fwd, e_dx, e_par, e_zero, e_stat = errors
    worst = max(e_par, key=e_par.get) if e_par else None
    print(f"[msg3d {label}] forward {e_fwd:.2e}, input gradient {e_dx:.2e}, worst parameter gradient "
          f"{e_par[worst] if worst else 0.0:.2e} ({worst}), zero-gradient biases {e_zero:.2e}, running statistics "
          f"{max(e_stat.values(), default=0.0):.2e}{note}")
    assert e_fwd < FWD_TOL, e_fwd
    assert e_dx < tol, e_dx
    for k, e in e_par.items():
        assert e < tol, (k, e)
    assert e_zero <= 1e-4, e_zero
    for k, e in e_stat.items():
        assert e < STAT_TOL, (k, e)


def _assert_one_batch_tracked(mod):
    bns = [m for m in mod.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)]
    assert bns and all(int(m.num_batches_tracked) == 1 for m in bns)


def _backward(got, ref):
    (got * guarded.to(_cl(ref["probe"]).float(), dev())).sum().backward()


@pytest.mark.parametrize("kind,case", [("gcn", c) for c in GCN_CASES] + [("stgcn", c) for c in G3D_CASES])
def test_masked_probe_of_the_relu_blocks_masks_at_most_one_percent(kind, case):
    """The condition under which the masked-probe comparison of the blocks that END in a ReLU says anything: the oracle alone
    (float64, CPU) puts at most 1 % of the pre-activations within MASK_EPS of zero (0.06-0.10 % with these fills)."""
    ref = (_gcn_reference if kind == "gcn" else _stgcn_reference)(*case)
    assert ref["masked"] <= MASK_CAP, ref["masked"]


@pytest.mark.parametrize("kind,case", [("g3d", c) for c in G3D_CASES] + [("g3d", G3D_CASES[2] + (False,)), ("multi-window", ("utd", 96, 192, 2, 11))])
def test_inputs_of_the_blocks_with_an_inner_relu_stay_off_its_kink(kind, case):
    """The condition of the flips convention's tight branch, from the oracle alone (float64, CPU): no hidden pre-activation of the input
    a pathway test uses is within KINK_EPS of zero, so float32 has no ReLU decision to take differently."""
    ref = (_g3d_reference if kind == "g3d" else _multi_window_reference)(*case)
    hidden = ref["hidden"] if isinstance(ref["hidden"], list) else [ref["hidden"]]
    assert min(float(h.abs().min()) for h in hidden) >= KINK_EPS


@pytest.mark.gpu
@pytest.mark.parametrize("tag,cin,cout", GCN_CASES)
def test_multi_scale_graph_conv_matches_the_oracle(tag, cin, cout, fgcn_math):
    """MultiScale_GraphConv (ms_gcn.py:53-64) vs O.ms_gcn.  utd: V * S = 260 columns, the packed-forms route (_NodeMixParams, whose
    A_res gradient is re-laid out on the host; node_mix_forms with its two source segments; 3 -> 96: scale_major_forms with one pad
    channel per scale group; every case: the grouped weight gradient); 12 -> 20: K = 156 and N = 20 are no multiple of a tile, cout % 8
    != 0; ntu: 325 columns, the torch route.  The block ends in a ReLU: the probe is masked where the oracle's pre-activation is within
    MASK_EPS of zero, so no ReLU decision of float32 enters and every gradient keeps the tight bound."""
    ref = _gcn_reference(tag, cin, cout)
    assert ref["masked"] <= MASK_CAP
    mod = guarded.to(_new_gcn(tag, cin, cout), dev()).train()
    xg = _device_input(ref["x"])
    got = mod(xg)
    assert ("A.a" in mod._forms.forms) == (tag == "utd")                   # the route the case is there for
    _backward(got, ref)
    _report_and_assert(f"gcn {tag} {cin}->{cout} {fgcn_math}", _errors(mod, ref, got, xg), GRAD_TOL, f", masked {ref['masked']:.2%}")
    _assert_one_batch_tracked(mod)


@pytest.mark.gpu
@pytest.mark.parametrize("tag,cin,cout,window,stride,T", G3D_CASES)
def test_spatial_temporal_graph_conv_matches_the_oracle(tag, cin, cout, window, stride, T, fgcn_math):
    """pathway.gcn3d of an MS_G3D -- UnfoldTemporalWindows -> SpatialTemporal_MS_GCN (ms_gtcn.py:37-45, 111-126) -- vs the first half of
    O.ms_g3d, with the masked probe of the graph-conv test (this block ends in a ReLU too).  utd: window * V * S = 360 / 600 columns, the
    forms route; ntu: 125 nodes, 750 columns, the torch route; (5, 1, 4): whole windows of padding."""
    ref = _stgcn_reference(tag, cin, cout, window, stride, T)
    assert ref["masked"] <= MASK_CAP
    mod = guarded.to(_new_g3d(tag, cin, cout, window, stride).gcn3d, dev()).train()
    xg = _device_input(ref["x"])
    got = mod(xg)
    _backward(got, ref)
    _report_and_assert(f"stgcn {tag} {cin}->{cout} w{window} s{stride} T{T} {fgcn_math}", _errors(mod, ref, got, xg), GRAD_TOL,
                       f", masked {ref['masked']:.2%}")
    _assert_one_batch_tracked(mod)


def _run_with_flips(mod, pathways, hiddens, xg):
    """forward with a hook on every pathway's gcn3d; -> (output, ReLU decisions that differ from the oracle's hidden tensors, their count)"""
    seen = []
    hooks = [p.gcn3d.register_forward_hook(lambda _m, _i, out: seen.append(out.detach())) for p in pathways]
    got = mod(xg)
    for h in hooks:
        h.remove()
    assert len(seen) == len(hiddens)
    flips = sum(int(((h.cpu() > 0) != (_cl(o) > 0)).sum()) for h, o in zip(seen, hiddens))
    return got, flips, sum(o.numel() for o in hiddens)


def _flip_tolerance(flips, total):
    assert flips <= FLIP_CAP * total, f"{flips} of {total} hidden ReLU decisions differ from the oracle's"
    return GRAD_TOL if flips == 0 else FLIP_TOL


@pytest.mark.gpu
@pytest.mark.parametrize("tag,cin,cout,window,stride,T", G3D_CASES)
def test_g3d_pathway_matches_the_oracle(tag, cin, cout, window, stride, T, fgcn_math):
    """MS_G3D (msg3d.py:60-73: unfold, SpatialTemporal_MS_GCN, the (1, window, 1) collapse as a temporal conv with tmap (ws, ws, 1, 0, 1),
    BatchNorm) vs O.ms_g3d.  The ReLU is inside: its decisions are compared with the oracle's hidden tensor through a forward hook; the
    tight gradient bound when none differs, 5e-3 otherwise, and never more than 1e-4 of them may differ."""
    ref = _g3d_reference(tag, cin, cout, window, stride, T)
    mod = guarded.to(_new_g3d(tag, cin, cout, window, stride), dev()).train()
    xg = _device_input(ref["x"])
    got, flips, total = _run_with_flips(mod, [mod], [ref["hidden"]], xg)
    _backward(got, ref)
    errors = _errors(mod, ref, got, xg)
    tol = _flip_tolerance(flips, total)
    _report_and_assert(f"g3d {tag} {cin}->{cout} w{window} s{stride} T{T} {fgcn_math}", errors, tol, f", flips {flips}/{total}")
    _assert_one_batch_tracked(mod)


@pytest.mark.gpu
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("shape", [(2, 7, 20, 96), (2, 5, 25, 20), (1, 3, 5, 12)])
def test_add_act_equals_torch_including_the_ties(shape, relu, fgcn_math):
    """fops.add_act (the join of the two windows and of the stage) on a coarse grid, so that a + b == 0 exactly at many elements: the
    forward is torch's bit for bit, and both input gradients are torch's -- zero at the ties.  (1, 3, 5, 12): 180 elements, no multiple
    of 8, so there is no sign image and the backward gates from the output."""
    from fusion_gcn_amd import fops
    g = torch.Generator().manual_seed(41)
    a, b = (torch.randint(-3, 4, shape, generator=g).float() * 0.5 for _ in range(2))
    assert int((a + b == 0).sum()) > a.numel() // 20
    ar, br = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    want = torch.relu(ar + br) if relu else ar + br
    probe = rnd(*shape, seed=42).float()
    ga, gb = torch.autograd.grad((want * probe).sum(), (ar, br))
    ag, bg = guarded.to(a, dev()).requires_grad_(True), guarded.to(b, dev()).requires_grad_(True)
    got = fops.add_act(ag, bg, relu=relu)
    assert torch.equal(got.detach().cpu(), want.detach())
    (got * guarded.to(probe, dev())).sum().backward()
    assert torch.equal(ag.grad.cpu(), ga) and torch.equal(bg.grad.cpu(), gb)
    if relu:
        assert not ag.grad.cpu()[a + b == 0].any()


@_cached
def _multi_window_reference(tag, cin, cout, stride, T):
    from fusion_gcn_amd.models.msg3d.msg3d import MultiWindow_MS_G3D
    p = "gcn3d2"
    mod = MultiWindow_MS_G3D(cin, cout, _a_binary(tag), G3D_SCALES, window_stride=stride)
    filler.fill_state_dict(mod.state_dict(), prefix=p + ".")
    params, live = _live(_state64(mod, p + "."))
    x, hidden = _off_the_kinks(lambda salt: _g3d_input(tag, cin, T, salt),
                               lambda x: [_g3d_hidden(x, live, f"{p}.gcn3d.{j}", _g3d_stack(tag, w), w, stride, True, None)
                                          for j, (w, _) in enumerate(O.WINDOWS)])
    xo, stats, want = x.clone().requires_grad_(True), O.Stats(), 0
    for j, (w, dil) in enumerate(O.WINDOWS):
        want = want + O.ms_g3d(xo, live, f"{p}.gcn3d.{j}", _g3d_stack(tag, w), G3D_SCALES, w, stride, dil, True, stats)
    return _finish({"x": x, "prefix": p + ".", "module": mod.state_dict()}, want, rnd(*want.shape, seed=34), xo, params, stats, hidden=hidden)


@pytest.mark.gpu
def test_multi_window_g3d_matches_the_sum_of_the_oracles_pathways(fgcn_math):
    """MultiWindow_MS_G3D(96, 192, stride 2) on utd at T = 11 (msg3d.py:104-110: the windows 3 and 5 joined by fops.add_act without an
    activation) vs the sum of the two O.ms_g3d pathways; the flips convention of the pathway test, summed over both pathways.
    (Measured with the filler's salt 0, whose oracle has one hidden pre-activation of 1.7e-7 in the window-5 pathway: float32 took
    that one ReLU decision of 184320 the other way in all three modes, the input gradient was off by 3.25e-3 and the 96-element
    gcn3d.1.gcn3d.1.mlp.layers.1.bias gradient by 5.20e-3, over the 5e-3 of the convention; every other error was below 1e-6.  The
    bounds stand; the input is now one whose oracle keeps KINK_EPS from the kink, see _off_the_kinks.)"""
    from fusion_gcn_amd.models.msg3d.msg3d import MultiWindow_MS_G3D
    tag, cin, cout, stride, T = "utd", 96, 192, 2, 11
    ref = _multi_window_reference(tag, cin, cout, stride, T)
    mod = MultiWindow_MS_G3D(cin, cout, _a_binary(tag), G3D_SCALES, window_stride=stride)
    mod.load_state_dict(ref["module"])
    mod = guarded.to(mod, dev()).train()
    xg = _device_input(ref["x"])
    got, flips, total = _run_with_flips(mod, list(mod.gcn3d), ref["hidden"], xg)
    _backward(got, ref)
    errors = _errors(mod, ref, got, xg)
    tol = _flip_tolerance(flips, total)
    _report_and_assert(f"multi-window {tag} {cin}->{cout} s{stride} T{T} {fgcn_math}", errors, tol, f", flips {flips}/{total}")
    _assert_one_batch_tracked(mod)


def _buffers(mod):
    return {k: v.detach().clone() for k, v in mod.state_dict().items() if k.endswith(("running_mean", "running_var", "num_batches_tracked"))}


def _assert_buffers_untouched(mod, before):
    after = _buffers(mod)
    assert before and all(torch.equal(after[k], v) for k, v in before.items())


@pytest.mark.gpu
def test_graph_conv_in_eval_mode_matches_the_oracle(fgcn_math):
    """MultiScale_GraphConv utd 96 -> 96 after .eval(): forward and input gradient vs the oracle at train=False on the filled running
    statistics (the masked probe again), which the forward must leave bit for bit as they were, like num_batches_tracked."""
    ref = _gcn_reference("utd", 96, 96, False)
    assert ref["masked"] <= MASK_CAP and not ref["stats"]
    mod = guarded.to(_new_gcn("utd", 96, 96), dev()).eval()
    before = _buffers(mod)
    xg = _device_input(ref["x"])
    got = mod(xg)
    _backward(got, ref)
    _report_and_assert(f"gcn eval utd 96->96 {fgcn_math}", _errors(mod, ref, got, xg, params=False), GRAD_TOL, f", masked {ref['masked']:.2%}")
    _assert_buffers_untouched(mod, before)


@pytest.mark.gpu
def test_g3d_pathway_in_eval_mode_matches_the_oracle(fgcn_math):
    """MS_G3D utd (96, 192, window 3, stride 2, T = 11) after .eval(), as the graph-conv eval test; the flips convention of the pathway test."""
    case = ("utd", 96, 192, 3, 2, 11)
    ref = _g3d_reference(*case, False)
    assert not ref["stats"]
    mod = guarded.to(_new_g3d(*case[:5]), dev()).eval()
    before = _buffers(mod)
    xg = _device_input(ref["x"])
    got, flips, total = _run_with_flips(mod, [mod], [ref["hidden"]], xg)
    _backward(got, ref)
    errors = _errors(mod, ref, got, xg, params=False)
    _report_and_assert(f"g3d eval utd 96->192 w3 s2 T11 {fgcn_math}", errors, _flip_tolerance(flips, total), f", flips {flips}/{total}")
    _assert_buffers_untouched(mod, before)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["gcn", "stgcn"])
def test_standalone_graph_conv_repacks_its_matrix_after_an_update(kind, fgcn_math):
    """The node-mix matrix of a MultiScale_GraphConv (utd 96 -> 96) and of a SpatialTemporal_MS_GCN (window 3) used on their own is a
    packed form with TWO sources, the constant stack (a plain attribute) and A_res.  After A_res and then the MLP weight change in
    place, after every parameter moves to new storage, and after the constant stack is replaced by another tensor, the next forward
    must compute with the NEW values; every step moves the oracle's result by more than 1e-2."""
    V, C, T = 20, 96, 10
    if kind == "gcn":
        from fusion_gcn_amd.models.msg3d.ms_gcn import MultiScale_GraphConv
        blk, S, nodes, const = MultiScale_GraphConv(GCN_SCALES, C, C, _a_binary("utd")), GCN_SCALES, V, "A_powers"
    else:
        from fusion_gcn_amd.models.msg3d.ms_gtcn import SpatialTemporal_MS_GCN
        blk, S, nodes, const = SpatialTemporal_MS_GCN(C, C, _a_binary("utd"), G3D_SCALES, 3), G3D_SCALES, 3 * V, "A_scales"
    filler.fill_state_dict(blk.state_dict(), prefix="stale.")
    blk = guarded.to(blk, dev()).train()
    x = torch.from_numpy(filler.bellish(f"x.{kind}.stale", (BATCH, C, T, nodes)))
    xg = guarded.to(_cl(x).float().contiguous(), dev())

    def oracle():
        sd = _state64(blk, "p.")
        a = getattr(blk, const).detach().double().cpu() + sd["p.A_res"]
        with torch.no_grad():
            return _cl(O.mlp(O.aggregate(x, a, S), sd, "p.mlp", True, None, relu=True)).numpy()

    def step(what, last):
        want = oracle()
        assert rel_l2(want, last) > 1e-2, what                  # the update matters
        assert rel_l2(blk(xg).detach().cpu().numpy(), want) < FWD_TOL, f"stale packed form after {what}"
        return want

    want = oracle()
    assert rel_l2(blk(xg).detach().cpu().numpy(), want) < FWD_TOL
    assert "A.a" in blk._forms.forms                            # the forms route
    with torch.no_grad():                                       # in place: versions bump, addresses stay
        blk.A_res.mul_(-8.0)
    want = step("an in-place update of A_res", want)
    with torch.no_grad():
        blk.mlp.layers[0].weight.mul_(-0.7).add_(0.02)
    want = step("an in-place update of the MLP weight", want)
    for p in blk.parameters():                                  # moved: new storage for every parameter
        p.data = p.data.clone().flip(0) * 1.25
    want = step("the parameters moved", want)
    fresh = getattr(blk, const).clone()                         # the constant stack: another tensor with other values
    fresh[:nodes] *= 0.25
    setattr(blk, const, fresh)
    step("the constant stack was replaced", want)


@pytest.mark.gpu
def test_bn_act_gates_from_the_output_when_there_is_no_sign_image(fgcn_math):
    """relu(BatchNorm(conv 1x1)) on (1, 5, 7, 12): 420 elements are no multiple of 8, so fops.bn_act keeps no sign image and its backward
    gates from the saved output (no block of the model reaches that branch).  Against torch in float64 with the masked probe."""
    import torch.nn.functional as F
    from fusion_gcn_amd import fops
    B, T, V, C = 1, 5, 7, 12
    x, w, b, gamma, beta = rnd(B, T, V, C, seed=51), rnd(C, C, seed=52) * C ** -0.5, rnd(C, seed=53), 1 + 0.2 * rnd(C, seed=54), rnd(C, seed=55)
    leaves = [t.clone().requires_grad_(True) for t in (x, w, gamma, beta)]
    u = F.batch_norm(F.conv2d(leaves[0].permute(0, 3, 1, 2), leaves[1][:, :, None, None], b), None, None, leaves[2], leaves[3], True)
    probe, masked = _masked_probe(u, seed=56)
    wants = torch.autograd.grad((torch.relu(u) * probe).sum(), leaves)
    bn = torch.nn.BatchNorm2d(C)
    with torch.no_grad():
        bn.weight.copy_(gamma), bn.bias.copy_(beta)
    bn = guarded.to(bn, dev()).train()
    xg, wg = guarded.to(x.float(), dev()).requires_grad_(True), guarded.to(w.float(), dev()).requires_grad_(True)
    y, part = fops.conv_rows(xg, wg.t().unsqueeze(0), guarded.to(b.float(), dev()), stats=True)
    got = fops.bn_act(y, part, bn, relu=True)
    (got * guarded.to(_cl(probe).float(), dev())).sum().backward()
    errs = [rel_l2(got.detach().cpu().numpy(), _cl(torch.relu(u)).detach().numpy())]
    errs += [rel_l2(g.grad.cpu().numpy(), want.numpy()) for g, want in zip((xg, wg, bn.weight, bn.bias), wants)]
    print(f"[msg3d bn_act without a sign image {fgcn_math}] forward {errs[0]:.2e}, gradients of x, w, gamma, beta " + ", ".join(f"{e:.2e}" for e in errs[1:]))
    assert masked <= 0.05 and errs[0] < FWD_TOL and max(errs[1:]) < GRAD_TOL, errs
