"""CTR-GCN on the MI355X against its float64 restatement (tests/ctrgcn_ref.py): the aggregation op ``fops.ctr_aggregate``, the graph
convolution unit and the block in every float32-class math mode (train and eval), one bf16 case, the ten-layer model, eager and through one
GraphStep recording.

Tolerances are the project's (tests/test_msg3d.py, test_block_routes_gpu.tolerances): 2e-5 relative L2 on a forward result, 2e-4 on dx and
on every parameter gradient separately, 1e-5 on running statistics; the conv biases in front of a train-mode BatchNorm, whose true
gradient is zero, are compared absolutely (1e-4 of the largest gradient entry).  The op, unit and block inputs are chosen by ctrgcn_ref's
salt rule from the reference alone; the model, which has too many ReLU decisions for that rule, is compared with the reference taking the
decisions the run took.  Every run is made on guarded allocations (tests/guarded.py)."""
import copy

import numpy as np
import pytest
import torch

import ctrgcn_ref as R
import guarded
from guarded import guarded_allocations  # noqa: F401  (the fixture)
from conftest import rel_l2

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F32_MODES = ("f32", "bf16x3", "f16x2")
TOL_OUT, TOL_GRAD, TOL_STAT, TOL_ZERO = 2e-5, 2e-4, 1e-5, 1e-4
ZERO_GRAD = (".0.bias", ".conv.bias")            # conv biases in front of a train-mode BatchNorm (down.0, residual.conv, MS-TCN's)


# ---- op level ---------------------------------------------------------------------------------------------------------------------------
def _run_op(ref):
    from fusion_gcn_amd import fops
    ins = [guarded.put(t.float(), device=DEV).requires_grad_(True) for t in ref["inputs"]]
    y = fops.ctr_aggregate(*ins)
    (y * guarded.put(ref["probe"].float(), device=DEV)).sum().backward()
    torch.cuda.synchronize()
    return y.detach(), [t.grad.detach() for t in ins]


def _op_errors(ref, y, grads):
    errs = {"y": rel_l2(y.cpu().numpy(), ref["y"].numpy())}
    for k, got, want in zip(R.OP_NAMES, grads, ref["grads"]):
        assert got.shape == want.shape, k
        errs["d" + k] = rel_l2(got.cpu().numpy(), want.numpy())
    return errs


@pytest.mark.parametrize("case", R.OP_CASES, ids=lambda c: R.tag_of(*c))
def test_ctr_aggregate_vs_reference(case, guarded_allocations):
    ref = R.op_case(case)
    assert ref["cond"] < R.COND_MAX
    y, grads = _run_op(ref)
    errs = _op_errors(ref, y, grads)
    print(f"{case}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()), flush=True)
    assert errs["y"] < TOL_OUT, errs
    assert all(v < TOL_GRAD for k, v in errs.items() if k != "y"), errs
    # every sum has one order: a second run gives the same bits
    y2, grads2 = _run_op(ref)
    assert torch.equal(y, y2) and all(torch.equal(a, b) for a, b in zip(grads, grads2))
    # one NaN in the last sample's x3: the other samples keep their bits, the sample is NaN where the definition makes it NaN
    bad = R.op_case(case, nan=True)
    y_n, grads_n = _run_op(bad)
    last = case[0] - 1
    assert torch.equal(y_n[:last], y[:last]) and torch.equal(grads_n[0][:last], grads[0][:last]) and torch.equal(grads_n[1][:last], grads[1][:last])
    assert torch.equal(torch.isnan(y_n[last]).cpu(), torch.isnan(bad["y"][last])) and bool(torch.isnan(bad["y"][last]).any())
    for k, got, want in zip(R.OP_NAMES, grads_n, bad["grads"]):
        assert torch.equal(torch.isnan(got).cpu(), torch.isnan(want)), k
    # alpha == 0, its initial value, still multiplies: y is the static-graph product and dalpha is still right
    zero = R.op_case(case, alpha=0.0)
    y0, grads0 = _run_op(zero)
    x3, pa = zero["inputs"][0], zero["inputs"][5]
    C = case[4]
    static = sum(torch.einsum("uv,btvc->btuc", pa[k], x3[..., k * C:(k + 1) * C]) for k in range(R.K))
    errs0 = _op_errors(zero, y0, grads0)
    print(f"    alpha = 0: y {rel_l2(y0.cpu().numpy(), static.numpy()):.2e}, dalpha {errs0['dalpha']:.2e}", flush=True)
    assert rel_l2(y0.cpu().numpy(), static.numpy()) < TOL_OUT and errs0["dalpha"] < TOL_GRAD and float(zero["grads"][4].abs()) > 0
    assert float(grads0[2].abs().max()) == 0.0 and float(grads0[3].abs().max()) == 0.0            # dW4 = db4 = 0 . (finite sums)
    guarded_allocations.check()


def test_a_workgroup_walks_three_frame_chunks_with_a_ragged_last_one():
    """the op case (3, 13, 25, 64 -> 64): through the host geometry query, one workgroup of the aggregation walks its frames in at least
    three LDS chunks, the last of them short"""
    from fusion_gcn_amd import ops
    B, T, V, _, C = R.OP_CASES[1]
    splits, fps, chunk = ops.ctr_geometry(B, T, V, C)
    last = min(fps, T - (splits - 1) * fps)
    assert splits * fps >= T and -(-fps // chunk) >= 3 and (fps % chunk != 0 or last % chunk != 0), (splits, fps, chunk)
    # the weight-gradient pass walks all T frames in one workgroup
    assert -(-T // chunk) >= 3 and T % chunk != 0


def test_the_split_case_runs_two_frame_splits_with_a_short_last_one():
    """(2, 37, 25, 64 -> 64), compared with the reference in test_ctr_aggregate_vs_reference: the aggregation and its dx3 run workgroups
    with blockIdx.y > 0, and the last split is shorter than the others"""
    from fusion_gcn_amd import ops
    B, T, V, _, C = R.SPLIT_CASE
    splits, fps, chunk = ops.ctr_geometry(B, T, V, C)
    assert splits >= 2 and (splits - 1) * fps < T < splits * fps and fps % chunk != 0, (splits, fps, chunk)


def test_temporal_mean_and_both_forms_of_its_backward(guarded_allocations):
    """xm = mean_t x at the 4-wide input and at 64 channels; dx = dxm / T into a fresh tensor and ADDED to a given one"""
    from fusion_gcn_amd import fops, ops
    for B, T, V, C in ((2, 7, 25, 4), (3, 13, 22, 64)):
        g = torch.Generator().manual_seed(T)
        x, dxm, acc = torch.randn(B, T, V, C, generator=g), torch.randn(B, V, C, generator=g), torch.randn(B, T, V, C, generator=g)
        xd = guarded.put(x, device=DEV).requires_grad_(True)
        xm = fops.ctr_mean_t(xd)
        xm.backward(guarded.put(dxm, device=DEV))
        assert rel_l2(xm.detach().cpu().numpy(), x.double().mean(1).numpy()) < 1e-6
        want = (dxm.double() / T).unsqueeze(1).expand(B, T, V, C)
        assert rel_l2(xd.grad.cpu().numpy(), want.numpy()) < 1e-6
        out = guarded.put(acc, device=DEV)
        assert ops.ctr_mean_t_bwd(guarded.put(dxm, device=DEV), T, out=out) is out
        assert rel_l2(out.cpu().numpy(), (acc.double() + want).numpy()) < 1e-6
    guarded_allocations.check()


def test_ctr_wrappers_refuse_what_the_kernels_do_not_take(guarded_allocations):
    from fusion_gcn_amd import _lib, fops
    z = lambda *s: torch.zeros(s, device=DEV)  # noqa: E731
    with pytest.raises(_lib.FgcnError, match="bad B/T/V"):
        fops.ctr_aggregate(z(2, 4, 33, 192), z(2, 33, 48), z(3, 64, 8), z(3, 64), z(1), z(3, 33, 33))
    with pytest.raises(_lib.FgcnError, match="multiple of 64"):
        fops.ctr_aggregate(z(2, 4, 25, 288), z(2, 25, 48), z(3, 96, 8), z(3, 96), z(1), z(3, 25, 25))
    with pytest.raises(_lib.FgcnError, match="bad B/T/V"):
        fops.ctr_mean_t(z(2, 4, 33, 4))


# ---- unit and block level ---------------------------------------------------------------------------------------------------------------
def _cl(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _product(kind, case, state):
    from fusion_gcn_amd.models.ctrgcn.ctrgcn import TCN_GCN_unit, unit_gcn
    A = np.zeros((R.K, case.V, case.V), np.float32)
    mod = unit_gcn(case.cin, case.cout, A) if kind == "unit" else TCN_GCN_unit(case.cin, case.cout, A, stride=case.stride, residual=case.cin != 3)
    mod.load_state_dict({k: (v.float() if v.is_floating_point() else v) for k, v in state.items()})
    return mod.to(DEV)


def _run_module(kind, case, ref, train):
    mod = _product(kind, case, ref["state"]).train(train)
    x = _cl(ref["x"]).float()
    if x.shape[-1] % 4:
        x = torch.nn.functional.pad(x, (0, 4 - x.shape[-1] % 4))
    xg = guarded.put(x, device=DEV).requires_grad_(True)
    out = mod(xg)
    (out * guarded.put(_cl(ref["probe"]).float(), device=DEV)).sum().backward()
    torch.cuda.synchronize()
    return mod, out.detach(), xg.grad


def _module_fails(mod, out, dx, ref, case, train, tol_out=TOL_OUT, tol_grad=TOL_GRAD):
    fails, errs = [], {}
    errs["out"] = rel_l2(out.cpu().numpy(), _cl(ref["out"]).numpy())
    if not errs["out"] < tol_out:
        fails.append(f"forward {errs['out']:.3e} >= {tol_out:g}")
    errs["dx"] = rel_l2(dx[..., :case.cin].cpu().numpy(), _cl(ref["dx"]).numpy())
    if not errs["dx"] < tol_grad:
        fails.append(f"dx {errs['dx']:.3e} >= {tol_grad:g}")
    if dx.shape[-1] != case.cin and bool(dx[..., case.cin:].any()):
        fails.append("the zero pad channel of the input received a gradient")
    scale = max(float(g.abs().max()) for g in ref["grads"].values())
    worst = ("", 0.0)
    for k, p in mod.named_parameters():
        want = ref["grads"][k]
        assert p.grad is not None and p.grad.shape == want.shape, k
        if train and k.endswith(ZERO_GRAD):
            assert float(want.abs().max()) <= 1e-9 * scale, k
            if not float(p.grad.abs().max()) <= TOL_ZERO * scale:
                fails.append(f"{k}: |gradient| {float(p.grad.abs().max()):.3e} of a zero gradient (scale {scale:.3e})")
            continue
        e = rel_l2(p.grad.cpu().numpy(), want.numpy())
        worst = max(worst, (k, e), key=lambda t: t[1])
        if not e < tol_grad:
            fails.append(f"{k} {e:.3e} >= {tol_grad:g}")
    state = mod.state_dict()
    for k, v in ref["buffers"].items():
        if train:
            e = rel_l2(state[k].cpu().numpy(), v.numpy())
            if not e < TOL_STAT:
                fails.append(f"{k} {e:.3e} >= {TOL_STAT:g}")
        elif not torch.equal(state[k].cpu(), ref["state"][k].float()):
            fails.append(f"buffer {k} changed in eval mode")
    return fails, errs, worst


@pytest.mark.parametrize("fgcn_math", F32_MODES, indirect=True)
@pytest.mark.parametrize("phase", ("train", "eval"))
@pytest.mark.parametrize("case", R.BLOCK_CASES, ids=[c.name for c in R.BLOCK_CASES])
@pytest.mark.parametrize("kind", R.KINDS)
def test_unit_and_block_vs_reference(kind, case, phase, fgcn_math, guarded_allocations):
    train = phase == "train"
    ref = R.block_ref(kind, case, train)
    assert ref["least"] >= R.KINK_EPS and ref["cond"] < R.COND_MAX
    mod, out, dx = _run_module(kind, case, ref, train)
    fails, errs, worst = _module_fails(mod, out, dx, ref, case, train)
    print(f"[{fgcn_math} {phase} {kind} {case.name}] salt {ref['salt']} fwd {errs['out']:.2e} dx {errs['dx']:.2e} worst {worst[1]:.2e} ({worst[0]})", flush=True)
    assert not fails, "\n".join(fails)
    guarded_allocations.check()


@pytest.mark.parametrize("fgcn_math", ["bf16"], indirect=True)
def test_block_in_bf16(fgcn_math, guarded_allocations):
    """math mode bf16 at that mode's contract: 1e-2 forward, cosine >= 0.98 per gradient; the new kernels' tensors stay float32"""
    case = R.BLOCK_CASES[1]
    ref = R.block_ref("block", case, True)
    mod, out, dx = _run_module("block", case, ref, True)
    fwd = rel_l2(out.cpu().numpy(), _cl(ref["out"]).numpy())
    cos = lambda a, b: float((a.double().flatten() @ b.double().flatten()) / (a.double().norm() * b.double().norm()))  # noqa: E731
    worst = ("dx", cos(dx.cpu(), _cl(ref["dx"])))
    for k, p in mod.named_parameters():
        if not k.endswith(ZERO_GRAD):
            worst = min(worst, (k, cos(p.grad.cpu(), ref["grads"][k])), key=lambda t: t[1])
    print(f"[bf16 train block {case.name}] fwd {fwd:.2e} worst cosine {worst[1]:.4f} ({worst[0]})", flush=True)
    assert fwd < 1e-2 and worst[1] >= 0.98, (fwd, worst)


# ---- model level ------------------------------------------------------------------------------------------------------------------------
def _model(state=None):
    from fusion_gcn_amd.datasets.ntu_rgb_d import constants as ntu
    from fusion_gcn_amd.util import Graph
    from fusion_gcn_amd.util.dynamic_import import import_model
    model = import_model("ctrgcn")({"skeleton": R.MODEL_SHAPE}, R.MODEL_CLASSES, Graph(ntu.skeleton_edges, center_joint=ntu.center_joint))
    if state is not None:
        model.load_state_dict({k: (v.float() if v.is_floating_point() else v) for k, v in state.items()})
    return model


def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _reference_order(outs):
    """the product's ReLU outputs (channels-last, in call order: per block the unit's, the three temporal heads' as one tensor, the block's)
    -> the decisions in the reference's order (NCHW: the unit's, each head's, the block's)"""
    assert len(outs) == 30, len(outs)
    masks = []
    for i in range(0, 30, 3):
        unit, heads, block = (_nchw(o > 0) for o in outs[i:i + 3])
        assert heads.shape[1] * 4 == unit.shape[1] * 3, (tuple(heads.shape), tuple(unit.shape))
        masks += [unit, *heads.chunk(3, dim=1), block]
    return masks


@pytest.mark.parametrize("fgcn_math", F32_MODES, indirect=True)
def test_model_vs_reference(fgcn_math, guarded_allocations, monkeypatch):
    """Logits at 2e-5 against the float64 reference; the loss's gradient for EVERY parameter separately at 2e-4 against the float64
    reference taking the ReLU decisions this run took (ctrgcn_ref.model_forced).  The model takes three million decisions, so a few of
    them differ from the reference's own in float32; those must be at most FLIP_CAP of all, each at a pre-activation of the reference
    within 1e-4 of zero (ten times KINK_EPS: rounding, not an error).  The ten alphas are held to the same 2e-4 although their terms
    cancel up to several hundred-fold in this input (printed); the conv biases in front of a train-mode BatchNorm are compared
    absolutely."""
    from fusion_gcn_amd import ops
    ref = R.model_ref()
    model = _model(ref["state"]).to(DEV).train()
    outs, bn_act = [], ops.bn_act

    def recording(*args, **kw):
        res = bn_act(*args, **kw)
        if kw.get("relu"):
            outs.append((res[0] if isinstance(res, tuple) else res).detach())
        return res
    monkeypatch.setattr(ops, "bn_act", recording)
    logits = model(guarded.put(ref["x"].float(), device=DEV))
    monkeypatch.setattr(ops, "bn_act", bn_act)
    torch.nn.functional.cross_entropy(logits, ref["labels"].to(DEV)).backward()
    torch.cuda.synchronize()
    e_logits = rel_l2(logits.detach().cpu().numpy(), ref["out"].numpy())
    forced = R.model_forced([m.cpu() for m in _reference_order(outs)])
    assert forced["flips"] <= R.FLIP_CAP * forced["decisions"] and forced["close"] < 10 * R.KINK_EPS, (forced["flips"], forced["close"])
    assert rel_l2(forced["out"].numpy(), ref["out"].numpy()) < 1e-6
    scale = max(float(g.abs().max()) for g in forced["grads"].values())
    fails, errs = [], {}
    for k, p in model.named_parameters():
        want = forced["grads"][k]
        assert p.grad is not None and p.grad.shape == want.shape, k
        if k.endswith(ZERO_GRAD) and not k.startswith("fc"):
            assert float(want.abs().max()) <= 1e-9 * scale, k
            if not float(p.grad.abs().max()) <= TOL_ZERO * scale:
                fails.append(f"{k}: |gradient| {float(p.grad.abs().max()):.3e} of a zero gradient")
            continue
        errs[k] = rel_l2(p.grad.cpu().numpy(), want.numpy())
        if not errs[k] < TOL_GRAD:
            fails.append(f"{k} {errs[k]:.3e} >= {TOL_GRAD:g}")
    top = sorted(errs.items(), key=lambda t: -t[1])[:5]
    print(f"[{fgcn_math} model] logits {e_logits:.2e}; {forced['flips']} of {forced['decisions']} ReLU decisions differ from the reference's own, the "
          f"farthest at |pre-activation| {forced['close']:.1e}; alpha terms cancel up to {max(forced['conds']):.0f}-fold; worst gradients: "
          + ", ".join(f"{k} {e:.2e}" for k, e in top), flush=True)
    assert e_logits < TOL_OUT, e_logits
    assert not fails, "\n".join(fails)
    guarded_allocations.check()


def test_model_graph_step_is_the_eager_step():
    """one GraphStep recording of the model replays the eager training bit for bit: losses, predictions, every parameter and buffer"""
    from fusion_gcn_amd.session.procedures import DefaultBatchProcessor, DefaultStep, GraphStep
    from test_session_gpu import assert_same_training, batches, train
    data = batches([R.MODEL_CLIPS] * 3, R.MODEL_SHAPE, R.MODEL_CLASSES)
    base = _model(R.model_ref()["state"])
    step = GraphStep()
    eager, keep_e = train(copy.deepcopy(base), DefaultBatchProcessor(DefaultStep()), data)
    graph, keep_g = train(copy.deepcopy(base), DefaultBatchProcessor(step), data)
    assert len(step._recorded) == 1 and step.replays == 3
    moved = [k for k, v in graph.state_dict().items() if k.endswith(("alpha", "PA")) and not torch.equal(v.cpu(), base.state_dict()[k])]
    assert len(moved) == 20, moved                       # the recording trains the refinement's parameters
    assert_same_training(graph, eager, keep_g, keep_e, tol=0.0)
