"""Shift-GCN on the MI355X against its float64 restatement (tests/shiftgcn_ref.py): the two shift operations ``fops.joint_shift`` and
``fops.frame_shift``, the graph unit, the temporal unit and the block in every float32-class math mode (train and eval), one bf16 case, the
ten-layer model, eager and through one GraphStep recording.

Tolerances are the project's (tests/test_msg3d.py, tests/test_ctrgcn_gpu.py): 2e-5 relative L2 on a forward result, 2e-4 on dx and on
every parameter gradient separately, 1e-5 on running statistics; the biases in front of a train-mode BatchNorm (Linear_bias, down.0.bias,
residual.conv.bias), whose true gradient is zero, are compared absolutely (1e-4 of the largest gradient entry).  A joint shift without a
gate or with a zero gate is a permutation (times 1.0): it is compared bit for bit with ``index_select``.  The op, unit and block inputs are
chosen by shiftgcn_ref's salt rule from the reference alone; the model, which has too many ReLU decisions for that rule, is compared with
the reference taking the decisions the run took.  Every run is made on guarded allocations (tests/guarded.py)."""
import copy

import pytest
import torch

import guarded
import shiftgcn_ref as R
from conftest import rel_l2
from guarded import guarded_allocations  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F32_MODES = ("f32", "bf16x3", "f16x2")
TOL_OUT, TOL_GRAD, TOL_STAT, TOL_ZERO = 2e-5, 2e-4, 1e-5, 1e-4
ZERO_GRAD = ("Linear_bias", "down.0.bias", "residual.conv.bias")


# ---- the joint shift --------------------------------------------------------------------------------------------------------------------
def _run_joint(ref, direction):
    from fusion_gcn_amd import fops
    x = guarded.put(ref["x"].float(), device=DEV).requires_grad_(True)
    mask = None if ref["mask"] is None else guarded.put(ref["mask"].float(), device=DEV).requires_grad_(True)
    out = fops.joint_shift(x, mask, direction)
    (out * guarded.put(ref["probe"].float(), device=DEV)).sum().backward()
    torch.cuda.synchronize()
    return out.detach(), x.grad, None if mask is None else mask.grad


def _index_select(t, direction):
    """the literal composition in float32 on the host: (B, T, V, C) -> (B, T, V, C); the 4-wide input shifts its three channels"""
    B, T, V, C = t.shape
    if C == 4:
        return torch.nn.functional.pad(_index_select(t[..., :3].contiguous(), direction), (0, 1))
    return torch.index_select(t.reshape(B * T, V * C), 1, R.shift_table(V, C, direction)).view(B, T, V, C)


@pytest.mark.parametrize("direction", (1, -1))
@pytest.mark.parametrize("case", R.JOINT_CASES, ids=R.tag_of)
def test_joint_shift_vs_reference(case, direction, guarded_allocations):
    B = case[0]
    # without a gate and with a zero gate: a permutation, bit for bit, forward and backward
    for gate in ("none", "zero"):
        ref = R.joint_case(case, direction, gate)
        out, dx, dmask = _run_joint(ref, direction)
        assert torch.equal(out.cpu(), _index_select(ref["x"].float(), direction)), gate
        assert torch.equal(dx.cpu(), _index_select(ref["probe"].float(), -direction)), gate
        if gate == "zero":
            e = rel_l2(dmask.cpu().numpy(), ref["dmask"].numpy())
            assert dmask.shape == ref["dmask"].shape and e < TOL_GRAD, e
    # with a random gate, against the reference
    ref = R.joint_case(case, direction, "random")
    assert ref["cond"] < R.COND_MAX
    out, dx, dmask = _run_joint(ref, direction)
    errs = dict(out=rel_l2(out.cpu().numpy(), ref["out"].numpy()), dx=rel_l2(dx.cpu().numpy(), ref["dx"].numpy()),
                dmask=rel_l2(dmask.cpu().numpy(), ref["dmask"].numpy()))
    print(f"{case} dir {direction:+d}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()), flush=True)
    assert errs["out"] < TOL_OUT and errs["dx"] < TOL_GRAD and errs["dmask"] < TOL_GRAD, errs
    if case[3] == 4:                                 # the pad channel stays zero
        assert not bool(out[..., 3].any()) and not bool(dx[..., 3].any())
    # every sum has one order: a second run gives the same bits
    out2, dx2, dmask2 = _run_joint(ref, direction)
    assert torch.equal(out, out2) and torch.equal(dx, dx2) and torch.equal(dmask, dmask2)
    # one NaN in the last sample: the other samples keep their bits, the sample is NaN where the definition makes it NaN
    bad = R.joint_case(case, direction, "random", nan=True)
    out_n, dx_n, dmask_n = _run_joint(bad, direction)
    assert torch.equal(out_n[:B - 1], out[:B - 1]) and torch.equal(dx_n, dx)
    assert torch.equal(torch.isnan(out_n).cpu(), torch.isnan(bad["out"])) and int(torch.isnan(bad["out"]).sum()) == 1
    assert torch.equal(torch.isnan(dmask_n).cpu(), torch.isnan(bad["dmask"])) and int(torch.isnan(bad["dmask"]).sum()) == 1
    guarded_allocations.check()


def test_the_chunk_case_walks_three_chunks_with_a_ragged_last_one():
    """CHUNK_CASE, compared with the reference in test_joint_shift_vs_reference: three workgroup chunks with a short last one, and a full
    chunk is three LDS stages with a short last one (the host geometry query)"""
    from fusion_gcn_amd import ops
    B, T, V, C = R.CHUNK_CASE
    chunks, rows, stage = ops.shift_geometry("joint", B, T, V, C)
    assert chunks >= 3 and 0 < B * T - (chunks - 1) * rows < rows and -(-rows // stage) >= 3 and rows % stage != 0, (chunks, rows, stage)
    for case in R.FRAME_SPLIT_CASES:
        splits, fps, _ = ops.shift_geometry("frame", *case)
        assert splits >= 3 and 0 < R.out_frames(case[1], case[4]) - (splits - 1) * fps < fps, (case, splits, fps)


# ---- the frame shift --------------------------------------------------------------------------------------------------------------------
def _run_frame(ref, stride, relu, stats):
    from fusion_gcn_amd import fops
    x = guarded.put(ref["x"].float(), device=DEV).requires_grad_(True)
    pos = guarded.put(ref["pos"].float(), device=DEV).requires_grad_(True)
    res = fops.frame_shift(x, pos, stride, relu=relu, stats=stats)
    out, part = res if stats else (res, None)
    (out * guarded.put(ref["probe"].float(), device=DEV)).sum().backward()
    torch.cuda.synchronize()
    return out.detach(), x.grad, pos.grad, part


@pytest.mark.parametrize("relu", (False, True), ids=("plain", "relu"))
@pytest.mark.parametrize("case", R.FRAME_CASES, ids=R.tag_of)
def test_frame_shift_vs_reference(case, relu, guarded_allocations):
    from fusion_gcn_amd import ops
    B, T, V, C, s = case
    ref = R.frame_case(case, relu)
    assert ref["cond"] < R.COND_MAX
    out, dx, dpos, _ = _run_frame(ref, s, relu, False)
    errs = dict(out=rel_l2(out.cpu().numpy(), ref["out"].numpy()), dx=rel_l2(dx.cpu().numpy(), ref["dx"].numpy()),
                dpos=rel_l2(dpos.cpu().numpy(), ref["dpos"].numpy()))
    assert out.shape == ref["out"].shape
    assert errs["out"] < TOL_OUT and errs["dx"] < TOL_GRAD and errs["dpos"] < TOL_GRAD, errs
    assert not bool(out[..., 14:16].any()) and not bool(dpos[14:16].any())                 # +-1e9: all-zero output, zero dpos
    # with the partial sums: the same bits, and the sums finalise to the mean and the variance of out
    out_s, dx_s, dpos_s, part = _run_frame(ref, s, relu, True)
    assert torch.equal(out_s, out) and torch.equal(dx_s, dx) and torch.equal(dpos_s, dpos)
    assert part.shape == (B * ops.shift_geometry("frame", *case)[0], 2, C)
    ones, zeros = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    vec = ops.bn_finalize(part, out.numel() // C, ones, zeros, eps=1e-5)
    mean, var = vec[0].double().cpu(), (1.0 / vec[1].double().cpu() ** 2 - 1e-5)
    errs.update(mean=rel_l2(mean.numpy(), ref["mean"].numpy()), var=rel_l2(var.numpy(), ref["var"].numpy()))
    print(f"{case} relu {relu}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()), flush=True)
    assert errs["mean"] < TOL_STAT and errs["var"] < TOL_STAT, errs
    # a second run gives the same bits
    out2, dx2, dpos2, part2 = _run_frame(ref, s, relu, True)
    assert torch.equal(out, out2) and torch.equal(dx, dx2) and torch.equal(dpos, dpos2) and torch.equal(part, part2)
    # one NaN in the last sample of x: the other samples keep their bits
    bad = R.frame_case(case, relu, "x")
    out_n, dx_n, dpos_n, _ = _run_frame(bad, s, relu, False)
    assert torch.equal(out_n[:B - 1], out[:B - 1]) and torch.equal(dx_n[:B - 1], dx[:B - 1])
    assert torch.equal(torch.isnan(out_n).cpu(), torch.isnan(bad["out"])) and torch.equal(torch.isnan(dx_n).cpu(), torch.isnan(bad["dx"]))
    assert torch.equal(torch.isnan(dpos_n).cpu(), torch.isnan(bad["dpos"]))
    # a NaN position makes its channel NaN and no other
    bad = R.frame_case(case, relu, "pos")
    out_p, dx_p, dpos_p, _ = _run_frame(bad, s, relu, False)
    keep = [c for c in range(C) if c != 17]
    assert bool(torch.isnan(out_p[..., 17]).all()) and torch.equal(out_p[..., keep], out[..., keep]) and torch.equal(dx_p[..., keep], dx[..., keep])
    assert torch.equal(dpos_p[keep], dpos[keep])
    guarded_allocations.check()


def test_shift_wrappers_refuse_what_the_kernels_do_not_take(guarded_allocations):
    from fusion_gcn_amd import _lib, fops
    z = lambda *s: torch.zeros(s, device=DEV)  # noqa: E731
    with pytest.raises(_lib.FgcnError, match="V=65 joints"):
        fops.joint_shift(z(2, 4, 65, 64))
    with pytest.raises(_lib.FgcnError, match="C=96 channels"):
        fops.joint_shift(z(2, 4, 25, 96))
    with pytest.raises(_lib.FgcnError, match="V=65 joints"):
        fops.frame_shift(z(2, 4, 65, 64), z(64))
    with pytest.raises(_lib.FgcnError, match="C=96 channels"):
        fops.frame_shift(z(2, 4, 25, 96), z(96))
    with pytest.raises(_lib.FgcnError, match="C=4 channels"):
        fops.frame_shift(z(2, 4, 25, 4), z(4))
    with pytest.raises(_lib.FgcnError, match="stride=3"):
        fops.frame_shift(z(2, 4, 25, 64), z(64), stride=3)
    with pytest.raises(_lib.FgcnError, match="direction=0"):
        fops.joint_shift(z(2, 4, 25, 64), None, 0)
    with pytest.raises(_lib.FgcnError, match="not a \\(V, C\\)"):
        fops.joint_shift(z(2, 4, 25, 64), z(25, 32))


# ---- unit and block level ---------------------------------------------------------------------------------------------------------------
def _cl(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _product(kind, case, state):
    from fusion_gcn_amd.models.shiftgcn.shiftgcn import Shift_gcn, Shift_tcn, TCN_GCN_unit
    if kind == "gcn":
        mod = Shift_gcn(case.cin, case.cout, case.V)
    elif kind == "tcn":
        mod = Shift_tcn(case.cout, case.cout, stride=case.stride)
    else:
        mod = TCN_GCN_unit(case.cin, case.cout, case.V, stride=case.stride, residual=case.cin != 3)
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


def _module_fails(mod, out, dx, ref, train, tol_out=TOL_OUT, tol_grad=TOL_GRAD):
    fails, errs = [], {}
    cin = ref["dx"].shape[1]
    errs["out"] = rel_l2(out.cpu().numpy(), _cl(ref["out"]).numpy())
    if not errs["out"] < tol_out:
        fails.append(f"forward {errs['out']:.3e} >= {tol_out:g}")
    errs["dx"] = rel_l2(dx[..., :cin].cpu().numpy(), _cl(ref["dx"]).numpy())
    if not errs["dx"] < tol_grad:
        fails.append(f"dx {errs['dx']:.3e} >= {tol_grad:g}")
    if dx.shape[-1] != cin and bool(dx[..., cin:].any()):
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
    fails, errs, worst = _module_fails(mod, out, dx, ref, train)
    print(f"[{fgcn_math} {phase} {kind} {case.name}] salt {ref['salt']} fwd {errs['out']:.2e} dx {errs['dx']:.2e} worst {worst[1]:.2e} ({worst[0]})", flush=True)
    assert not fails, "\n".join(fails)
    guarded_allocations.check()


@pytest.mark.parametrize("fgcn_math", ["bf16"], indirect=True)
def test_block_in_bf16(fgcn_math, guarded_allocations):
    """math mode bf16 at that mode's contract: 1e-2 forward, cosine >= 0.98 per gradient; the shift kernels' tensors stay float32"""
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
    model = import_model("shiftgcn")({"skeleton": R.MODEL_SHAPE}, R.MODEL_CLASSES, Graph(ntu.skeleton_edges, center_joint=ntu.center_joint))
    if state is not None:
        model.load_state_dict({k: (v.float() if v.is_floating_point() else v) for k, v in state.items()})
    return model


@pytest.mark.parametrize("fgcn_math", F32_MODES, indirect=True)
def test_model_vs_reference(fgcn_math, guarded_allocations, monkeypatch):
    """Logits at 2e-5 against the float64 reference; the loss's gradient for EVERY parameter separately at 2e-4 against the float64
    reference taking the ReLU decisions this run took (shiftgcn_ref.model_forced).  The model takes over three million decisions, so a
    few of them differ from the reference's own in float32; those must be at most FLIP_CAP of all, each at a pre-activation of the
    reference within ten times KINK_EPS of zero (rounding, not an error).  The biases in front of a train-mode BatchNorm are compared
    absolutely.  The decisions are read where the product takes them: the fused BatchNorm + ReLU passes and the second frame shift's
    ReLU on its input."""
    from fusion_gcn_amd import ops
    ref = R.model_ref()
    model = _model(ref["state"]).to(DEV).train()
    masks, bn_act, frame_fwd = [], ops.bn_act, ops.frame_shift_forward

    def bn_act_recording(*args, **kw):
        res = bn_act(*args, **kw)
        if kw.get("relu"):
            masks.append((res[0] if isinstance(res, tuple) else res).detach() > 0)
        return res

    def frame_recording(x, pos, stride=1, relu=False, stats=False):
        if relu:
            masks.append(x.detach() > 0)
        return frame_fwd(x, pos, stride, relu, stats)
    monkeypatch.setattr(ops, "bn_act", bn_act_recording)
    monkeypatch.setattr(ops, "frame_shift_forward", frame_recording)
    logits = model(guarded.put(ref["x"].float(), device=DEV))
    monkeypatch.setattr(ops, "bn_act", bn_act)
    monkeypatch.setattr(ops, "frame_shift_forward", frame_fwd)
    torch.nn.functional.cross_entropy(logits, ref["labels"].to(DEV)).backward()
    torch.cuda.synchronize()
    assert len(masks) == 30, len(masks)
    shaped = [m.view(want.shape[0], want.shape[2], want.shape[3], want.shape[1]) for m, want in zip(masks, ref["masks"])]      # (the graph unit's are (B T, V C) views)
    e_logits = rel_l2(logits.detach().cpu().numpy(), ref["out"].numpy())
    forced = R.model_forced([_nchw(m).cpu() for m in shaped])
    assert forced["flips"] <= R.FLIP_CAP * forced["decisions"] and forced["close"] < 10 * R.KINK_EPS, (forced["flips"], forced["close"])
    assert rel_l2(forced["out"].numpy(), ref["out"].numpy()) < 1e-6
    scale = max(float(g.abs().max()) for g in forced["grads"].values())
    fails, errs = [], {}
    for k, p in model.named_parameters():
        want = forced["grads"][k]
        assert p.grad is not None and p.grad.shape == want.shape, k
        if k.endswith(ZERO_GRAD):
            assert float(want.abs().max()) <= 1e-9 * scale, k
            if not float(p.grad.abs().max()) <= TOL_ZERO * scale:
                fails.append(f"{k}: |gradient| {float(p.grad.abs().max()):.3e} of a zero gradient")
            continue
        errs[k] = rel_l2(p.grad.cpu().numpy(), want.numpy())
        if not errs[k] < TOL_GRAD:
            fails.append(f"{k} {errs[k]:.3e} >= {TOL_GRAD:g}")
    top = sorted(errs.items(), key=lambda t: -t[1])[:5]
    print(f"[{fgcn_math} model] logits {e_logits:.2e}; {forced['flips']} of {forced['decisions']} ReLU decisions differ from the reference's own, the "
          f"farthest at |pre-activation| {forced['close']:.1e}; worst gradients: " + ", ".join(f"{k} {e:.2e}" for k, e in top), flush=True)
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
    moved = [k for k, v in graph.state_dict().items() if k.endswith(("ypos", "Feature_Mask")) and not torch.equal(v.cpu(), base.state_dict()[k])]
    assert len(moved) == 30, moved                       # the recording trains every frame position and every joint gate
    assert_same_training(graph, eager, keep_g, keep_e, tol=0.0)
