"""The STC attention module (MS-AAGCN) on the MI355X against its float64 restatement (tests/stc_ref.py): the differentiable op
``fops.stc_attention``, an AGCN block with ``attention=True`` in every float32-class math mode (train and eval-with-autograd, the
inference route, one bf16 case) and a four-layer model, eager and through one GraphStep recording.

Tolerances are the project's: 2e-5 relative L2 on a forward result, 2e-4 on dx / dG and on every parameter gradient separately with no
ReLU decision flipped (test_block_routes_gpu.tolerances; the block's backward runs with the oracle's decisions injected, and the one
decision inside the module is kept away from rounding by the cases' filler salts -- stc_ref.PRE_MIN, asserted of the reference; a block
case's salt also keeps the two scalar bias gradients of the reference from being the residue of a cancelled sum, stc_ref.block_salt says
why).  Every run is made on guarded allocations (tests/guarded.py)."""
import copy
import types

import numpy as np
import pytest
import torch

import block_routes as R
import guarded
from guarded import guarded_allocations  # noqa: F401  (the fixture)
import stc_ref
from conftest import rel_l2
from oracle import filler
from oracle import relu_masks as RM

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F32_MODES = ("f32", "bf16x3", "f16x2")
TOL_OUT, TOL_GRAD = 2e-5, 2e-4
SIX = ("fuse_g", "bn_sums_in_dgrad", "g_bf16", "u_bf16", "dg_bf16", "dx_bf16")


# ---- op level ---------------------------------------------------------------------------------------------------------------------------
def _gate_modules(case):
    B, T, V, C = case["g"].shape
    k = stc_ref.sa_kernel(V)
    mods = (torch.nn.Conv1d(C, 1, k, padding=(k - 1) // 2), torch.nn.Conv1d(C, 1, 9, padding=4), torch.nn.Linear(C, C // 2), torch.nn.Linear(C // 2, C))
    params = [p for m in mods for p in (m.weight, m.bias)]
    with torch.no_grad():
        for p, v in zip(params, case["params"]):
            assert p.shape == v.shape
            p.copy_(v)
    return [m.to(DEV) for m in mods]


def _run_op(case, mods):
    from fusion_gcn_amd import fops
    params = [p for m in mods for p in (m.weight, m.bias)]
    for p in params:
        p.grad = None
    g = guarded.put(case["g"].float(), device=DEV).requires_grad_(True)
    probe = guarded.put(case["probe"].float(), device=DEV)
    out = fops.stc_attention(g, *mods)
    (out * probe).sum().backward()
    torch.cuda.synchronize()
    return out.detach(), g.grad.detach(), [p.grad.detach().clone() for p in params]


@pytest.mark.parametrize("shape", stc_ref.OP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stc_attention_vs_reference(shape, guarded_allocations):
    case = stc_ref.op_case(shape)
    assert case["least_pre"] > stc_ref.PRE_MIN
    mods = _gate_modules(case)
    out, dg, grads = _run_op(case, mods)
    errs = {"out": rel_l2(out.cpu().numpy(), case["out"].numpy()), "dG": rel_l2(dg.cpu().numpy(), case["dg"].numpy())}
    for k, got, want in zip(stc_ref.STC_KEYS, grads, case["grads"]):
        assert got.shape == want.shape, k
        errs[k] = rel_l2(got.cpu().numpy(), want.numpy())
    print(f"{shape}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()), flush=True)
    assert errs["out"] < TOL_OUT, errs
    assert all(v < TOL_GRAD for k, v in errs.items() if k != "out"), errs
    # every sum has one order: a second run gives the same bits
    out2, dg2, grads2 = _run_op(case, mods)
    assert torch.equal(out, out2) and torch.equal(dg, dg2) and all(torch.equal(a, b) for a, b in zip(grads, grads2))
    # one NaN in sample 1: the other samples keep their bits, sample 1 is NaN where the definition makes it NaN
    bad = stc_ref.op_case(shape, nan=True)
    out_n, dg_n, grads_n = _run_op(bad, mods)
    others = [b for b in range(shape[0]) if b != 1]
    assert torch.equal(out_n[others], out[others]) and torch.equal(dg_n[others], dg[others])
    assert torch.equal(torch.isnan(out_n[1]).cpu(), torch.isnan(bad["out"][1])) and bool(torch.isnan(bad["out"][1]).any())
    assert torch.equal(torch.isnan(dg_n[1]).cpu(), torch.isnan(bad["dg"][1]))
    for k, got, want in zip(stc_ref.STC_KEYS, grads_n, bad["grads"]):
        assert torch.equal(torch.isnan(got).cpu(), torch.isnan(want)), k
    guarded_allocations.check()


def test_stc_wrappers_refuse_what_the_kernels_do_not_take(guarded_allocations):
    from fusion_gcn_amd import _lib, ops
    case = stc_ref.op_case(stc_ref.OP_SHAPES[0])
    params = [p.float().to(DEV) for p in case["params"]]
    with pytest.raises(_lib.FgcnError, match="multiple of 64"):
        ops.stc_mean_t(torch.zeros((2, 4, 25, 32), device=DEV))
    with pytest.raises(_lib.FgcnError, match="bad B/T/V"):
        ops.stc_mean_t(torch.zeros((2, 4, 65, 64), device=DEV))
    with pytest.raises(_lib.FgcnError, match="conv_sa.weight"):
        ops.stc_forward(torch.zeros((2, 4, 24, 64), device=DEV), params)       # 24 joints: a 23-tap spatial gate, not this 25-tap one


# ---- block level ------------------------------------------------------------------------------------------------------------------------
class AttRun(R.BlockRun):
    """block_routes.BlockRun over an attention block and its composed oracle"""

    def __init__(self, case, device):
        self.case, self.device, self.margin = case, device, guarded.MARGIN
        self.blk = stc_ref.make_block(case, stc_ref.block_salt(case)).to(device)
        self.buffers0 = {k: v.detach().clone() for k, v in self.blk.named_buffers()}
        ora = stc_ref.block_oracle(case, "train")
        xc = ora["x"].float().permute(0, 2, 3, 1)
        pad = self.blk.cfg.cx - case.cin
        self.x_host = (torch.nn.functional.pad(xc, (0, pad)) if pad else xc).contiguous()
        self.probe_host = ora["probe"].float().permute(0, 2, 3, 1).contiguous()


def _entry(case, mode, spec: str = ""):
    from fusion_gcn_amd.paths import PathOptions
    return R.Entry(case, False, "default", PathOptions().update_from(spec) if spec else PathOptions(), types.SimpleNamespace(mode=mode), None)


def _check_plan(res, mode, train):
    assert len(res["plans"]) == 1
    pl = res["plans"][0]
    assert (pl.mode, pl.train) == (mode, train)
    assert not any(getattr(pl, f) for f in SIX), pl


@pytest.mark.parametrize("fgcn_math", F32_MODES, indirect=True)
@pytest.mark.parametrize("phase", R.PHASES)
@pytest.mark.parametrize("case", stc_ref.BLOCK_CASES, ids=[c.name for c in stc_ref.BLOCK_CASES])
def test_attention_block_vs_oracle(fgcn_math, phase, case):
    from test_block_routes_gpu import tolerances
    tol_out, tol_c, tol_rs, tol_grad = tolerances(False, 0)
    assert (tol_out, tol_grad) == (TOL_OUT, TOL_GRAD)
    ora = stc_ref.block_oracle(case, phase)
    run = AttRun(case, DEV)
    res = run.run(_entry(case, fgcn_math), phase, inject=ora["images"])          # the backward gates on the oracle's ReLU decisions
    _check_plan(res, fgcn_math, phase == "train")
    fails = []
    fwd = rel_l2(res["out"].cpu().numpy(), ora["out"].numpy())
    if not fwd < tol_out:
        fails.append(f"forward {fwd:.3e} >= {tol_out:g}")
    if ora["adj_c"] is not None:
        c_err = rel_l2(res["adj_c"].cpu().numpy(), ora["adj_c"].numpy())
        if not c_err < tol_c:
            fails.append(f"adj_c {c_err:.3e} >= {tol_c:g}")
    for k, v in run.buffers0.items():
        got = res["buffers"][k]
        if phase == "eval" or k.endswith("adj_a"):
            if not torch.equal(got, v):
                fails.append(f"buffer {k} changed")
        elif not k.endswith("num_batches_tracked"):
            err = rel_l2(got.cpu().numpy(), ora["stats"][k].numpy())
            if not err < tol_rs:
                fails.append(f"{k} {err:.3e} >= {tol_rs:g}")
    assert set(res["grads"]) >= {"gcn1." + k for k in stc_ref.STC_KEYS}
    worst = R.compare_grads(res, ora, tol_grad, fails, "injected")
    print(f"[{fgcn_math} {phase} {case.name}] fwd {fwd:.2e} worst {worst[1]:.2e} ({worst[0]}) flips {R.flips_of(res['signs'], ora)}", flush=True)
    if phase == "eval":
        # eval() + no_grad(): the inference route (BatchNorm + shortcut + ReLU in the kernels' epilogues where the forms exist), gated too
        from fusion_gcn_amd import ops
        run.blk.eval()
        with guarded.Guard() as g, ops.context(fgcn_math), torch.no_grad():
            out = run.blk(guarded.put(run.x_host, device=DEV))
            torch.cuda.synchronize()
            g.check()
        inf = rel_l2(out.float().permute(0, 3, 1, 2).cpu().numpy(), ora["out"].numpy())
        print(f"    inference route {inf:.2e}", flush=True)
        if not inf < tol_out:
            fails.append(f"inference forward {inf:.3e} >= {tol_out:g}")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("fgcn_math", ["bf16"], indirect=True)
def test_attention_block_in_bf16(fgcn_math):
    """math mode bf16 at that mode's contract (1e-2 forward, cosine >= 0.98 per gradient); G, G', dU and dG stay float32"""
    from test_block_routes_gpu import tolerances
    case = stc_ref.BLOCK_CASES[0]
    ora = stc_ref.block_oracle(case, "train")
    res = AttRun(case, DEV).run(_entry(case, "bf16"), "train")
    _check_plan(res, "bf16", True)
    fwd = rel_l2(res["out"].cpu().numpy(), ora["out"].numpy())
    fails = []
    worst = R.compare_grads_bf16(res, ora, fails, "bf16")
    print(f"[bf16 train {case.name}] fwd {fwd:.2e} worst cosine {worst[1]:.4f} ({worst[0]})", flush=True)
    assert fwd < tolerances(True, 0)[0] and tolerances(True, 0)[3] == 0.98
    assert not fails, "\n".join(fails)


# ---- model level ------------------------------------------------------------------------------------------------------------------------
SHAPE, CLASSES, LAYERS, CLIPS = (1, 16, 20, 3), 27, 4, 2


def _model(salt: int = 0):
    from fusion_gcn_amd.datasets.utd_mhad import constants as utd
    from fusion_gcn_amd.models.mmargcn.agcn import Model
    from fusion_gcn_amd.util import Graph
    model = Model(SHAPE, CLASSES, Graph(utd.skeleton_edges, center_joint=utd.center_joint), num_layers=LAYERS, attention=True)
    filler.fill_state_dict(model.state_dict(), salt=salt)
    return model


_oracle_cache = {}


def _model_oracle():
    if _oracle_cache:
        return _oracle_cache
    x = torch.from_numpy(filler.skeleton_input("x.stc.model", (CLIPS,) + SHAPE))
    labels = torch.from_numpy(filler.uniform("y.stc.model", (CLIPS,), 0, CLASSES).astype(np.int64))
    for salt in range(64):
        model = _model(salt)
        sd = {k: (v.detach().double() if v.is_floating_point() else v.detach().clone()) for k, v in model.state_dict().items()}
        params = {k: sd[k].clone().requires_grad_(True) for k, _ in model.named_parameters()}
        live = dict(sd)
        live.update(params)
        cap, pre = {}, {}
        logits = stc_ref.model_forward(x, live, LAYERS, train=True, stats=stc_ref.O.Stats(), capture=cap, pre=pre)
        if stc_ref.least_pre(pre) > stc_ref.PRE_MIN:
            break
    else:
        raise AssertionError("no salt below 64 keeps the model's pre-activations away from zero")
    loss = torch.nn.functional.cross_entropy(logits, labels)
    grads = torch.autograd.grad(loss, list(params.values()))
    _oracle_cache.update(x=x, labels=labels, salt=salt, least_pre=stc_ref.least_pre(pre),
                         oracle=dict(logits=logits.detach(), loss=float(loss.detach()), flat=torch.cat([g.flatten() for g in grads]),
                                     images=RM.oracle_sign_images(cap, LAYERS)))
    return _oracle_cache


@pytest.mark.parametrize("fgcn_math", F32_MODES, indirect=True)
def test_attention_model_vs_oracle(fgcn_math, guarded_allocations):
    ref = _model_oracle()
    assert ref["least_pre"] > stc_ref.PRE_MIN
    model = _model(ref["salt"]).to(DEV).train()
    assert sum(1 for k in model.state_dict() if ".conv_sa." in k) == 2 * LAYERS
    rep = RM.gradient_parity_report(model, guarded.put(ref["x"].float(), device=DEV), ref["labels"].to(DEV), oracle=ref["oracle"])
    print(f"[{fgcn_math} model] logits {rep['logits_err']:.2e} flips {rep['flips']} of {rep['decisions']} grad {rep['err_plain']:.2e} / "
          f"{rep['err_injected']:.2e}", flush=True)
    assert rep["logits_err"] < TOL_OUT, rep
    assert rep["err_injected"] < TOL_GRAD, rep
    guarded_allocations.check()


def test_attention_model_graph_step_is_the_eager_step():
    """one GraphStep recording of the attention model replays the eager training bit for bit: losses, predictions, every parameter and buffer"""
    from fusion_gcn_amd.session.procedures import DefaultBatchProcessor, DefaultStep, GraphStep
    from test_session_gpu import assert_same_training, batches, train
    data = batches([CLIPS] * 3, SHAPE, CLASSES)
    base = _model()
    with torch.no_grad():                # every gate parameter takes part (the zero-initialised ones are filled by the filler already)
        assert all(float(p.abs().max()) > 0 for n, p in base.named_parameters() if ".conv_ta." in n or ".fc2c." in n)
    step = GraphStep()
    eager, keep_e = train(copy.deepcopy(base), DefaultBatchProcessor(DefaultStep()), data)
    graph, keep_g = train(copy.deepcopy(base), DefaultBatchProcessor(step), data)
    assert len(step._recorded) == 1 and step.replays == 3
    moved = [k for k, v in graph.state_dict().items() if ".conv_sa." in k and not torch.equal(v.cpu(), base.state_dict()[k])]
    assert len(moved) == 2 * LAYERS, moved                       # the recording trains the gate parameters
    assert_same_training(graph, eager, keep_g, keep_e, tol=0.0)
