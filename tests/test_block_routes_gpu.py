"""Every kernel route of one AGCN block, train and eval-with-autograd, executed on the MI355X and compared per parameter with the float64 oracle.

tests/block_routes.py holds the matrix (one option set per distinct routes.BlockPlan of every case; tests/test_block_routes.py proves on the host
that it leaves no route out).  Per entry, here:

  * NaN is written into the allocator's free memory before the forward and again between forward and backward (block_routes.poison), so a
    ``torch.empty`` buffer that a route reads before it writes gives NaN instead of a lucky zero;
  * the plan the block really used (block.plan_block, wrapped) must EQUAL the plan the matrix predicted: a silent fall-back is a failure;
  * forward: output, adj_c and (train) the BatchNorm running statistics at the tolerances of test_block_forward_backward_vs_oracle
    (2e-5 / 1e-5 / 1e-5; math mode bf16: 1e-2, the contract of tests/test_bf16_gpu.py);
  * backward with the ORACLE's ReLU decisions written into the sign images (oracle/relu_masks.py): dx and every parameter gradient separately
    <= 2e-4 (rel-L2), the project's no-flip tolerance, in f32 / bf16x3 / f16x2; the backward as is: 2e-4 without a flipped decision, 5e-3 with;
    bf16: cosine >= 0.98 per parameter and for dx, all finite;
  * train: the analytically-zero bias gradients <= 1e-4 x the largest reference gradient entry.  eval: the conv biases in front of a BatchNorm
    have real gradients (|d tcn1.conv.bias| ~ 1e2 in the oracle) and are compared like every other parameter; only theta's bias, which the
    softmax cancels in both phases, stays on the absolute check (block_routes.oracle_case asserts that of the oracle's own value); running
    statistics and batch counters are bit-unchanged;
  * f32 / bf16x3 / f16x2: a second poisoned forward + backward is bit-identical in output, dx and every gradient.

Every run is made on guarded allocations (tests/guarded.py: NaN in front of and behind every tensor the host layer creates and the inputs x and probe,
the margins verified after the backward), so each entry also carries the check that no route stores outside its tensors or lets a load past an
extent reach a result; ``test_the_guard_changes_no_bit`` fixes that the guard only moves tensors.

All failures of a case's entries are collected and raised once.  One model-level leg runs the pooled last block and the block-to-block hand-off
under non-default option sets, under the same guard."""
import functools
import math

import numpy as np
import pytest
import torch

import block_routes as R
import guarded
from oracle import filler
from oracle import relu_masks as RM

pytestmark = pytest.mark.gpu
ALL_MODES = list(R.ALL_MODES)
INJECTED_TOL = 2e-4         # the project's no-flip tolerance (tests/test_block_model_gpu.py); no entry needed more


def dev():
    return torch.device("cuda:0")


def tolerances(bf16: bool, flips: int) -> tuple:
    """What an entry is held to (the module docstring): (output, adj_c, running statistics, the un-injected backward's dx and parameter
    gradients) -- relative L2, except the last in math mode bf16: the least cosine.  tests/test_nonfinite_gpu.py holds the finite part of a
    poisoned run of the same entry to these."""
    if bf16:
        return 1e-2, 1e-2, 1e-2, 0.98
    return 2e-5, 1e-5, 1e-5, (2e-4 if flips == 0 else 5e-3)


def _check_entry(run: R.BlockRun, e: R.Entry, phase: str, ora: dict, fails: list) -> str:
    mode, bf16 = e.plan.mode, e.plan.mode == "bf16"
    tag = f"[{mode} {phase} {e.case.name}{' bf16-in' if e.half else ''} | {e.option_name}]"
    print(f"{tag} {dict(zip(R.ROUTE_TUPLE, R.route_tuple(e.plan)))}", flush=True)      # before the kernels start
    n0 = len(fails)
    a = run.run(e, phase)
    if a["plans"] != [e.plan]:
        fails.append(f"{tag}: the block planned {a['plans']}, the matrix predicted {e.plan}")
    # ---- forward
    fwd = R.rel_l2(a["out"].cpu().numpy(), ora["out"].numpy())
    tol_out, tol_c, tol_rs, _ = tolerances(bf16, 0)
    if not fwd < tol_out:
        fails.append(f"{tag}: forward {fwd:.3e} >= {tol_out:g}")
    if a["out_dtype"] != (torch.bfloat16 if e.plan.o_bf16 else torch.float32) or a["dx_dtype"] != (torch.bfloat16 if e.half else torch.float32):
        fails.append(f"{tag}: output {a['out_dtype']} / dx {a['dx_dtype']}")
    if ora["adj_c"] is not None:
        c_err = R.rel_l2(a["adj_c"].cpu().numpy(), ora["adj_c"].numpy())
        if not c_err < tol_c:
            fails.append(f"{tag}: adj_c {c_err:.3e} >= {tol_c:g}")
    for k, v in run.buffers0.items():
        got = a["buffers"][k]
        if phase == "eval" or k.endswith("adj_a"):
            if not torch.equal(got, v):
                fails.append(f"{tag}: buffer {k} changed")
        elif k.endswith("num_batches_tracked"):
            if int(got) != int(ora["stats"][k]):
                fails.append(f"{tag}: {k} = {int(got)}")
        else:
            err = R.rel_l2(got.cpu().numpy(), ora["stats"][k].numpy())
            if not err < tol_rs:
                fails.append(f"{tag}: {k} {err:.3e} >= {tol_rs:g}")
    flips = R.flips_of(a["signs"], ora)
    # ---- backward
    if bf16:
        worst = R.compare_grads_bf16(a, ora, fails, tag)
        line = f"fwd {fwd:.2e} worst cosine {worst[1]:.4f} ({worst[0]}) flips {flips}"
    else:
        R.compare_grads(a, ora, tolerances(bf16, flips)[3], fails, tag + " as is")
        b = run.run(e, phase, inject=ora["images"])
        worst = R.compare_grads(b, ora, INJECTED_TOL, fails, tag + " injected")
        c = run.run(e, phase)           # a second run of the same entry on freshly poisoned memory: every sum has a fixed order
        same = torch.equal(a["out"], c["out"]) and torch.equal(a["dx"], c["dx"]) and all(torch.equal(g, c["grads"][k]) for k, g in a["grads"].items())
        if not same:
            fails.append(f"{tag}: the second run differs from the first in " + ", ".join(
                ["out"] * (not torch.equal(a["out"], c["out"])) + ["dx"] * (not torch.equal(a["dx"], c["dx"]))
                + [k for k, g in a["grads"].items() if not torch.equal(g, c["grads"][k])]))
        line = f"fwd {fwd:.2e} worst injected {worst[1]:.2e} ({worst[0]}) flips {flips}"
    print(f"    {line}{'' if len(fails) == n0 else '  FAILED'}", flush=True)
    return line


@pytest.mark.parametrize("fgcn_math", ALL_MODES, indirect=True)
@pytest.mark.parametrize("phase", R.PHASES)
@pytest.mark.parametrize("case", R.CASES, ids=[c.name for c in R.CASES])
def test_every_route_of_the_block_vs_oracle(fgcn_math, phase, case):
    from fusion_gcn_amd import _lib
    entries = [e for e in R.matrix(fgcn_math, phase) if e.case == case]
    assert entries
    ora = R.oracle_case(case, phase)
    run = R.BlockRun(case, dev())
    fails = []
    for e in entries:
        try:
            _check_entry(run, e, phase, ora, fails)
        except _lib.FgcnError as exc:       # the library refused a call of a planned route (an argument check, before any launch): a failure of
            fails.append(f"[{fgcn_math} {phase} {case.name} | {e.option_name}]: {exc}")      # this entry, and the next one still runs
    print(f"[{fgcn_math} {phase} {case.name}] {len(entries)} entries, {len(fails)} failures")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("fgcn_math", ["bf16x3", "bf16"], indirect=True)
def test_the_guard_changes_no_bit(fgcn_math):
    """identity64, train, default options: the run on guarded allocations and the run on the allocator's own tensors (poisoned both) give the
    same bits in the output, dx and every parameter gradient -- the guard moves tensors (512-byte aligned, as the allocator's are) and selects
    no other kernel form"""
    case = next(c for c in R.CASES if c.name == "identity64")
    entry = next(e for e in R.matrix(fgcn_math, "train") if e.case == case and e.option_name == "default" and not e.half)
    run = R.BlockRun(case, dev())
    with_guard = run.run(entry, "train")
    without = run.run(entry, "train", guard=False)
    assert with_guard["plans"] == without["plans"] == [entry.plan]
    assert torch.isfinite(with_guard["out"]).all() and with_guard["out_dtype"] == without["out_dtype"]
    assert torch.equal(with_guard["out"], without["out"])
    assert torch.equal(with_guard["dx"], without["dx"])
    assert set(with_guard["grads"]) == set(without["grads"]) and len(with_guard["grads"]) > 10
    for k, g in with_guard["grads"].items():
        assert torch.equal(g, without["grads"][k]), k
    if without["adj_c"] is not None:
        assert torch.equal(with_guard["adj_c"], without["adj_c"])


# ---- model level: the pooled last block and the block-to-block hand-off under non-default routes ----------------------------------------------
# name -> (FGCN_PATHS spec, what the ten plans of the step must show: the option set really took effect)
MODEL_SETS = {
    "default": ("", lambda P: any(p.pool_groups and p.pool_rows for p in P) and any(p.spatial_bwd == "tile" for p in P)),
    "all_unfused": (R.ALL_UNFUSED, lambda P: all("tile" not in (p.emb_fwd, p.emb_bwd, p.spatial_bwd, p.spatial_wgrad) and not p.bn_sums_in_dgrad for p in P)),
    "fuse_g=1": ("fuse_g=1", lambda P: any(p.fuse_g for p in P)),
    "spatial_bwd_tile=0+gated_shortcuts=1": ("spatial_bwd_tile=0,gated_shortcuts=1",
                                             lambda P: any(p.gate_in_dagg and p.spatial_bwd == "dagg" for p in P) and all(p.spatial_bwd != "tile" for p in P)),
    "pool_epilogue=0": ("pool_epilogue=0", lambda P: not any(p.pool_groups for p in P)),
    "pool_backward_rows=0": ("pool_backward_rows=0", lambda P: any(p.pool_groups for p in P) and not any(p.pool_rows for p in P)),
}
# (the conv's fused input stage is not built for the f16x2 products: fuse_g=1 plans nothing else there, so that leg is bf16x3's alone)
MODEL_LEGS = [(m, n) for n in MODEL_SETS for m in ("bf16x3", "f16x2") if (m, n) != ("f16x2", "fuse_g=1")]


def _ntu_model():
    from fusion_gcn_amd.datasets.ntu_rgb_d import constants as ntu
    from fusion_gcn_amd.models.mmargcn.agcn import Model
    from fusion_gcn_amd.util import Graph
    model = Model((2, 40, 25, 3), 60, Graph(ntu.skeleton_edges, center_joint=ntu.center_joint))
    filler.fill_state_dict(model.state_dict())
    with torch.no_grad():
        for m in model.modules():                       # the gains of test_model_with_and_without_the_pooling_epilogue
            if hasattr(m, "gcn1"):
                m.gcn1.bn.weight.fill_(1.0)
    return model


@functools.lru_cache(maxsize=None)
def _model_oracle():
    model = _ntu_model()
    shape = (3, 2, 40, 25, 3)
    x = torch.from_numpy(filler.skeleton_input("x.routes.model", shape, empty_second_body=True))
    labels = torch.from_numpy(filler.uniform("y.routes.model", (shape[0],), 0, 60).astype(np.int64))
    sd64 = {k: (v.detach().double() if v.is_floating_point() else v.detach().clone()) for k, v in model.state_dict().items()}
    return x, labels, sd64, RM.oracle_side(x.double(), labels, sd64, [n for n, _ in model.named_parameters()])


@pytest.mark.parametrize("fgcn_math,name", MODEL_LEGS, indirect=["fgcn_math"], ids=[f"{n}-{m}" for m, n in MODEL_LEGS])
def test_model_under_non_default_routes_vs_oracle(fgcn_math, name):
    """agcn.Model (two bodies, 40 frames, NTU graph) against the float64 oracle with the three assertions of test_two_person_model_vs_oracle;
    the plans the ten blocks really made (block.plan_block, wrapped) must show the option set's routes"""
    from fusion_gcn_amd import block, ops
    spec, took_effect = MODEL_SETS[name]
    x, labels, sd64, oracle = _model_oracle()
    model = _ntu_model().to(dev()).train()
    plans, real = [], block.plan_block

    def spy(*a, **kw):
        plans.append(real(*a, **kw))
        return plans[-1]
    block.plan_block = spy
    try:
        with ops.context(fgcn_math) as ctx, guarded.Guard() as guard:
            ctx.paths.update_from(spec)
            R.poison(dev())
            rep = RM.gradient_parity_report(model, guard.put(x.float()), labels.to(dev()), oracle=oracle)
            guard.check()
    finally:
        block.plan_block = real
    print(f"[{fgcn_math} model | {name}] logits {rep['logits_err']:.2e} flips {rep['flips']} of {rep['decisions']} grad {rep['err_plain']:.2e} / "
          f"{rep['err_injected']:.2e}")
    assert len(plans) == 20 and plans[:10] == plans[10:] and all(p.mode == fgcn_math and p.train for p in plans)      # two steps of ten blocks
    assert took_effect(plans[:10]), (name, plans[:10])
    assert rep["logits_err"] < 1e-5 and rep["loss_err"] < 1e-5, rep
    assert rep["err_injected"] < 1e-4, rep
    assert rep["err_plain"] <= 1e-4 + 2.0 * math.sqrt(rep["flips"] / (rep["decisions"] / 20)), rep
