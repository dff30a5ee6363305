"""AGCN blocks and models at channel widths beyond 64 / 128 / 256: what ``Model(..., start_feature_size=128)`` and ``=192`` run.

The planner sends blocks of 192 .. 512 channels to the same tile kernels as the headline model's, on tile geometry no narrower case reaches:
three and four 128-column tiles (a ragged 64-column third one at 320) in the halo conv and pw_gemm, 6 .. 16 k-steps of 32 channels per tap,
3 .. 5 channel groups in the spatial weight gradient, the BatchNorm-sums epilogue of the halo data gradient over three and more column tiles.

  * ``test_every_route_of_a_wide_block_vs_oracle``: block_routes.WIDE_CASES x the route matrix (``block_routes.matrix(mode, phase, WIDE_CASES)``;
    tests/test_block_routes.py proves on the host that it leaves no route combination of a wide case out), every entry held to exactly what
    tests/test_block_routes_gpu.py holds an entry of CASES to -- ``_check_entry`` is that module's: the plan used equals the plan predicted,
    forward / adj_c / running statistics, the injected, as-is and bf16-cosine backward checks, the bitwise second run, poisoned free memory.
  * ``test_wide_model_vs_oracle``: agcn.Model on the UTD graph with start_feature_size=128 (ten blocks, 128 / 256 / 512) and 192 (five blocks,
    192 / 384) against the float64 oracle built at the same ``start``: the three assertions of test_model_under_non_default_routes_vs_oracle
    in bf16x3 / f16x2, the bf16 contract of tests/test_bf16_gpu.py (logits 1e-2, loss 1e-2, gradient cosine 0.98) in bf16; the plans the blocks
    really made must hold the tile forms at cout >= 384 where the mode builds them, and the pooling epilogue on the last block.
  * ``test_wide_model_inference_vs_oracle``: the same models in eval mode under torch.no_grad() against the oracle's running-statistics
    forward, with the inference routes (tile_bn_relu, temporal_bn_relu) planned, in the modes that build them (bf16x3, bf16).

The guard's design condition, re-derived for these cases: the largest block one workgroup stores is a row tile of 128 rows over a tensor's
whole row, 128 rows x 512 channels x 4 B = 256 KiB -- all of guarded.MARGIN, not half of it.  Every run here is made under
``Guard(margin=WIDE_MARGIN)``, 512 KiB, twice that block.  (The stacked aggregate gradient of the unfused spatial backward has rows of 3 x 512
channels; a row tile of it is 768 KiB.  An overrun that starts at the tensor's end still crosses the margin first and is found; one that
starts more than 512 KiB past it is the guard's stated blind spot, here as at 256 channels.)"""
import functools
import math

import numpy as np
import pytest
import torch

import block_routes as R
import guarded
from oracle import filler
from oracle import relu_masks as RM
from test_block_routes_gpu import ALL_MODES, _check_entry, dev

pytestmark = pytest.mark.gpu
WIDE_MARGIN = 512 * 1024
assert WIDE_MARGIN >= 2 * 128 * max(c.cout for c in R.WIDE_CASES) * 4


@pytest.mark.parametrize("fgcn_math", ALL_MODES, indirect=True)
@pytest.mark.parametrize("phase", R.PHASES)
@pytest.mark.parametrize("case", R.WIDE_CASES, ids=[c.name for c in R.WIDE_CASES])
def test_every_route_of_a_wide_block_vs_oracle(fgcn_math, phase, case):
    from fusion_gcn_amd import _lib
    entries = [e for e in R.matrix(fgcn_math, phase, R.WIDE_CASES) if e.case == case]
    assert entries
    ora = R.oracle_case(case, phase)
    run = R.BlockRun(case, dev(), margin=WIDE_MARGIN)
    fails = []
    for e in entries:
        try:
            _check_entry(run, e, phase, ora, fails)
        except _lib.FgcnError as exc:       # the library refused a call of a planned route in the middle of a step: a width it does not take
            fails.append(f"[{fgcn_math} {phase} {case.name} | {e.option_name}]: {exc}")      # has to be declined by validate() or the query
    print(f"[{fgcn_math} {phase} {case.name}] {len(entries)} entries, {len(fails)} failures")
    assert not fails, "\n".join(fails)


# ---- model level ----------------------------------------------------------------------------------------------------------------------------
SHAPE, CLASSES = (2, 1, 16, 20, 3), 27
MODELS = {"start128": dict(start=128, num_layers=10), "start192x5": dict(start=192, num_layers=5)}
MODEL_MODES = ("bf16x3", "f16x2", "bf16")
MODEL_LEGS = [(m, n) for n in MODELS for m in MODEL_MODES]
# the inference leg runs in the modes that build the inference routes (f16x2 builds neither fused epilogue; its eval phase runs per block above)
INFERENCE_LEGS = [(m, n) for m, n in MODEL_LEGS if m != "f16x2"]
# Eval-mode logits (running statistics: nothing re-normalises the ten blocks, |logits| reaches 2.8e3 in start128) are worse conditioned than
# train-mode ones.  The oracle's own error on these exact inputs against its float64 run, measured on the host: in float32, and under
# torch.autocast(bfloat16) -- the reference's realisation of bf16 operands.  A leg is held to the larger of the project's bound (1e-5; bf16: 1e-2)
# and 4 x that figure: 1e-5 in bf16x3 for both models, 5.0e-2 / 2.0e-2 in bf16 (5e-2 is also what test_inference_kernels_in_bf16_mode allows ten
# blocks' bf16 roundings in eval mode)
ORACLE_EVAL_ERR = {"start128": {"f32": 1.63e-6, "bf16": 1.25e-2}, "start192x5": {"f32": 1.33e-7, "bf16": 5.03e-3}}


def _utd_model(name):
    from fusion_gcn_amd.datasets.utd_mhad import constants as utd
    from fusion_gcn_amd.models.mmargcn.agcn import Model
    from fusion_gcn_amd.util import Graph
    kw = MODELS[name]
    model = Model(SHAPE[1:], CLASSES, Graph(utd.skeleton_edges, center_joint=utd.center_joint), num_layers=kw["num_layers"],
                  start_feature_size=kw["start"])
    filler.fill_state_dict(model.state_dict())
    with torch.no_grad():
        for m in model.modules():                       # O(1) BatchNorm gains in the graph convolutions, as the other model legs set them
            if hasattr(m, "gcn1"):
                m.gcn1.bn.weight.fill_(1.0)
    return model


@functools.lru_cache(maxsize=None)
def _model_oracle(name):
    """inputs, the float64 state and the oracle's two sides (train: loss and gradients; eval: logits), computed once per model"""
    from oracle import agcn_oracle as O
    model, kw = _utd_model(name), MODELS[name]
    widths = [b["cout"] for b in O.block_plan(SHAPE[-1], kw["num_layers"], kw["start"])]
    assert widths == [blk.out_channels for blk in model.layers] and max(widths) >= 384, widths
    x = torch.from_numpy(filler.skeleton_input(f"x.wide.{name}", SHAPE))
    labels = torch.from_numpy(filler.uniform(f"y.wide.{name}", (SHAPE[0],), 0, CLASSES).astype(np.int64))
    sd64 = {k: (v.detach().double() if v.is_floating_point() else v.detach().clone()) for k, v in model.state_dict().items()}
    train = RM.oracle_side(x.double(), labels, sd64, [n for n, _ in model.named_parameters()], **kw)
    with torch.no_grad():
        eval_logits = O.model_forward(x.double(), sd64, train=False, **kw)
    return x, labels, sd64, train, eval_logits


class _PlanSpy:
    """block.plan_block wrapped: (BlockConfig, plan) of every block call"""

    def __enter__(self):
        from fusion_gcn_amd import block
        self.block, self.real, self.calls = block, block.plan_block, []

        def spy(cfg, *a, **kw):
            self.calls.append((cfg, self.real(cfg, *a, **kw)))
            return self.calls[-1][1]
        block.plan_block = spy
        return self

    def __exit__(self, *exc):
        self.block.plan_block = self.real
        return False


def _tile_queries():
    """plan field -> the availability query of its tile form (asked inside the math mode's context)"""
    from fusion_gcn_amd import ops
    return {"spatial_fwd": ops.spatial_fwd_tile_available, "spatial_bwd": ops.spatial_bwd_tile_available,
            "spatial_wgrad": ops.spatial_wgrad_tile_available}


@pytest.mark.parametrize("fgcn_math,name", MODEL_LEGS, indirect=["fgcn_math"], ids=[f"{n}-{m}" for m, n in MODEL_LEGS])
def test_wide_model_vs_oracle(fgcn_math, name):
    from fusion_gcn_amd import ops
    x, labels, sd64, oracle, _ = _model_oracle(name)
    layers = MODELS[name]["num_layers"]
    model = _utd_model(name).to(dev()).train()
    with _PlanSpy() as spy, ops.context(fgcn_math), guarded.Guard(margin=WIDE_MARGIN) as guard:
        R.poison(dev())
        rep = RM.gradient_parity_report(model, guard.put(x.float()), labels.to(dev()), oracle=oracle)
        guard.check()
        wide = [(cfg, p) for cfg, p in spy.calls[:layers] if cfg.cout >= 384]
        have = {f: any(q(SHAPE[3], cfg.cin, cfg.cout) for cfg, _ in wide) for f, q in _tile_queries().items()}
    plans = [p for _, p in spy.calls]
    print(f"[{fgcn_math} {name}] logits {rep['logits_err']:.2e} loss {rep['loss_err']:.2e} flips {rep['flips']} of {rep['decisions']} grad "
          f"{rep['err_plain']:.2e} / {rep['err_injected']:.2e} cosine {rep['cos_plain']:.5f} / {rep['cos_injected']:.5f}")
    assert len(plans) == 2 * layers and plans[:layers] == plans[layers:] and all(p.mode == fgcn_math and p.train for p in plans)
    assert wide and have["spatial_bwd"] and have["spatial_wgrad"], (fgcn_math, have)        # every split-bf16 mode builds these two
    for f, built in have.items():
        assert any(getattr(p, f) == "tile" for _, p in wide) == built, (fgcn_math, f, built, [getattr(p, f) for _, p in wide])
    assert plans[layers - 1].pool_groups == SHAPE[0] and plans[layers - 1].pool_rows and not any(p.pool_groups for p in plans[:layers - 1])
    if fgcn_math == "bf16":
        assert rep["logits_err"] < 1e-2 and rep["loss_err"] < 1e-2 and rep["cos_plain"] > 0.98, rep
        assert rep["logits_err"] > 1e-5, rep                        # the mode really changes the arithmetic
    else:
        assert rep["logits_err"] < 1e-5 and rep["loss_err"] < 1e-5, rep
        assert rep["err_injected"] < 1e-4, rep
        assert rep["err_plain"] <= 1e-4 + 2.0 * math.sqrt(rep["flips"] / (rep["decisions"] / 20)), rep


@pytest.mark.parametrize("fgcn_math,name", INFERENCE_LEGS, indirect=["fgcn_math"], ids=[f"{n}-{m}" for m, n in INFERENCE_LEGS])
def test_wide_model_inference_vs_oracle(fgcn_math, name):
    from fusion_gcn_amd import ops
    bf16 = fgcn_math == "bf16"
    bound = max(1e-2 if bf16 else 1e-5, 4 * ORACLE_EVAL_ERR[name]["bf16" if bf16 else "f32"])
    x, _, _, _, want = _model_oracle(name)
    layers = MODELS[name]["num_layers"]
    model = _utd_model(name).to(dev()).eval()
    with _PlanSpy() as spy, ops.context(fgcn_math), guarded.Guard(margin=WIDE_MARGIN) as guard, torch.no_grad():
        built = bool(ops.inference_kernels_available() and ops.paths().fused_inference)
        R.poison(dev())
        logits = model(guard.put(x.float()))
        torch.cuda.synchronize()
        guard.check()
    plans = [p for _, p in spy.calls]
    err = R.rel_l2(logits.double().cpu().numpy(), want.numpy())
    print(f"[{fgcn_math} {name}] inference logits {err:.2e}; tile_bn_relu at cout {[c.cout for c, p in spy.calls if p.spatial_fwd == 'tile_bn_relu']}, "
          f"temporal_bn_relu at cout {[c.cout for c, p in spy.calls if p.temporal_bn_relu]}")
    assert built and len(plans) == layers and all(p.mode == fgcn_math and not p.train for p in plans)
    # the two fused epilogues, up to the widest block that has the form (the temporal one: stride 1, not the pooled last block)
    took = [c.cout for c, p in spy.calls if p.spatial_fwd == "tile_bn_relu"]
    assert took and max(took) == max(c.cout for c, _ in spy.calls), (fgcn_math, took)
    took = [c.cout for c, p in spy.calls if p.temporal_bn_relu]
    assert took and max(took) == max(c.cout for c, p in spy.calls if c.stride == 1 and not p.pool_groups), (fgcn_math, took)
    assert bool(torch.isfinite(logits).all()) and err < bound, (err, bound)
