"""Parameter groups of the fused optimizer step on the device (fgcn_optim_step over several groups, plain and with a guard).

Oracles: the single-group FlatOptimizer, bit for bit (the grouped kernel runs the same per-element arithmetic with a group's scalars,
so equal groups ARE the single group and every group IS its own optimizer: no tolerance applies); torch's own optimizer objects over
the same groups on the CPU, per-group ``LambdaLR`` schedules included (2e-6 relative L2 per parameter, the figure tests/test_optim.py
holds the single group to); ``clip_grad_norm_`` over all parameters in front of them for the guarded form (the tolerances of
tests/test_optim_guard_gpu.py); and for the skip bit-equality with the buffers as they were.

Model and groups: tests/test_optim_groups.py (padding, a 1-element tensor, a tensor longer than a tile row, groups that interleave
in the model's order).  6 steps, gradients ``randn * (1 + step)`` as in tests/test_optim.py."""
import copy
import math

import pytest
import torch
import torch.nn as nn

from test_optim_groups import CASES, TORCH, group_model, three_groups

import guarded
from guarded import guarded_allocations  # noqa: F401  (the fixture)

to_device = guarded.to           # (tests here take a parameter named ``guarded``)

# every test runs on guarded allocations: NaN around each tensor the host layer creates, margins verified at teardown (tests/guarded.py)
pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_allocations")]
DEV = torch.device("cuda:0")
SCHEDULES = [lambda e: 0.9 ** e, lambda e: 1.0 / (1 + e), lambda e: 1.0 if e < 3 else 0.5]     # one per group


def _grad_steps(model, steps=6, seed=7):
    g = torch.Generator().manual_seed(seed)
    return [[torch.randn(p.shape, generator=g) * (1.0 + it) for p in model.parameters()] for it in range(steps)]


def _set_grads(params, grads):
    for p, grad in zip(params, grads):
        p.grad = grad.clone().to(p.device)


def _shared(model, overrides, kind, lr=0.05, **kw):
    """The grouped optimizer over a model-order gradient buffer (what GraphStep and dp.py share): the groups interleave."""
    from fusion_gcn_amd.dp import FlatGradients
    from fusion_gcn_amd.optim import FlatOptimizer
    opt = FlatOptimizer(three_groups(model, overrides), kind, lr, grads=FlatGradients(model.parameters()), **kw)
    assert opt._group_of == [0, 2, 1, 1, 0, 2, 1, 1, 0, 2]
    return opt


def _assert_padding_is_zero(opt):
    used = torch.zeros_like(opt.flat, dtype=torch.bool)
    for v, p in zip(opt.grads.views, opt.params):
        used[v.storage_offset():v.storage_offset() + p.numel()] = True
    assert int((~used).sum()) >= 3 + 2 + 1                     # the 1-element tensor, 4690 and 67 / 335 floats
    for buf in (opt.flat, opt.state1, opt.state2):
        if buf is not None:
            assert float(buf[~used].abs().sum()) == 0.0


def _rel(po, pr):
    return float((po.detach().cpu() - pr.detach()).norm() / pr.detach().norm())


def _bits(t):
    return int(t.view(torch.int64))


# ---- 1. equal groups are the single group ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_norm", [None, 3.0])
@pytest.mark.parametrize("kind,args,_overrides", CASES)
def test_equal_groups_are_the_single_group_bit_for_bit(kind, args, _overrides, max_norm):
    from fusion_gcn_amd.optim import FlatOptimizer
    base = group_model(3)
    ma, mb = to_device(copy.deepcopy(base), DEV), to_device(copy.deepcopy(base), DEV)
    single = FlatOptimizer(ma.parameters(), kind, 0.05, max_grad_norm=max_norm, **args)
    grouped = _shared(mb, ({}, {}, {}), kind, max_grad_norm=max_norm, **args)
    scheds = [torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(o, T_0=3) for o in (single, grouped)]
    for it, grads in enumerate(_grad_steps(base)):
        for model, opt, sched in ((ma, single, scheds[0]), (mb, grouped, scheds[1])):
            opt.zero_grad()
            _set_grads(model.parameters(), grads)
            opt.step()
            sched.step()
        assert [g["lr"] for g in grouped.param_groups] == [single.param_groups[0]["lr"]] * 3
        for a, b in ((grouped.flat, single.flat), (grouped.state1, single.state1), (grouped.state2, single.state2)):
            assert (a is None) == (b is None)
            if a is not None:
                assert torch.equal(a, b), (kind, max_norm, it, int((a != b).sum()))          # the padding included
        if max_norm is not None:
            assert _bits(grouped.grad_norm) == _bits(single.grad_norm) and _bits(grouped.clip_coef) == _bits(single.clip_coef)
    assert float((single.flat - base_flat(single, base)).abs().max()) > 0              # (the steps did move the parameters)
    _assert_padding_is_zero(grouped)
    if max_norm is not None:
        assert grouped.steps == single.steps == 6 and grouped.clipped_steps == single.clipped_steps == 6
        assert grouped.skipped_steps == single.skipped_steps == 0
    else:
        assert grouped.steps == single.steps == 6


def base_flat(opt, base):
    """The initial values of ``base`` laid out like ``opt.flat``."""
    flat = torch.zeros_like(opt.flat)
    for v, p in zip(opt.grads.views, base.parameters()):
        flat[v.storage_offset():v.storage_offset() + p.numel()] = p.detach().reshape(-1).to(flat.device)
    return flat


# ---- 2. each group is its own optimizer ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,args,overrides", CASES)
def test_each_group_is_its_own_optimizer_bit_for_bit(kind, args, overrides):
    """The check that catches a wrong group at a tile or tensor boundary: a 3-group optimizer with different lr / weight_decay /
    betas / momentum against one single-group FlatOptimizer per group, over copies of just that group's parameters."""
    from fusion_gcn_amd.optim import FlatOptimizer
    base = group_model(3)
    model = to_device(copy.deepcopy(base), DEV)
    opt = _shared(model, overrides, kind, **args)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, SCHEDULES)
    where = {id(p): i for i, p in enumerate(model.parameters())}
    m1 = dict(zip(map(id, opt.params), opt._views(opt.state1))) if opt.state1 is not None else None
    m2 = dict(zip(map(id, opt.params), opt._views(opt.state2))) if opt.state2 is not None else None
    solos = []
    for gi, group in enumerate(opt.param_groups):
        copies = [nn.Parameter(p.detach().clone()) for p in group["params"]]
        hyper = {k: v for k, v in group.items() if k not in ("params", "initial_lr")}
        solo = FlatOptimizer(copies, kind, hyper.pop("lr"), **hyper)
        solos.append((copies, solo, torch.optim.lr_scheduler.LambdaLR(solo, SCHEDULES[gi]), [where[id(p)] for p in group["params"]]))
    for it, grads in enumerate(_grad_steps(base)):
        opt.zero_grad()
        _set_grads(model.parameters(), grads)
        opt.step()
        sched.step()
        for gi, (copies, solo, solo_sched, idx) in enumerate(solos):
            solo.zero_grad()
            _set_grads(copies, [grads[i] for i in idx])
            solo.step()
            solo_sched.step()
            assert solo.param_groups[0]["lr"] == opt.param_groups[gi]["lr"]
            s1 = solo._views(solo.state1) if solo.state1 is not None else None
            s2 = solo._views(solo.state2) if solo.state2 is not None else None
            for j, (p, c) in enumerate(zip(opt.param_groups[gi]["params"], copies)):
                assert torch.equal(p, c), (kind, it, gi, j, int((p != c).sum()))
                if m1 is not None:
                    if s1 is not None:
                        assert torch.equal(m1[id(p)], s1[j]), (kind, it, gi, j)
                    else:
                        assert float(m1[id(p)].abs().sum()) == 0.0          # SGD: the group without a momentum leaves the buffer alone
                if m2 is not None:
                    assert torch.equal(m2[id(p)], s2[j]), (kind, it, gi, j)
    _assert_padding_is_zero(opt)


# ---- 3. against torch's optimizer over the same groups ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,args,overrides", CASES)
def test_grouped_update_matches_torch_optim(kind, args, overrides):
    from fusion_gcn_amd.optim import FlatOptimizer
    ref_model = group_model(3)
    model = to_device(copy.deepcopy(ref_model), DEV)
    ref = TORCH[kind](three_groups(ref_model, overrides), 0.05, **args)
    opt = FlatOptimizer(three_groups(model, overrides), kind, 0.05, **args)      # its own buffers: the concatenation of the groups
    assert opt._group_of == [0, 0, 0, 1, 1, 1, 1, 2, 2, 2]
    sched_r = torch.optim.lr_scheduler.LambdaLR(ref, SCHEDULES)
    sched_o = torch.optim.lr_scheduler.LambdaLR(opt, SCHEDULES)
    worst = 0.0
    for it, grads in enumerate(_grad_steps(ref_model)):
        ref.zero_grad()
        opt.zero_grad()
        _set_grads(ref_model.parameters(), grads)
        _set_grads(model.parameters(), grads)
        ref.step()
        opt.step()
        sched_r.step()
        sched_o.step()
        for gr, go in zip(ref.param_groups, opt.param_groups):
            assert abs(gr["lr"] - go["lr"]) < 1e-12
        for i, (pr, po) in enumerate(zip(ref_model.parameters(), model.parameters())):
            err = _rel(po, pr)
            worst = max(worst, err)
            assert err < 2e-6, (kind, args, it, i, err)
    print(f"{kind} {args} {overrides}: worst relative error {worst:.3e}")
    v0 = [p._version for p in model.parameters()]
    _set_grads(model.parameters(), [torch.zeros_like(p) for p in ref_model.parameters()])
    opt.step()
    assert all(p._version > v for p, v in zip(model.parameters(), v0))
    _assert_padding_is_zero(opt)
    # the state dict loads into the torch optimizer of the same grouping and back
    sd = opt.state_dict()
    other = TORCH[kind](three_groups(copy.deepcopy(ref_model), overrides), 0.05, **args)
    other.load_state_dict(sd)
    opt2 = FlatOptimizer(three_groups(to_device(copy.deepcopy(ref_model), DEV), overrides), kind, 0.05, **args)
    opt2.load_state_dict(ref.state_dict())
    if kind != "SGD":
        assert opt2.steps == 6 and opt.steps == 7
        for i in (0, 4, 9):
            assert torch.equal(opt2.state_dict()["state"][i]["exp_avg_sq"].cpu(), ref.state_dict()["state"][i]["exp_avg_sq"])


# ---- 4. guarded: clip_grad_norm_ over ALL parameters, then the torch optimizer of the same groups ------------------------------------------
@pytest.mark.parametrize("kind,args,overrides", CASES)
def test_clipped_grouped_update_matches_clip_grad_norm_and_torch_optim(kind, args, overrides):
    ref_model = group_model(3)
    model = to_device(copy.deepcopy(ref_model), DEV)
    steps = _grad_steps(ref_model)
    norms = [math.sqrt(sum(float(t.double().pow(2).sum()) for t in grads)) for grads in steps]
    max_norm = norms[2]
    assert sum(n > max_norm * (1 + 1e-6) for n in norms) >= 2 and sum(n < max_norm * (1 - 1e-6) for n in norms) >= 2, norms
    ref = TORCH[kind](three_groups(ref_model, overrides), 0.05, **args)
    opt = _shared(model, overrides, kind, max_grad_norm=max_norm, **args)
    sched_r = torch.optim.lr_scheduler.LambdaLR(ref, SCHEDULES)
    sched_o = torch.optim.lr_scheduler.LambdaLR(opt, SCHEDULES)
    worst = 0.0
    for it, grads in enumerate(steps):
        ref.zero_grad()
        opt.zero_grad()
        _set_grads(ref_model.parameters(), grads)
        _set_grads(model.parameters(), grads)
        torch.nn.utils.clip_grad_norm_(list(ref_model.parameters()), max_norm)
        ref.step()
        opt.step()
        sched_r.step()
        sched_o.step()
        coef = min(1.0, max_norm / (norms[it] + 1e-6))
        assert abs(float(opt.clip_coef) - coef) <= 1e-9 * coef, (it, float(opt.clip_coef), coef)
        assert abs(float(opt.grad_norm) - norms[it]) <= 1e-9 * norms[it]
        for i, (pr, po) in enumerate(zip(ref_model.parameters(), model.parameters())):
            err = _rel(po, pr)
            worst = max(worst, err)
            assert err < 2e-6, (kind, args, it, i, err)
    print(f"{kind} {args} {overrides}: worst relative error {worst:.3e}")
    assert opt.steps == 6 and opt.skipped_steps == 0
    assert opt.clipped_steps == sum(max_norm / (n + 1e-6) < 1.0 for n in norms)
    _assert_padding_is_zero(opt)


# ---- 5. a non-finite gradient in ONE group skips every group -----------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
@pytest.mark.parametrize("kind,args,overrides", CASES)
def test_nonfinite_gradient_in_one_group_skips_every_group(kind, args, overrides, bad):
    ref_model = group_model(3)
    model = to_device(copy.deepcopy(ref_model), DEV)
    ref = TORCH[kind](three_groups(ref_model, overrides), 0.05, **args)
    opt = _shared(model, overrides, kind, skip_nonfinite=True, **args)
    steps = _grad_steps(ref_model, steps=4)

    def good(grads):
        ref.zero_grad()
        opt.zero_grad()
        _set_grads(ref_model.parameters(), grads)
        _set_grads(model.parameters(), grads)
        ref.step()
        opt.step()

    good(steps[0])
    good(steps[1])
    assert opt.steps == 2 and opt.skipped_steps == 0
    poisoned = [g.clone() for g in steps[2]]
    poisoned[3].view(-1)[-1] = bad                          # 1.bias: the second group only
    assert opt._group_of[3] == 1
    before = [t.clone() if t is not None else None for t in (opt.flat, opt.state1, opt.state2)]
    opt.zero_grad()
    _set_grads(model.parameters(), poisoned)
    opt.step()
    for now, was in zip((opt.flat, opt.state1, opt.state2), before):
        assert (now is None) == (was is None)
        if now is not None:
            assert torch.equal(now, was)                    # every group, bit for bit
    assert opt.skipped_steps == 1 and opt.steps == 2 and not math.isfinite(float(opt.grad_norm))
    good(steps[3])                                          # the torch optimizer never saw the bad batch
    assert opt.steps == 3 and opt.skipped_steps == 1
    for p, v in zip(opt.params, opt._views(before[0])):
        assert not torch.equal(p, v)                        # the next finite step applies, in every group
    for i, (pr, po) in enumerate(zip(ref_model.parameters(), model.parameters())):
        assert _rel(po, pr) < 2e-6, (kind, bad, i, _rel(po, pr))


# ---- 6. step-level properties ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("guarded", [False, True])
def test_grouped_step_never_waits_for_the_device(guarded):
    model = to_device(group_model(3), DEV)
    kw = dict(max_grad_norm=1.0, skip_nonfinite=True) if guarded else {}
    opt = _shared(model, CASES[1][2], "ADAM", weight_decay=0.01, **kw)
    tiles = opt._tiles.clone()
    for p in model.parameters():
        p.grad = torch.ones_like(p)
    opt.step()                                   # (loads the library)
    torch.cuda.synchronize()
    v0 = [p._version for p in model.parameters()]
    probe = torch.ones(1, device=DEV)
    torch.cuda.set_sync_debug_mode("error")
    try:
        honoured = False
        try:
            probe.item()
        except RuntimeError:
            honoured = True
        opt.param_groups[1]["lr"] = 0.5          # a scheduler's new value: by value with the next launch
        opt.step()
        opt.step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert honoured, "this torch build does not raise on .item() under set_sync_debug_mode('error')"
    assert all(p._version >= v + 2 for p, v in zip(model.parameters(), v0))
    assert opt.steps == 3 and torch.equal(opt._tiles, tiles)
    _assert_padding_is_zero(opt)


# ---- 7. a shared model-order buffer under GraphStep -------------------------------------------------------------------------------------
def test_groups_over_a_shared_buffer_train_the_same_under_graph_step():
    """FlatOptimizer(groups, grads=FlatGradients(model.parameters())) with GraphStep recording into that buffer: three training steps
    equal the same optimizer under DefaultStep, to the agreement tests/test_session_gpu.py asserts between the two step types."""
    from fusion_gcn_amd.dp import FlatGradients
    from fusion_gcn_amd.optim import FlatOptimizer, groups_from_rules
    from fusion_gcn_amd.session.procedures import DefaultBatchProcessor, DefaultStep, GraphStep
    from fusion_gcn_amd.session.session import Session
    from test_session_gpu import agcn, assert_same_training, batches
    import torch.nn.functional as F
    shape, classes = (1, 24, 20, 3), 27
    data = batches([4, 4, 4], shape, classes)
    base = agcn(shape, classes)
    rules = [{"match": r"bn|bias$|adj_b$", "weight_decay": 0.0}, {"match": r"^fc\.", "lr": 0.02}]

    class Keep:
        def __init__(self):
            self.losses, self.preds = [], []

        def update_training(self, loss, pair, m, idx):
            self.losses.append(loss)
            self.preds.append(pair[0])

        def format_training(self):
            return ""

    def train(graph):
        model = to_device(copy.deepcopy(base), DEV).train()
        grads = FlatGradients(model.parameters())
        opt = FlatOptimizer(groups_from_rules(model, rules), "SGD", 0.01, momentum=0.9, weight_decay=1e-4, grads=grads)
        assert len(opt.param_groups) == 3 and len(set(opt._group_of[:8])) > 1           # interleaved in the model's order
        step = GraphStep(grads=grads) if graph else DefaultStep()
        keep = Keep()
        Session.train_epoch(DefaultBatchProcessor(step), model, F.cross_entropy, data, opt, None, keep)
        torch.cuda.synchronize()
        if graph:
            assert step.replays == 3 and step.grads is opt.grads
        assert opt.steps == 3
        return model, keep

    eager, keep_e = train(False)
    graph, keep_g = train(True)
    assert_same_training(graph, eager, keep_g, keep_e)
    # (biases in front of a train-mode BatchNorm have a zero gradient and, in their group, no decay: they stay)
    moved = [float((a - to_device(b, DEV)).abs().max()) > 0 for a, b in zip(eager.parameters(), base.parameters())]
    assert sum(moved) > len(moved) // 2 and moved[-2]
