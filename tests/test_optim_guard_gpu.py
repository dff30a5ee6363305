"""The guard of the fused optimizer step on the device (fgcn_optim_step with an fgcn_optim_guard, FlatOptimizer(max_grad_norm=, skip_nonfinite=)).

Oracles: the float64 norm ``g.double().pow(2).sum().sqrt()`` on the CPU; torch's own ``clip_grad_norm_`` + optimizer objects on the
CPU (tolerance 2e-6 relative, the one of tests/test_optim.py: the clip adds one float32 multiplication per element); and for the skip
bit-equality with the buffers as they were."""
import copy
import math

import pytest
import torch

from fusion_gcn_amd import _lib
from test_optim import CASES, TORCH, small_model

import guarded
from guarded import guarded_allocations  # noqa: F401  (the fixture)

# every test runs on guarded allocations: NaN around each tensor the host layer creates, margins verified at teardown (tests/guarded.py)
pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_allocations")]
DEV = torch.device("cuda:0")


# ---- 1. the norm, on raw buffers ---------------------------------------------------------------------------------------------------
def _search(lib, pred, hi):
    """The largest multiple of 4 in [4, hi] for which pred(tiles) holds (the query is monotone)."""
    lo = 4
    assert pred(lib.fgcn_grad_norm_tiles(lo)) and not pred(lib.fgcn_grad_norm_tiles(hi))
    while hi - lo > 4:
        mid = (lo + hi) // 8 * 4
        if pred(lib.fgcn_grad_norm_tiles(mid)):
            lo = mid
        else:
            hi = mid
    return lo


def _lengths(lib):
    one = _search(lib, lambda t: t == 1, 1 << 20)                      # the largest n with one partial
    cap = lib.fgcn_grad_norm_tiles(1 << 40)
    below = _search(lib, lambda t: t < cap, 1 << 26)                   # the largest n below the cap of the partial count
    many = below + 4 + 3 * one + 8                                     # past it: workgroups 0..3 take a second chunk, the last one ragged
    assert lib.fgcn_grad_norm_tiles(many) == cap and many <= 8_000_000
    return [4, one, one + 4, many]


def _raw_norm(lib, g, max_norm=1.0, grad_scale=1.0):
    """SGD with lr = 0 over a zero parameter buffer: the update changes nothing, the guard state holds norm and coefficient."""
    n = g.numel()
    p = torch.zeros(n, device=DEV)
    tiles = lib.fgcn_grad_norm_tiles(n)
    partials = torch.full((tiles + 1,), -7.0, dtype=torch.float64, device=DEV)        # one guard element behind the last partial
    guard = torch.zeros(_lib.GUARD_WORDS, dtype=torch.int64, device=DEV)
    sched = torch.zeros(2 * _lib.OPT_MAX_GROUPS, dtype=torch.float64, device=DEV)
    rows = torch.arange(0, n // 4, _lib.OPT_TILE4, dtype=torch.int32)
    table = guarded.to(torch.stack([rows, (n // 4 - rows).clamp(max=_lib.OPT_TILE4), torch.zeros_like(rows)], dim=1).contiguous(), DEV)
    group = (_lib.OptimGroup * 1)(_lib.OptimGroup(0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0))
    rc = lib.fgcn_optim_step(p.data_ptr(), g.data_ptr(), None, None, n, 0, group, 1, table.data_ptr(), table.shape[0], grad_scale, 0,
                             _lib.OptimGuard(max_norm, 1, tiles, partials.data_ptr(), guard.data_ptr(), sched.data_ptr()),
                             torch.cuda.current_stream(DEV).cuda_stream)
    _lib.check(rc, "fgcn_optim_step")
    torch.cuda.synchronize()
    assert float(partials[tiles]) == -7.0 and float(p.abs().max()) == 0.0
    return guard.cpu(), partials[:tiles].cpu()


@pytest.mark.parametrize("which", [0, 1, 2, 3])
def test_norm_against_float64(which):
    lib = _lib.load()
    n = _lengths(lib)[which]
    gen = torch.Generator().manual_seed(11 + which)
    expo = torch.randint(-18, 19, (n,), generator=gen).double()
    g_cpu = (torch.randn(n, generator=gen).double() * torch.pow(torch.tensor(10.0, dtype=torch.float64), expo)).float()
    assert bool(torch.isfinite(g_cpu).all())
    want = float(g_cpu.double().pow(2).sum().sqrt())
    g = guarded.to(g_cpu, DEV)
    guard, partials = _raw_norm(lib, g)
    got = float(guard.view(torch.float64)[_lib.GUARD_NORM])
    err = abs(got - want) / want
    print(f"n={n} tiles={partials.numel()} norm={got:.17g} oracle={want:.17g} rel_err={err:.3e}")
    assert err <= 1e-9, (n, got, want, err)
    assert abs(float(partials.sum().sqrt()) - want) / want <= 1e-9
    coef = float(guard.view(torch.float64)[_lib.GUARD_COEF])
    assert abs(coef - min(1.0, 1.0 / (want + 1e-6))) <= 1e-9 * coef
    assert int(guard[_lib.GUARD_APPLY]) == 1 and int(guard[_lib.GUARD_STEP]) == 1 and int(guard[_lib.GUARD_SKIPPED]) == 0
    # the same buffer gives the same bits
    guard2, partials2 = _raw_norm(lib, g)
    assert int(guard2[_lib.GUARD_NORM]) == int(guard[_lib.GUARD_NORM])
    assert torch.equal(partials2.view(torch.int64), partials.view(torch.int64))
    # grad_scale is part of the norm
    guard3, _ = _raw_norm(lib, g, grad_scale=0.25)
    assert abs(float(guard3.view(torch.float64)[_lib.GUARD_NORM]) - 0.25 * want) <= 1e-9 * 0.25 * want


def test_huge_finite_gradients_have_a_finite_norm_and_are_clipped():
    """1e30 per element: the squares overflow float32, the float64 norm is finite -- not a skip case."""
    lib = _lib.load()
    n = _lengths(lib)[2]
    g = torch.full((n,), 1e30, device=DEV)
    want = float(g.cpu().double().pow(2).sum().sqrt())
    assert math.isfinite(want) and not math.isfinite(float(g.cpu().pow(2).sum().sqrt()))
    guard, _ = _raw_norm(lib, g, max_norm=2.0)
    got, coef = (float(guard.view(torch.float64)[w]) for w in (_lib.GUARD_NORM, _lib.GUARD_COEF))
    print(f"n={n} norm={got:.17g} oracle={want:.17g} coef={coef:.17g}")
    assert abs(got - want) / want <= 1e-9
    assert abs(coef - 2.0 / (want + 1e-6)) <= 1e-9 * coef
    assert [int(guard[w]) for w in (_lib.GUARD_APPLY, _lib.GUARD_STEP, _lib.GUARD_SKIPPED, _lib.GUARD_CLIPPED)] == [1, 1, 0, 1]
    # through the optimizer: the clipped gradient has norm max_grad_norm, SGD moves the parameter by lr * that
    from fusion_gcn_amd.optim import FlatOptimizer
    p = torch.nn.Parameter(torch.zeros(64, device=DEV))
    opt = FlatOptimizer([p], "SGD", 1.0, max_grad_norm=2.0, skip_nonfinite=True)
    p.grad = torch.full((64,), 1e30, device=DEV)
    opt.step()
    assert opt.skipped_steps == 0 and opt.steps == 1 and opt.clipped_steps == 1
    assert abs(float(p.detach().double().norm()) - 2.0) <= 1e-6 * 2.0


# ---- 2. the clipped update against torch's own objects -----------------------------------------------------------------------------------
def _rel(po, pr):
    return float((po.detach().cpu() - pr.detach()).norm() / pr.detach().norm())


@pytest.mark.parametrize("name,args", CASES)
def test_clipped_update_matches_clip_grad_norm_and_torch_optim(name, args):
    from fusion_gcn_amd.optim import FlatOptimizer
    ref_model = small_model(3)
    model = guarded.to(copy.deepcopy(ref_model), DEV)
    g = torch.Generator().manual_seed(7)
    steps = [[torch.randn(p.shape, generator=g) * (1.0 + it) for p in ref_model.parameters()] for it in range(6)]
    norms = [math.sqrt(sum(float(t.double().pow(2).sum()) for t in grads)) for grads in steps]
    max_norm = norms[2]
    assert sum(n > max_norm * (1 + 1e-6) for n in norms) >= 2 and sum(n < max_norm * (1 - 1e-6) for n in norms) >= 2, norms
    ref = TORCH[name](ref_model.parameters(), 0.05, **args)
    opt = FlatOptimizer(model.parameters(), name, 0.05, max_grad_norm=max_norm, **args)
    sched_r = torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(ref, T_0=3)
    sched_o = torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(opt, T_0=3)
    worst = 0.0
    for it, grads in enumerate(steps):
        ref.zero_grad()
        opt.zero_grad()
        for pr, po, grad in zip(ref_model.parameters(), model.parameters(), grads):
            pr.grad = grad.clone()
            po.grad = guarded.to(grad, DEV)
        torch.nn.utils.clip_grad_norm_(list(ref_model.parameters()), max_norm)
        ref.step()
        opt.step()
        sched_r.step()
        sched_o.step()
        coef = min(1.0, max_norm / (norms[it] + 1e-6))
        assert abs(float(opt.clip_coef) - coef) <= 1e-9 * coef, (it, float(opt.clip_coef), coef)
        assert abs(float(opt.grad_norm) - norms[it]) <= 1e-9 * norms[it]
        for pr, po in zip(ref_model.parameters(), model.parameters()):
            err = _rel(po, pr)
            worst = max(worst, err)
            assert err < 2e-6, (name, args, it, err)
    print(f"{name} {args}: worst relative error {worst:.3e}")
    assert opt.steps == 6 and opt.skipped_steps == 0
    assert opt.clipped_steps == sum(max_norm / (n + 1e-6) < 1.0 for n in norms)


# ---- 3. the skip ----------------------------------------------------------------------------------------------------------------------
SKIP_CASES = [("SGD", dict(momentum=0.9, weight_decay=1e-4)), ("ADAM", dict(weight_decay=0.01)), ("ADAMW", dict())]


def _good_step(ref, opt, ref_model, model, gen, max_norm):
    ref.zero_grad()
    opt.zero_grad()
    for pr, po in zip(ref_model.parameters(), model.parameters()):
        grad = torch.randn(pr.shape, generator=gen)
        pr.grad = grad.clone()
        po.grad = guarded.to(grad, DEV)
    if max_norm is not None:
        torch.nn.utils.clip_grad_norm_(list(ref_model.parameters()), max_norm)
    ref.step()
    opt.step()


def _bad_step(opt, model, gen, bad):
    opt.zero_grad()
    params = list(model.parameters())
    for i, po in enumerate(params):
        grad = torch.randn(po.shape, generator=gen)
        if i == len(params) - 2:
            grad.view(-1)[-1] = bad
        po.grad = guarded.to(grad, DEV)
    before = [t.clone() if t is not None else None for t in (opt.flat, opt.state1, opt.state2)]
    opt.step()
    for now, was in zip((opt.flat, opt.state1, opt.state2), before):
        assert (now is None) == (was is None)
        if now is not None:
            assert torch.equal(now, was)


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
@pytest.mark.parametrize("max_norm", [None, 3.0])
@pytest.mark.parametrize("name,args", SKIP_CASES)
def test_nonfinite_step_is_skipped_bit_for_bit(name, args, max_norm, bad):
    from fusion_gcn_amd.optim import FlatOptimizer
    ref_model = small_model(3)
    model = guarded.to(copy.deepcopy(ref_model), DEV)
    ref = TORCH[name](ref_model.parameters(), 0.05, **args)
    opt = FlatOptimizer(model.parameters(), name, 0.05, max_grad_norm=max_norm, skip_nonfinite=True, **args)
    gen, gen_bad = torch.Generator().manual_seed(7), torch.Generator().manual_seed(8)
    for _ in range(2):
        _good_step(ref, opt, ref_model, model, gen, max_norm)
    assert opt.steps == 2 and opt.skipped_steps == 0
    _bad_step(opt, model, gen_bad, bad)
    assert opt.skipped_steps == 1 and opt.steps == 2
    assert not math.isfinite(float(opt.grad_norm))
    for _ in range(2):
        _good_step(ref, opt, ref_model, model, gen, max_norm)     # the torch optimizer never saw the bad batch
    assert opt.steps == 4 and opt.skipped_steps == 1
    if max_norm is not None:
        assert opt.clipped_steps == 4                             # randn over ~250 values: norm ~ 16 > 3
    for pr, po in zip(ref_model.parameters(), model.parameters()):
        assert _rel(po, pr) < 2e-6, (name, args, max_norm, bad, _rel(po, pr))


@pytest.mark.parametrize("max_norm", [None, 3.0])
def test_skipped_first_step_leaves_the_momentum_buffer_uninitialised(max_norm):
    """SGD's first step sets buf = d_p; when the first step EVER is the skipped one, the next good step is torch's first step."""
    from fusion_gcn_amd.optim import FlatOptimizer
    args = dict(momentum=0.8, dampening=0.1)
    ref_model = small_model(3)
    model = guarded.to(copy.deepcopy(ref_model), DEV)
    ref = torch.optim.SGD(ref_model.parameters(), 0.05, **args)
    opt = FlatOptimizer(model.parameters(), "SGD", 0.05, max_grad_norm=max_norm, skip_nonfinite=True, **args)
    _bad_step(opt, model, torch.Generator().manual_seed(8), float("nan"))
    assert opt.steps == 0 and opt.skipped_steps == 1 and float(opt.state1.abs().sum()) == 0.0
    assert opt.state_dict()["state"] == {}
    gen = torch.Generator().manual_seed(7)
    for _ in range(3):
        _good_step(ref, opt, ref_model, model, gen, max_norm)
    for pr, po in zip(ref_model.parameters(), model.parameters()):
        assert _rel(po, pr) < 2e-6, _rel(po, pr)


def test_nonfinite_norm_without_skip_propagates_like_torch():
    """max_grad_norm set, skip_nonfinite off: clip_grad_norm_(error_if_nonfinite=False) -- the coefficient is NaN and propagates."""
    from fusion_gcn_amd.optim import FlatOptimizer
    model = guarded.to(small_model(3), DEV)
    opt = FlatOptimizer(model.parameters(), "ADAM", 0.05, max_grad_norm=1.0)
    for i, po in enumerate(model.parameters()):
        po.grad = torch.ones_like(po)
        if i == 0:
            po.grad.view(-1)[0] = float("nan")
    opt.step()
    assert math.isnan(float(opt.clip_coef)) and math.isnan(float(opt.grad_norm))
    assert opt.steps == 1 and opt.skipped_steps == 0 and opt.clipped_steps == 0
    assert all(bool(torch.isnan(p).all()) for p in model.parameters())


# ---- 4. grad_scale ---------------------------------------------------------------------------------------------------------------------
def test_grad_scale_is_the_data_parallel_average_under_the_clip():
    from fusion_gcn_amd.optim import FlatOptimizer
    a, b = guarded.to(small_model(5), DEV), guarded.to(small_model(5), DEV)
    oa = FlatOptimizer(a.parameters(), "ADAM", 0.01, weight_decay=0.01, max_grad_norm=0.5)
    ob = FlatOptimizer(b.parameters(), "ADAM", 0.01, weight_decay=0.01, max_grad_norm=0.5)
    ob.grad_scale = 0.25
    g = torch.Generator().manual_seed(1)
    for pa, pb in zip(a.parameters(), b.parameters()):
        grad = guarded.to(torch.randn(pa.shape, generator=g), DEV)
        pa.grad, pb.grad = grad.clone(), grad * 4.0
    oa.step(), ob.step()
    assert oa.clipped_steps == 1 and ob.clipped_steps == 1
    for pa, pb in zip(a.parameters(), b.parameters()):
        assert torch.allclose(pa, pb, rtol=1e-6, atol=1e-7)
    na, nb = float(oa.grad_norm), float(ob.grad_norm)
    assert na > 0.5 and abs(na - nb) <= 1e-9 * na


# ---- 5. no device wait -----------------------------------------------------------------------------------------------------------------
def test_guarded_step_never_waits_for_the_device():
    from fusion_gcn_amd.optim import FlatOptimizer
    model = guarded.to(small_model(3), DEV)
    opt = FlatOptimizer(model.parameters(), "ADAM", 0.05, max_grad_norm=1.0, skip_nonfinite=True)
    for po in model.parameters():
        po.grad = torch.ones_like(po)
    opt.step()                                   # (loads the library)
    torch.cuda.synchronize()
    probe = torch.ones(1, device=DEV)
    raised = False
    torch.cuda.set_sync_debug_mode("error")
    try:
        honoured = False
        try:
            probe.item()
        except RuntimeError:
            honoured = True
        opt.step()
        ptr = opt.grad_norm.data_ptr()
        opt.max_grad_norm = 2.0
        opt.step()
        try:
            opt.skipped_steps
        except RuntimeError:
            raised = True
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert honoured, "this torch build does not raise on .item() under set_sync_debug_mode('error')"
    assert ptr == opt._guard.data_ptr() + 8 * _lib.GUARD_NORM
    assert raised, "reading a device counter did not wait for the device"
    assert opt.steps == 3 and opt.skipped_steps == 0


# ---- 6. checkpoint ---------------------------------------------------------------------------------------------------------------------
def test_checkpoint_counts_applied_steps_only():
    from fusion_gcn_amd.optim import FlatOptimizer
    ref_model = small_model(3)
    model = guarded.to(copy.deepcopy(ref_model), DEV)
    ref = torch.optim.Adam(ref_model.parameters(), 0.05, weight_decay=0.01)
    opt = FlatOptimizer(model.parameters(), "ADAM", 0.05, weight_decay=0.01, skip_nonfinite=True)
    gen = torch.Generator().manual_seed(7)
    for it in range(3):
        if it == 2:
            _bad_step(opt, model, torch.Generator().manual_seed(8), float("inf"))
        _good_step(ref, opt, ref_model, model, gen, None)
    assert opt.steps == 3 and opt.skipped_steps == 1
    sd = opt.state_dict()
    other = torch.optim.Adam(copy.deepcopy(ref_model).parameters(), 0.05, weight_decay=0.01)
    other.load_state_dict(sd)
    assert all(float(e["step"]) == 3.0 for e in other.state_dict()["state"].values())
    assert torch.allclose(other.state_dict()["state"][0]["exp_avg"], ref.state_dict()["state"][0]["exp_avg"], rtol=1e-5, atol=1e-8)
    # torch's state into a guarded optimizer: the device counter is set and the next update uses it
    model2 = guarded.to(copy.deepcopy(ref_model), DEV)
    opt2 = FlatOptimizer(model2.parameters(), "ADAM", 0.05, weight_decay=0.01, skip_nonfinite=True)
    opt2.load_state_dict(ref.state_dict())
    assert int(opt2._guard[_lib.GUARD_STEP]) == 3 and opt2.steps == 3
    _good_step(ref, opt2, ref_model, model2, gen, None)
    assert opt2.steps == 4
    for pr, po in zip(ref_model.parameters(), model2.parameters()):
        assert _rel(po, pr) < 2e-6, _rel(po, pr)


# ---- 7. through the session --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def session_case():
    from fusion_gcn_amd.datasets.utd_mhad import constants as utd
    from fusion_gcn_amd.models.mmargcn.agcn import Model
    from fusion_gcn_amd.util import Graph
    torch.manual_seed(4)
    model = Model((1, 16, 20, 3), 27, Graph(utd.skeleton_edges, center_joint=utd.center_joint), num_layers=2)
    g = torch.Generator().manual_seed(5)
    data = [(torch.randn(2, 1, 16, 20, 3, generator=g), torch.randint(0, 27, (2,), generator=g), torch.arange(2)) for _ in range(3)]
    return model, data


@pytest.mark.parametrize("skip", [True, False])
def test_overflowing_batch_through_the_session(session_case, skip):
    """The scaler-overflow case: the second batch's loss is multiplied by inf, so its forward and BatchNorm statistics stay finite and
    only its gradients overflow."""
    from fusion_gcn_amd.loss import cross_entropy
    from fusion_gcn_amd.optim import create_optimizer
    from fusion_gcn_amd.session.procedures import DefaultBatchProcessor, DefaultStep
    from fusion_gcn_amd.session.session import Session
    base, data = session_case
    model = guarded.to(copy.deepcopy(base), DEV)
    opt = create_optimizer("ADAM", model, 1e-3, weight_decay=0.01, skip_nonfinite=skip)
    calls = []

    def loss_function(y_pred, label):
        calls.append(1)
        return cross_entropy(y_pred, label) * (float("inf") if len(calls) == 2 else 1.0)

    Session.train_epoch(DefaultBatchProcessor(DefaultStep()), model, loss_function, data, opt)
    torch.cuda.synchronize()
    assert len(calls) == 3
    if skip:
        # the bad batch's forward was finite, and no later forward ran on poisoned parameters
        assert all(bool(torch.isfinite(b).all()) for b in model.buffers())
        assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
        assert opt.skipped_steps == 1 and opt.steps == 2
    else:
        assert any(bool(torch.isnan(p).any()) for p in model.parameters())
        assert opt.steps == 3
