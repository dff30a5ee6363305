"""ASGD in FlatOptimizer (torch.optim.ASGD, the reference's fourth optimizer name): what can be checked without a GPU -- the
construction, torch's names, defaults and state-dict layout, the errors, the host-side validation of the C entry points (it precedes
every HIP call) and the host-side recurrence of eta / mu.  The arithmetic is checked on the device in tests/test_optim_asgd_gpu.py.

Oracle: torch.optim.ASGD on the CPU (float32, the single-tensor path)."""
import ctypes as C

import pytest
import torch
import torch.nn as nn

from fusion_gcn_amd import _lib, build

ARGS = [dict(), dict(t0=2, weight_decay=0.01), dict(t0=2, lambd=0.05, alpha=0.5, weight_decay=0.01)]


def small_model(seed=0):
    """The shape class of tests/test_optim.py: a few thousand floats, tensors with numel % 4 != 0 (135, 5, 35, 7, 21, 3: padding)."""
    torch.manual_seed(seed)
    return nn.Sequential(nn.Conv2d(3, 5, (9, 1)), nn.BatchNorm2d(5), nn.Conv2d(5, 7, 1), nn.Linear(7, 3))


def two_groups(model, overrides=({}, {})):
    """Weights | biases: interleaved in the model's order."""
    named = list(model.named_parameters())
    w = [p for n, p in named if n.endswith("weight")]
    b = [p for n, p in named if n.endswith("bias")]
    return [dict(params=w, **overrides[0]), dict(params=b, **overrides[1])]


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def test_asgd_is_built_with_torchs_names_and_defaults():
    """Fails on a tree without the feature (ValueError: Unsupported optimizer: ASGD)."""
    from fusion_gcn_amd.optim import KINDS, FlatOptimizer, create_optimizer
    assert KINDS["ASGD"] == 3
    m = small_model()
    before = [p.detach().clone() for p in m.parameters()]
    opt = FlatOptimizer(m.parameters(), "ASGD", 0.05)
    assert isinstance(opt, torch.optim.Optimizer) and opt.kind == "ASGD"
    g = opt.param_groups[0]
    assert (g["lr"], g["lambd"], g["alpha"], g["t0"], g["weight_decay"]) == (0.05, 1e-4, 0.75, 1e6, 0)
    for p, b in zip(m.parameters(), before):
        assert torch.equal(p, b) and p.data_ptr() % 16 == 0
    # state1 is ax, there is no state2; every row of the one-group table names group 0
    assert opt.state1 is not None and opt.state1.shape == opt.flat.shape and opt.state2 is None
    assert opt._tiles.dtype == torch.int32 and opt._tiles.shape[1] == 3 and opt._sched.numel() == 4 * _lib.OPT_MAX_GROUPS
    assert opt._tiles.tolist() == opt.tile_table() and all(r[2] == 0 for r in opt.tile_table())
    opt = create_optimizer("asgd", small_model(), 0.1, lambd=0.05, alpha=0.5, t0=2, weight_decay=0.01, max_grad_norm=3.0)
    g = opt.param_groups[0]
    assert opt.kind == "ASGD" and (g["lambd"], g["alpha"], g["t0"], g["weight_decay"]) == (0.05, 0.5, 2, 0.01)
    assert opt.max_grad_norm == 3.0
    # per-group overrides: group dicts and the rules of a config
    opt = FlatOptimizer(two_groups(small_model(), ({}, dict(lr=0.01, lambd=0.0, t0=0, weight_decay=0.1))), "ASGD", 0.05, lambd=0.02)
    assert [(g["lr"], g["lambd"], g["t0"], g["weight_decay"]) for g in opt.param_groups] == [(0.05, 0.02, 1e6, 0), (0.01, 0.0, 0, 0.1)]
    opt = create_optimizer("ASGD", small_model(), 0.05, t0=2, param_groups=[{"match": "bias$", "alpha": 0.5, "weight_decay": 0.0}],
                           weight_decay=0.01)
    assert [len(g["params"]) for g in opt.param_groups] == [4, 4]
    assert [(g["alpha"], g["t0"], g["weight_decay"]) for g in opt.param_groups] == [(0.75, 2, 0.01), (0.5, 2, 0.0)]


def test_foreign_arguments_and_ranges_raise():
    from fusion_gcn_amd.optim import FlatOptimizer
    for foreign in (dict(betas=(0.9, 0.99)), dict(momentum=0.9), dict(eps=1e-8), dict(nesterov=True)):
        with pytest.raises(TypeError, match="unexpected optimizer_args"):
            FlatOptimizer(small_model().parameters(), "ASGD", 0.1, **foreign)
    with pytest.raises(TypeError, match=r"\['momentum'\] in parameter group 1"):
        FlatOptimizer(two_groups(small_model(), ({}, dict(momentum=0.9))), "ASGD", 0.1)
    for other in ("SGD", "ADAM", "ADAMW"):
        with pytest.raises(TypeError, match="lambd"):
            FlatOptimizer(small_model().parameters(), other, 0.1, lambd=1e-4)
    with pytest.raises(ValueError, match="lambd"):
        FlatOptimizer(small_model().parameters(), "ASGD", 0.1, lambd=-1e-4)
    with pytest.raises(ValueError, match="lambd"):
        FlatOptimizer(two_groups(small_model(), ({}, dict(alpha=float("inf")))), "ASGD", 0.1)
    with pytest.raises(ValueError, match="negative lr / weight_decay"):
        FlatOptimizer(small_model().parameters(), "ASGD", 0.1, weight_decay=-0.1)
    # what stays as it was
    with pytest.raises(ValueError, match="Unsupported optimizer: RMSPROP"):
        FlatOptimizer(small_model().parameters(), "RMSPROP", 0.1)
    with pytest.raises(NotImplementedError):
        FlatOptimizer(small_model().parameters(), "ADAM", 0.1, amsgrad=True)
    with pytest.raises(NotImplementedError):
        FlatOptimizer(small_model().parameters(), "ASGD", 0.1, maximize=True)


def test_state_dict_has_torch_asgds_layout_before_any_step():
    from fusion_gcn_amd.optim import FlatOptimizer
    for args in ARGS:
        ref = torch.optim.ASGD(small_model().parameters(), 0.05, **args)
        opt = FlatOptimizer(small_model().parameters(), "ASGD", 0.05, **args)
        mine, theirs = opt.state_dict(), ref.state_dict()
        assert mine["state"] == {} and theirs["state"] == {}
        assert len(mine["param_groups"]) == len(theirs["param_groups"]) == 1
        a, b = mine["param_groups"][0], theirs["param_groups"][0]
        assert a["params"] == b["params"] and set(a) <= set(b)
        assert set(a) == {"params", "lr", "lambd", "alpha", "t0", "weight_decay"}
        for k in a:
            assert a[k] == b[k], (k, a[k], b[k])
    ref = torch.optim.ASGD(two_groups(small_model(), ({}, dict(lr=0.01, lambd=0.0))), 0.05)
    opt = FlatOptimizer(two_groups(small_model(), ({}, dict(lr=0.01, lambd=0.0))), "ASGD", 0.05)
    mine, theirs = opt.state_dict(), ref.state_dict()
    assert [g["params"] for g in mine["param_groups"]] == [g["params"] for g in theirs["param_groups"]] == [[0, 1, 2, 3], [4, 5, 6, 7]]
    for a, b in zip(mine["param_groups"], theirs["param_groups"]):
        assert all(a[k] == b[k] for k in a)


def test_step_fails_loudly_without_a_gpu():
    """(parameters on the CPU: no eager fallback on either path, for one group or two)"""
    from fusion_gcn_amd.optim import FlatOptimizer
    for kw in (dict(), dict(max_grad_norm=1.0, skip_nonfinite=True)):
        for grouped in (False, True):
            m = small_model()
            opt = FlatOptimizer(two_groups(m) if grouped else m.parameters(), "ASGD", 0.1, **kw)
            for p in m.parameters():
                p.grad = torch.ones_like(p)
            with pytest.raises(_lib.FgcnError):
                opt.step()


def test_averaged_refuses_other_kinds_and_an_untrained_optimizer():
    from fusion_gcn_amd.optim import FlatOptimizer
    with pytest.raises(TypeError, match="ASGD"):
        with FlatOptimizer(small_model().parameters(), "ADAM", 0.1).averaged():
            pass
    m = small_model()
    opt = FlatOptimizer(m.parameters(), "ASGD", 0.1)
    with pytest.raises(RuntimeError, match="before the first applied step"):
        with opt.averaged():
            pass
    opt._check_homes()
    # the swap itself needs no device: pretend one step was applied
    opt.steps = 1
    opt.state1.fill_(2.0)
    homes = [p.data_ptr() for p in m.parameters()]
    versions = [p._version for p in m.parameters()]
    with opt.averaged() as inside:
        assert inside is opt
        assert all(float(p.detach().min()) == 2.0 for p in m.parameters())
        assert all(p.data_ptr() == v.data_ptr() for p, v in zip(opt.params, opt._views(opt.state1)))
        assert all(p._version > v for p, v in zip(m.parameters(), versions))
        versions = [p._version for p in m.parameters()]
        with pytest.raises(RuntimeError, match="inside averaged"):
            opt.step()
        with pytest.raises(RuntimeError, match="already active"):
            with opt.averaged():
                pass
    assert [p.data_ptr() for p in m.parameters()] == homes
    assert all(p._version > v for p, v in zip(m.parameters(), versions))
    opt._check_homes()


@pytest.mark.parametrize("args", ARGS)
def test_host_side_eta_mu_recurrence_is_torchs(args):
    """optim._asgd_next -- the two formulas in Python doubles, rounded through float32 -- against the eta / mu tensors of
    torch.optim.ASGD's state, 8 steps under a per-step CosineAnnealingWarmRestarts(T_0=3).  eta lags the scheduler by one step: it is
    computed after a step from that step's lr.  Observed: equal to the float32 bit on all 8 steps and all three argument sets (both
    sides evaluate the same double expression with the interpreter's pow), so equality is asserted, not 1 ulp."""
    from fusion_gcn_amd.optim import _asgd_next, _f32
    m = small_model(3)
    ref = torch.optim.ASGD(m.parameters(), 0.05, **args)
    sched = torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(ref, T_0=3)
    group = dict(dict(lambd=1e-4, alpha=0.75, t0=1e6), **args)
    gen = torch.Generator().manual_seed(7)
    eta, mu = _f32(0.05), 1.0                              # the first step: eta = lr, mu = 1
    seen_mu = set()
    for it in range(8):
        for p in m.parameters():
            p.grad = torch.randn(p.shape, generator=gen) * (1.0 + it)
        lr_of_this_step = ref.param_groups[0]["lr"]
        ref.step()
        eta, mu = _asgd_next(dict(group, lr=lr_of_this_step), it + 1)
        sched.step()
        for st in ref.state.values():
            assert st["eta"].dtype == torch.float32 and float(st["step"]) == it + 1
            assert float(st["eta"]) == eta and float(st["mu"]) == mu, (it, float(st["eta"]), eta, float(st["mu"]), mu)
        if it >= 1:        # the lag: with the lr the scheduler has just set, eta would be another number
            assert _asgd_next(dict(group, lr=ref.param_groups[0]["lr"]), it + 1)[0] != eta
        seen_mu.add(mu)
    if args.get("t0") == 2:
        assert mu == _f32(1 / 6) and len(seen_mu) == 6     # mu < 1 from the count 4 on: the fifth step averages
    else:
        assert seen_mu == {1.0}


def test_asgd_entry_points_validate_on_the_host(lib):
    """FGCN_OPT_ASGD is declared; the ranges are checked before any HIP call (host pointers here: nothing is launched), for one group
    and for two, plain and with a guard."""
    import os
    import re

    from conftest import ROOT
    text = open(os.path.join(ROOT, "include", "fgcn.h")).read()
    assert re.search(r"#define FGCN_OPT_ASGD 3\b", text)
    assert _lib.GUARD_WORDS == 7 and lib.fgcn_optim_guard_bytes() == 56
    buf = (C.c_double * 128)()
    p16 = (C.addressof(buf) + 15) // 16 * 16
    n, err = 16, lib.fgcn_last_error
    asgd = dict(lr=0.1, weight_decay=0.0, beta1=1e-4, beta2=0.75, eps=1e6, momentum=0.1, dampening=1.0, nesterov=0)

    def grouped(guarded, s1=p16, s2=None, overrides=({}, {})):
        groups = (_lib.OptimGroup * len(overrides))(*[_lib.OptimGroup(**dict(asgd, **o)) for o in overrides])
        head = (p16, p16, s1, s2, n, 3, groups, len(groups), p16, 1, 1.0)
        if guarded:
            return lib.fgcn_optim_step(*head, 0, _lib.OptimGuard(1.0, 1, lib.fgcn_grad_norm_tiles(n), p16, p16, p16), None)
        return lib.fgcn_optim_step(*head, 1, None, None)

    def single(guarded, s1=p16, s2=None, **o):
        return grouped(guarded, s1, s2, overrides=(o,))

    assert single(False, beta1=-1e-4) == -1 and b"lambd" in err()
    assert single(False, s1=None) == -1 and b"state1" in err()
    assert single(False, s2=p16) == -1 and b"state2 must be NULL" in err()
    assert single(False, beta2=float("inf")) == -1 and single(False, eps=float("nan")) == -1
    assert single(False, lr=-0.1) == -1 and single(False, weight_decay=-0.1) == -1
    assert single(False, dampening=0.0) == -1 and b"mu in (0, 1]" in err()
    assert single(False, momentum=-0.1) == -1
    for guarded in (False, True):
        assert grouped(guarded, overrides=({}, dict(beta1=-1e-4))) == -1 and b"group 1: ASGD: negative lambd" in err()
        assert grouped(guarded, overrides=(dict(beta2=float("nan")), {})) == -1 and b"group 0" in err()
        assert grouped(guarded, overrides=({}, dict(eps=float("inf")))) == -1 and b"group 1" in err()
        assert grouped(guarded, overrides=({}, dict(lr=-0.1))) == -1 and b"group 1: negative lr / weight_decay" in err()
        assert grouped(guarded, s1=None) == -1 and b"state1" in err()
        assert grouped(guarded, s2=p16) == -1 and b"state2 must be NULL" in err()
    assert grouped(False, overrides=({}, dict(dampening=1.5))) == -1 and b"group 1: ASGD: eta" in err()
