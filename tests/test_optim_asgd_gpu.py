"""ASGD in FlatOptimizer on the device: the fused update (one launch; three on the guarded path) against torch.optim.ASGD on the CPU --
the reference's optimizer object for ``optimizer: ASGD`` -- step by step on identical parameters and gradients, for the parameters AND
the averaged iterate ax.  Tolerance: 2e-6 relative L2 per tensor after every step, the bound tests/test_optim.py holds the other kinds
to (float32 elementwise arithmetic in torch's operation order; torch's own float32 run stays within 1.1e-7 of its float64 run on these
argument sets).  The model is the shape class of tests/test_optim.py: a few thousand floats, tensors with numel % 4 != 0."""
import copy
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from test_optim_asgd import ARGS, small_model, two_groups

import guarded
from guarded import guarded_allocations  # noqa: F401  (the fixture)

to_device = guarded.to           # (tests here take a parameter named ``guarded``)

# every test runs on guarded allocations: NaN around each tensor the host layer creates, margins verified at teardown (tests/guarded.py)
pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_allocations")]
DEV = torch.device("cuda:0")
TOL = 2e-6
LR = 0.05


def rel(a, b):
    return float((a.detach().cpu() - b.detach().cpu()).norm() / b.detach().norm())


def gradients(model, steps, seed=7):
    """Per step one gradient per parameter, scaled by 1 + it (the harness of test_fused_update_matches_torch_optim)."""
    g = torch.Generator().manual_seed(seed)
    return [[torch.randn(p.shape, generator=g) * (1.0 + it) for p in model.parameters()] for it in range(steps)]


def pair(args, seed=3, groups=None, **guard):
    """(CPU model, torch.optim.ASGD), (device model, FlatOptimizer) from one state, each under a CosineAnnealingWarmRestarts(T_0=3)."""
    from fusion_gcn_amd.optim import FlatOptimizer
    ref_model = small_model(seed)
    model = to_device(copy.deepcopy(ref_model), DEV)
    ref = torch.optim.ASGD(groups(ref_model) if groups else ref_model.parameters(), LR, **args)
    opt = FlatOptimizer(groups(model) if groups else model.parameters(), "ASGD", LR, **args, **guard)
    sched = [torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(o, T_0=3) for o in (ref, opt)]
    return ref_model, ref, model, opt, sched


def ours(model, args=None, seed=3, groups=None, **guard):
    from fusion_gcn_amd.optim import FlatOptimizer
    opt = FlatOptimizer(groups(model) if groups else model.parameters(), "ASGD", LR, **(args or {}), **guard)
    return opt, torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(opt, T_0=3)


def feed(model, grads, dev=None):
    for p, g in zip(model.parameters(), grads):
        p.grad = g.clone() if dev is None else to_device(g, dev)


def assert_matches_torch(ref_model, ref, model, opt, what):
    axs = dict(zip((id(p) for p in opt.params), opt._views(opt.state1)))
    for pr, po in zip(ref_model.parameters(), model.parameters()):
        err_p, err_ax = rel(po, pr), rel(axs[id(po)], ref.state[pr]["ax"])
        assert err_p < TOL and err_ax < TOL, (what, err_p, err_ax)


def assert_padding_is_zero(opt):
    used = torch.zeros_like(opt.flat, dtype=torch.bool)
    for v, p in zip(opt.grads.views, opt.params):
        used[v.storage_offset():v.storage_offset() + p.numel()] = True
    assert int((~used).sum()) > 0
    assert float(opt.flat[~used].abs().sum()) == 0.0 and float(opt.state1[~used].abs().sum()) == 0.0


@pytest.mark.parametrize("guarded", [False, True], ids=["plain", "guarded"])
@pytest.mark.parametrize("args", ARGS, ids=["defaults", "t0_wd", "t0_lambd_alpha_wd"])
def test_fused_asgd_matches_torch_optim(args, guarded):
    """8 steps under a per-step scheduler (eta lags it by one step); t0 = 2 makes mu < 1 from the fifth step on, so the copy branch
    (mu == 1) and the averaging branch both run.  ``guarded``: the same through the three-launch path with a clip threshold nothing
    reaches (eta / mu computed on the device)."""
    ref_model, ref, model, opt, sched = pair(args, **(dict(max_grad_norm=1e9) if guarded else {}))
    for it, grads in enumerate(gradients(ref_model, 8)):
        feed(ref_model, grads), feed(model, grads, DEV)
        ref.step(), opt.step()
        for s in sched:
            s.step()
        assert abs(ref.param_groups[0]["lr"] - opt.param_groups[0]["lr"]) < 1e-12
        assert_matches_torch(ref_model, ref, model, opt, (args, it))
    assert opt.steps == 8 and (not guarded or opt.clipped_steps == 0)
    mu = float(next(iter(ref.state.values()))["mu"])
    assert (mu < 1) == ("t0" in args)
    assert_padding_is_zero(opt)


def test_guard_that_never_clips_is_the_plain_update():
    """max_grad_norm so large that the coefficient is exactly 1: parameters and ax of the guarded run against the plain run, 8 steps.
    The two paths compute eta differently -- the host from the Python double lr, the decision launch from the float32 lr that travels
    in fgcn_optim_group and with the device's pow -- so bitwise equality holds only while both round to the same float32; the bound is
    2e-6 and the first step whose bits differ (None: bitwise throughout) is printed.
    Observed on an MI355X: NOT bitwise.  The first step takes eta = (float)lr on both paths and is bitwise; the bits first differ on
    step 2 for the first two argument sets (the eta computed after step 1 already rounds differently) and on step 3 for the third;
    the eta left after step 8 is 0.03749915957 on the device against the host's and torch's 0.03749915585 for the first two sets
    (one float32 ulp) and equal for the third; mu is equal throughout, and every tensor stays inside 2e-6 on all 8 steps."""
    first = {}
    for name, args in zip(("defaults", "t0_wd", "t0_lambd_alpha_wd"), ARGS):
        base = small_model(3)
        ma, mb = to_device(copy.deepcopy(base), DEV), to_device(copy.deepcopy(base), DEV)
        (oa, sa), (ob, sb) = ours(ma, args), ours(mb, args, max_grad_norm=1e30)
        first[name] = None
        for it, grads in enumerate(gradients(base, 8)):
            feed(ma, grads, DEV), feed(mb, grads, DEV)
            oa.step(), ob.step()
            sa.step(), sb.step()
            assert float(ob.clip_coef) == 1.0
            for x, y in ((oa.flat, ob.flat), (oa.state1, ob.state1)):
                if first[name] is None and not torch.equal(x, y):
                    first[name] = it + 1
            for va, vb in zip(oa._views(oa.flat) + oa._views(oa.state1), ob._views(ob.flat) + ob._views(ob.state1)):
                assert rel(vb, va.cpu()) < TOL, (name, it)
        ea, eb = oa._read_eta_mu(), ob._read_eta_mu()
        print(f"asgd guarded vs plain [{name}]: first step with different bits {first[name]}; eta/mu host {ea} device {eb}")
        assert ea[0][1] == eb[0][1] and abs(ea[0][0] - eb[0][0]) <= 2.0 ** -23 * ea[0][0]     # mu exact, eta within 1 float32 ulp


def test_clipping_is_clip_grad_norm_then_step():
    args = ARGS[2]
    ref_model, ref, model, opt, sched = pair(args, max_grad_norm=0.5)
    for it, grads in enumerate(gradients(ref_model, 8)):
        feed(ref_model, grads), feed(model, grads, DEV)
        torch.nn.utils.clip_grad_norm_(ref_model.parameters(), 0.5)
        ref.step(), opt.step()
        for s in sched:
            s.step()
        assert_matches_torch(ref_model, ref, model, opt, it)
    assert opt.clipped_steps == 8 and opt.steps == 8


def test_skipped_step_leaves_every_bit_and_the_run_continues_as_torchs():
    """One inf gradient in the third call: parameters, ax, the step count and the eta / mu that state_dict() reports keep their bits;
    the following steps match a torch run that never saw that call (its scheduler does not advance either)."""
    args = ARGS[1]
    ref_model, ref, model, opt, sched = pair(args, skip_nonfinite=True)
    all_grads = gradients(ref_model, 8)
    for it, grads in enumerate(all_grads):
        if it == 2:
            before = (opt.flat.clone(), opt.state1.clone(), opt.steps, opt.state_dict()["state"][0], opt._sched.clone())
            bad = [g.clone() for g in grads]
            bad[1][0] = float("inf")
            feed(model, bad, DEV)
            opt.step()
            after = (opt.flat, opt.state1, opt.steps, opt.state_dict()["state"][0])
            assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1]) and before[2] == after[2] == 2
            for k in ("step", "eta", "mu", "ax"):
                assert torch.equal(before[3][k], after[3][k]), k
            assert opt.skipped_steps == 1 and torch.equal(before[4], opt._sched)      # use and next, all four values per group
            continue
        feed(ref_model, grads), feed(model, grads, DEV)
        ref.step(), opt.step()
        for s in sched:
            s.step()
        assert_matches_torch(ref_model, ref, model, opt, it)
    assert opt.steps == 7 and opt.skipped_steps == 1
    mine, theirs = opt.state_dict()["state"][0], ref.state_dict()["state"][0]
    assert float(mine["step"]) == float(theirs["step"]) == 7.0 and float(mine["mu"]) == float(theirs["mu"])


@pytest.mark.parametrize("guarded", [False, True], ids=["plain", "guarded"])
def test_two_groups_match_torch_asgd_over_the_same_groups(guarded):
    overrides = (dict(t0=2, weight_decay=0.01), dict(lr=0.02, lambd=0.05, t0=0, weight_decay=0.0))
    ref_model, ref, model, opt, sched = pair(dict(lambd=0.01), groups=lambda m: two_groups(m, overrides),
                                             **(dict(max_grad_norm=1e9) if guarded else {}))
    assert len(opt.param_groups) == 2 and opt._group_of == [0] * 4 + [1] * 4
    for it, grads in enumerate(gradients(ref_model, 8)):
        feed(ref_model, grads), feed(model, grads, DEV)
        ref.step(), opt.step()
        for s in sched:
            s.step()
        assert_matches_torch(ref_model, ref, model, opt, it)
    # the groups' own eta / mu, as torch's state has them (guarded: within one float32 ulp, see the guard test)
    mine, theirs = opt.state_dict()["state"], ref.state_dict()["state"]
    for slot in (0, 4):
        assert float(mine[slot]["mu"]) == float(theirs[slot]["mu"])
        assert abs(float(mine[slot]["eta"]) - float(theirs[slot]["eta"])) <= (2.0 ** -23 * float(theirs[slot]["eta"]) if guarded else 0.0)
    assert float(theirs[0]["eta"]) != float(theirs[4]["eta"]) and float(theirs[0]["mu"]) != float(theirs[4]["mu"])
    assert_padding_is_zero(opt)


def test_one_group_through_the_grouped_call_is_the_single_group_call():
    """include/fgcn.h: how the rows of the tile table cut the buffer does not change a bit of the result.  One group, 2085 16-byte groups,
    three tables -- full rows and a short one, rows of 250 (a quarter of a workgroup's 1024), unequal rows from 1 up -- for ASGD in both
    branches of the average and for ADAM, each plain and behind a guard whose clip bites."""
    from fusion_gcn_amd import _lib
    lib = _lib.load()
    n = 4 * 2085
    cuts = ([1024, 1024, 37], [250] * 8 + [85], [1, 1023, 512, 549])
    g = torch.Generator().manual_seed(11)
    p0, grad, ax0 = (to_device(torch.randn(n, generator=g), DEV) for _ in range(3))
    v0 = to_device(torch.rand(n, generator=g), DEV)                   # ADAM's exp_avg_sq
    stream = torch.cuda.current_stream(DEV).cuda_stream

    def run(kind, scalars, counts, guarded):
        """One call with the count going from 2 to 3 and grad_scale 0.5 -> (params, state1[, state2][, guard state, group_sched])."""
        assert sum(counts) == n // 4
        tiles = to_device(torch.tensor([[sum(counts[:i]), c, 0] for i, c in enumerate(counts)], dtype=torch.int32), DEV)
        out = [p0.clone(), ax0.clone()] + ([v0.clone()] if kind == 1 else [])
        groups = (_lib.OptimGroup * 1)(_lib.OptimGroup(*scalars))
        guard = None
        if guarded:
            state = torch.zeros(_lib.GUARD_WORDS, dtype=torch.int64, device=DEV)
            state[_lib.GUARD_STEP] = 2
            partials = torch.zeros(_lib.GRAD_NORM_MAX_TILES, dtype=torch.float64, device=DEV)
            sched = torch.zeros((4 if kind == 3 else 2) * _lib.OPT_MAX_GROUPS, dtype=torch.float64)
            if kind == 3:
                sched[:4] = torch.tensor([scalars[5], scalars[6]] * 2, dtype=torch.float32).double()      # eta, mu: use and next
            sched = to_device(sched, DEV)
            guard = _lib.OptimGuard(1.0, 1, lib.fgcn_grad_norm_tiles(n), partials.data_ptr(), state.data_ptr(), sched.data_ptr())
            out += [state, sched]
        rc = lib.fgcn_optim_step(out[0].data_ptr(), grad.data_ptr(), out[1].data_ptr(), out[2].data_ptr() if kind == 1 else None, n, kind,
                                 groups, 1, tiles.data_ptr(), tiles.shape[0], 0.5, 0 if guarded else 3, guard, stream)
        _lib.check(rc, "fgcn_optim_step")
        torch.cuda.synchronize()
        if guarded:                                           # the norm of 0.5 * grad is about 45: the clip to 1 bites
            assert int(state[_lib.GUARD_STEP]) == 3 and int(state[_lib.GUARD_CLIPPED]) == 1
            assert 0.0 < float(state.view(torch.float64)[_lib.GUARD_COEF]) < 0.1
        return out

    asgd = [(0.05, 0.01, 0.05, 0.5, 2.0, eta, mu, 0) for eta, mu in ((0.05, 1.0), (0.0371, 0.25))]
    adam = (0.05, 0.01, 0.9, 0.999, 1e-8, 0.0, 0.0, 0)
    for kind, scalars in ((3, asgd[0]), (3, asgd[1]), (1, adam)):
        for guarded in (False, True):
            first, *others = [run(kind, scalars, counts, guarded) for counts in cuts]
            for other in others:
                assert len(other) == len(first) and all(torch.equal(a, b) for a, b in zip(first, other)), (kind, scalars, guarded)
            pa, axa = first[0], first[1]
            assert not torch.equal(pa, p0) and not torch.equal(axa, ax0)
            if kind == 3:
                mu = scalars[6]
                assert torch.equal(axa, pa) if mu == 1.0 else not torch.equal(axa, pa)
            if kind == 3 and not guarded:
                # and it is torch's arithmetic: one tensor, the same scalars
                eta, mu = scalars[5], scalars[6]
                pr = p0.cpu().clone().requires_grad_()
                pr.grad = grad.cpu() * 0.5
                ref = torch.optim.ASGD([pr], 0.05, lambd=0.05, alpha=0.5, t0=2.0, weight_decay=0.01)
                ref.state[pr].update(step=torch.tensor(2.0), eta=torch.tensor(eta), mu=torch.tensor(mu), ax=ax0.cpu().clone())
                ref.step()
                assert rel(pa, pr) < TOL and rel(axa, ref.state[pr]["ax"]) < TOL


def test_two_optimizers_from_one_state_agree_bit_for_bit():
    base = small_model(3)
    ma, mb = to_device(copy.deepcopy(base), DEV), to_device(copy.deepcopy(base), DEV)
    (oa, sa), (ob, sb) = ours(ma, ARGS[2]), ours(mb, ARGS[2])
    for grads in gradients(base, 5):
        feed(ma, grads, DEV), feed(mb, grads, DEV)
        oa.step(), ob.step()
        sa.step(), sb.step()
    assert torch.equal(oa.flat, ob.flat) and torch.equal(oa.state1, ob.state1)
    assert float(oa.state1.abs().sum()) > 0 and not torch.equal(oa.flat, oa.state1)
    assert_padding_is_zero(oa), assert_padding_is_zero(ob)


@pytest.mark.parametrize("guarded", [False, True], ids=["plain", "guarded"])
def test_state_dict_loads_into_torch_asgd_and_back(guarded):
    from fusion_gcn_amd.optim import FlatOptimizer
    guard = dict(max_grad_norm=1e9) if guarded else {}
    args = ARGS[2]
    ref_model, ref, model, opt, sched = pair(args, **guard)
    for grads in gradients(ref_model, 6):
        feed(ref_model, grads), feed(model, grads, DEV)
        ref.step(), opt.step()
        for s in sched:
            s.step()
    # ours into torch's
    mine = opt.state_dict()
    assert set(mine["state"]) == set(range(8)) and list(mine["state"][0]) == ["step", "eta", "mu", "ax"]
    other = torch.optim.ASGD(copy.deepcopy(ref_model).parameters(), LR, **args)
    other.load_state_dict(mine)
    got = other.state_dict()["state"]
    for i in range(8):
        for k in ("step", "eta", "mu", "ax"):
            assert torch.equal(got[i][k].cpu(), mine["state"][i][k].cpu()), (i, k)
        assert float(got[i]["step"]) == 6.0 and got[i]["eta"].dtype == torch.float32
    # torch's into a fresh one of ours (on the guarded path the load writes group_sched) and out again
    model2 = to_device(copy.deepcopy(ref_model), DEV)
    opt2 = FlatOptimizer(model2.parameters(), "ASGD", LR, **args, **guard)
    theirs = ref.state_dict()
    opt2.load_state_dict(theirs)
    assert opt2.steps == 6 and opt2.param_groups[0]["lr"] == ref.param_groups[0]["lr"]
    back = opt2.state_dict()["state"]
    for i in range(8):
        for k in ("step", "eta", "mu", "ax"):
            assert torch.equal(back[i][k].cpu(), theirs["state"][i][k]), (i, k)
    # and the loaded state is the one the next step uses
    grads = gradients(ref_model, 1, seed=9)[0]
    feed(ref_model, grads), feed(model2, grads, DEV)
    ref.step(), opt2.step()
    assert_matches_torch(ref_model, ref, model2, opt2, "after load")
    assert opt2.steps == 7


def test_averaged_evaluates_the_model_with_ax():
    """An AGCN model of the smallest shape tests/test_session_gpu.py uses, three training steps with t0 = 0 (ax is a true average from
    the second step on): inside the context the eval logits are those of a deep copy whose parameters were overwritten with ax, bit for
    bit; outside they are what they were."""
    from fusion_gcn_amd.datasets.utd_mhad import constants as utd
    from fusion_gcn_amd.models.mmargcn.agcn import Model
    from fusion_gcn_amd.optim import FlatOptimizer
    from fusion_gcn_amd.util import Graph
    from oracle import filler
    shape, classes = (1, 24, 20, 3), 27
    model = Model(shape, classes, Graph(utd.skeleton_edges, center_joint=utd.center_joint))
    filler.fill_state_dict(model.state_dict())
    model = to_device(model, DEV).train()
    opt = FlatOptimizer(model.parameters(), "ASGD", 0.01, t0=0)
    g = torch.Generator().manual_seed(5)
    x, y = to_device(torch.randn(4, *shape, generator=g), DEV), to_device(torch.randint(0, classes, (4,), generator=g), DEV)
    with pytest.raises(RuntimeError, match="before the first applied step"):
        with opt.averaged():
            pass
    for _ in range(3):
        opt.zero_grad()
        F.cross_entropy(model(x), y).backward()
        opt.step()
    model.eval()
    with torch.no_grad():
        last = model(x).clone()
        twin = copy.deepcopy(model)
        for q, ax in zip((q for q in twin.parameters() if q.requires_grad), opt._views(opt.state1)):
            q.copy_(ax)
        want = twin(x).clone()
        assert not torch.equal(want, last)
        with opt.averaged():
            inside = model(x).clone()
            with pytest.raises(RuntimeError, match="inside averaged"):
                opt.step()
        outside = model(x).clone()
    assert torch.equal(inside, want)
    assert torch.equal(outside, last)
    # training goes on in the home buffers
    model.train()
    opt.zero_grad()
    F.cross_entropy(model(x), y).backward()
    opt._check_homes()
    opt.step()
    assert opt.steps == 4


def test_c_abi_refuses_what_the_header_says():
    from fusion_gcn_amd import _lib
    lib = _lib.load()
    n = 64
    p, grad, ax = (torch.zeros(n, device=DEV) for _ in range(3))
    tiles = to_device(torch.tensor([[0, n // 4, 0]], dtype=torch.int32), DEV)

    def call(state1, lambd):
        groups = (_lib.OptimGroup * 1)(_lib.OptimGroup(0.1, 0.0, lambd, 0.75, 1e6, 0.1, 1.0, 0))
        return lib.fgcn_optim_step(p.data_ptr(), grad.data_ptr(), state1, None, n, 3, groups, 1, tiles.data_ptr(), 1, 1.0, 1, None, None)

    assert call(ax.data_ptr(), -1e-4) == -1 and b"lambd" in lib.fgcn_last_error()
    assert call(None, 1e-4) == -1 and b"state1" in lib.fgcn_last_error()
    with pytest.raises(_lib.FgcnError, match="state1"):
        _lib.check(-1, "fgcn_optim_step")
    torch.cuda.synchronize()
    assert float(p.abs().sum()) == 0.0
