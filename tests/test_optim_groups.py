"""Parameter groups of FlatOptimizer (a list of dicts, as every torch.optim.Optimizer takes): what can be checked without a GPU -- the
construction and its errors, torch's state-dict layout, the element-to-group tile table the grouped kernel walks, the groups a config
spells with ``param_groups=``, and the host-side validation of fgcn_optim_step, plain and with a guard (it precedes
every HIP call).  The arithmetic is checked on the device in tests/test_optim_groups_gpu.py.

The model is chosen so that the flat buffers hold: tensor sizes that are no multiple of 4 (4690, 67, 335, 5: padding), a 1-element
tensor, one tensor longer than a tile row (Linear(70, 67).weight: 4690 floats = 1173 16-byte groups > FGCN_OPT_TILE4), and -- with
``three_groups`` -- groups that interleave in the model's order (A C B B A C B B A C)."""
import ctypes as C
import os
import re

import pytest
import torch
import torch.nn as nn

from conftest import ROOT
from fusion_gcn_amd import _lib, build

TORCH = {"SGD": torch.optim.SGD, "ADAM": torch.optim.Adam, "ADAMW": torch.optim.AdamW}
# (kind, the arguments of the optimizer = the defaults, the overrides of the three groups)
CASES = [("SGD", dict(momentum=0.9, nesterov=True),
          [dict(weight_decay=1e-4), dict(lr=0.02, momentum=0.8, nesterov=False, dampening=0.1), dict(lr=0.1, momentum=0.0, nesterov=False)]),
         ("ADAM", dict(weight_decay=0.01),
          [dict(), dict(lr=0.01, weight_decay=0.0, betas=(0.8, 0.99)), dict(lr=0.1, weight_decay=0.1, eps=1e-6)]),
         ("ADAMW", dict(),
          [dict(), dict(lr=0.01, weight_decay=0.0, betas=(0.8, 0.99)), dict(lr=0.1, weight_decay=0.1, eps=1e-6)])]


def group_model(seed=0):
    torch.manual_seed(seed)
    return nn.Sequential(nn.Linear(70, 67), nn.BatchNorm1d(67), nn.Linear(67, 5), nn.BatchNorm1d(5), nn.Linear(5, 1))


def three_groups(model, overrides=({}, {}, {})):
    """Linear weights | BatchNorm scales and biases | Linear biases: interleaved in the model's order."""
    named = list(model.named_parameters())
    bn = {f"{i}." for i, m in enumerate(model) if isinstance(m, nn.BatchNorm1d)}
    a = [p for n, p in named if n[:2] not in bn and n.endswith("weight")]
    b = [p for n, p in named if n[:2] in bn]
    c = [p for n, p in named if n[:2] not in bn and n.endswith("bias")]
    assert len(a) == 3 and len(b) == 4 and len(c) == 3
    return [dict(params=ps, **o) for ps, o in zip((a, b, c), overrides)]


def split_groups(model, k):
    """k groups over the model's tensors, round-robin (so they interleave)."""
    ps = list(model.parameters())
    return [dict(params=ps[i::k]) for i in range(k)]


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def test_construction_with_2_3_and_8_groups_and_the_limit():
    """Fails on a tree without the feature (NotImplementedError: one parameter group)."""
    from fusion_gcn_amd.optim import MAX_GROUPS, FlatOptimizer
    assert MAX_GROUPS == 8 == _lib.OPT_MAX_GROUPS
    for k in (2, 3, 8):
        m = group_model()
        before = [p.detach().clone() for p in m.parameters()]
        opt = FlatOptimizer(split_groups(m, k), "ADAM", 0.1, weight_decay=0.01)
        assert isinstance(opt, torch.optim.Optimizer) and len(opt.param_groups) == k
        assert all(g["lr"] == 0.1 and g["weight_decay"] == 0.01 for g in opt.param_groups)
        for p, b in zip(m.parameters(), before):
            assert torch.equal(p, b) and p.data_ptr() % 16 == 0
        # the optimizer's own flat buffers: the concatenation of the groups
        assert [id(p) for p in opt.params] == [id(p) for g in opt.param_groups for p in g["params"]]
        assert opt._group_of == [i for i, g in enumerate(opt.param_groups) for _ in g["params"]]
        assert opt._tiles.dtype == torch.int32 and opt._tiles.shape[1] == 3 and opt._sched.numel() == 2 * MAX_GROUPS
    with pytest.raises(ValueError, match="at most 8"):
        FlatOptimizer(split_groups(group_model(), 9), "ADAM", 0.1)
    # per-group overrides land in param_groups; torch's schedulers drive every group through them
    m = group_model()
    opt = FlatOptimizer(three_groups(m, ({}, dict(lr=0.01, weight_decay=0.0), dict(betas=(0.8, 0.99)))), "ADAM", 0.1, weight_decay=0.01)
    assert [g["lr"] for g in opt.param_groups] == [0.1, 0.01, 0.1]
    assert [g["weight_decay"] for g in opt.param_groups] == [0.01, 0.0, 0.01] and opt.param_groups[2]["betas"] == (0.8, 0.99)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, [lambda e: 0.5 ** e, lambda e: 1.0, lambda e: 1.0 / (1 + e)])
    sched.step()
    assert [g["lr"] for g in opt.param_groups] == pytest.approx([0.05, 0.01, 0.05])
    # one group given as a list of one dict: the same call, every row of its table names group 0
    one = FlatOptimizer([dict(params=list(group_model().parameters()), lr=0.3)], "SGD", 0.1)
    assert one._tiles.tolist() == one.tile_table() and all(r[2] == 0 for r in one.tile_table()) and one.param_groups[0]["lr"] == 0.3


def test_per_group_validation_errors():
    from fusion_gcn_amd.optim import FlatOptimizer

    def build_with(kind, override, **args):
        return FlatOptimizer(three_groups(group_model(), ({}, override, {})), kind, 0.1, **args)

    with pytest.raises(ValueError, match="negative lr / weight_decay"):
        build_with("ADAM", dict(lr=-0.1))
    with pytest.raises(ValueError, match="negative lr / weight_decay"):
        build_with("SGD", dict(weight_decay=-1e-4))
    with pytest.raises(ValueError, match="Nesterov momentum requires"):
        build_with("SGD", dict(nesterov=True))                              # no momentum in that group
    with pytest.raises(ValueError, match="Nesterov momentum requires"):
        build_with("SGD", dict(momentum=0.0), momentum=0.9, nesterov=True)  # the default's Nesterov, the group's momentum
    with pytest.raises(ValueError, match="Nesterov momentum requires"):
        build_with("SGD", dict(dampening=0.1), momentum=0.9, nesterov=True)
    with pytest.raises(TypeError, match=r"unexpected optimizer_args \['betas'\] in parameter group 1"):
        build_with("SGD", dict(betas=(0.9, 0.99)))
    with pytest.raises(TypeError, match="momentum"):
        build_with("ADAMW", dict(momentum=0.9))
    with pytest.raises(TypeError, match="max_grad_norm"):
        build_with("ADAM", dict(max_grad_norm=1.0))                         # the guard belongs to the optimizer, not to a group
    with pytest.raises(NotImplementedError, match="amsgrad"):
        build_with("ADAM", dict(amsgrad=True))
    m = group_model()
    groups = three_groups(m)
    groups[2]["params"].append(groups[0]["params"][0])
    with pytest.raises(ValueError, match="more than one parameter group"):      # torch's own error
        FlatOptimizer(groups, "ADAM", 0.1)
    # a shared buffer has to cover exactly the trainable parameters of all groups
    from fusion_gcn_amd.dp import FlatGradients
    m = group_model()
    with pytest.raises(ValueError, match="exactly the trainable parameters of all groups"):
        FlatOptimizer(three_groups(m)[:2], "ADAM", 0.1, grads=FlatGradients(m.parameters()))


def test_add_param_group_after_construction_raises():
    from fusion_gcn_amd.optim import FlatOptimizer
    m = group_model()
    opt = FlatOptimizer(three_groups(m), "SGD", 0.1)
    single = FlatOptimizer(group_model().parameters(), "SGD", 0.1)
    extra = nn.Parameter(torch.zeros(3))
    for o in (opt, single):
        with pytest.raises(NotImplementedError, match="final parameter groups"):
            o.add_param_group({"params": [extra]})
    assert len(opt.param_groups) == 3 and len(single.param_groups) == 1


def test_frozen_parameter_keeps_its_slot():
    from fusion_gcn_amd.optim import FlatOptimizer
    m = group_model()
    groups = three_groups(m)
    frozen = groups[1]["params"][1]                   # the second tensor of the second group: global position 3 + 1
    frozen.requires_grad_(False)
    opt = FlatOptimizer(groups, "SGD", 0.1, momentum=0.9)
    assert all(p is not frozen for p in opt.params) and len(opt.params) == 9
    assert opt._slots() == [0, 1, 2, 3, 5, 6, 7, 8, 9]
    sd = opt.state_dict()
    assert [g["params"] for g in sd["param_groups"]] == [[0, 1, 2], [3, 4, 5, 6], [7, 8, 9]]
    ref = torch.optim.SGD(three_groups(group_model()), 0.1, momentum=0.9)
    assert [g["params"] for g in ref.state_dict()["param_groups"]] == [g["params"] for g in sd["param_groups"]]
    assert frozen.data_ptr() < opt.flat.data_ptr() or frozen.data_ptr() >= opt.flat.data_ptr() + 4 * opt.flat.numel()


@pytest.mark.parametrize("kind,args,overrides", CASES)
def test_state_dict_has_torchs_layout_and_round_trips(kind, args, overrides):
    from fusion_gcn_amd.optim import FlatOptimizer
    ref_model = group_model(3)
    ref = TORCH[kind](three_groups(ref_model, overrides), 0.05, **args)
    opt = FlatOptimizer(three_groups(group_model(3), overrides), kind, 0.05, **args)
    mine, theirs = opt.state_dict(), ref.state_dict()
    assert mine["state"] == {} and theirs["state"] == {}

    def same_groups(mine, theirs):
        assert len(mine["param_groups"]) == len(theirs["param_groups"]) == 3
        for a, b in zip(mine["param_groups"], theirs["param_groups"]):
            assert a["params"] == b["params"]
            assert set(a) <= set(b)
            for k in a:
                assert a[k] == b[k], (k, a[k], b[k])
    same_groups(mine, theirs)
    assert [g["params"] for g in mine["param_groups"]] == [[0, 1, 2], [3, 4, 5, 6], [7, 8, 9]]
    # three steps of the torch optimizer, its state into ours and back into a fresh torch optimizer
    gen = torch.Generator().manual_seed(1)
    for _ in range(3):
        for p in ref_model.parameters():
            p.grad = torch.randn(p.shape, generator=gen)
        ref.step()
    theirs = ref.state_dict()
    theirs["param_groups"][1]["lr"] = 0.123                      # a scheduler's value travels in the group entry
    opt.load_state_dict(theirs)
    assert opt.param_groups[1]["lr"] == 0.123 and opt.param_groups[0]["lr"] == 0.05
    mine = opt.state_dict()
    same_groups(mine, theirs)
    assert set(mine["state"]) == set(theirs["state"])                            # global positions
    assert set(mine["state"]) == set(range(7 if kind == "SGD" else 10))          # (SGD: the group without a momentum keeps no state)
    for i in mine["state"]:
        assert set(mine["state"][i]) == set(theirs["state"][i]) & {"step", "exp_avg", "exp_avg_sq", "momentum_buffer"}
        for k, v in mine["state"][i].items():
            assert torch.equal(torch.as_tensor(v), torch.as_tensor(theirs["state"][i][k])), (i, k)
    if kind != "SGD":
        assert opt.steps == 3
    back = TORCH[kind](three_groups(group_model(3), overrides), 0.05, **args)
    back.load_state_dict(mine)
    again = back.state_dict()
    assert again["param_groups"][1]["lr"] == 0.123
    assert set(again["state"]) == set(theirs["state"])
    for i in theirs["state"]:
        for k, v in theirs["state"][i].items():
            if v is not None:
                assert torch.equal(torch.as_tensor(again["state"][i][k]), torch.as_tensor(v)), (i, k)
    with pytest.raises(ValueError, match="number of parameter groups"):
        opt.load_state_dict(torch.optim.SGD(group_model().parameters(), 0.1).state_dict())


def _assert_table_is_closed(opt, tile4):
    """Every 16-byte group of every tensor exactly once, with its tensor's group; the padding rides in the tensor's last group."""
    n4 = opt.flat.numel() // 4
    rows = opt.tile_table(tile4)
    owner = [-1] * n4
    for start4, count4, gi in rows:
        assert 1 <= count4 <= tile4 and 0 <= start4 and start4 + count4 <= n4 and 0 <= gi < len(opt.param_groups)
        for i in range(start4, start4 + count4):
            assert owner[i] == -1, f"16-byte group {i} is covered twice"
            owner[i] = gi
    assert -1 not in owner
    end = 0
    for p, v, gi in zip(opt.params, opt.grads.views, opt._group_of):
        off = v.storage_offset()
        assert off % 4 == 0 and off // 4 == end                    # (the next tensor starts where this one's padding ends)
        end = off // 4 + (p.numel() + 3) // 4
        assert owner[off // 4:end] == [gi] * (end - off // 4)      # the tensor and its <= 3 floats of padding
    assert end == n4
    return rows


def test_tile_table_is_closed_in_group_order_and_in_model_order():
    from fusion_gcn_amd.dp import FlatGradients
    from fusion_gcn_amd.optim import FlatOptimizer
    m = group_model()
    own = FlatOptimizer(three_groups(m), "ADAM", 0.1)              # the optimizer's own buffer: groups are contiguous segments
    rows = _assert_table_is_closed(own, _lib.OPT_TILE4)
    assert [r[2] for r in rows] == sorted(r[2] for r in rows)
    assert sum(r[2] == 0 for r in rows) == 2                        # 4690 + 335 + 5 floats: 1173 + 84 + 2 = 1259 groups, two rows
    assert own._tiles.tolist() == rows
    m = group_model()
    shared = FlatGradients(m.parameters())
    opt = FlatOptimizer(three_groups(m), "ADAM", 0.1, grads=shared)
    assert opt.grads is shared and [id(p) for p in opt.params] == [id(p) for p in m.parameters()]
    assert opt._group_of == [0, 2, 1, 1, 0, 2, 1, 1, 0, 2]          # interleaved
    rows = _assert_table_is_closed(opt, _lib.OPT_TILE4)
    assert rows[0] == [0, 1024, 0] and rows[1] == [1024, 149, 0]    # the first tensor crosses a row boundary; 4690 floats = 1173 groups
    assert rows[2] == [1173, 17, 2] and rows[3] == [1190, 34, 1]    # 67 floats + 1 of padding; the two BatchNorm tensors are one run
    assert rows[-1] == [opt.flat.numel() // 4 - 1, 1, 2]            # the 1-element tensor and its 3 floats of padding
    assert opt._tiles.tolist() == rows
    for tile4 in (1, 7, 256):
        _assert_table_is_closed(opt, tile4)
    # eight round-robin groups
    m = group_model()
    _assert_table_is_closed(FlatOptimizer(split_groups(m, 8), "SGD", 0.1, grads=FlatGradients(m.parameters())), _lib.OPT_TILE4)


def test_create_optimizer_builds_groups_from_a_config():
    from fusion_gcn_amd.optim import create_optimizer
    m = group_model()
    names = dict(m.named_parameters())
    rules = [{"match": r"^[13]\.|bias$", "weight_decay": 0.0}, {"match": r"^4\.", "lr": 0.01}, {"match": r"^0\.weight$", "betas": (0.8, 0.99)}]
    opt = create_optimizer("ADAM", m, 0.1, weight_decay=0.01, param_groups=rules, max_grad_norm=2.0)
    assert len(opt.param_groups) == 4 and opt.max_grad_norm == 2.0
    got = [[n for n, p in names.items() if any(p is q for q in g["params"])] for g in opt.param_groups]
    assert got[0] == ["2.weight"]                                          # unmatched: the first group, with the defaults
    assert got[1] == ["0.bias", "1.weight", "1.bias", "2.bias", "3.weight", "3.bias", "4.bias"]
    assert got[2] == ["4.weight"]                                          # first match wins: 4.bias went to the rule before
    assert got[3] == ["0.weight"]
    assert [g["weight_decay"] for g in opt.param_groups] == [0.01, 0.0, 0.01, 0.01]
    assert [g["lr"] for g in opt.param_groups] == [0.1, 0.1, 0.01, 0.1] and opt.param_groups[3]["betas"] == (0.8, 0.99)
    assert "match" not in opt.param_groups[1] and "param_groups" not in opt.defaults
    assert rules[0] == {"match": r"^[13]\.|bias$", "weight_decay": 0.0}    # the config's objects are left alone
    # every parameter matched: no empty default group
    opt = create_optimizer("SGD", group_model(), 0.1, param_groups=[{"match": "weight", "lr": 0.2}, {"match": "bias"}])
    assert [len(g["params"]) for g in opt.param_groups] == [5, 5] and [g["lr"] for g in opt.param_groups] == [0.2, 0.1]
    with pytest.raises(ValueError, match="fc.*matches no parameter"):
        create_optimizer("ADAM", group_model(), 0.1, param_groups=[{"match": r"^fc\.", "lr": 0.01}])
    with pytest.raises(ValueError, match="matches no parameter"):
        create_optimizer("ADAM", group_model(), 0.1, param_groups=[{"match": "weight"}, {"match": r"0\.weight"}])   # shadowed by the first
    with pytest.raises(ValueError, match="match"):
        create_optimizer("ADAM", group_model(), 0.1, param_groups=[{"lr": 0.01}])
    with pytest.raises(TypeError, match="momentum"):
        create_optimizer("ADAM", group_model(), 0.1, param_groups=[{"match": "bias", "momentum": 0.9}])
    assert len(create_optimizer("ADAM", group_model(), 0.1).param_groups) == 1


def test_new_entry_points_are_declared_and_bound(lib):
    text = open(os.path.join(ROOT, "include", "fgcn.h")).read()
    assert re.search(r"\bint fgcn_optim_step\(", text) and "fgcn_optim_step" in _lib.SIGNATURES and hasattr(lib, "fgcn_optim_step")
    assert [n for n in _lib.SIGNATURES if n.startswith("fgcn_optim_step")] == ["fgcn_optim_step"]       # the one call
    assert re.search(r"#define FGCN_OPT_MAX_GROUPS 8\b", text) and f"#define FGCN_OPT_TILE4 {_lib.OPT_TILE4}\n" in text
    for name, mirror, size in (("fgcn_optim_group", _lib.OptimGroup, 32), ("fgcn_optim_guard", _lib.OptimGuard, 40)):
        assert C.sizeof(mirror) == size
        fields = re.search(rf"typedef struct {name} \{{(.*?)\}}", text, re.S).group(1)
        fields = re.sub(r"/\*.*?\*/", "", fields)
        assert re.findall(r"\b(\w+)\s*[,;]", fields) == [f[0] for f in mirror._fields_]
    # the guard state: seven words (the Adam step sizes live in group_sched)
    assert re.search(r"FGCN_GUARD_WORDS = 7\b", text) and _lib.GUARD_WORDS == 7 and lib.fgcn_optim_guard_bytes() == 56


def test_grouped_steps_validate_on_the_host(lib):
    buf = (C.c_double * 128)()
    p16 = (C.addressof(buf) + 15) // 16 * 16
    n = 16
    adam = dict(lr=0.1, weight_decay=0.0, beta1=0.9, beta2=0.999, eps=1e-8, momentum=0.0, dampening=0.0, nesterov=0)

    def groups_of(*overrides):
        return (_lib.OptimGroup * max(1, len(overrides)))(*[_lib.OptimGroup(**dict(adam, **o)) for o in overrides])

    def call(guarded, params=p16, grads=p16, s1=p16, s2=p16, n=n, kind=1, groups=None, ngroups=None, tiles=p16, ntiles=1, step=None,
             max_norm=1.0, partials=p16, n_partials=None, guard=p16, sched=p16):
        groups = groups_of({}, {}) if groups is None else groups
        ngroups = len(groups) if ngroups is None else ngroups
        head = (params, grads, s1, s2, n, kind, groups, ngroups, tiles, ntiles, 1.0)
        if not guarded:
            return lib.fgcn_optim_step(*head, 1 if step is None else step, None, None)
        n_partials = lib.fgcn_grad_norm_tiles(n) if n_partials is None else n_partials
        return lib.fgcn_optim_step(*head, 0 if step is None else step, _lib.OptimGuard(max_norm, 1, n_partials, partials, guard, sched),
                                   None)

    for guarded in (False, True):
        err = lib.fgcn_last_error
        assert call(guarded, params=None) == -1 and b"null pointer" in err()
        assert call(guarded, grads=None) == -1
        assert call(guarded, n=0) == -1
        assert call(guarded, n=18) == -2 and b"multiple of 4" in err()
        assert call(guarded, grads=p16 + 8) == -2 and call(guarded, params=p16 + 4) == -2
        assert call(guarded, n=2 ** 33 + 4) == -1 and b"tile table indexes" in err()
        assert call(guarded, kind=3) == -1 and b"kind 3" in err()
        assert call(guarded, ngroups=0) == -1 and b"1 to 8 parameter groups (got 0)" in err()
        assert call(guarded, groups=groups_of(*[{}] * 9)) == -1 and b"1 to 8 parameter groups (got 9)" in err()
        assert call(guarded, groups=C.cast(None, C.POINTER(_lib.OptimGroup)), ngroups=2) == -1 and b"null groups" in err()
        assert call(guarded, tiles=None) == -1 and b"null or empty tile table" in err()
        assert call(guarded, ntiles=0) == -1 and b"null or empty tile table" in err()
        assert call(guarded, tiles=p16 + 2) == -2 and b"4-byte aligned" in err()
        assert call(guarded, s2=None) == -1 and b"Adam needs" in err()
        # per-group ranges: the message names the group
        assert call(guarded, groups=groups_of({}, dict(lr=-0.1))) == -1 and b"group 1: negative lr / weight_decay" in err()
        assert call(guarded, groups=groups_of(dict(weight_decay=-1.0), {})) == -1 and b"group 0: negative" in err()
        assert call(guarded, groups=groups_of({}, {}, dict(lr=float("nan")))) == -1 and b"group 2" in err()
        assert call(guarded, groups=groups_of({}, dict(beta1=1.0))) == -1 and b"group 1: betas / eps out of range" in err()
        assert call(guarded, groups=groups_of(dict(beta2=-0.1), {})) == -1 and call(guarded, groups=groups_of(dict(eps=-1.0), {})) == -1
        sgd = dict(kind=0, s2=None)
        assert call(guarded, groups=groups_of({}, dict(momentum=0.9, nesterov=1, dampening=0.1)), **sgd) == -1
        assert b"group 1: Nesterov momentum requires" in err()
        assert call(guarded, groups=groups_of(dict(nesterov=1), {}), **sgd) == -1 and b"group 0: Nesterov" in err()
        assert call(guarded, groups=groups_of({}, dict(momentum=-0.5)), **sgd) == -1
        assert call(guarded, groups=groups_of({}, dict(momentum=0.9)), s1=None, **sgd) == -1 and b"needs the momentum buffer" in err()
    assert call(False, step=0) == -1 and b"step counts from 1" in lib.fgcn_last_error()
    # the guard's own arguments
    assert call(True, step=1) == -1 and b"step must be 0" in lib.fgcn_last_error()
    assert call(True, guard=p16 + 4) == -2 and b"8-byte aligned" in lib.fgcn_last_error()
    assert call(True, partials=p16 + 4) == -2
    assert call(True, partials=None) == -1 and b"null partials" in lib.fgcn_last_error()
    assert call(True, guard=None) == -1
    assert call(True, n_partials=2) == -1 and b"n_partials must be 1" in lib.fgcn_last_error()
    assert call(True, max_norm=-1.0) == -1 and call(True, max_norm=float("nan")) == -1 and b"max_norm" in lib.fgcn_last_error()
    assert call(True, sched=None) == -1 and b"null group_sched" in lib.fgcn_last_error()
    assert call(True, sched=p16 + 4) == -2 and b"group_sched must be 8-byte aligned" in lib.fgcn_last_error()
    with pytest.raises(_lib.FgcnError, match="group 1"):
        _lib.check(call(False, groups=groups_of({}, dict(lr=-1.0))), "fgcn_optim_step")


def test_grouped_step_fails_loudly_without_a_gpu():
    """(parameters on the CPU: there is no eager fallback for the grouped path either)"""
    from fusion_gcn_amd.optim import FlatOptimizer
    for kw in (dict(), dict(max_grad_norm=1.0, skip_nonfinite=True)):
        m = group_model()
        opt = FlatOptimizer(three_groups(m), "SGD", 0.1, **kw)
        for p in m.parameters():
            p.grad = torch.ones_like(p)
        with pytest.raises(_lib.FgcnError):
            opt.step()
