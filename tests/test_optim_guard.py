"""The guard of the fused optimizer step (clip by global norm, skip non-finite steps): what can be checked without a GPU -- the
options of FlatOptimizer / create_optimizer, the host-side validation of fgcn_optim_step's guard (it precedes every HIP call) and
the partial-count query.  The arithmetic is checked on the device in tests/test_optim_guard_gpu.py."""
import ctypes as C

import pytest
import torch

from fusion_gcn_amd import _lib, build
from test_optim import small_model


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def test_options_are_attributes_and_not_param_group_entries():
    from fusion_gcn_amd.optim import FlatOptimizer, create_optimizer
    plain = FlatOptimizer(small_model().parameters(), "ADAM", 0.1, weight_decay=0.01)
    assert plain.max_grad_norm is None and plain.skip_nonfinite is False
    opt = FlatOptimizer(small_model().parameters(), "ADAM", 0.1, weight_decay=0.01, max_grad_norm=2.5, skip_nonfinite=True)
    assert opt.max_grad_norm == 2.5 and opt.skip_nonfinite is True
    via = create_optimizer("SGD", small_model(), 0.1, momentum=0.9, max_grad_norm=1, skip_nonfinite=True)
    assert via.max_grad_norm == 1 and via.skip_nonfinite is True
    only_skip = create_optimizer("ADAMW", small_model(), 0.1, skip_nonfinite=True)
    assert only_skip.max_grad_norm is None and only_skip.skip_nonfinite is True
    # the state-dict layout stays torch's: exactly the keys of an optimizer without the options
    assert set(opt.state_dict()["param_groups"][0]) == set(plain.state_dict()["param_groups"][0])
    assert set(opt.state_dict()["param_groups"][0]) == {"lr", "weight_decay", "betas", "eps", "params"}
    assert "max_grad_norm" not in opt.param_groups[0] and "skip_nonfinite" not in opt.param_groups[0]
    assert opt.state_dict()["state"] == {}
    # readable without a device: 0-dim float64 views of one state buffer, allocated with the optimizer
    assert opt.grad_norm.dtype == torch.float64 and opt.grad_norm.dim() == 0 and opt.clip_coef.dtype == torch.float64
    assert opt.grad_norm.data_ptr() == opt._guard.data_ptr() + 8 * _lib.GUARD_NORM
    assert opt.clip_coef.data_ptr() == opt._guard.data_ptr() + 8 * _lib.GUARD_COEF
    assert opt._partials.numel() == _lib.GRAD_NORM_MAX_TILES and opt._partials.dtype == torch.float64
    assert opt.steps == 0 and opt.skipped_steps == 0 and opt.clipped_steps == 0
    opt.max_grad_norm = 0.5                       # may be reassigned between steps
    assert opt.max_grad_norm == 0.5
    opt.max_grad_norm = None
    assert opt.max_grad_norm is None


@pytest.mark.parametrize("bad", [0, 0.0, -1.0, float("nan"), "1.0", [1.0], True])
def test_bad_max_grad_norm_is_a_value_error(bad):
    from fusion_gcn_amd.optim import FlatOptimizer, create_optimizer
    with pytest.raises(ValueError, match="max_grad_norm"):
        FlatOptimizer(small_model().parameters(), "ADAM", 0.1, max_grad_norm=bad)
    with pytest.raises(ValueError, match="max_grad_norm"):
        create_optimizer("SGD", small_model(), 0.1, max_grad_norm=bad)
    opt = FlatOptimizer(small_model().parameters(), "ADAM", 0.1, max_grad_norm=1.0)
    with pytest.raises(ValueError, match="max_grad_norm"):
        opt.max_grad_norm = bad
    assert opt.max_grad_norm == 1.0


def test_state_dict_round_trip_keeps_the_step_count_on_the_guarded_path():
    """load_state_dict writes the count of applied updates into the guard state (here on the CPU: the same tensor code)."""
    from fusion_gcn_amd.optim import FlatOptimizer
    ref_model = small_model()
    ref = torch.optim.Adam(ref_model.parameters(), 0.1)
    for _ in range(3):
        for p in ref_model.parameters():
            p.grad = torch.ones_like(p)
        ref.step()
    opt = FlatOptimizer(small_model().parameters(), "ADAM", 0.1, skip_nonfinite=True)
    opt.load_state_dict(ref.state_dict())
    assert int(opt._guard[_lib.GUARD_STEP]) == 3 and opt.steps == 3
    sd = opt.state_dict()
    assert float(sd["state"][0]["step"]) == 3.0
    assert torch.equal(sd["state"][0]["exp_avg"], ref.state_dict()["state"][0]["exp_avg"])


def test_grad_norm_tiles_is_monotone_and_at_least_one(lib):
    assert lib.fgcn_optim_guard_bytes() == 8 * _lib.GUARD_WORDS
    prev = 0
    for n in [0, 4, 8, 1000, 4092, 4096, 4100, 8192, 8196, 10 ** 5, 10 ** 6, 3_500_000, 2 ** 21, 2 ** 21 + 4, 2 ** 24, 2 ** 31 + 4, 2 ** 40]:
        t = lib.fgcn_grad_norm_tiles(n)
        assert 1 <= t <= _lib.GRAD_NORM_MAX_TILES, (n, t)
        assert t >= prev, (n, t, prev)
        prev = t
    assert lib.fgcn_grad_norm_tiles(4) == 1 and prev == _lib.GRAD_NORM_MAX_TILES
    one = max(n for n in range(4, 1 << 14, 4) if lib.fgcn_grad_norm_tiles(n) == 1)
    assert lib.fgcn_grad_norm_tiles(one + 4) == 2


def test_guarded_step_validates_on_the_host(lib):
    buf = (C.c_double * 64)()
    p = C.addressof(buf)
    p16 = (p + 15) // 16 * 16
    n = 16

    tiles = (C.c_int * 3)(0, n // 4, 0)

    def call(params=p16, grads=p16, s1=p16, s2=p16, n=n, kind=1, lr=0.1, max_norm=1.0, partials=p16, n_partials=None, guard=p16,
             sched=p16, step=0):
        n_partials = lib.fgcn_grad_norm_tiles(n) if n_partials is None else n_partials
        group = (_lib.OptimGroup * 1)(_lib.OptimGroup(lr, 0.0, 0.9, 0.999, 1e-8, 0.0, 0.0, 0))
        return lib.fgcn_optim_step(params, grads, s1, s2, n, kind, group, 1, tiles, 1, 1.0, step,
                                   _lib.OptimGuard(max_norm, 1, n_partials, partials, guard, sched), None)

    assert call(guard=p16 + 4) == -2 and b"8-byte aligned" in lib.fgcn_last_error()           # misaligned state
    assert call(partials=p16 + 4) == -2
    assert call(n=18) == -2 and b"multiple of 4" in lib.fgcn_last_error()                     # n % 4 != 0
    assert call(grads=p16 + 8) == -2                                                          # buffers 16-byte aligned
    assert call(partials=None) == -1 and b"null partials" in lib.fgcn_last_error()            # null partial buffer
    assert call(guard=None) == -1 and b"null partials / guard state" in lib.fgcn_last_error()
    assert call(sched=None) == -1 and b"null group_sched" in lib.fgcn_last_error()
    assert call(sched=p16 + 4) == -2 and b"group_sched must be 8-byte aligned" in lib.fgcn_last_error()
    assert call(step=1) == -1 and b"step must be 0" in lib.fgcn_last_error()                  # the count lives in the guard state
    assert call(params=None) == -1 and b"null pointer" in lib.fgcn_last_error()
    assert call(n_partials=2) == -1 and b"n_partials must be 1" in lib.fgcn_last_error()      # wrong partial count
    assert call(n=8192, n_partials=1) == -1 and b"n_partials must be 2" in lib.fgcn_last_error()
    assert call(max_norm=-1.0) == -1 and b"max_norm" in lib.fgcn_last_error()
    assert call(max_norm=float("nan")) == -1 and b"max_norm" in lib.fgcn_last_error()
    assert call(kind=3) == -1
    assert call(s2=None) == -1 and b"Adam needs" in lib.fgcn_last_error()
    assert call(lr=-0.1) == -1
    with pytest.raises(_lib.FgcnError, match="max_norm"):
        _lib.check(call(max_norm=-2.0), "fgcn_optim_step")


def test_guarded_step_fails_loudly_without_a_gpu():
    """(parameters on the CPU: there is no eager fallback for the guarded path either)"""
    from fusion_gcn_amd.optim import FlatOptimizer
    m = small_model()
    opt = FlatOptimizer(m.parameters(), "SGD", 0.1, max_grad_norm=1.0, skip_nonfinite=True)
    for p in m.parameters():
        p.grad = torch.ones_like(p)
    with pytest.raises(_lib.FgcnError):
        opt.step()
