"""The step after the hot path: one fused parameter update over flat buffers.

The reference builds ``torch.optim.{SGD, ASGD, Adam, AdamW}(model.parameters(), lr, **optimizer_args)`` and an optional
``torch.optim.lr_scheduler`` over it (torch_src/session_helper.py:48-89; ADAM + weight_decay 0.01 + ``cawr`` in
config/utd-mhad/skeleton/agcn.yaml:15-22) and calls ``optimizer.step()`` after every batch (session/session.py:176-183):
one small launch chain per parameter tensor, 274 tensors.  ``FlatOptimizer`` keeps that interface -- it *is* a
``torch.optim.Optimizer`` (``param_groups[0]["lr"]``, ``zero_grad``, ``state_dict``; torch's LR schedulers drive it
unchanged) -- but re-homes every trainable parameter into ONE contiguous float32 buffer, shares the flat gradient buffer of
the data-parallel exchange (``dp.FlatGradients``), and applies the update with a single libfgcn launch
(``fgcn_optim_step``, include/fgcn.h) whose arithmetic follows torch's formulas operation by operation.

``max_grad_norm=`` / ``skip_nonfinite=`` put a guard in front of that launch that is decided on the device (the call's
``fgcn_optim_guard``): clipping by the global gradient norm (``torch.nn.utils.clip_grad_norm_`` before ``step()``) and
the skip of a step whose gradients are not finite, which the reference gets from ``GradScaler.step`` in its
``MixedPrecisionStep`` (torch_src/session/procedures/step.py:55-78) -- without a host read per step.

Parameter groups (a list of dicts, as every ``torch.optim.Optimizer`` takes; ``create_optimizer(..., param_groups=[{"match": regex,
...}])`` from a config) keep all of that: the same call and still one update launch, which group an element belongs to comes from a
tile table built and uploaded once at construction (one group: every row names group 0), the groups' scalars travel by value with
every launch.

ASGD (``torch.optim.ASGD``) keeps its product, the averaged iterate ``ax``, in ``state1``; ``FlatOptimizer.averaged()`` evaluates the
model with it.  Its step size ``eta`` and averaging weight ``mu`` are state, computed AFTER a step from that step's ``lr`` and used in
the next one: on the host on the plain path, on the device (``group_sched``) on the guarded one.

No fallback: without libfgcn.so / off gfx950 ``step()`` raises ``FgcnError``.
"""
from __future__ import annotations

import contextlib
import ctypes
import math
import numbers
import re
from typing import Dict, Iterable, List, Optional, Tuple

import torch

from . import _lib
from .dp import FlatGradients

KINDS = {"SGD": 0, "ADAM": 1, "ADAMW": 2, "ASGD": 3}     # FGCN_OPT_* (include/fgcn.h); names as in session_helper.available_optimizers
MAX_GROUPS = _lib.OPT_MAX_GROUPS              # FGCN_OPT_MAX_GROUPS


class FlatOptimizer(torch.optim.Optimizer):
    """``FlatOptimizer(model.parameters(), "ADAM", lr, weight_decay=0.01)`` == ``create_optimizer("ADAM", model, lr, ...)``.

    Supported ``optimizer_args`` (torch names and defaults): SGD ``momentum, dampening, weight_decay, nesterov``;
    ADAM / ADAMW ``betas, eps, weight_decay`` (AdamW's default decay is 0.01); ASGD ``lambd, alpha, t0, weight_decay``.
    ``amsgrad`` / ``maximize`` are not built (the reference does not use them) and raise.
    ``params``: an iterable of parameters, or torch's list of group dicts -- ``{"params": [...], "lr": ..., "weight_decay": ...}`` with
    any of the kind's scalars above as overrides; one kind for all groups, at most ``MAX_GROUPS`` (8) of them.  The groups are final:
    ``add_param_group`` on a built optimizer raises (it would have to re-home parameters into live flat buffers).  The order of the
    flat buffers is the order of the ``FlatGradients`` in use -- the concatenation of the groups for the optimizer's own, the model's
    order for a shared one, where the groups interleave; ``_group_of`` maps every tensor to its group.
    ``grads``: an existing ``FlatGradients`` over the trainable parameters of all groups (the data-parallel buffer) to share.
    ``allow_unused``: a trainable parameter without a gradient in a step counts as a zero gradient instead of an error
    (forwarded to the FlatGradients this optimizer creates).

    The guard (both off by default: the plain launch, a host-side step count).  They are attributes of the optimizer, not entries
    of ``param_groups``: the state dict keeps torch's layout.  With several groups the norm is still the global one over all of them
    (``clip_grad_norm_(model.parameters())``), a skipped step skips every group, and there is one step count.
    ``max_grad_norm``: clip by the global norm of the gradient the update applies (``grad_scale`` included), that is
    ``g *= min(1, max_grad_norm / (norm + 1e-6))`` before weight decay is added -- ``clip_grad_norm_`` followed by ``step()``,
    with the norm and the coefficient in float64 (gradients of 1e30 have a finite norm and are clipped; torch's float32 norm
    overflows there).  May be reassigned between steps.
    ``skip_nonfinite``: a step whose gradient norm is inf or NaN leaves the parameters, the moments and the step count
    untouched and counts in ``skipped_steps``.
    The norm, the decision, the step count and Adam's bias corrections are computed on the device; ``step()`` makes no
    synchronising call.  ``grad_norm`` / ``clip_coef`` are 0-dim float64 device tensors (views of the guard state; reading
    the attribute never waits for the device).  ``steps``, ``skipped_steps`` and ``clipped_steps`` read device counters and
    DO wait for the device.  An optimizer that took the guarded path once keeps taking it (its step count lives on the device).
    Data-parallel runs: ``Step.run_optimizer_step`` all-reduces before it calls ``step()``, so every rank sees the same averaged
    buffer, computes the same bits from it (the sum has a fixed order) and takes the same decision.
    """

    def __init__(self, params: Iterable[torch.nn.Parameter], name: str = "ADAM", lr: float = 1e-3, *,
                 grads: Optional[FlatGradients] = None, allow_unused: bool = False, max_grad_norm: Optional[float] = None,
                 skip_nonfinite: bool = False, **optimizer_args):
        kind = name.upper()
        _check_max_grad_norm(max_grad_norm)
        if kind not in KINDS:
            raise ValueError("Unsupported optimizer: " + kind + " (SGD | ASGD | ADAM | ADAMW)")
        if optimizer_args.get("amsgrad") or optimizer_args.get("maximize"):
            raise NotImplementedError("amsgrad / maximize are not built")
        defaults = dict(lr=lr, weight_decay=0.01 if kind == "ADAMW" else 0.0)
        if kind == "SGD":
            defaults.update(momentum=0.0, dampening=0.0, nesterov=False)
        elif kind == "ASGD":
            defaults.update(lambd=1e-4, alpha=0.75, t0=1e6)
        else:
            defaults.update(betas=(0.9, 0.999), eps=1e-8)
        unknown = set(optimizer_args) - set(defaults) - {"amsgrad", "maximize"}
        if unknown:
            raise TypeError(f"{kind}: unexpected optimizer_args {sorted(unknown)}")
        defaults.update({k: v for k, v in optimizer_args.items() if k in defaults})
        _check_group(kind, defaults)
        params = list(params)
        if params and isinstance(params[0], dict):
            if len(params) > MAX_GROUPS:
                raise ValueError(f"FlatOptimizer takes at most {MAX_GROUPS} parameter groups (FGCN_OPT_MAX_GROUPS), got {len(params)}")
            for i, group in enumerate(params):
                if group.get("amsgrad") or group.get("maximize"):
                    raise NotImplementedError("amsgrad / maximize are not built")
                unknown = set(group) - set(defaults) - {"params", "amsgrad", "maximize"}
                if unknown:
                    raise TypeError(f"{kind}: unexpected optimizer_args {sorted(unknown)} in parameter group {i}")
            params = [{k: v for k, v in group.items() if k not in ("amsgrad", "maximize")} for group in params]
        self._built = False
        super().__init__(params, defaults)      # (calls add_param_group once per group; a parameter in two groups is torch's error)
        for group in self.param_groups:
            _check_group(kind, group)
        self._built = True
        self.kind = kind
        every = [p for group in self.param_groups for p in group["params"]]
        self.grads = grads if grads is not None else FlatGradients(every, allow_unused=allow_unused)
        self.params = self.grads.params                      # trainable parameters, in the order of the flat buffers
        if len(self.param_groups) == 1:
            if grads is not None and [id(p) for p in self.params] != [id(p) for p in every if p.requires_grad]:
                raise ValueError("the shared FlatGradients must cover the same parameters in the same order")
        elif grads is not None and sorted(id(p) for p in self.params) != sorted(id(p) for p in every if p.requires_grad):
            raise ValueError("the shared FlatGradients must cover exactly the trainable parameters of all groups")
        group_index = {id(p): i for i, group in enumerate(self.param_groups) for p in group["params"]}
        self._group_of: List[int] = [group_index[id(p)] for p in self.params]       # per tensor of the flat buffers
        # one contiguous home for the parameter values, laid out like the gradient buffer (16-byte aligned views)
        self.flat = torch.zeros_like(self.grads.flat)
        with torch.no_grad():
            for p, gv in zip(self.params, self.grads.views):
                off = gv.storage_offset()
                home = self.flat[off:off + p.numel()].view_as(p)
                home.copy_(p)
                p.data = home
        need1 = kind != "SGD" or any(group["momentum"] != 0 for group in self.param_groups)
        self.state1 = torch.zeros_like(self.flat) if need1 else None       # momentum buffer / exp_avg / ASGD's ax
        self.state2 = torch.zeros_like(self.flat) if kind in ("ADAM", "ADAMW") else None   # exp_avg_sq
        self._steps = 0           # the host-side count of the unguarded path
        self.grad_scale = 1.0     # set to 1/world when the flat gradients hold an un-averaged all-reduce sum
        # the guard's state (enum fgcn_guard_word) and the partial sums of the norm: allocated once, zero = reset
        self._guard = torch.zeros(_lib.GUARD_WORDS, dtype=torch.int64, device=self.flat.device)
        self._partials = torch.zeros(_lib.GRAD_NORM_MAX_TILES, dtype=torch.float64, device=self.flat.device)
        self.grad_norm = self._guard.view(torch.float64)[_lib.GUARD_NORM]
        self.clip_coef = self._guard.view(torch.float64)[_lib.GUARD_COEF]
        self.skip_nonfinite = bool(skip_nonfinite)
        self._max_grad_norm = max_grad_norm
        self._guarded = max_grad_norm is not None or self.skip_nonfinite
        # the element-to-group table and the per-group step sizes of the guarded form, built and uploaded ONCE
        self._tiles = torch.tensor(self.tile_table(), dtype=torch.int32).to(self.flat.device)
        self._sched = torch.zeros((4 if kind == "ASGD" else 2) * MAX_GROUPS, dtype=torch.float64, device=self.flat.device)
        # ASGD: (eta, mu) of the NEXT step per group, float32 values; None until the first step takes eta = lr.  On the guarded path
        # they live in _sched ({eta_use, mu_use, eta_next, mu_next} per group), written once when the path is entered
        self._eta_mu: Optional[List[Tuple[float, float]]] = None
        self._sched_seeded = False
        self._averaging = False

    def add_param_group(self, param_group) -> None:
        if getattr(self, "_built", False):
            raise NotImplementedError("FlatOptimizer must be built with its final parameter groups: add_param_group on a built "
                                      "optimizer would re-home parameters into live flat buffers, which is not built")
        super().add_param_group(param_group)

    def tile_table(self, tile4: int = _lib.OPT_TILE4) -> List[List[int]]:
        """Rows ``[start4, count4, group]`` of fgcn_optim_step's table (units: 16-byte groups of the flat buffers): runs of
        consecutive tensors of one group, cut into rows of at most ``tile4``.  A tensor's last 16-byte group carries its <= 3 floats
        of alignment padding, so the rows cover the buffers exactly once."""
        runs: List[List[int]] = []
        for p, v, gi in zip(self.params, self.grads.views, self._group_of):
            start4, count4 = v.storage_offset() // 4, (p.numel() + 3) // 4
            if runs and runs[-1][2] == gi and runs[-1][0] + runs[-1][1] == start4:
                runs[-1][1] += count4
            else:
                runs.append([start4, count4, gi])
        return [[s + o, min(tile4, c - o), gi] for s, c, gi in runs for o in range(0, c, tile4)]

    @property
    def max_grad_norm(self) -> Optional[float]:
        return self._max_grad_norm

    @max_grad_norm.setter
    def max_grad_norm(self, value: Optional[float]) -> None:
        _check_max_grad_norm(value)
        self._max_grad_norm = value
        if value is not None:
            self._enter_guarded()

    def _enter_guarded(self) -> None:
        """The step count moves to the device (one fill, no wait) and stays there."""
        if not self._guarded:
            self._guard[_lib.GUARD_STEP].fill_(self._steps)
            self._guarded = True
            if self.kind == "ASGD":
                self._write_sched()

    @property
    def steps(self) -> int:
        """Updates applied so far.  On the guarded path this reads the device counter: it waits for the device."""
        return int(self._guard[_lib.GUARD_STEP].item()) if self._guarded else self._steps

    @steps.setter
    def steps(self, value: int) -> None:
        self._steps = int(value)
        if self._guarded:
            self._guard[_lib.GUARD_STEP].fill_(int(value))

    @property
    def skipped_steps(self) -> int:
        """Steps the guard skipped (gradient norm not finite).  Reads a device counter: it waits for the device."""
        return int(self._guard[_lib.GUARD_SKIPPED].item())

    @property
    def clipped_steps(self) -> int:
        """Applied steps whose clip coefficient was below 1.  Reads a device counter: it waits for the device."""
        return int(self._guard[_lib.GUARD_CLIPPED].item())

    # ---- ASGD: eta / mu and the averaged iterate ------------------------------------------------------------------------------
    def _write_sched(self) -> None:
        """The host's (eta, mu) -- or (lr, 1) before the first step -- into group_sched's ``next`` pair (and ``use``, which the decision
        launch overwrites before the update reads it).  One small copy, stream-ordered."""
        pairs = self._eta_mu or [(_f32(g["lr"]), 1.0) for g in self.param_groups]
        rows = [[eta, mu, eta, mu] for eta, mu in pairs] + [[0.0] * 4] * (MAX_GROUPS - len(pairs))
        self._sched.copy_(torch.tensor(rows, dtype=torch.float64).reshape(-1))
        self._sched_seeded = True

    def _read_eta_mu(self) -> List[Tuple[float, float]]:
        """(eta, mu) the next step will use, per group.  On the guarded path this reads the device: it waits for it."""
        if self._guarded and self._sched_seeded:
            rows = self._sched.view(MAX_GROUPS, 4)[:len(self.param_groups), 2:].cpu().tolist()
            return [(eta, mu) for eta, mu in rows]
        return list(self._eta_mu or [(_f32(g["lr"]), 1.0) for g in self.param_groups])

    @contextlib.contextmanager
    def averaged(self):
        """``with optimizer.averaged(): session.validate_epoch(...)`` -- evaluate with ASGD's averaged iterate ``ax`` (torch keeps it in
        the optimizer state and offers no way to use it).  Inside the context every trainable parameter aliases its view of ``ax``
        instead of its home in ``flat``: a swap of ``p.data``, no copy and no launch; the tensor versions are bumped on entry and on
        exit, so the blocks' packed-weight caches refresh both ways.  ``step()`` inside raises ``RuntimeError``; so does entering before
        the first applied step (``ax`` is still zeros; on the guarded path this check reads the device counter), ``TypeError`` for
        another kind.  Only parameters are averaged: BatchNorm running statistics are buffers, ASGD keeps no average of them, and the
        model evaluates with the statistics of the last iterate."""
        if self.kind != "ASGD":
            raise TypeError(f"averaged() is ASGD's averaged iterate; this optimizer is {self.kind}")
        if self._averaging:
            raise RuntimeError("averaged() is already active")
        if self.steps == 0:
            raise RuntimeError("averaged() before the first applied step: ax is still zeros")
        self._check_homes()
        homes = [p.data for p in self.params]
        self._averaging = True
        try:
            for p, ax in zip(self.params, self._views(self.state1)):
                p.data = ax
                torch.autograd.graph.increment_version(p)
            yield self
        finally:
            for p, home in zip(self.params, homes):
                p.data = home
                torch.autograd.graph.increment_version(p)
            self._averaging = False

    def zero_grad(self, set_to_none: bool = True) -> None:
        if set_to_none:
            self.grads.zero()
        else:
            self.grads.zero_in_place()

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self._averaging:
            raise RuntimeError("FlatOptimizer.step inside averaged(): the parameters alias ax, the averaged iterate")
        self._check_homes()
        self.grads.gather()                   # p.grad -> the flat buffer (no copy when they already are views of it)
        lib = _lib.load()
        if not self.flat.is_cuda:
            raise _lib.FgcnError("FlatOptimizer.step needs the parameters on an MI355X (no CPU fallback)")
        if self.skip_nonfinite:
            self._enter_guarded()
        s1 = self.state1.data_ptr() if self.state1 is not None else None
        s2 = self.state2.data_ptr() if self.state2 is not None else None
        n = self.flat.numel()
        asgd = self.kind == "ASGD"
        if asgd and self._guarded:
            if not self._sched_seeded:         # (built guarded: eta = the lr of the first step() call)
                self._write_sched()
        elif asgd and self._eta_mu is None:
            self._eta_mu = [(_f32(g["lr"]), 1.0) for g in self.param_groups]
        pairs = self._eta_mu if asgd and not self._guarded else [None] * len(self.param_groups)
        groups = (_lib.OptimGroup * len(self.param_groups))(*[_group_scalars(g, em) for g, em in zip(self.param_groups, pairs)])
        guard = None
        if self._guarded:         # norm -> decision -> update, stream-ordered; the step count is the device's
            guard = _lib.OptimGuard(float(self._max_grad_norm or 0.0), int(self.skip_nonfinite), lib.fgcn_grad_norm_tiles(n),
                                    self._partials.data_ptr(), self._guard.data_ptr(), self._sched.data_ptr())
        else:
            self._steps += 1
        # one launch over the tile table; the groups' scalars by value
        rc = lib.fgcn_optim_step(self.flat.data_ptr(), self.grads.flat.data_ptr(), s1, s2, n, KINDS[self.kind], groups, len(groups),
                                 self._tiles.data_ptr(), self._tiles.shape[0], float(self.grad_scale),
                                 0 if self._guarded else self._steps, guard, torch.cuda.current_stream(self.flat.device).cuda_stream)
        _lib.check(rc, "fgcn_optim_step")
        if asgd and not self._guarded:     # torch computes the next step's eta / mu after the update, from this step's lr
            self._eta_mu = [_asgd_next(g, self._steps) for g in self.param_groups]
        # the kernel wrote through raw pointers: tell autograd (and everything keyed on tensor versions, like the blocks'
        # cache of packed weights) that every parameter changed in place -- metadata only, no launches
        for p in self.params:
            torch.autograd.graph.increment_version(p)
        return loss

    def _check_homes(self) -> None:
        """Every parameter must still live in the flat buffer: a later model.to() / .float() / load_state_dict(assign=True) /
        ``p.data = ...`` gives it new storage, and the fused update would then train an orphaned copy while the model's weights
        stay frozen.  Pointer comparisons only (no launches).  Create the optimizer after the model's final .to() / cast."""
        base = self.flat.data_ptr()
        for p, v in zip(self.params, self.grads.views):
            if p.data_ptr() != base + 4 * v.storage_offset():
                raise _lib.FgcnError("FlatOptimizer: a parameter no longer aliases the flat parameter buffer (the model was moved, "
                                     "cast or re-assigned after the optimizer was created); build the optimizer after the final "
                                     ".to() / cast")

    # ---- torch.optim state-dict layout (per-parameter entries are views of the flat state) ---------------------------------
    def _views(self, flat: torch.Tensor):
        return [flat[v.storage_offset():v.storage_offset() + p.numel()].view_as(p) for p, v in zip(self.params, self.grads.views)]

    def _slots(self):
        """Position of every trainable parameter in the concatenation of the groups' ``"params"`` -- torch's state index (frozen
        parameters keep their slot, stateless)."""
        where = {id(p): i for i, p in enumerate(p for group in self.param_groups for p in group["params"])}
        return [where[id(p)] for p in self.params]

    def state_dict(self) -> Dict:
        """Same layout as the torch optimizer of that name over the same groups: {"state": {i: {...}}, "param_groups": [...]}, the
        groups' ``"params"`` consecutive indices, the state keyed by them.  ``step`` is the count of APPLIED updates (on the guarded
        path the device counter: skipped steps do not count, as in torch after GradScaler.step)."""
        state = {}
        steps = self.steps
        if steps:
            s1 = self._views(self.state1) if self.state1 is not None else None
            s2 = self._views(self.state2) if self.state2 is not None else None
            eta_mu = self._read_eta_mu() if self.kind == "ASGD" else None
            for i, slot in enumerate(self._slots()):      # torch's layout: state index = position over all groups' "params"
                if self.kind == "ASGD":
                    eta, mu = eta_mu[self._group_of[i]]
                    state[slot] = {"step": torch.tensor(float(steps)), "eta": torch.tensor(eta), "mu": torch.tensor(mu),
                                   "ax": s1[i].clone()}
                elif self.kind == "SGD":
                    if s1 is None:
                        state[slot] = {"momentum_buffer": None}
                    elif self.param_groups[self._group_of[i]]["momentum"] != 0:      # (torch keeps no state without a momentum)
                        state[slot] = {"momentum_buffer": s1[i].clone()}
                else:
                    state[slot] = {"step": torch.tensor(float(steps)), "exp_avg": s1[i].clone(), "exp_avg_sq": s2[i].clone()}
        groups, first = [], 0
        for g in self.param_groups:
            group = {k: v for k, v in g.items() if k != "params"}
            group["params"] = list(range(first, first + len(g["params"])))
            first += len(g["params"])
            groups.append(group)
        return {"state": state, "param_groups": groups}

    def load_state_dict(self, sd: Dict) -> None:
        if len(sd["param_groups"]) != len(self.param_groups):
            raise ValueError("loaded state dict has a different number of parameter groups")
        for mine, group in zip(self.param_groups, sd["param_groups"]):
            if len(group["params"]) != len(mine["params"]):
                raise ValueError("loaded state dict contains a parameter group that doesn't match the size of optimizer's group")
            for k, v in group.items():
                if k != "params":
                    mine[k] = v
        st = sd.get("state", {})
        steps = 0
        eta_mu: Dict[int, Tuple[float, float]] = {}
        if st:
            s1 = self._views(self.state1) if self.state1 is not None else None
            s2 = self._views(self.state2) if self.state2 is not None else None
            with torch.no_grad():
                for i, slot in enumerate(self._slots()):
                    e = st[slot] if slot in st else st.get(str(slot))
                    if self.kind == "ASGD":
                        s1[i].copy_(e["ax"])
                        steps = int(e["step"])
                        eta_mu.setdefault(self._group_of[i], (_f32(float(e["eta"])), _f32(float(e["mu"]))))
                    elif self.kind == "SGD":
                        if s1 is not None and e is not None and e.get("momentum_buffer") is not None:
                            s1[i].copy_(e["momentum_buffer"])
                            steps = max(steps, 1)
                    else:
                        s1[i].copy_(e["exp_avg"])
                        s2[i].copy_(e["exp_avg_sq"])
                        steps = int(e["step"])
        self.steps = steps          # (guarded: written to the device counter)
        if self.kind == "ASGD":     # a group without trainable tensors has no entry: what torch would have computed for it
            self._eta_mu = [eta_mu.get(i, _asgd_next(g, steps)) for i, g in enumerate(self.param_groups)] if steps else None
            if self._guarded:
                self._write_sched()


def _check_group(kind: str, group: Dict) -> None:
    """The range checks of one group's scalars (the defaults are a group too)."""
    if group["lr"] < 0 or group["weight_decay"] < 0:
        raise ValueError("negative lr / weight_decay")
    if kind == "SGD" and group["nesterov"] and (group["momentum"] <= 0 or group["dampening"] != 0):
        raise ValueError("Nesterov momentum requires a momentum and zero dampening")
    if kind == "ASGD" and not (group["lambd"] >= 0 and math.isfinite(group["alpha"]) and math.isfinite(group["t0"])):
        raise ValueError("ASGD: lambd must be >= 0, alpha and t0 finite")


def _f32(x: float) -> float:
    """x rounded through float32, as a value stored in one of torch's float32 state tensors."""
    return ctypes.c_float(x).value


def _asgd_next(g: Dict, step: int) -> Tuple[float, float]:
    """(eta, mu) for the step after the one that made the count ``step``, from that step's lr: torch/optim/asgd.py's new_eta / new_mu,
    Python doubles rounded through float32."""
    lr, step = float(g["lr"]), float(step)
    return _f32(lr / ((1 + g["lambd"] * lr * step) ** g["alpha"])), _f32(1 / max(1, step - g["t0"]))


def _group_scalars(g: Dict, eta_mu: Optional[Tuple[float, float]] = None) -> _lib.OptimGroup:
    if "lambd" in g:      # ASGD: lambd, alpha, t0 in the slots beta1, beta2, eps; the step's eta, mu in momentum, dampening
        eta, mu = eta_mu or (0.0, 0.0)       # (the guarded form reads them from group_sched)
        return _lib.OptimGroup(float(g["lr"]), float(g["weight_decay"]), float(g["lambd"]), float(g["alpha"]), float(g["t0"]),
                               eta, mu, 0)
    b1, b2 = g.get("betas", (0.0, 0.0))
    return _lib.OptimGroup(float(g["lr"]), float(g["weight_decay"]), float(b1), float(b2), float(g.get("eps", 0.0)),
                           float(g.get("momentum", 0.0)), float(g.get("dampening", 0.0)), int(bool(g.get("nesterov", False))))


def _check_max_grad_norm(value) -> None:
    if value is None:
        return
    if isinstance(value, bool) or not isinstance(value, numbers.Real) or math.isnan(value) or value <= 0:
        raise ValueError(f"max_grad_norm must be a positive number or None (got {value!r})")


def groups_from_rules(model: torch.nn.Module, rules) -> List[Dict]:
    """``param_groups=`` of a config -> torch's list of group dicts.  Every rule is ``{"match": regex, <overrides>}``; a parameter joins
    the FIRST rule whose regex ``re.search``es its ``named_parameters()`` name, the unmatched ones form the first group with the
    defaults.  A rule that matches nothing is an error (a typo would otherwise train with the defaults, silently)."""
    rules = [dict(r) for r in rules]
    for r in rules:
        if "match" not in r:
            raise ValueError(f"param_groups: a rule needs a \"match\" regex (got {r!r})")
    rest, matched = [], [[] for _ in rules]
    for name, p in model.named_parameters():
        hit = next((i for i, r in enumerate(rules) if re.search(r["match"], name)), None)
        (rest if hit is None else matched[hit]).append(p)
    for r, ps in zip(rules, matched):
        if not ps:
            raise ValueError(f"param_groups: the rule {r['match']!r} matches no parameter of the model")
    groups = [{"params": rest}] if rest else []
    return groups + [dict({k: v for k, v in r.items() if k != "match"}, params=ps) for r, ps in zip(rules, matched)]


def create_optimizer(name: str, model: torch.nn.Module, lr: float, **optimizer_args) -> FlatOptimizer:
    """Signature of the reference's session_helper.create_optimizer (torch_src/session_helper.py:80-84); ``max_grad_norm`` and
    ``skip_nonfinite`` travel in ``optimizer_args`` like every other option of the config, and so does ``param_groups``: a list of
    ``{"match": regex, <overrides>}`` rules (``groups_from_rules``), e.g.
    ``[{"match": r"bn\\.|bias$|adj_b$", "weight_decay": 0.0}, {"match": r"^fc\\.", "lr": 0.01}]``."""
    rules = optimizer_args.pop("param_groups", None)
    if rules is None:
        return FlatOptimizer(model.parameters(), name, lr, **optimizer_args)
    return FlatOptimizer(groups_from_rules(model, rules), name, lr, **optimizer_args)
