"""Non-finite values in the kernels' inputs: the class comparison and the poisoned references (a helper module: no test, no conftest).

The contract is the one of include/fgcn.h ("Non-finite values in the inputs") and DESIGN.md section 8l.  Every output element is
classified as finite, NaN, +inf or -inf; "the reference" is the float64 restatement of the kernel run on the same float32-rounded input
with the same non-finite element in it.

  rule 1 ("class"):   elementwise kernels and epilogues give the reference's class at every position;
  rule 3 ("contain"): contractions are non-finite wherever the reference is (NaN against an inf need not match: an inf that went through
                      a bf16 / f16 split is a NaN), and where the reference is finite they are within the unpoisoned tolerance or
                      non-finite -- a finite wrong value is the failure;
  rule 4 (``clean``): inside a mask of positions the poison cannot reach (other samples, rows outside the receptive field) the kernel
                      is finite.  The tolerance check of the jointly finite positions then covers them.

``compare`` counts, per tensor, the elements that meet the rule and the three ways of missing it:
  swallowed -- the reference is non-finite, the kernel returned a finite number (fmaxf(NaN, 0) = 0 is this);
  corrupted -- rule 1: any other class mismatch; rule 3: reference and kernel are finite and the kernel is outside the tolerance;
  spilled   -- a non-finite kernel value inside ``clean``.
The tolerance is the one the unpoisoned test of the same kernel uses, applied as there (relative L2, or a cosine) over the positions
where both sides are finite."""
from __future__ import annotations

import functools
from collections import namedtuple
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

FINITE, NAN, PINF, NINF = 0, 1, 2, 3
CLASS_NAMES = ("finite", "NaN", "+inf", "-inf")
POISONS = {"nan": float("nan"), "+inf": float("inf"), "-inf": float("-inf")}      # by name: NaN != NaN makes a poor cache key

Report = namedtuple("Report", "ok matching swallowed corrupted spilled err message")


def _np(a) -> np.ndarray:
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu()
        a = a.double().numpy() if a.is_floating_point() else a.numpy()
    return np.asarray(a, dtype=np.float64)


def classes(a) -> np.ndarray:
    """the four-way class map of an array or tensor (uint8, same shape)"""
    a = _np(a)
    out = np.zeros(a.shape, dtype=np.uint8)
    out[np.isnan(a)] = NAN
    out[a == np.inf] = PINF
    out[a == -np.inf] = NINF
    return out


def _where(idx: np.ndarray, shape, limit: int = 6) -> str:
    pos = [tuple(int(i) for i in np.unravel_index(int(f), shape)) for f in idx[:limit]]
    return ", ".join(map(str, pos)) + (f", ... ({idx.size} in all)" if idx.size > limit else "")


def compare(got, want, rule: str, tol: Optional[float], where: str = "", clean=None, cosine: bool = False, exact: bool = False) -> Report:
    """``rule``: "class" (rule 1) or "contain" (rule 3).  ``tol``: relative L2 over the jointly finite positions (``cosine``: the least
    cosine instead; ``exact``: bitwise equality of those positions; None: no check of finite values).  ``clean``: boolean mask of positions
    that must be finite (rule 4).  -> Report; ``message`` names the rule, the counts and the first indices of each kind."""
    assert rule in ("class", "contain"), rule
    g, w = _np(got), _np(want)
    assert g.shape == w.shape, (where, g.shape, w.shape)
    cg, cw = classes(g).reshape(-1), classes(w).reshape(-1)
    gf, wf = cg == FINITE, cw == FINITE
    swallowed = ~wf & gf
    if rule == "class":
        corrupted = (cg != cw) & ~swallowed
    else:
        corrupted = np.zeros_like(gf)
    both = gf & wf
    err = 0.0
    if both.any() and (tol is not None or exact):
        a, b = g.reshape(-1)[both], w.reshape(-1)[both]
        d = np.abs(a - b)
        bad = None
        if exact:
            err = float(d.max())
            bad = d != 0
        elif cosine:
            err = float(np.dot(a, b) / (np.linalg.norm(a) * np.linalg.norm(b) + 1e-300))
            if not err >= tol:
                bad = d > np.sqrt(2.0 * (1.0 - tol)) * np.linalg.norm(b) / np.sqrt(b.size)
                if not bad.any():                        # the aggregate decides: without an element to point at, the largest difference
                    bad = d == d.max()
        else:
            den = float(np.linalg.norm(b))
            err = float(np.linalg.norm(d) / den) if den > 0 else float(np.linalg.norm(d))
            if not err < tol:
                bad = d > tol * (den if den > 0 else 1.0) / np.sqrt(b.size)      # the elements above their share of the bound
                if not bad.any():
                    bad = d == d.max()
        if bad is not None and bad.any():
            corrupted = corrupted.copy()
            corrupted[np.flatnonzero(both)[bad]] = True
    spilled = np.zeros_like(gf)
    if clean is not None:
        spilled = np.asarray(clean, dtype=bool).reshape(-1) & ~gf
    miss = swallowed | corrupted | spilled
    counts = dict(matching=int((~miss).sum()), swallowed=int(swallowed.sum()), corrupted=int(corrupted.sum()), spilled=int(spilled.sum()))
    ok = counts["swallowed"] == counts["corrupted"] == counts["spilled"] == 0
    msg = ""
    if not ok:
        parts = [f"{where}: rule {'1 (class at every position)' if rule == 'class' else '3 (never swallow, never corrupt)'} broken: {counts}, "
                 f"finite-position error {err:.3e} against {'bitwise' if exact else tol}"]
        for name, m in (("swallowed", swallowed), ("corrupted", corrupted), ("spilled (rule 4)", spilled)):
            if m.any():
                idx = np.flatnonzero(m)
                f = int(idx[0])
                parts.append(f"  {name} at {_where(idx, g.shape)}: got {g.reshape(-1)[f]!r}, reference {w.reshape(-1)[f]!r}")
        msg = "\n".join(parts)
    return Report(ok, counts["matching"], counts["swallowed"], counts["corrupted"], counts["spilled"], err, msg)


def check(fails: list, *args, **kw) -> Report:
    """``compare``; a miss is appended to ``fails`` (the caller raises them all at once)"""
    rep = compare(*args, **kw)
    if not rep.ok:
        fails.append(rep.message)
    return rep


def put_poison(t: torch.Tensor, index, value: float) -> torch.Tensor:
    """a copy of ``t`` with ``value`` written to one element"""
    t = t.clone()
    t[tuple(index)] = value
    return t


def relu_gate(y: torch.Tensor) -> torch.Tensor:
    """torch's ReLU gate as the backward kernels state it: the gradient passes unless y <= 0, so a NaN output passes it"""
    return ~(y <= 0)


def pack_gate(y: torch.Tensor) -> np.ndarray:
    """the sign image (bit e % 8 of byte e / 8) of a flat channels-last tensor under ``relu_gate``"""
    return np.packbits(relu_gate(y).reshape(-1).numpy(), bitorder="little")


# ---- the block leg --------------------------------------------------------------------------------------------------------------------------
BLOCK_CASES = ("first", "identity64", "down_s2", "static64")
POISONED_SAMPLE = 1      # of block_routes.B = 3


def block_poison(case, value_name: str) -> tuple:
    """(sample, channel, frame, joint, value name): sample 1 of 3, a middle channel, frame and joint"""
    return (POISONED_SAMPLE, case.cin // 2, case.T // 2, case.V // 2, value_name)


@functools.lru_cache(maxsize=None)
def oracle_case(case, phase: str, poison: Optional[tuple] = None) -> dict:
    """block_routes.oracle_case with one element of the input replaced: ``poison`` = (sample, channel, frame, joint, value name of POISONS).
    Without a poison it IS block_routes.oracle_case.  With one: the same input, probe and parameters, and every result kept as the
    oracle gives it, non-finite entries included (no zero-gradient bookkeeping: the class comparison needs none)."""
    import block_routes as R
    if poison is None:
        return R.oracle_case(case, phase)
    from oracle import agcn_oracle as O
    from oracle import relu_masks as RM
    base = R.oracle_case(case, phase)
    b, c, t, v, name = poison
    train = phase == "train"
    blk = R.make_block(case)
    sd = {"l0." + k: (p.detach().double() if p.is_floating_point() else p.detach().clone()) for k, p in blk.state_dict().items()}
    x = base["x"].float().double()             # the float32-rounded input the device gets (BlockRun), then the poison
    x[b, c, t, v] = POISONS[name]
    params = {k: p.clone().requires_grad_(True) for k, p in sd.items()
              if p.is_floating_point() and not k.endswith(("running_mean", "running_var", "adj_a"))}
    live = dict(sd)
    live.update(params)
    xo = x.clone().requires_grad_(True)
    stats, cap = O.Stats(), {}
    out, adj_c = O.st_block(xo, live, "l0", case.stride, case.residual, train, stats if train else None, static_adjacency=case.static, capture=cap)
    grads = torch.autograd.grad((out * base["probe"]).sum(), [xo] + list(params.values()), allow_unused=True)
    return dict(x=x, probe=base["probe"], out=out.detach(), adj_c=None if case.static else torch.stack(adj_c, 1).detach(), dx=grads[0],
                want={k[3:]: g.numpy() for k, g in zip(params.keys(), grads[1:]) if g is not None},
                unused=tuple(k[3:] for k, g in zip(params.keys(), grads[1:]) if g is None),
                stats={k[3:]: s for k, s in stats.updates.items()}, g=cap["l0.g"], o=cap["l0.o"],
                images={n: RM.pack_sign_image(cap[f"l0.{n}"]) for n in RM.RELU_NAMES})


def flips_outside_the_poisoned_sample(signs: Dict[str, np.ndarray], ora: dict, samples: int) -> int:
    """ReLU decisions of a device run that differ from the poisoned oracle's in the samples the poison cannot reach (the images are sample-major:
    a sample owns numel / 8 / samples consecutive bytes): what picks the bound of the un-injected backward, as in tests/test_block_routes_gpu.py"""
    n = 0
    for name, h in signs.items():
        o = ora["images"][name]
        per = h.size // samples
        assert h.size == o.size == per * samples
        for b in range(samples):
            if b != POISONED_SAMPLE:
                n += int(np.unpackbits(np.bitwise_xor(h[b * per:(b + 1) * per], o[b * per:(b + 1) * per])).sum())
    return n


def route_values(entries: Sequence) -> set:
    """the (field, value) pairs of block_routes.ROUTE_TUPLE that the plans of ``entries`` hold"""
    import block_routes as R
    return {(f, getattr(e.plan, f)) for e in entries for f in R.ROUTE_TUPLE}


@functools.lru_cache(maxsize=None)
def covering_subset(mode: str, phase: str) -> tuple:
    """Entries of block_routes.matrix(mode, phase) among BLOCK_CASES such that every value of every ROUTE_TUPLE field that the matrix
    reaches in those cases is run at least once, every case at least once.  Greedy set cover (the entry with the most values still
    missing, ties by matrix order), then entries that became redundant are dropped: small, not proven smallest."""
    import block_routes as R
    pool = [e for e in R.matrix(mode, phase) if e.case.name in BLOCK_CASES and not e.half]
    need = route_values(pool) | {("case", n) for n in BLOCK_CASES}
    have = lambda e: route_values([e]) | {("case", e.case.name)}      # noqa: E731
    chosen, missing = [], set(need)
    while missing:
        best = max(pool, key=lambda e: len(have(e) & missing))
        assert have(best) & missing
        chosen.append(best)
        missing -= have(best)
    for e in list(chosen):
        rest = [o for o in chosen if o is not e]
        if rest and set().union(*(have(o) for o in rest)) >= need:
            chosen = rest
    return tuple(chosen)
