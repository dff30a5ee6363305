"""Shift-GCN (Cheng et al., CVPR 2020) restated in float64 torch (a helper module: no test, no conftest).  Nothing here calls a kernel of
fusion_gcn_amd.

Each of the two shift operations is written twice: ``joint_shift_cl`` / ``frame_shift_cl`` channels-last from the formulas of
include/fgcn.h ("Shift graph convolution"), and ``joint_shift_nchw`` / ``frame_shift_nchw``, the literal NCHW composition: ``index_select``
over the flattened (V C) axis with the tables (i C + j + j C) mod (V C) and (i C + j - j C) mod (V C), and an explicit zero-padded gather
and lerp per channel for the frame shift.  The unit, the block and the model are plain torch modules with the product's state-dict keys, so
a product state dict loads into them.

The salt rule, ``KINK_EPS``, ``COND_MAX``, ``MAX_SALT`` and ``FLIP_CAP`` are tests/ctrgcn_ref.py's (tests/test_msg3d.py's convention).  A
case's input is the first filler salt for which the float64 reference ALONE meets both conditions:
  * every ReLU pre-activation is at least ``KINK_EPS`` from zero, so float32 has no decision to flip;
  * no ``ypos`` / ``Feature_Mask`` gradient is the residue of a sum that cancels more than ``COND_MAX``-fold.
The condition number of a gradient VECTOR that is compared in relative L2 is ||a|| / ||g|| with g[c] = sum of the terms of entry c and
a[c] = sum of their magnitudes: a float32 sum of entry c errs by about eps a[c], so the vector's relative L2 error is eps ||a|| / ||g||.  The
terms are the sums a workgroup hands on at the least: per (sample, joint) for ``ypos``, per row (b, t) for ``Feature_Mask``.
The kernels never decide which input is used."""
from __future__ import annotations

import functools
import math
from collections import namedtuple

import numpy as np
import torch
import torch.nn as nn

from ctrgcn_ref import COND_MAX, FLIP_CAP, KINK_EPS, MAX_SALT, layer_plan, tag_of  # noqa: F401  (re-exported)
from oracle import filler

K_LIMIT = float(1 << 26)          # the clamp of floor(pos) stated in include/fgcn.h


# ---- the joint shift, twice -------------------------------------------------------------------------------------------------------------
def joint_shift_cl(x, mask=None, direction: int = 1):
    """x (B, T, V, C), mask None or V C elements -> out[r, v, c] = x[r, (v + direction c) mod V, c] (tanh(mask[v, c]) + 1)"""
    B, T, V, C = x.shape
    src = (torch.arange(V)[:, None] + direction * torch.arange(C)[None, :]) % V          # (python's % : the true modulo)
    out = torch.gather(x, 2, src.expand(B, T, V, C))
    if mask is not None:
        out = out * (torch.tanh(mask.reshape(V, C)) + 1)
    return out


def shift_table(V: int, C: int, direction: int):
    """upstream's index table: position i C + j reads (i C + j + direction j C) mod (V C)"""
    return torch.tensor([(i * C + j + direction * j * C) % (V * C) for i in range(V) for j in range(C)], dtype=torch.long)


def joint_shift_nchw(x, mask=None, direction: int = 1):
    """the literal composition: x (N, C, T, V) -> (N, C, T, V)"""
    n, c, t, v = x.shape
    y = x.permute(0, 2, 3, 1).contiguous().view(n * t, v * c)
    y = torch.index_select(y, 1, shift_table(v, c, direction)).view(n * t, v, c)
    if mask is not None:
        y = y * (torch.tanh(mask.reshape(1, v, c)) + 1)
    return y.view(n, t, v, c).permute(0, 3, 1, 2)


# ---- the frame shift, twice -------------------------------------------------------------------------------------------------------------
def out_frames(T: int, stride: int) -> int:
    return (T - 1) // stride + 1


def frame_shift_cl(x, pos, stride: int = 1, relu: bool = False):
    """x (B, T, V, C), pos (C) [or (B, V, C): one copy per (sample, joint), for the terms of its gradient] ->
    out[b, to, v, c] = (1 - f) tap(to s + k) + f tap(to s + k + 1), k = floor(pos) held constant, f = pos - k"""
    B, T, V, C = x.shape
    T_out = out_frames(T, stride)
    p = pos.view(1, 1, 1, C) if pos.numel() == C else pos.view(B, 1, V, C)
    kf = torch.floor(p.detach())
    f = p - kf
    k = torch.nan_to_num(kf, nan=-K_LIMIT).clamp(-K_LIMIT, K_LIMIT).long()
    phi = torch.relu(x) if relu else x
    to = torch.arange(T_out).view(1, T_out, 1, 1) * stride

    def tap(t):
        t = t.expand(B, T_out, V, C)
        inside = (t >= 0) & (t < T)
        return torch.where(inside, torch.gather(phi, 1, t.clamp(0, T - 1)), torch.zeros((), dtype=x.dtype))
    return (1 - f) * tap(to + k) + f * tap(to + k + 1)


def frame_shift_nchw(x, pos, stride: int = 1, relu: bool = False):
    """the explicit gather and lerp, channel by channel: x (N, C, T, V) -> (N, C, T_out, V)"""
    n, c, t, v = x.shape
    t_out = out_frames(t, stride)
    pad = t + 2
    outs = []
    for j in range(c):
        xj = torch.relu(x[:, j]) if relu else x[:, j]                                     # (N, T, V)
        pj = float(pos[j].detach())
        kf = math.floor(pj) if math.isfinite(pj) else (K_LIMIT if pj > 0 else -K_LIMIT)
        kf = max(-K_LIMIT, min(K_LIMIT, kf))
        f = pos[j] - (math.floor(pj) if math.isfinite(pj) else pj)
        if -(t + 1) <= kf <= t:
            xp = torch.nn.functional.pad(xj, (0, 0, pad, pad))
            idx = torch.arange(t_out) * stride + int(kf) + pad
            lo, hi = xp[:, idx], xp[:, idx + 1]
        else:                                                                            # both taps are outside the clip for every frame
            lo = hi = torch.zeros((n, t_out, v), dtype=x.dtype)
        outs.append((1 - f) * lo + f * hi)
    return torch.stack(outs, 1)


def cond_of(terms: torch.Tensor) -> float:
    """``terms`` (n, ...): n terms per entry of a gradient -> ||sum |terms||| / ||sum terms|| (the module docstring)"""
    g, a = terms.sum(0), terms.abs().sum(0)
    return float(a.norm() / g.norm()) if float(g.norm()) > 0 else math.inf


# ---- unit, block, model on plain torch modules (NCHW) -----------------------------------------------------------------------------------
class Capture:
    """what a reference run records: the least |ReLU pre-activation|, every ReLU's decisions, the per-term copies of ypos / Feature_Mask"""
    active = None

    def __init__(self):
        self.least, self.near, self.total = math.inf, 0, 0
        self.decisions, self.terms = [], []
        self.forced, self.flips, self.close = None, 0, 0.0

    def force(self, masks):
        """the ReLUs that follow take these decisions (one bool NCHW tensor per ReLU, in forward order) instead of their own; ``flips``
        counts the decisions that differ from the reference's own, ``close`` is the largest |pre-activation| among those"""
        self.forced = list(masks)
        return self

    def __enter__(self):
        Capture.active = self
        return self

    def __exit__(self, *exc):
        Capture.active = None

    def expand(self, p, shape):
        """``p`` broadcast to ``shape`` (leading axes = the terms) as a tensor of the graph whose gradient holds the terms"""
        e = p.expand(shape).clone()
        e.retain_grad()
        self.terms.append(e)
        return e

    def conds(self) -> list:
        return [cond_of(e.grad.reshape(-1, *e.shape[-2:]) if e.dim() == 4 else e.grad.reshape(-1, e.shape[-1])) for e in self.terms]

    def cond(self) -> float:
        return max(self.conds(), default=1.0)


class KinkReLU(nn.Module):
    def forward(self, x):
        cap = Capture.active
        if cap is not None:
            mag = x.detach().abs()
            cap.least, cap.near, cap.total = min(cap.least, float(mag.min())), cap.near + int((mag < KINK_EPS).sum()), cap.total + mag.numel()
            cap.decisions.append(x.detach() > 0)
            if cap.forced is not None:
                mask = cap.forced.pop(0)
                assert mask.shape == x.shape, (tuple(mask.shape), tuple(x.shape))
                differ = mask != (x.detach() > 0)
                if bool(differ.any()):
                    cap.flips, cap.close = cap.flips + int(differ.sum()), max(cap.close, float(mag[differ].max()))
                return x * mask.to(x.dtype)
        return torch.relu(x)


def _cl(t):
    return t.permute(0, 2, 3, 1)


def _nchw(t):
    return t.permute(0, 3, 1, 2)


class RefShiftGCN(nn.Module):
    def __init__(self, cin, cout, V):
        super().__init__()
        self.Linear_weight = nn.Parameter(torch.zeros(cin, cout))
        self.Linear_bias = nn.Parameter(torch.zeros(1, 1, cout))
        self.Feature_Mask = nn.Parameter(torch.zeros(1, V, cin))
        self.bn = nn.BatchNorm1d(V * cout)
        self.down = nn.Sequential(nn.Conv2d(cin, cout, 1), nn.BatchNorm2d(cout)) if cin != cout else None
        self.relu = KinkReLU()

    def forward(self, x0):
        n, c, t, v = x0.shape
        x = _cl(x0)
        mask = self.Feature_Mask
        if Capture.active is not None:
            mask = Capture.active.expand(self.Feature_Mask.view(1, 1, v, c), (n, t, v, c))
            s = joint_shift_cl(x, None, 1) * (torch.tanh(mask) + 1)
        else:
            s = joint_shift_cl(x, mask, 1)
        z = s @ self.Linear_weight + self.Linear_bias.view(1, 1, 1, -1)
        y = joint_shift_cl(z, None, -1)
        y = self.bn(y.reshape(n * t, -1)).view(n, t, v, -1)
        return self.relu(_nchw(y) + (x0 if self.down is None else self.down(x0)))


class RefShift(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.ypos = nn.Parameter(torch.zeros(c))

    def forward(self, x, stride=1):
        n, c, t, v = x.shape
        pos = self.ypos if Capture.active is None else Capture.active.expand(self.ypos.view(1, 1, c), (n, v, c))
        return _nchw(frame_shift_cl(_cl(x), pos, stride))


class RefShiftTCN(nn.Module):
    def __init__(self, cin, cout, stride=1):
        super().__init__()
        self.stride = stride
        self.bn, self.bn2 = nn.BatchNorm2d(cin), nn.BatchNorm2d(cin)
        self.shift_in, self.shift_out = RefShift(cin), RefShift(cout)
        self.temporal_linear = nn.Conv2d(cin, cout, 1)
        self.relu = KinkReLU()

    def forward(self, x):
        h = self.temporal_linear(self.shift_in(self.bn(x)))
        return self.bn2(self.shift_out(self.relu(h), self.stride))


class RefTemporalConv(nn.Module):
    def __init__(self, cin, cout, stride=1):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, (1, 1), stride=(stride, 1))
        self.bn = nn.BatchNorm2d(cout)

    def forward(self, x):
        return self.bn(self.conv(x))


class RefBlock(nn.Module):
    def __init__(self, cin, cout, V, stride=1, residual=True):
        super().__init__()
        self.gcn1 = RefShiftGCN(cin, cout, V)
        self.tcn1 = RefShiftTCN(cout, cout, stride)
        self.has_residual = residual
        if residual and (cin != cout or stride != 1):
            self.residual = RefTemporalConv(cin, cout, stride)
        self.relu = KinkReLU()

    def forward(self, x):
        y = self.tcn1(self.gcn1(x))
        if self.has_residual:
            y = y + (self.residual(x) if hasattr(self, "residual") else x)
        return self.relu(y)


class RefModel(nn.Module):
    def __init__(self, shape, num_classes, base_channel=64):
        super().__init__()
        M, T, V, C = shape
        self.data_bn = nn.BatchNorm1d(M * V * C)
        for i, (cin, cout, stride, residual) in enumerate(layer_plan(C, base_channel), start=1):
            setattr(self, f"l{i}", RefBlock(cin, cout, V, stride, residual))
        self.fc = nn.Linear(4 * base_channel, num_classes)

    def forward(self, x):
        N, M, T, V, C = x.shape
        h = self.data_bn(x.permute(0, 1, 3, 4, 2).reshape(N, M * V * C, T))
        h = h.view(N, M, V, C, T).permute(0, 1, 3, 4, 2).reshape(N * M, C, T, V)
        for i in range(1, 11):
            h = getattr(self, f"l{i}")(h)
        return self.fc(h.view(N, M, h.shape[1], -1).mean(3).mean(1))


def expected_keys(shape, num_classes: int, base_channel: int = 64):
    """[(key, shape)] of the product's state dict, in its order (a module's own parameters come before its children's)"""
    M, T, V, C = shape
    out = []

    def bn(p, n):
        out.extend([(p + "weight", (n,)), (p + "bias", (n,)), (p + "running_mean", (n,)), (p + "running_var", (n,)), (p + "num_batches_tracked", ())])

    def conv(p, o, i):
        out.extend([(p + "weight", (o, i, 1, 1)), (p + "bias", (o,))])
    bn("data_bn.", M * V * C)
    for i, (cin, cout, stride, residual) in enumerate(layer_plan(C, base_channel), start=1):
        g, t = f"l{i}.gcn1.", f"l{i}.tcn1."
        out.extend([(g + "Linear_weight", (cin, cout)), (g + "Linear_bias", (1, 1, cout)), (g + "Feature_Mask", (1, V, cin))])
        bn(g + "bn.", V * cout)
        if cin != cout:
            conv(g + "down.0.", cout, cin), bn(g + "down.1.", cout)
        bn(t + "bn.", cout), bn(t + "bn2.", cout)
        out.extend([(t + "shift_in.ypos", (cout,)), (t + "shift_out.ypos", (cout,))])
        conv(t + "temporal_linear.", cout, cout)
        if residual and (cin != cout or stride != 1):
            conv(f"l{i}.residual.conv.", cout, cin), bn(f"l{i}.residual.bn.", cout)
    out.extend([("fc.weight", (num_classes, 4 * base_channel)), ("fc.bias", (num_classes,))])
    return out


# ---- filling ------------------------------------------------------------------------------------------------------------------------------
OWN_LEAVES = ("Linear_weight", "Linear_bias", "Feature_Mask", "ypos")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def f32(a) -> torch.Tensor:
    """float64 values that float32 holds exactly: what the product is handed and what the reference computes from"""
    return _t(a).float().double()


def fill(module: nn.Module, salt: int, prefix: str = "") -> None:
    """filler values for every entry, all away from their initial values: Linear_weight bell-shaped with the fan-in's scale, Linear_bias in
    +-0.2, Feature_Mask in +-1 (gates 0.24 .. 1.76), ypos in +-1.5; the rest by oracle.filler's rules"""
    sd = module.state_dict()
    filler.fill_state_dict(sd, salt=salt, prefix=prefix, skip=OWN_LEAVES)
    with torch.no_grad():
        for k, v in sd.items():
            leaf, name, shape = k.rsplit(".", 1)[-1], prefix + k, tuple(v.shape)
            if leaf == "Linear_weight":
                v.copy_(_t(filler.bellish(name, shape, scale=math.sqrt(1.0 / shape[0]), salt=salt)))
            elif leaf == "Linear_bias":
                v.copy_(_t(filler.uniform(name, shape, -0.2, 0.2, salt)))
            elif leaf == "Feature_Mask":
                v.copy_(_t(filler.uniform(name, shape, -1.0, 1.0, salt)))
            elif leaf == "ypos":
                v.copy_(_t(filler.uniform(name, shape, -1.5, 1.5, salt)))


# ---- op level -----------------------------------------------------------------------------------------------------------------------------
# (B, T, V, C): the 4-wide input; C = 64 at V = 25 wraps twice; even V, two tiles; V far below a wave; V = 40, whose rows fill the LDS stage
# raggedly; V and C at their limits; a single element row; CHUNK_CASE
JOINT_CASES = ((2, 3, 25, 4), (3, 5, 25, 64), (2, 7, 22, 128), (2, 3, 5, 64), (1, 9, 40, 64), (2, 2, 64, 512), (1, 1, 1, 64), (1, 19, 40, 64))
CHUNK_CASE = JOINT_CASES[7]       # three workgroup chunks of 8, 8 and 3 rows; a full chunk is three LDS stages of 3, 3 and 2 rows
# (B, T, V, C, stride)
FRAME_CASES = ((2, 7, 25, 64, 1), (2, 7, 25, 64, 2), (3, 8, 22, 128, 2), (1, 1, 25, 64, 1), (2, 5, 40, 256, 1), (1, 11, 25, 64, 1), (1, 21, 5, 64, 2))
FRAME_SPLIT_CASES = FRAME_CASES[5:]   # three frame splits of 4, 4 and 3 output frames, at stride 1 and at stride 2 with an odd T


def joint_inputs(case, salt: int, gate: str):
    """-> (x, mask or None); ``gate``: "none" | "zero" | "random".  The pad channel of the 4-wide input is zero"""
    B, T, V, C = case
    t = "shift.joint." + tag_of(*case)
    x = f32(filler.bellish(t + ".x", case, salt=salt))
    if C == 4:
        x[..., 3] = 0
    cm = 3 if C == 4 else C
    mask = {"none": None, "zero": torch.zeros(V, cm, dtype=torch.float64),
            "random": f32(filler.uniform(t + ".mask", (V, cm), -1.5, 1.5, salt))}[gate]
    return x, mask


def _joint_ref_op(x, mask, direction):
    """the contract on the 4-wide input: three channels shift, the pad stays zero"""
    if x.shape[-1] == 4:
        return torch.nn.functional.pad(joint_shift_cl(x[..., :3], mask, direction), (0, 1))
    return joint_shift_cl(x, mask, direction)


def _joint_run(case, direction: int, gate: str, salt: int, nan: bool):
    B, T, V, C = case
    x, mask = joint_inputs(case, salt, gate)
    if nan:
        x[B - 1, T // 2, V // 2, 1] = float("nan")
    probe = f32(filler.uniform("shift.joint.probe." + tag_of(*case), case, -1, 1))
    xl = x.clone().requires_grad_(True)
    res = dict(x=x, mask=mask, probe=probe, cond=1.0)
    if mask is None:
        out = _joint_ref_op(xl, None, direction)
        (out * probe).sum().backward()
    else:
        ml = mask.clone().requires_grad_(True)
        me = ml.view(1, 1, V, -1).expand(B, T, V, mask.shape[1]).clone()
        me.retain_grad()
        raw = _joint_ref_op(xl, None, direction)
        out = raw * torch.nn.functional.pad(torch.tanh(me) + 1, (0, C - mask.shape[1]))
        (out * probe).sum().backward()
        res.update(dmask=ml.grad, cond=cond_of(me.grad.reshape(B * T, V, -1)))
    res.update(out=out.detach(), dx=xl.grad)
    return res


@functools.lru_cache(maxsize=None)
def joint_salt(case, direction: int) -> int:
    for salt in range(MAX_SALT):
        if _joint_run(case, direction, "random", salt, False)["cond"] < COND_MAX:
            return salt
    raise AssertionError(f"no salt below {MAX_SALT} gives {case} a well-conditioned Feature_Mask gradient")


@functools.lru_cache(maxsize=None)
def joint_case(case, direction: int, gate: str, nan: bool = False) -> dict:
    """float64 reference of one joint-shift case: x, mask, probe, out, dx, dmask (with a gate); ``nan``: one NaN in the LAST row of x"""
    ref = _joint_run(case, direction, gate, joint_salt(case, direction), nan)
    assert nan or gate != "random" or ref["cond"] < COND_MAX
    return ref


def frame_positions(case, salt: int):
    """the fixed positions in the channels' first slots, the rest uniform in (-2, 2)"""
    B, T, V, C, s = case
    fixed = [0.0, 1.0, -1.0, T - 1.0, -(T - 1.0), float(T), -float(T), T + 0.5, -(T + 0.5), 0.25, -0.25, -0.75, 1e-8, -1e-8, 1e9, -1e9]
    pos = f32(filler.uniform("shift.frame." + tag_of(*case) + ".pos", (C,), -2, 2, salt))
    pos[:len(fixed)] = torch.tensor(fixed, dtype=torch.float64).float().double()
    return pos


def _frame_run(case, relu: bool, salt: int, nan: str = ""):
    B, T, V, C, s = case
    t = "shift.frame." + tag_of(*case)
    x = f32(filler.bellish(t + ".x", (B, T, V, C), salt=salt))
    pos = frame_positions(case, salt)
    if nan == "x":
        x[B - 1, T // 2, V // 2, 20] = float("nan")
    if nan == "pos":
        pos[17] = float("nan")
    probe = f32(filler.uniform(t + ".probe", (B, out_frames(T, s), V, C), -1, 1))
    xl, pl = x.clone().requires_grad_(True), pos.clone().requires_grad_(True)
    pe = pl.view(1, 1, C).expand(B, V, C).clone()
    pe.retain_grad()
    out = frame_shift_cl(xl, pe, s, relu)
    (out * probe).sum().backward()
    o = out.detach()
    return dict(x=x, pos=pos, probe=probe, out=o, dx=xl.grad, dpos=pl.grad, cond=cond_of(pe.grad.reshape(B * V, C)),
                mean=o.mean((0, 1, 2)), var=o.var((0, 1, 2), unbiased=False))


@functools.lru_cache(maxsize=None)
def frame_salt(case, relu: bool) -> int:
    for salt in range(MAX_SALT):
        if _frame_run(case, relu, salt)["cond"] < COND_MAX:
            return salt
    raise AssertionError(f"no salt below {MAX_SALT} gives {case} a well-conditioned ypos gradient")


@functools.lru_cache(maxsize=None)
def frame_case(case, relu: bool, nan: str = "") -> dict:
    """float64 reference of one frame-shift case; ``nan``: "x" = one NaN in the LAST sample of x, "pos" = a NaN position in channel 17"""
    ref = _frame_run(case, relu, frame_salt(case, relu), nan)
    assert nan or ref["cond"] < COND_MAX
    return ref


# ---- unit and block level -----------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "name cin cout stride V T")
BLOCK_B = 2
BLOCK_CASES = (Case("first3to64", 3, 64, 1, 25, 8), Case("id64", 64, 64, 1, 25, 8), Case("down64to128s2", 64, 128, 2, 25, 9),
               Case("id128v40", 128, 128, 1, 40, 8))
KINDS = ("gcn", "tcn", "block")


def make_ref(kind: str, case: Case, salt: int) -> nn.Module:
    if kind == "gcn":
        mod = RefShiftGCN(case.cin, case.cout, case.V)
    elif kind == "tcn":
        mod = RefShiftTCN(case.cout, case.cout, case.stride)
    else:
        mod = RefBlock(case.cin, case.cout, case.V, case.stride, residual=case.cin != 3)
    mod = mod.double()
    fill(mod, salt, prefix=f"{kind}.{case.name}.")
    return mod


def _ref_run(mod: nn.Module, x, probe_name: str, train: bool, loss=None, forced=None, terms: bool = True) -> dict:
    """one float64 run with autograd: output, dx, every parameter gradient, the running statistics afterwards, the margins;
    ``forced``: the ReLU decisions to take instead of the run's own (``Capture.force``)"""
    mod.train(train)
    before = {k: v.clone() for k, v in mod.state_dict().items()}
    xi = x.clone().requires_grad_(True)
    cap = Capture() if forced is None else Capture().force(forced)
    if terms:
        with cap:
            out = mod(xi)
    else:                                   # (the model: no per-term copies, only the ReLU bookkeeping)
        expand, Capture.expand = Capture.expand, lambda self, p, shape: p
        try:
            with cap:
                out = mod(xi)
        finally:
            Capture.expand = expand
    assert not cap.forced, "more ReLU decisions were handed in than the reference takes"
    if loss is None:
        probe = f32(filler.uniform(probe_name, tuple(out.shape), -1, 1))
        (out * probe).sum().backward()
    else:
        probe = None
        loss(out).backward()
    conds = cap.conds() if terms else []
    res = dict(conds=conds, cond=max(conds, default=1.0), flips=cap.flips, close=cap.close, out=out.detach(), dx=xi.grad, probe=probe,
               grads={k: p.grad.clone() for k, p in mod.named_parameters()}, least=cap.least, near=cap.near, decisions=cap.total,
               masks=cap.decisions, buffers={k: v.clone() for k, v in mod.state_dict().items() if "running" in k})
    mod.load_state_dict(before)
    for p in mod.parameters():
        p.grad = None
    return res


def block_input(kind: str, case: Case, salt: int):
    c = case.cout if kind == "tcn" else case.cin
    return f32(filler.bellish(f"x.shift.{kind}.{case.name}", (BLOCK_B, c, case.T, case.V), salt=salt))


@functools.lru_cache(maxsize=None)
def block_salt(kind: str, case: Case) -> int:
    for salt in range(MAX_SALT):
        mod, x = make_ref(kind, case, salt), block_input(kind, case, salt)
        runs = [_ref_run(mod, x, f"probe.shift.{kind}.{case.name}", train) for train in (True, False)]
        if all(r["least"] >= KINK_EPS and r["cond"] < COND_MAX for r in runs):
            return salt
    raise AssertionError(f"no salt below {MAX_SALT} keeps {kind} {case.name} off the ReLU kinks with well-conditioned ypos / Feature_Mask gradients")


@functools.lru_cache(maxsize=None)
def block_ref(kind: str, case: Case, train: bool) -> dict:
    """the float64 reference of a gcn / tcn / block case: NCHW tensors; ``state`` = the filled state dict the product loads"""
    salt = block_salt(kind, case)
    mod, x = make_ref(kind, case, salt), block_input(kind, case, salt)
    res = _ref_run(mod, x, f"probe.shift.{kind}.{case.name}", train)
    assert res["least"] >= KINK_EPS and res["cond"] < COND_MAX, (kind, case.name, train, res["least"], res["cond"])
    res.update(x=x, state={k: v.clone() for k, v in mod.state_dict().items()}, salt=salt)
    return res


# ---- model level ----------------------------------------------------------------------------------------------------------------------------
MODEL_SHAPE, MODEL_CLASSES, MODEL_CLIPS = (2, 16, 25, 3), 7, 2


def _model_and_input(dtype=torch.float64):
    labels = _t(filler.uniform("y.shift.model", (MODEL_CLIPS,), 0, MODEL_CLASSES).astype(np.int64))
    model = RefModel(MODEL_SHAPE, MODEL_CLASSES).double()
    fill(model, 0)
    x = f32(filler.skeleton_input("x.shift.model", (MODEL_CLIPS,) + MODEL_SHAPE))
    return model.to(dtype), x.to(dtype), labels


def _loss(labels):
    return lambda logits: torch.nn.functional.cross_entropy(logits, labels)


@functools.lru_cache(maxsize=None)
def model_ref() -> dict:
    """The model's float64 reference (the plain filler, salt 0).  The salt rule cannot choose this input: the model takes over two million
    ReLU decisions, so some pre-activation of EVERY input lies within KINK_EPS of zero.  What the rule was for is met another way: the
    gradients are compared with ``model_forced``, this reference taking the ReLU decisions the code under test took."""
    model, x, labels = _model_and_input()
    res = _ref_run(model, x, "", True, loss=_loss(labels), terms=False)
    res.update(x=x, labels=labels, state={k: v.clone() for k, v in model.state_dict().items()}, salt=0)
    return res


def model_forced(masks) -> dict:
    """``model_ref`` with every ReLU taking the decision in ``masks`` (bool NCHW tensors in forward order: per block the graph unit's, the
    temporal unit's, the block's).  ``flips`` = how many differ from the reference's own decisions, ``close`` = the largest
    |pre-activation| of the reference among those."""
    model, x, labels = _model_and_input()
    return _ref_run(model, x, "", True, loss=_loss(labels), forced=masks, terms=False)


@functools.lru_cache(maxsize=None)
def model_float32_decisions() -> list:
    """the ReLU decisions stock float32 torch takes on the CPU for the model input (the same modules and values in float32)"""
    model, x, labels = _model_and_input(torch.float32)
    model.train()
    with Capture() as cap, torch.no_grad():
        expand, Capture.expand = Capture.expand, lambda self, p, shape: p
        try:
            model(x)
        finally:
            Capture.expand = expand
    return cap.decisions
