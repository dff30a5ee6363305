"""CTR-GCN (Chen et al., ICCV 2021) restated in float64 torch (a helper module: no test, no conftest).  Nothing here calls a kernel of
fusion_gcn_amd.

The graph convolution is written twice: ``gc_cl`` channels-last, as include/fgcn.h states it ("CTR graph convolution"), and ``gc_nchw``,
the literal NCHW transcription of the paper's module (``conv(x).mean(-2)``, ``unsqueeze(-1) - unsqueeze(-2)``,
``einsum('ncuv,nctv->nctu')``).  The unit, the block and the model are plain ``nn.Conv2d`` / ``nn.BatchNorm2d`` modules with the product's
state-dict keys, so a product state dict loads into them.

The salt rule.  A case's input is the first filler salt for which the float64 reference ALONE meets both conditions:
  * every ReLU pre-activation is at least ``KINK_EPS`` from zero (tests/test_msg3d.py's convention), so float32 has no decision to flip;
  * no ``alpha`` gradient is the residue of a sum that cancels more than ``COND_MAX``-fold (tests/stc_ref.block_salt's convention).
The kernels never decide which input is used."""
from __future__ import annotations

import functools
import math
from collections import namedtuple

import numpy as np
import torch
import torch.nn as nn

from oracle import filler

K = 3
KINK_EPS = 1e-5
COND_MAX = 20.0
MAX_SALT = 256


def reduction(cin: int) -> int:
    return 8 if cin in (3, 9) else cin // 8


# ---- the graph convolution, twice -------------------------------------------------------------------------------------------------------
def op_ref(x3, x12, w4, b4, alpha, pa, terms: list = None):
    """the aggregation op: x3 (B, T, V, K C), x12 (B, V, 2 K R), w4 (K, C, R), b4 (K, C), alpha (1), pa (K, V, V) -> y (B, T, V, C).
    ``terms``: receives alpha expanded to one entry per (b, u, v, c) of every subset, in the graph (its gradient = the terms of dalpha)"""
    B, T, V, KC = x3.shape
    C, R = KC // K, w4.shape[2]
    y = 0
    for k in range(K):
        x1, x2 = x12[..., k * R:(k + 1) * R], x12[..., (K + k) * R:(K + k + 1) * R]
        th = torch.tanh(x1[:, :, None, :] - x2[:, None, :, :])                                  # (B, u, v, R)
        inner = th @ w4[k].t() + b4[k]                                                          # (B, u, v, C)
        a_e = alpha.expand_as(inner)
        if terms is not None:
            a_e = a_e.clone()
            a_e.retain_grad()
            terms.append(a_e)
        a = a_e * inner + pa[k][None, :, :, None]
        y = y + torch.einsum("buvc,btvc->btuc", a, x3[..., k * C:(k + 1) * C])
    return y


def gc_cl(x, sd, p: str = "", terms: list = None):
    """channels-last x (B, T, V, Cin) with the parameters under ``p`` of a state dict: the three subsets' 1x1 convolutions + ``op_ref``"""
    def lin(t, name):
        w = sd[f"{p}{name}.weight"]
        return t @ w.view(w.shape[0], -1).t() + sd[f"{p}{name}.bias"]
    xm = x.mean(1)
    x3 = torch.cat([lin(x, f"convs.{k}.conv3") for k in range(K)], -1)
    x12 = torch.cat([lin(xm, f"convs.{k}.conv1") for k in range(K)] + [lin(xm, f"convs.{k}.conv2") for k in range(K)], -1)
    w4 = torch.stack([sd[f"{p}convs.{k}.conv4.weight"].flatten(1) for k in range(K)])
    b4 = torch.stack([sd[f"{p}convs.{k}.conv4.bias"] for k in range(K)])
    return op_ref(x3, x12, w4, b4, sd[f"{p}alpha"], sd[f"{p}PA"], terms)


def gc_nchw(x, sd, p: str = ""):
    """the paper's module, literally: x (N, C, T, V)"""
    F = torch.nn.functional
    y = None
    for k in range(K):
        conv = lambda t, n: F.conv2d(t, sd[f"{p}convs.{k}.conv{n}.weight"], sd[f"{p}convs.{k}.conv{n}.bias"])  # noqa: E731
        x1, x2, x3 = conv(x, 1).mean(-2), conv(x, 2).mean(-2), conv(x, 3)
        x1 = torch.tanh(x1.unsqueeze(-1) - x2.unsqueeze(-2))
        x1 = conv(x1, 4) * sd[f"{p}alpha"] + sd[f"{p}PA"][k].unsqueeze(0).unsqueeze(0)
        z = torch.einsum("ncuv,nctv->nctu", x1, x3)
        y = z if y is None else y + z
    return y


def alpha_cond(terms) -> float:
    """sum |terms| / |sum terms| of one alpha's gradient, the terms being the sums per (sample, subset, output joint): what one wave of
    the backward hands on.  (Per element the ratio only measures the probe: a random probe makes it about the root of the element count.)"""
    g = torch.cat([t.grad.sum((2, 3)).flatten() for t in terms])
    return float(g.abs().sum() / g.sum().abs())


# ---- unit, block, model on plain torch modules (NCHW) -----------------------------------------------------------------------------------
class Capture:
    """what a reference run records: the least |ReLU pre-activation| and the expanded alphas"""
    active = None

    def __init__(self):
        self.least, self.terms, self.near, self.total = math.inf, [], 0, 0
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

    def cond(self) -> float:
        """largest sum |terms| / |sum terms| over the alphas (one per unit: its K subsets' terms together)"""
        return max(self.conds(), default=1.0)

    def conds(self) -> list:
        """per unit, in forward order"""
        return [alpha_cond(self.terms[i:i + K]) for i in range(0, len(self.terms), K)]


class KinkReLU(nn.Module):
    def forward(self, x):
        if Capture.active is not None:
            cap, mag = Capture.active, x.detach().abs()
            cap.least, cap.near, cap.total = min(cap.least, float(mag.min())), cap.near + int((mag < KINK_EPS).sum()), cap.total + mag.numel()
            if cap.forced is not None:
                mask = cap.forced.pop(0)
                assert mask.shape == x.shape, (tuple(mask.shape), tuple(x.shape))
                differ = mask != (x.detach() > 0)
                if bool(differ.any()):
                    cap.flips, cap.close = cap.flips + int(differ.sum()), max(cap.close, float(mag[differ].max()))
                return x * mask.to(x.dtype)
        return torch.relu(x)


class RefCTRGC(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        r = reduction(cin)
        self.conv1, self.conv2 = nn.Conv2d(cin, r, 1), nn.Conv2d(cin, r, 1)
        self.conv3, self.conv4 = nn.Conv2d(cin, cout, 1), nn.Conv2d(r, cout, 1)


class RefUnitGCN(nn.Module):
    def __init__(self, cin, cout, V, adaptive=True):
        super().__init__()
        self.convs = nn.ModuleList(RefCTRGC(cin, cout) for _ in range(K))
        self.bn = nn.BatchNorm2d(cout)
        self.down = nn.Sequential(nn.Conv2d(cin, cout, 1), nn.BatchNorm2d(cout)) if cin != cout else None
        self.PA = nn.Parameter(torch.zeros(K, V, V))
        self.alpha = nn.Parameter(torch.zeros(1))
        self.relu = KinkReLU()

    def forward(self, x):
        sd = dict(self.named_parameters())
        terms = Capture.active.terms if Capture.active is not None else None
        y = gc_cl(x.permute(0, 2, 3, 1), sd, "", terms).permute(0, 3, 1, 2)
        return self.relu(self.bn(y) + (x if self.down is None else self.down(x)))


class RefTemporalConv(nn.Module):
    def __init__(self, cin, cout, kernel_size, stride=1, dilation=1):
        super().__init__()
        pad = (kernel_size + (kernel_size - 1) * (dilation - 1) - 1) // 2
        self.conv = nn.Conv2d(cin, cout, (kernel_size, 1), padding=(pad, 0), stride=(stride, 1), dilation=(dilation, 1))
        self.bn = nn.BatchNorm2d(cout)

    def forward(self, x):
        return self.bn(self.conv(x))


class RefMSTCN(nn.Module):
    def __init__(self, cin, cout, kernel_size=5, stride=1, dilations=(1, 2)):
        super().__init__()
        bc = cout // (len(dilations) + 2)
        self.branches = nn.ModuleList(nn.Sequential(nn.Conv2d(cin, bc, 1), nn.BatchNorm2d(bc), KinkReLU(),
                                                    RefTemporalConv(bc, bc, kernel_size, stride, d)) for d in dilations)
        self.branches.append(nn.Sequential(nn.Conv2d(cin, bc, 1), nn.BatchNorm2d(bc), KinkReLU(),
                                           nn.MaxPool2d((3, 1), (stride, 1), (1, 0)), nn.BatchNorm2d(bc)))
        self.branches.append(nn.Sequential(nn.Conv2d(cin, bc, 1, stride=(stride, 1)), nn.BatchNorm2d(bc)))

    def forward(self, x):
        return torch.cat([b(x) for b in self.branches], 1)


class RefBlock(nn.Module):
    def __init__(self, cin, cout, V, stride=1, residual=True):
        super().__init__()
        self.gcn1 = RefUnitGCN(cin, cout, V)
        self.tcn1 = RefMSTCN(cout, cout, stride=stride)
        self.has_residual = residual
        if residual and (cin != cout or stride != 1):
            self.residual = RefTemporalConv(cin, cout, 1, stride)
        self.relu = KinkReLU()

    def forward(self, x):
        y = self.tcn1(self.gcn1(x))
        if self.has_residual:
            y = y + (self.residual(x) if hasattr(self, "residual") else x)
        return self.relu(y)


def layer_plan(c: int, b: int):
    """(cin, cout, stride, residual) of l1 .. l10"""
    return [(c, b, 1, False)] + [(b, b, 1, True)] * 3 + [(b, 2 * b, 2, True)] + [(2 * b, 2 * b, 1, True)] * 2 + [(2 * b, 4 * b, 2, True)] \
        + [(4 * b, 4 * b, 1, True)] * 2


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


def expected_keys(shape, num_classes: int, base_channel: int = 64, adaptive: bool = True):
    """[(key, shape)] of the product's state dict, in its order (a module's own parameters come before its children's)"""
    M, T, V, C = shape
    out = []

    def bn(p, n):
        out.extend([(p + "weight", (n,)), (p + "bias", (n,)), (p + "running_mean", (n,)), (p + "running_var", (n,)), (p + "num_batches_tracked", ())])

    def conv(p, o, i, k=1):
        out.extend([(p + "weight", (o, i, k, 1)), (p + "bias", (o,))])
    bn("data_bn.", M * V * C)
    for i, (cin, cout, stride, residual) in enumerate(layer_plan(C, base_channel), start=1):
        g, r = f"l{i}.gcn1.", reduction(cin)
        if adaptive:
            out.append((g + "PA", (K, V, V)))
        out.append((g + "alpha", (1,)))
        for k in range(K):
            conv(f"{g}convs.{k}.conv1.", r, cin), conv(f"{g}convs.{k}.conv2.", r, cin), conv(f"{g}convs.{k}.conv3.", cout, cin)
            conv(f"{g}convs.{k}.conv4.", cout, r)
        bn(g + "bn.", cout)
        if cin != cout:
            conv(g + "down.0.", cout, cin), bn(g + "down.1.", cout)
        t, bc = f"l{i}.tcn1.branches.", cout // 4
        for j in range(2):
            conv(f"{t}{j}.0.", bc, cout), bn(f"{t}{j}.1.", bc), conv(f"{t}{j}.3.conv.", bc, bc, 5), bn(f"{t}{j}.3.bn.", bc)
        conv(f"{t}2.0.", bc, cout), bn(f"{t}2.1.", bc), bn(f"{t}2.4.", bc)
        conv(f"{t}3.0.", bc, cout), bn(f"{t}3.1.", bc)
        if residual and (cin != cout or stride != 1):
            conv(f"l{i}.residual.conv.", cout, cin), bn(f"l{i}.residual.bn.", cout)
    out.extend([("fc.weight", (num_classes, 4 * base_channel)), ("fc.bias", (num_classes,))])
    return out


# ---- filling ------------------------------------------------------------------------------------------------------------------------------
ALPHA = 0.5          # the refinement's weight in every case (its initial value 0 would switch the refinement and its gradients off)


def fill(module: nn.Module, salt: int, prefix: str = "") -> None:
    """filler values for every entry; alpha = ALPHA; PA is the filler's asymmetric +-0.15"""
    sd = module.state_dict()
    filler.fill_state_dict(sd, salt=salt, prefix=prefix, skip=("alpha",))
    with torch.no_grad():
        for k, v in sd.items():
            if k.endswith("alpha"):
                v.fill_(ALPHA)


def tag_of(*dims) -> str:
    return "x".join(map(str, dims))


# ---- op level -----------------------------------------------------------------------------------------------------------------------------
# (B, T, V, Cin, Cout): R = 8 with the 4-wide input; odd T; even V; R = 16; V at the limit, three channel tiles, R = 24; V far below a wave; T long enough
# for the frames to be split over workgroups
OP_CASES = ((2, 8, 25, 3, 64), (3, 13, 25, 64, 64), (2, 10, 22, 64, 128), (2, 6, 27, 128, 128), (1, 5, 32, 192, 192), (2, 7, 5, 64, 64),
            (2, 37, 25, 64, 64))
SPLIT_CASE = OP_CASES[6]            # two frame splits per workgroup column, 19 and 18 frames: blockIdx.y > 0 and a ragged last split
OP_NAMES = ("x3", "x12", "w4", "b4", "alpha", "pa")


def op_inputs(case, salt: int, alpha: float = ALPHA):
    B, T, V, cin, C = case
    R, t = reduction(cin), "ctr.op." + tag_of(*case)
    f64 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double()  # noqa: E731
    return [f64(filler.bellish(t + ".x3", (B, T, V, K * C), salt=salt)), f64(filler.bellish(t + ".x12", (B, V, 2 * K * R), salt=salt)),
            f64(filler.bellish(t + ".w4", (K, C, R), scale=math.sqrt(1.0 / R), salt=salt)), f64(filler.uniform(t + ".b4", (K, C), -0.2, 0.2, salt)),
            torch.full((1,), alpha, dtype=torch.float64), f64(filler.uniform(t + ".pa", (K, V, V), -0.15, 0.15, salt))]


def _op_run(case, salt: int, alpha: float, nan_sample=None):
    B, T, V, cin, C = case
    ins = op_inputs(case, salt, alpha)
    if nan_sample is not None:
        ins[0][nan_sample, T // 2, V // 2, 5] = float("nan")
    probe = torch.from_numpy(filler.uniform("ctr.op.probe." + tag_of(*case), (B, T, V, C), -1, 1)).double()
    live = [t.clone().requires_grad_(True) for t in ins]
    terms = []
    y = op_ref(*live, terms=terms)
    (y * probe).sum().backward()
    return dict(inputs=ins, probe=probe, y=y.detach(), grads=[t.grad for t in live], cond=alpha_cond(terms))


@functools.lru_cache(maxsize=None)
def op_salt(case, alpha: float = ALPHA) -> int:
    for salt in range(MAX_SALT):
        if _op_run(case, salt, alpha)["cond"] < COND_MAX:
            return salt
    raise AssertionError(f"no salt below {MAX_SALT} gives {case} a well-conditioned alpha gradient")


@functools.lru_cache(maxsize=None)
def op_case(case, alpha: float = ALPHA, nan: bool = False) -> dict:
    """float64 reference of one op case (inputs, probe, y, the six gradients in OP_NAMES order); ``nan``: one NaN in the LAST sample's x3"""
    ref = _op_run(case, op_salt(case, alpha), alpha, nan_sample=case[0] - 1 if nan else None)
    assert nan or ref["cond"] < COND_MAX
    return ref


# ---- unit and block level -----------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "name cin cout stride V T")
BLOCK_B = 2
BLOCK_CASES = (Case("first3to64", 3, 64, 1, 25, 8), Case("id64", 64, 64, 1, 25, 8), Case("down64to128s2", 64, 128, 2, 25, 9),
               Case("id128", 128, 128, 1, 25, 6), Case("id192v32", 192, 192, 1, 32, 5))
KINDS = ("unit", "block")


def make_ref(kind: str, case: Case, salt: int) -> nn.Module:
    if kind == "unit":
        mod = RefUnitGCN(case.cin, case.cout, case.V)
    else:
        mod = RefBlock(case.cin, case.cout, case.V, case.stride, residual=case.cin != 3)
    mod = mod.double()
    fill(mod, salt, prefix=f"{case.name}.")
    return mod


def _ref_run(mod: nn.Module, x, probe_name: str, train: bool, loss=None, forced=None) -> dict:
    """one float64 run with autograd: output, dx, every parameter gradient, the running statistics afterwards, the two margins;
    ``forced``: the ReLU decisions to take instead of the run's own (``Capture.force``)"""
    mod.train(train)
    before = {k: v.clone() for k, v in mod.state_dict().items()}
    xi = x.clone().requires_grad_(True)
    with (Capture() if forced is None else Capture().force(forced)) as cap:
        out = mod(xi)
        assert not cap.forced, "more ReLU decisions were handed in than the reference takes"
        if loss is None:
            probe = torch.from_numpy(filler.uniform(probe_name, tuple(out.shape), -1, 1)).double()
            (out * probe).sum().backward()
        else:
            probe = None
            loss(out).backward()
        cond, conds = cap.cond(), cap.conds()
    res = dict(conds=conds, flips=cap.flips, close=cap.close, out=out.detach(), dx=xi.grad, probe=probe, grads={k: p.grad.clone() for k, p in mod.named_parameters()}, least=cap.least, cond=cond,
               near=cap.near, decisions=cap.total, buffers={k: v.clone() for k, v in mod.state_dict().items() if "running" in k})
    mod.load_state_dict(before)          # (the module is shared between the phases: the train run's running statistics are rolled back)
    for p in mod.parameters():
        p.grad = None
    return res


def block_input(kind: str, case: Case, salt: int):
    t = case.T if kind == "block" else (case.T - 1) // case.stride + 1
    return torch.from_numpy(filler.bellish(f"x.ctr.{case.name}", (BLOCK_B, case.cin, t, case.V), salt=salt)).double()


@functools.lru_cache(maxsize=None)
def block_salt(kind: str, case: Case) -> int:
    for salt in range(MAX_SALT):
        mod, x = make_ref(kind, case, salt), block_input(kind, case, salt)
        runs = [_ref_run(mod, x, f"probe.ctr.{kind}.{case.name}", train) for train in (True, False)]
        if all(r["least"] >= KINK_EPS and r["cond"] < COND_MAX for r in runs):
            return salt
    raise AssertionError(f"no salt below {MAX_SALT} keeps {kind} {case.name} off the ReLU kinks with a well-conditioned alpha gradient")


@functools.lru_cache(maxsize=None)
def block_ref(kind: str, case: Case, train: bool) -> dict:
    """the float64 reference of a unit / block case: NCHW tensors; ``state`` = the filled state dict the product loads"""
    salt = block_salt(kind, case)
    mod, x = make_ref(kind, case, salt), block_input(kind, case, salt)
    res = _ref_run(mod, x, f"probe.ctr.{kind}.{case.name}", train)
    assert res["least"] >= KINK_EPS and res["cond"] < COND_MAX, (kind, case.name, train, res["least"], res["cond"])
    res.update(x=x, state={k: v.clone() for k, v in mod.state_dict().items()}, salt=salt)
    return res


# ---- model level ----------------------------------------------------------------------------------------------------------------------------
MODEL_SHAPE, MODEL_CLASSES, MODEL_CLIPS = (2, 16, 25, 3), 7, 2
FLIP_CAP = 1e-4          # tests/test_msg3d.py's: the share of the ReLU decisions that float32 may take differently


def _model_and_input():
    labels = torch.from_numpy(filler.uniform("y.ctr.model", (MODEL_CLIPS,), 0, MODEL_CLASSES).astype(np.int64))
    model = RefModel(MODEL_SHAPE, MODEL_CLASSES).double()
    fill(model, 0)
    x = torch.from_numpy(filler.skeleton_input("x.ctr.model", (MODEL_CLIPS,) + MODEL_SHAPE)).double()
    return model, x, labels


@functools.lru_cache(maxsize=None)
def model_ref() -> dict:
    """The model's float64 reference; gcn1.bn.weight keeps the filler's 0.6 .. 1.4 and alpha is ALPHA, both away from their initial values.
    The salt rule cannot choose this input: the model takes over three million ReLU decisions, so some pre-activation of EVERY input lies
    within KINK_EPS of zero (about 3e6 x 2e-5 x the density at zero), and ten alphas behind a softmax loss are not all well conditioned
    at once in any of 256 salts.  The plain filler (salt 0) is used, and what the rule was for is met another way: the gradients are
    compared with ``model_forced``, this reference taking the ReLU decisions the code under test took."""
    model, x, labels = _model_and_input()
    res = _ref_run(model, x, "", True, loss=lambda logits: torch.nn.functional.cross_entropy(logits, labels))
    res.update(x=x, labels=labels, state={k: v.clone() for k, v in model.state_dict().items()}, salt=0)
    return res


def model_forced(masks) -> dict:
    """``model_ref`` with every ReLU taking the decision in ``masks`` (bool NCHW tensors in the reference's forward order: per block the
    unit's ReLU, the three temporal heads', the block's).  ``flips`` = how many differ from the reference's own decisions, ``close`` =
    the largest |pre-activation| of the reference among those; ``conds`` = each alpha's cancellation in this run."""
    model, x, labels = _model_and_input()
    return _ref_run(model, x, "", True, loss=lambda logits: torch.nn.functional.cross_entropy(logits, labels), forced=masks)
