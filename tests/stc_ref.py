"""The STC attention module of MS-AAGCN restated in plain torch (a helper module: no test, no conftest), and the float64 oracle of an
attention block / model composed from it and oracle/agcn_oracle.py.

``stc_ref`` IS the definition the kernels are held to (include/fgcn.h, "STC attention"): channels-last G (B, T, V, C), any float dtype,

    mt = mean_t G            s  = sigmoid(conv_sa(mt))  over the joints, kernel k = V (odd V) or V - 1, zero padding (k - 1) / 2
    G1 = G (1 + s)           m  = mean_v G1             tg = sigmoid(conv_ta(m)) over the frames, nine taps, zero padding 4
    G2 = G1 (1 + tg)         cm = mean_{t, v} G2        h  = relu(fc1c(cm))      cg = sigmoid(fc2c(h))
    G' = G2 (1 + cg)

The only decision inside the module is the ReLU of the channel gate: ``op_case`` / ``block_oracle`` pick filler salts at which every
pre-activation of the float64 reference is further than ``PRE_MIN`` from zero, and assert that, so that no comparison depends on a decision
that float32 rounding can flip.  ``block_salt`` states the second property a block case's salt is chosen by, the conditioning of the two
scalar bias gradients."""
from __future__ import annotations

import functools
from collections import namedtuple
from typing import Dict, Optional

import numpy as np
import torch
import torch.nn.functional as F

from oracle import agcn_oracle as O
from oracle import filler

STC_KEYS = ("conv_sa.weight", "conv_sa.bias", "conv_ta.weight", "conv_ta.bias", "fc1c.weight", "fc1c.bias", "fc2c.weight", "fc2c.bias")
PRE_MIN = 1e-4       # least |fc1c pre-activation| of the float64 reference in every case


def sa_kernel(V: int) -> int:
    return V if V % 2 else V - 1


def param_shapes(C: int, V: int):
    return ((1, C, sa_kernel(V)), (1,), (1, C, 9), (1,), (C // 2, C), (C // 2,), (C, C // 2), (C,))


def stc_ref(g, w_sa, b_sa, w_ta, b_ta, w1, b1, w2, b2, capture: Optional[dict] = None):
    B, T, V, C = g.shape
    p = (sa_kernel(V) - 1) // 2
    mt = g.mean(1)                                                                     # (B, V, C)
    zs = F.conv1d(mt.transpose(1, 2), w_sa, b_sa, padding=p)                           # (B, 1, V)
    s = torch.sigmoid(zs)
    g1 = g * (1 + s.view(B, 1, V, 1))
    m = g1.mean(2)                                                                     # (B, T, C)
    zt = F.conv1d(m.transpose(1, 2), w_ta, b_ta, padding=4)                            # (B, 1, T)
    tg = torch.sigmoid(zt)
    g2 = g1 * (1 + tg.view(B, T, 1, 1))
    cm = g2.mean((1, 2))                                                               # (B, C)
    pre = F.linear(cm, w1, b1)
    cg = torch.sigmoid(F.linear(torch.relu(pre), w2, b2))
    if capture is not None:
        capture.setdefault("pre", []).append(pre.detach())
        capture.setdefault("z", []).extend((zs, zt))         # the two scalar-bias convolutions' outputs, in the graph (``block_salt``)
    return g2 * (1 + cg.view(B, 1, 1, C))


def stc_nchw(g_nchw, sd: Dict[str, torch.Tensor], prefix: str, capture: Optional[dict] = None):
    """the module on the oracle's (B, C, T, V) layout with its parameters under ``prefix`` of a state dict"""
    out = stc_ref(g_nchw.permute(0, 2, 3, 1), *(sd[f"{prefix}.{k}"] for k in STC_KEYS), capture=capture)
    return out.permute(0, 3, 1, 2)


# ---- op level -------------------------------------------------------------------------------------------------------------------------
OP_SHAPES = ((3, 7, 25, 64), (2, 37, 22, 192), (2, 12, 40, 64), (2, 1, 25, 64), (2, 300, 25, 64))
NAN_AT = (1, 0, 3, 5)        # the element of sample 1 the non-finite case overwrites (frame 0 exists at T = 1)


def op_params(shape, salt: int):
    B, T, V, C = shape
    tag = "x".join(map(str, shape))
    return [torch.from_numpy(filler.fill_value_for(f"stc.{tag}.{k}", s, salt)) for k, s in zip(STC_KEYS, param_shapes(C, V))]


def least_pre(cap: dict) -> float:
    return min(float(p.abs().min()) for p in cap["pre"])


@functools.lru_cache(maxsize=None)
def op_salt(shape) -> int:
    """the first filler salt at which the float64 reference's ReLU pre-activations all exceed PRE_MIN in magnitude"""
    g = op_input(shape)
    for salt in range(64):
        cap = {}
        stc_ref(g, *op_params(shape, salt), capture=cap)
        if least_pre(cap) > PRE_MIN:
            return salt
    raise AssertionError(f"no salt below 64 keeps the pre-activations of {shape} away from zero")


def op_input(shape) -> torch.Tensor:
    return torch.from_numpy(filler.bellish("g.stc." + "x".join(map(str, shape)), shape))


@functools.lru_cache(maxsize=None)
def op_case(shape, nan: bool = False) -> dict:
    """float64 reference of one op-level case: output, dG and the eight parameter gradients under a fixed probe; ``nan``: with one NaN
    written into sample 1"""
    g = op_input(shape)
    if nan:
        g[NAN_AT] = float("nan")
    probe = torch.from_numpy(filler.uniform("probe.stc." + "x".join(map(str, shape)), shape, -1, 1))
    params = [p.requires_grad_(True) for p in op_params(shape, op_salt(shape))]
    gi = g.clone().requires_grad_(True)
    cap = {}
    out = stc_ref(gi, *params, capture=cap)
    if not nan:
        assert least_pre(cap) > PRE_MIN, (shape, least_pre(cap))
    grads = torch.autograd.grad((out * probe).sum(), [gi] + params)
    return dict(g=g, probe=probe, params=[p.detach() for p in params], out=out.detach(), dg=grads[0], grads=list(grads[1:]), least_pre=least_pre(cap))


# ---- block and model level: composed from the oracle ------------------------------------------------------------------------------------
def st_block(x, sd, p: str, stride: int, residual: bool, train: bool, stats=None, static_adjacency: bool = False, capture: Optional[dict] = None,
             pre: Optional[dict] = None):
    """oracle.agcn_oracle.st_block with the attention between its two halves; ``capture`` as there (g = the PRE-gate ReLU output, whose sign
    is the gated tensor's too)"""
    g, adj_c = O.spatial_graph_conv(x, sd, f"{p}.gcn1", train, stats, static_adjacency)
    z = O.temporal_conv(stc_nchw(g, sd, f"{p}.gcn1", pre), sd, f"{p}.tcn1", stride, train, stats)
    if not residual:
        res = 0
    elif f"{p}.residual.conv.weight" in sd:
        res = O.temporal_conv(x, sd, f"{p}.residual", stride, train, stats)
    else:
        res = x
    o = torch.relu(z + res)
    if capture is not None:
        capture[f"{p}.g"], capture[f"{p}.o"] = g.detach(), o.detach()
    return o, adj_c


def model_forward(x, sd, num_layers: int, train: bool = True, stats=None, capture: Optional[dict] = None, pre: Optional[dict] = None):
    """oracle.agcn_oracle.model_forward over attention blocks"""
    n, m, t, v, c = x.shape
    h = x.permute(0, 1, 3, 4, 2).reshape(n, m * v * c, t)
    h = O.batch_norm(h, sd, "data_bn", train, stats)
    h = h.reshape(n, m, v, c, t).permute(0, 1, 3, 4, 2).reshape(n * m, c, t, v)
    for i, b in enumerate(O.block_plan(c, num_layers)):
        h, _ = st_block(h, sd, f"l{i}", b["stride"], b["residual"], train, stats, capture=capture, pre=pre)
    feat = h.reshape(n, m, h.shape[1], -1).mean(3).mean(1)
    return F.linear(feat, sd["fc.weight"], sd["fc.bias"])


Case = namedtuple("Case", "name cin cout stride residual V T fused static")
BLOCK_B = 4
# the issue's four blocks: identity 64 -> 64 at (B, T, V) = (4, 12, 25), 64 -> 128 with stride 2 over 13 frames, the first block 3 -> 64 without
# a residual, a static-adjacency block
BLOCK_CASES = (
    Case("att_identity64", 64, 64, 1, True, 25, 12, True, False),
    Case("att_down_s2", 64, 128, 2, True, 25, 13, True, False),
    Case("att_first", 3, 64, 1, False, 25, 12, True, False),
    Case("att_static64", 64, 64, 1, True, 25, 12, True, True),
)


GATE_SCALE = 8.0     # the two gate convolutions' filler weights are multiplied by this in the block cases (``make_block``)
COND_MAX = 20.0      # largest sum |terms| / |sum terms| of a scalar bias gradient of the reference in a block case (``block_salt``)


def make_block(case: Case, salt: int = 0):
    """The case's attention block with filler parameters.  The filler's convolution weights (variance 1 / fan-in) leave the spatial and the
    temporal gate within a few percent of one value over all joints / frames; GATE_SCALE spreads them over (0, 1), so that the gates the
    kernels apply differ from element to element."""
    from fusion_gcn_amd.models.mmargcn.agcn import SpatialTemporalConv
    from test_block_model_gpu import adj_for
    blk = SpatialTemporalConv(case.cin, case.cout, adj_for(case.V), stride=case.stride, residual=case.residual, static_adjacency=case.static,
                              fused_spatial=case.fused, attention=True)
    filler.fill_state_dict(blk.state_dict(), salt=salt, prefix="l0.")
    with torch.no_grad():
        blk.gcn1.conv_sa.weight.mul_(GATE_SCALE)
        blk.gcn1.conv_ta.weight.mul_(GATE_SCALE)
    return blk


def _block_oracle(case: Case, salt: int, phase: str) -> dict:
    from oracle import relu_masks as RM
    from block_routes import ZERO_IN_EVAL
    from test_block_model_gpu import ZERO_GRAD_SUFFIXES
    train = phase == "train"
    blk = make_block(case, salt)
    sd = {"l0." + k: (v.detach().double() if v.is_floating_point() else v.detach().clone()) for k, v in blk.state_dict().items()}
    x = torch.from_numpy(filler.bellish(f"x.blk.{case.name}", (BLOCK_B, case.cin, case.T, case.V))).double()
    Tp = (case.T - 1) // case.stride + 1
    probe = torch.from_numpy(filler.uniform(f"probe.blk.{case.name}", (BLOCK_B, case.cout, Tp, case.V), -1, 1)).double()
    params = {k: v.clone().requires_grad_(True) for k, v in sd.items()
              if v.is_floating_point() and not k.endswith(("running_mean", "running_var", "adj_a"))}
    live = dict(sd)
    live.update(params)
    xo = x.clone().requires_grad_(True)
    stats, cap, pre = O.Stats(), {}, {}
    out, adj_c = st_block(xo, live, "l0", case.stride, case.residual, train, stats if train else None, static_adjacency=case.static, capture=cap,
                          pre=pre)
    grads = torch.autograd.grad((out * probe).sum(), [xo] + list(params.values()) + pre["z"], allow_unused=True)
    dz, grads = grads[-2:], grads[:-2]
    want = {k[3:]: g.numpy() for k, g in zip(params.keys(), grads[1:]) if g is not None}
    scale_ref = max(float(np.abs(v).max()) for v in want.values())
    zero = tuple(k for k in want if k.endswith(ZERO_GRAD_SUFFIXES if train else ZERO_IN_EVAL))
    for k in zero:
        assert float(np.abs(want[k]).max()) <= 1e-9 * scale_ref, (k, float(np.abs(want[k]).max()), scale_ref)
    return dict(x=x, probe=probe, out=out.detach(), adj_c=None if case.static else torch.stack(adj_c, 1).detach(), dx=grads[0], want=want,
                zero=zero, scale_ref=scale_ref, unused=tuple(k[3:] for k, g in zip(params.keys(), grads[1:]) if g is None),
                images={n: RM.pack_sign_image(cap[f"l0.{n}"]) for n in RM.RELU_NAMES}, stats={k[3:]: v for k, v in stats.updates.items()},
                least_pre=least_pre(pre), bias_cond=max(float(g.abs().sum() / g.sum().abs()) for g in dz))


@functools.lru_cache(maxsize=None)
def block_salt(case: Case) -> int:
    """The first filler salt at which, in the float64 reference of both phases, (1) every ReLU pre-activation of the channel gate exceeds
    PRE_MIN in magnitude and (2) the gradients of the two SCALAR parameters, conv_sa.bias and conv_ta.bias, are sums of their per-joint /
    per-frame terms that cancel less than COND_MAX-fold.  Why (2): behind the gates sits a batch-statistics BatchNorm, which removes a common
    scale of its input; a bias that moves a whole gate up or down mostly rescales G', so its gradient is the small residue of a large sum
    (37 to 490-fold cancellation with the plain filler in train mode, 5 to 13-fold with running statistics).  The relative error of such a
    scalar is the relative error of the incoming gradient times that factor whatever the kernels do; the project's 2e-4 is 20 times the 1e-5
    its float32-class kernels deliver at worst on a block's gradients, hence 20.  Both numbers are properties of the reference alone."""
    for salt in range(64):
        ok = True
        for phase in ("train", "eval"):
            ora = _block_oracle(case, salt, phase)
            ok = ok and ora["least_pre"] > PRE_MIN and ora["bias_cond"] < COND_MAX
        if ok:
            return salt
    raise AssertionError(f"no salt below 64 gives {case.name} well-conditioned scalar gradients and pre-activations away from zero")


@functools.lru_cache(maxsize=None)
def block_oracle(case: Case, phase: str) -> dict:
    """tests/block_routes.oracle_case for an attention block (the same dict, plus the two margins ``block_salt`` chose the salt by)"""
    ora = _block_oracle(case, block_salt(case), phase)
    assert ora["least_pre"] > PRE_MIN and ora["bias_cond"] < COND_MAX, (case.name, phase, ora["least_pre"], ora["bias_cond"])
    return ora
