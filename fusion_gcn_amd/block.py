"""One AGCN / ST-GCN block (SpatialTemporalConv) on the HIP kernels: forward, backward, autograd glue.

Reference semantics: torch_src/models/mmargcn/agcn.py:96-115 (SpatialGraphConv.forward), :49-51 (TemporalConv),
:134-136 (SpatialTemporalConv.forward) and the autograd backward of that graph (formulas: SURVEY.md Appendix A).

Internal layout is channels-last (B, T, V, C) with C padded to a multiple of 4 (only the 3-channel network input
needs padding).  Every arithmetic step is a libfgcn kernel (fusion_gcn_amd/ops.py); torch is used for buffers,
the stream and trivial weight re-layout (cat / permute of the small parameter tensors, cached per parameter version).

Which of the forms below a stage runs, and which activation-sized tensor is stored as bfloat16, is decided once per block call by
routes.plan_block; block_forward keeps the plan in its saved dict and the backward follows it (fusion_gcn_amd/routes.py).

Kernel schedule of one block, train mode (B = N*M samples):
  forward   emb_fwd_tile [split modes: theta|phi 1x1 with the V x V affinity gram formed from the tile on chip]
               (else: rows_gemm / pw_gemm(theta|phi 1x1) -> joint_gram) -> adj_softmax (A^ = A + B + C)
            spatial_fwd  [fused x.A^_k + conv_d, BN partial sums]   (or joint_mix + rows_gemm when fused_spatial=False)
            bn_finalize -> [rows_gemm(down) -> bn_finalize] -> bn_act (BN + down/identity + ReLU = G)
            [BlockConfig.attention: stc_forward, MS-AAGCN's STC attention G' = G (1 + s)(1 + tg)(1 + cg); the temporal conv reads G']
            tconv_halo (9x1 temporal conv, stride 1; rows_gemm for stride 2) with BN partial sums -> bn_finalize
            [rows_gemm(residual 1x1 stride s) -> bn_finalize] -> bn_act (BN + residual + ReLU = O)
  backward  bn_act_bwd (O)  -> tconv_halo(data gradient 9x1; two parity passes when strided) / tconv_wgrad(all taps)
            [-> stc_backward (dG' -> dG in place, the attention's eight parameter gradients)] -> bn_act_bwd (G)
            spatial_wgrad_tile [bf16x3, channels in 64s: conv_d's weight gradient, aggregation on chip, whole frame tiles]
               (else: spatial_wgrad up to 128 outputs; beyond: joint_mix_vec(agg) -> pw_wgrad)
            -> spatial_bwd_tile [bf16x3, >= 64 inputs: dagg = dY.Wd on chip, dx and dA^ in one launch]
               (else: pw_gemm / rows_gemm(dY.Wd) -> joint_dagg(dx, dA^))
            -> adj_softmax_bwd -> emb_dx_tile + emb_wgrad_tile [split modes, channels in 64s: the embedding gradient on chip]
               (else: joint_mix_vec(dtheta, dphi) -> pw_gemm / rows_gemm(dx) / rows_wgrad(theta|phi))
            + down / residual conv dgrad & wgrad, bias gradients by col_sum; every weight gradient is reduced from its
            slabs straight into the parameter's (out, in, taps, 1) layout (reduce_sum_strided).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

from . import ops
from .packing import Form, PackedWeights, Seg
from .routes import BlockPlan, plan_block, pw_routed, temporal_route

NUM_SUBSETS = 3


def _r4(c: int) -> int:
    return (c + 3) // 4 * 4


@dataclass(frozen=True)
class BlockConfig:
    cin: int
    cout: int
    stride: int = 1
    residual: str = "identity"      # "none" | "identity" | "conv"
    has_down: bool = False
    static_adjacency: bool = False  # ST-GCN special case: A^ = A + B, no data-dependent C_k
    fused_spatial: bool = True      # north-star fused kernel vs. joint_mix + rows_gemm
    attention: bool = False         # MS-AAGCN's STC attention between the graph convolution and the temporal conv

    @property
    def ic(self) -> int:
        return self.cout // 4

    @property
    def cx(self) -> int:            # padded input channels
        return _r4(self.cin)

    def validate(self) -> None:
        if self.cout % 64 != 0:
            raise ValueError(f"HIP AGCN block needs out_channels % 64 == 0 (got {self.cout}): the embedding "
                             "channels (out_channels/4 per subset) are tiled in groups of 16")
        if self.residual == "identity" and not (self.cin == self.cout and self.stride == 1):
            raise ValueError("identity residual needs cin == cout and stride 1")
        if not self.has_down and self.cin != self.cout:
            raise ValueError("cin != cout needs the down branch")


# parameter order of a block (autograd.Function inputs); bn buffers travel separately
def param_names(cfg: BlockConfig) -> List[str]:
    names = ["gcn1.adj_b"]
    for grp in ("conv_a", "conv_b", "conv_d"):
        for k in range(NUM_SUBSETS):
            names += [f"gcn1.{grp}.{k}.weight", f"gcn1.{grp}.{k}.bias"]
    names += ["gcn1.bn.weight", "gcn1.bn.bias"]
    if cfg.has_down:
        names += ["gcn1.down.0.weight", "gcn1.down.0.bias", "gcn1.down.1.weight", "gcn1.down.1.bias"]
    names += ["tcn1.conv.weight", "tcn1.conv.bias", "tcn1.bn.weight", "tcn1.bn.bias"]
    if cfg.residual == "conv":
        names += ["residual.conv.weight", "residual.conv.bias", "residual.bn.weight", "residual.bn.bias"]
    if cfg.attention:                # (appended: the positions of a block's other parameters do not depend on it)
        names += stc_names()
    return names


def stc_names() -> List[str]:
    """the eight tensors of the STC attention module, registered on gcn1 behind everything else it holds"""
    return [f"gcn1.{n}" for n in ops.STC_PARAMS]


def bn_names(cfg: BlockConfig) -> List[str]:
    out = ["gcn1.bn"]
    if cfg.has_down:
        out.append("gcn1.down.1")
    out.append("tcn1.bn")
    if cfg.residual == "conv":
        out.append("residual.bn")
    return out


# ---- weight re-layout (tiny tensors; torch plumbing) ---------------------------------------------------------------
def _pad_last(t: torch.Tensor, n: int) -> torch.Tensor:
    return t if t.shape[-1] == n else F.pad(t, (0, n - t.shape[-1]))


def pack_weights(P: Dict[str, torch.Tensor], cfg: BlockConfig) -> PackedWeights:
    """Reference-layout parameters -> the packed forms rows_gemm / spatial_fwd / tconv_halo stream, as DATA (packing.Form: the
    logical (taps, K, N) matrix as windows of the parameter tensors + the consumer's layout); a form is materialised on first use
    and refreshed with all the others in one launch afterwards.  The input-channel dimension is zero-padded from cin to cx (= cin
    rounded up to 4): the kernels then see a cx-channel block whose extra input channel is identically zero (only the 3-channel
    network input pads).  The math mode is read once, here (the block keys its set of forms on it)."""
    cin, cout, ic, cx = cfg.cin, cfg.cout, cfg.ic, cfg.cx
    mode = ops.get_math_mode()
    x3 = mode in ops.SPLIT_MODES                     # modes whose halo kernel takes the split weight form
    split_form = "split2h" if mode == "f16x2" else "split3"      # f16x2: block-scaled two-way f16 split (FGCN_PACK_SPLIT2H)
    conv_form = split_form if x3 else "k4"
    F: Dict[str, Form] = {}
    conv = lambda name: P[name].detach()             # noqa: E731  (O, I, kt, 1) contiguous: strides o: I*kt, i: kt, tap: 1

    def one_by_one(name, K_in):
        """(1, K_in-padded, O) and its transpose from a 1x1 conv weight (O, K_in, 1, 1)"""
        w = conv(name)
        o = w.shape[0]
        return ([Seg(w, st_k=1, st_n=K_in, klen=K_in, nlen=o)], [Seg(w, st_k=K_in, st_n=1, klen=o, nlen=K_in)])

    if not cfg.static_adjacency:
        # embedding channel order [th0 ph0 th1 ph1 th2 ph2]
        emb = [conv(f"gcn1.conv_{g}.{k}.weight") for k in range(NUM_SUBSETS) for g in "ab"]
        F["emb"] = Form("plain", 1, cx, 6 * ic, [Seg(w, st_k=1, st_n=cin, klen=cin, nlen=ic, n0=j * ic) for j, w in enumerate(emb)])
        F["emb_t"] = Form("plain", 1, 6 * ic, cx, [Seg(w, st_k=cin, st_n=1, klen=ic, nlen=cin, k0=j * ic) for j, w in enumerate(emb)])
        F["emb_b"] = Form("plain", 1, 1, 6 * ic, [Seg(P[f"gcn1.conv_{g}.{k}.bias"].detach(), st_k=0, st_n=1, klen=1, nlen=ic, n0=(2 * k + j) * ic)
                                                   for k in range(NUM_SUBSETS) for j, g in enumerate("ab")], shape=(6 * ic,))
    wd = [conv(f"gcn1.conv_d.{k}.weight") for k in range(NUM_SUBSETS)]
    d_rows = [Seg(w, st_k=1, st_n=cin, klen=cin, nlen=cout, k0=k * cx) for k, w in enumerate(wd)]          # (3cx, cout)
    F["d"] = Form("plain", 1, 3 * cx, cout, d_rows, shape=(3 * cx, cout))
    if mode in ops.X3_MODES and cx % 32 == 0:        # the fused spatial kernel's form (ops.pack_spatial)
        F["d4"] = Form("split2h_acc" if mode == "f16x2" else "split3_acc", 1, 3 * cx, cout, d_rows)
    else:
        F["d4"] = Form("k4", 1, 3 * cx, cout, d_rows, shape=(3 * cx // 4, cout, 4))
    if mode in ("bf16x3", "bf16") and cx % 64 == 0:  # the tile form of the fused spatial kernel (ops.spatial_fwd_tile): plain split form (bf16: its part 0)
        F["d_s3"] = Form("split3", 1, 3 * cx, cout, d_rows)
    d_cols = [Seg(w, st_k=cin, st_n=1, klen=cout, nlen=cin, n0=k * cx) for k, w in enumerate(wd)]          # (1, cout, 3cx)
    F["d_t"] = Form("plain", 1, cout, 3 * cx, d_cols)
    # the kernel adds the sum of the three biases: overlapping segments are summed
    F["d_b"] = Form("plain", 1, 1, cout, [Seg(P[f"gcn1.conv_d.{k}.bias"].detach(), st_k=0, st_n=1, klen=1, nlen=cout)
                                          for k in range(NUM_SUBSETS)], shape=(cout,))
    if cfg.has_down:
        fwd, bwd = one_by_one("gcn1.down.0.weight", cin)
        F["down"], F["down_t"] = Form("plain", 1, cx, cout, fwd), Form("plain", 1, cout, cx, bwd)
    wt = conv("tcn1.conv.weight")                    # (o, c, kt, 1)
    kt = wt.shape[2]
    t_seg = lambda **kw: [Seg(wt, st_tap=1, st_k=kt, st_n=cout * kt, klen=cout, nlen=cout, **kw)]           # noqa: E731  (kt, c, o)
    tt_seg = lambda **kw: [Seg(wt, st_tap=1, st_k=cout * kt, st_n=kt, klen=cout, nlen=cout, **kw)]          # noqa: E731  (kt, o, c)
    F["t"] = Form("plain", kt, cout, cout, t_seg(tlen=kt))
    F["t_t"] = Form("plain", kt, cout, cout, tt_seg(tlen=kt))
    # the halo-tile kernel's forms (ops.pack_conv: k-interleaved f32, or the three-way bf16 split in the bf16 math modes); a
    # stride-2 conv runs as an even-tap and an odd-tap pass
    if cfg.stride == 1:
        F["t4"] = Form(conv_form, kt, cout, cout, t_seg(tlen=kt))
        F["t_t4"] = Form(conv_form, kt, cout, cout, tt_seg(tlen=kt))
    else:
        for par, tag in ((0, "e"), (1, "o")):        # data gradient; forward too in the split modes (see temporal_fwd)
            n_par = (kt - par + 1) // 2
            F[f"t_t4_{tag}"] = Form(conv_form, n_par, cout, cout, tt_seg(tlen=n_par, tap0=par, tap_step=2))
            if x3:
                F[f"t4_{tag}"] = Form(conv_form, n_par, cout, cout, t_seg(tlen=n_par, tap0=par, tap_step=2))
    if cfg.residual == "conv":
        fwd, bwd = one_by_one("residual.conv.weight", cin)
        F["res"], F["res_t"] = Form("plain", 1, cx, cout, fwd), Form("plain", 1, cout, cx, bwd)
    if x3:                                           # split forms of the 1x1 weights pw_gemm may route to the halo kernel
        for key in ("emb", "emb_t", "d_t", "down", "down_t"):
            if key in F and F[key].K % 32 == 0:
                F[key + "_s3"] = Form(split_form, 1, F[key].K, F[key].N, F[key].segs)
    # the fused spatial backward (ops.spatial_bwd_tile) multiplies three-way bf16 splits in every float32-class mode: with the f16x2
    # products the block keeps that form of d_t beside the two-way f16 one
    if mode in ("bf16x3", "f16x2", "bf16") and cx % 64 == 0 and cout % 64 == 0:
        F["d_t_b3"] = Form("split3", 1, cout, 3 * cx, d_cols)      # (a form of its own: forms are materialised per key; bf16 reads its part 0)
    # the embedding backward in tile form (ops.emb_dx_tile: the embedding gradient on chip) streams the three-way bf16 split of emb_t in
    # every split mode (bf16: its part 0)
    if "emb_t" in F and mode in ops.SPLIT_MODES and cx % 64 == 0:
        F["emb_t_b3"] = Form("split3", 1, 6 * ic, cx, F["emb_t"].segs)
    # ... and the embedding forward with the gram on chip (ops.emb_fwd_tile) the split of emb
    if "emb" in F and mode in ops.SPLIT_MODES and cx % 32 == 0:
        F["emb_b3"] = Form("split3", 1, cx, 6 * ic, F["emb"].segs)
    return PackedWeights(F, P["tcn1.conv.weight"].device)


def pw_gemm(x: torch.Tensor, W: Dict[str, torch.Tensor], key: str, out: torch.Tensor, *, K: int, N: int,
            bias: Optional[torch.Tensor] = None, stats: bool = False, accumulate: bool = False, amax_out: Optional[torch.Tensor] = None):
    """1x1 convolution over all rows: in the split-bf16 math modes (the packed set then holds the split form of the weight) the
    persistent split-bf16 row GEMM from the contraction depth routes.pw_min_k on; the exact-f32 row GEMM otherwise.  ``amax_out``: see
    ops.pw_gemm (ignored by the f32 kernel)."""
    w3 = W.get(key + "_s3")      # (materialises the split form on first use, routed or not)
    if w3 is not None and x.shape[3] == K and pw_routed(W, key, K, x.numel() // K):
        return ops.pw_gemm(x, w3, out, bias=bias, stats=stats, accumulate=accumulate, amax_out=amax_out)
    return ops.rows_gemm(x, W[key], out, K=K, N=N, bias=bias, stats=stats, accumulate=accumulate)


# ---- joint-mix item tables -----------------------------------------------------------------------------------------
def spec_agg(cin: int) -> List[dict]:
    """agg[(k, c)] = sum_v x[v, c] A^_k[v, w]: out joint = column index of A^_k -> transpose = 1."""
    out = []
    for k in range(NUM_SUBSETS):
        for c0 in range(0, cin, 32):
            out.append(dict(out_c=k * cin + c0, width=min(32, cin - c0), terms=[(k, 1, c0, c0 + 16, 3)]))
    return out


def spec_dx(cin: int) -> List[dict]:
    """dx[v, c] = sum_k sum_w dagg[(k, c), w] A^_k[v, w]."""
    return [dict(out_c=c0, width=min(32, cin - c0),
                 terms=[(k, 0, k * cin + c0, k * cin + c0 + 16, 3) for k in range(NUM_SUBSETS)])
            for c0 in range(0, cin, 32)]


def _vec_width(c: int, order: Sequence[int] = None) -> int:
    """Channels per lane (1/2) for a group-of-``c``-channels mix: groups of 32*vw channels must tile ``c`` exactly
    (first such vw in preference order), or ``c`` is a single narrower group (smallest such vw: most lanes busy).
    0: no such tiling, use the dword kernel with 16-lane masks."""
    order = order or ops.paths().mix_vw_order
    for vw in order:
        if c % (32 * vw) == 0:
            return vw
    narrow = [vw for vw in order if c % vw == 0 and c < 32 * vw]
    return min(narrow) if narrow else 0


def _mix_groups(c: int, V: int) -> Tuple[List[Tuple[int, int]], int]:
    """-> ([(first channel, width)] of the channel groups of a ``c``-channel mix on a graph of V joints, channels per lane): 32-channel
    groups on the wide joint kernel (channels per lane 0; the last group may be narrower), groups of 32 * vw on the vector kernel (they
    tile ``c`` or are one narrower group), or ([], 0): the dword kernel with its own tables (spec_*)."""
    wide = ops.wide_graph(V)
    vw = 0 if wide else _vec_width(c)
    g = 32 if wide else 32 * vw
    return ([(c0, min(g, c - c0)) for c0 in range(0, c, g)] if g else []), vw


def mix_agg(x: torch.Tensor, agg: torch.Tensor, a_hat: torch.Tensor, cin: int, amax_out=None) -> bool:
    """agg[(k, c)] = x . A^_k for the three subsets (items of one channel group are adjacent: x is loaded once).  ``amax_out``:
    records max |agg| (ops.joint_mix_vec); -> whether it was recorded (never on a wide graph)."""
    groups, vw = _mix_groups(cin, x.shape[2])
    spec = [dict(out_c=k * cin + c0, nch=w, terms=[(k, 1, c0)]) for c0, w in groups for k in range(NUM_SUBSETS)]
    if vw:
        ops.joint_mix_vec(x, agg, a_hat, spec, vw=vw, amax_out=amax_out)
        return amax_out is not None
    if spec:
        ops.joint_mix_wide(x, agg, a_hat, spec)
    else:
        ops.joint_mix(x, agg, a_hat, spec_agg(cin), in_channels=cin, out_channels=3 * cin)
    return False


def mix_dx(dagg: torch.Tensor, dx: torch.Tensor, a_hat: torch.Tensor, cin: int, accumulate: bool) -> None:
    """dx (+)= sum_k dagg_k . A^_k^T."""
    groups, vw = _mix_groups(cin, dagg.shape[2])
    spec = [dict(out_c=c0, nch=w, terms=[(k, 0, k * cin + c0) for k in range(NUM_SUBSETS)]) for c0, w in groups]
    if vw:
        ops.joint_mix_vec(dagg, dx, a_hat, spec, vw=vw, accumulate=accumulate)
    elif spec:
        ops.joint_mix_wide(dagg, dx, a_hat, spec, accumulate=accumulate)
    else:
        ops.joint_mix(dagg, dx, a_hat, spec_dx(cin), in_channels=3 * cin, out_channels=cin, accumulate=accumulate)


def mix_demb(emb: torch.Tensor, demb: torch.Tensor, d_s: torch.Tensor, ic: int) -> torch.Tensor:
    """dtheta_k = dS_k . phi_k, dphi_k = dS_k^T . theta_k over the embedding layout [th0 ph0 th1 ph1 th2 ph2];
    returns the column sums of demb (the theta|phi bias gradient), fused into the mix where the kernel allows."""
    groups, vw = _mix_groups(ic, emb.shape[2])
    spec = []
    for k in range(NUM_SUBSETS):
        th, ph = 2 * k * ic, (2 * k + 1) * ic
        for c0, w in groups:
            spec.append(dict(out_c=th + c0, nch=w, terms=[(k, 0, ph + c0)]))
            spec.append(dict(out_c=ph + c0, nch=w, terms=[(k, 1, th + c0)]))
    if vw and len(spec) <= ops.MIX_MAX_ITEMS:
        return ops.joint_mix_vec(emb, demb, d_s, spec, vw=vw, colsum=True)[1]
    if vw:
        ops.joint_mix_vec(emb, demb, d_s, spec, vw=vw)
    elif spec:
        ops.joint_mix_wide(emb, demb, d_s, spec)
    else:
        ops.joint_mix(emb, demb, d_s, spec_demb(ic), in_channels=6 * ic, out_channels=6 * ic)
    return ops.col_sum(demb, 6 * ic)


def temporal_fwd(g: torch.Tensor, u: torch.Tensor, W: Dict[str, torch.Tensor], bias: torch.Tensor, kt: int, s: int,
                 stats: bool, fuse_in=None, amax_out=None, route: Optional[str] = None):
    """u = Conv(kt x 1, stride s, pad (kt-1)//2)(g) + bias, with BatchNorm partial sums of u when ``stats``.  ``route``: the block's
    plan (routes.temporal_route, asked here when a caller has none).
    ``fuse_in = (vec, shortcut, g_out, g_sign)`` (stride 1, split-bf16 kernel): the first argument is the BatchNorm input y and
    g = relu(BatchNorm(y) + shortcut) is formed inside the conv (ops.tconv_halo)."""
    pad = (kt - 1) // 2
    T, Tp = g.shape[1], u.shape[1]
    route = route or temporal_route(W, kt, s, T, ops.wide_graph(g.shape[2]), "fwd")
    if route == "halo":
        return ops.tconv_halo(g, W["t4"], u, Th=T, taps=kt, tb=1, tc=-pad, bias=bias, stats=stats, fuse_in=fuse_in, amax_out=amax_out)
    assert fuse_in is None
    if route == "halo_parity":
        # output frame to meets tap j = 2j' + par at input frame 2 (to + j' - pad/2) + par: one pass over the even input
        # frames (taps 0, 2, ..), one accumulating pass over the odd ones (which also takes the BatchNorm sums)
        ops.tconv_halo(g, W["t4_e"], u, Th=Tp, taps=(kt + 1) // 2, tb=1, tc=-(pad // 2), in_view=(2, 0, (T + 1) // 2),
                       bias=bias, amax_out=amax_out)
        return ops.tconv_halo(g, W["t4_o"], u, Th=Tp, taps=kt // 2, tb=1, tc=-(pad // 2), in_view=(2, 1, T // 2),
                              stats=stats, accumulate=True, amax_out=amax_out)
    # the per-tap row GEMM.  A graph of more than 32 joints: the halo kernel's image is sized for V <= 32.  Strided forward
    # in f32: it measures faster than two accumulating halo passes over the even / odd input frames (1.26 vs 1.54 ms at 128 channels, T 300 ->
    # 150); on the split-bf16 kernels (the packed set then holds t4_e / t4_o) the two passes win
    return ops.rows_gemm(g, W["t"], u, K=g.shape[3], N=u.shape[3], tmap=ops.conv_tmap(kt, s), bias=bias, stats=stats)


def temporal_dgrad(du: torch.Tensor, dg: torch.Tensor, W: Dict[str, torch.Tensor], kt: int, s: int, bn_bwd=None, amax_out=None,
                   route: Optional[str] = None):
    """dg = data gradient of that convolution: dg[t] = sum_j W_j^T du[(t + pad - j) / s].  ``bn_bwd`` (stride 1, split-bf16 kernel):
    the BatchNorm-backward sums of dg against (a, sign image, vec) from the kernel's epilogue -> partials, else None."""
    pad = (kt - 1) // 2
    T = dg.shape[1]
    route = route or temporal_route(W, kt, s, T, ops.wide_graph(dg.shape[2]), "dgrad")
    if route == "halo":
        return ops.tconv_halo(du, W["t_t4"], dg, Th=T, taps=kt, tb=-1, tc=pad, bn_bwd=bn_bwd, amax_out=amax_out)
    assert bn_bwd is None
    if route == "halo_parity":
        # frame t = 2*th + par only meets taps j = 2j' + par, at du frame th + pad/2 - j'
        ops.tconv_halo(du, W["t_t4_e"], dg, Th=(T + 1) // 2, taps=(kt + 1) // 2, tb=-1, tc=pad // 2, out_view=(2, 0), amax_out=amax_out)
        if T > 1:
            ops.tconv_halo(du, W["t_t4_o"], dg, Th=T // 2, taps=kt // 2, tb=-1, tc=pad // 2, out_view=(2, 1), amax_out=amax_out)
    else:
        ops.rows_gemm(du, W["t_t"], dg, K=du.shape[3], N=dg.shape[3], tmap=ops.conv_dgrad_tmap(kt, s))


def spec_demb(ic: int) -> List[dict]:
    """dtheta_k = dS_k . phi_k (transpose 0), dphi_k = dS_k^T . theta_k (transpose 1); embedding channels are
    [th0 ph0 th1 ph1 th2 ph2], each ``ic`` (a multiple of 16) wide, so a 32-lane tile may straddle two groups."""
    def source(c):                       # 16-channel group starting at c -> (mat, transpose, source channel)
        grp, off = divmod(c, ic)
        k, is_phi = divmod(grp, 2)
        return (k, 1, 2 * k * ic + off) if is_phi else (k, 0, (2 * k + 1) * ic + off)
    out = []
    for c0 in range(0, 6 * ic, 32):
        lo, hi = source(c0), source(c0 + 16)
        if lo[:2] == hi[:2]:
            terms = [(lo[0], lo[1], lo[2], hi[2], 3)]
        else:
            terms = [(lo[0], lo[1], lo[2], lo[2], 1), (hi[0], hi[1], hi[2], hi[2], 2)]
        out.append(dict(out_c=c0, width=32, terms=terms))
    return out


# ---- forward ---------------------------------------------------------------------------------------------------------
def _bn_vec(part, count, P, bufs, name, train):
    g, b = P[f"{name}.weight"], P[f"{name}.bias"]
    rm, rv = bufs[f"{name}.running_mean"], bufs[f"{name}.running_var"]
    if train:
        return ops.bn_finalize(part, count, g, b, rm, rv)
    return ops.bn_eval_coeffs(g, b, rm, rv)


def _f32_once(x: torch.Tensor):
    """-> a function returning x as float32, for the kernels without a bfloat16-input form: converted once, on first use"""
    cache = [] if x.dtype == torch.bfloat16 else [x]

    def get() -> torch.Tensor:
        if not cache:
            cache.append(x.float())
        return cache[0]
    return get


def block_forward(x: torch.Tensor, P: Dict[str, torch.Tensor], bufs: Dict[str, torch.Tensor], W: Dict[str, torch.Tensor],
                  cfg: BlockConfig, train: bool, pool_groups: int = 0, inference: bool = False, out_half: bool = False):
    """x (B, T, V, cx) -> O (B, T', V, cout); returns (O, saved-for-backward dict).  ``pool_groups`` > 0 (the model's last block): O is
    not formed, the first result is its mean over the rows of every group of B / pool_groups consecutive samples, (pool_groups, cout).
    ``inference`` (eval mode, no autograd graph): BatchNorm + shortcut + ReLU run as the EPILOGUES of the two north-star kernels where
    their inference forms exist (paths.fused_inference) -- no pre-BatchNorm tensors, no bn_act passes, nothing saved for a backward.
    Math mode bf16 (paths.half_activations): ``x`` may be a bfloat16 tensor (the previous block's output), Y / U are stored as bfloat16 where
    their producers have the form, and ``out_half`` (the caller takes a bfloat16 output: the next block) makes O one too.
    Every kernel form and storage type is a field of the routes.BlockPlan made here, first, from the math mode and the context's options
    read once; it travels to the backward in the saved dict (``S["plan"]``), and the backward follows it."""
    B, T, V, cx = x.shape
    cout, ic = cfg.cout, cfg.ic
    assert cx == cfg.cx, (cx, cfg.cx)
    cin = cx                     # kernels work on the padded channel count; the pad channel is identically zero
    dev = x.device
    pl = plan_block(cfg, B, T, V, x_bf16=x.dtype == torch.bfloat16, train=train, inference=inference, pool_groups=pool_groups, out_half=out_half,
                    forms=W, mode=ops.get_math_mode(), paths=ops.paths(), kt=P["tcn1.conv.weight"].shape[2])
    new = lambda *shape: torch.empty(shape, device=dev, dtype=torch.float32)  # noqa: E731
    S: Dict[str, Optional[torch.Tensor]] = {"x": x, "plan": pl}
    x32 = _f32_once(x)
    # math mode f16x2: the largest magnitudes of x and G, recorded by the kernels that stage them (pw_gemm / tconv_halo), scale the same tensors
    # in the backward's weight gradients; slot 0 = x, 1 = G (plan.x_amax / g_amax: really recorded -- a row-GEMM fallback records nothing)
    amax = S["amax"] = torch.zeros(4, device=dev, dtype=torch.int32) if pl.mode == "f16x2" else None

    # -- data-dependent adjacency ------------------------------------------------------------------------------------
    adj_a, adj_b = bufs["gcn1.adj_a"], P["gcn1.adj_b"].detach()
    if pl.emb_fwd is None:
        emb, c_mat = None, None
        _, a_hat = ops.adj_softmax_fwd(None, 1.0, adj_a, 1, use_softmax=False, adj_b=adj_b)
    else:
        if pl.emb_fwd == "tile":
            # emb written once, the gram from the tile on chip (inference: not written at all -- only the backward reads it)
            emb, part = ops.emb_fwd_tile(x, W["emb_b3"], W["emb_b"], ic=ic, write_emb=pl.write_emb, emb_bf16=pl.emb_bf16)
        else:
            emb = new(B, T, V, 6 * ic)
            pw_gemm(x, W, "emb", emb, K=cin, N=6 * ic, bias=W["emb_b"], amax_out=amax[0:1] if pl.x_amax else None)
            part = ops.joint_gram(emb, emb, [(2 * k * ic, (2 * k + 1) * ic, ic) for k in range(NUM_SUBSETS)])
        c_mat, a_hat = ops.adj_softmax_fwd(part, 1.0 / (ic * T), adj_a, B, adj_b=adj_b)
    S.update(emb=emb, c_mat=c_mat, a_hat=a_hat)

    # -- spatial aggregation + conv_d ------------------------------------------------------------------------------------
    if pl.spatial_fwd == "tile_bn_relu":
        # north-star kernel 1, inference form: aggregation + feature contraction + BatchNorm + shortcut + ReLU in one kernel
        vec_y = _bn_vec(None, B * T * V, P, bufs, "gcn1.bn", False)
        d, vec_d = None, None
        if cfg.has_down:
            d = new(B, T, V, cout)
            pw_gemm(x32(), W, "down", d, K=cin, N=cout, bias=P["gcn1.down.0.bias"])
            vec_d = _bn_vec(None, B * T * V, P, bufs, "gcn1.down.1", False)
        g = ops.spatial_fwd_tile_bn_relu(x, a_hat, W["d_s3"], W["d_b"], vec_y, Cin=cin, Cout=cout, res=d if cfg.has_down else x, res_vec=vec_d)
        S.update(y=None, vec_y=vec_y, d=None, vec_d=vec_d, g=g, g_sign=None)
        return _temporal_stage(x, S, P, bufs, W, cfg, pl, x32)
    if pl.spatial_fwd == "tile":
        y, part = ops.spatial_fwd_tile(x if pl.y_bf16 else x32(), a_hat, W["d_s3"], W["d_b"], Cin=cin, Cout=cout, stats=train, y_bf16=pl.y_bf16)
    elif pl.spatial_fwd == "fused":
        y, part = ops.spatial_fwd(x32(), a_hat, W["d4"], W["d_b"], Cin=cin, Cout=cout, stats=train)
    else:
        agg = new(B, T, V, 3 * cin)
        mix_agg(x32(), agg, a_hat, cin)
        y = new(B, T, V, cout)
        part = ops.rows_gemm(agg, W["d"].unsqueeze(0), y, K=3 * cin, N=cout, bias=W["d_b"], stats=train)
    vec_y = _bn_vec(part, B * T * V, P, bufs, "gcn1.bn", train)
    # (plan.g_bf16: G, the temporal conv's input, as bfloat16 -- only bf16 MFMA staging reads it, so the values multiplied are the same)
    d, vec_d = None, None
    if cfg.has_down:
        # (plan.shortcuts_bf16: the shortcut conv reads the bfloat16 x and writes a bfloat16 d -- the typed row GEMMs)
        d = torch.empty((B, T, V, cout), device=dev, dtype=torch.bfloat16) if pl.shortcuts_bf16 else new(B, T, V, cout)
        part = pw_gemm(x if pl.shortcuts_bf16 else x32(), W, "down", d, K=cin, N=cout, bias=P["gcn1.down.0.bias"], stats=train)
        vec_d = _bn_vec(part, B * T * V, P, bufs, "gcn1.down.1", train)
        g, g_sign = ops.bn_act(y, vec_y, d, vec_d, relu=True, sign_mask=True, out_bf16=pl.g_bf16)
    elif pl.fuse_g:
        # identity blocks on the split-bf16 kernels: G = relu(BatchNorm(y) + x) is formed INSIDE the temporal conv while it stages its
        # image (north-star kernel 2: "temporal 9x1 conv + BN + ReLU"), G and its sign image come out as by-products -- no bn_act pass
        g = new(B, T, V, cout)
        g_sign = torch.empty((B * T * V * cout) // 8, device=dev, dtype=torch.uint8)
    else:
        g, g_sign = ops.bn_act(y, vec_y, x, None, relu=True, sign_mask=True, out_bf16=pl.g_bf16)
    S.update(y=y, vec_y=vec_y, d=d, vec_d=vec_d, g=g, g_sign=g_sign)   # *_sign: 1 bit per element, the backward's ReLU gate
    return _temporal_stage(x, S, P, bufs, W, cfg, pl, x32)


def _temporal_stage(x, S, P, bufs, W, cfg: BlockConfig, pl: BlockPlan, x32):
    """The second half of block_forward: the temporal conv, its BatchNorm, the block's shortcut and ReLU (agcn.py:49-51,125-136)."""
    B, T, V, cin = x.shape
    cout, s, train, pool_groups = cfg.cout, cfg.stride, pl.train, pl.pool_groups
    kt = P["tcn1.conv.weight"].shape[2]
    Tp = (T - 1) // s + 1
    dev = x.device
    new = lambda *shape: torch.empty(shape, device=dev, dtype=torch.float32)  # noqa: E731
    if cfg.attention:
        # G' = G (1 + s)(1 + tg)(1 + cg): the temporal conv and its weight gradient read G'; the pre-gate G stays for the attention's
        # backward and the ReLU gate (every gate is > 0: G's sign image is G''s too)
        S["g_att"], S["stc"] = ops.stc_forward(S["g"], [P[n] for n in stc_names()])
    g_t = S["g_att"] if cfg.attention else S["g"]        # the temporal conv's input
    if pl.temporal_bn_relu:
        # north-star kernel 2 as the north star states it, inference form: temporal conv + BatchNorm + shortcut + ReLU in one kernel
        vec_u = _bn_vec(None, B * Tp * V, P, bufs, "tcn1.bn", False)
        r, vec_r = None, None
        if cfg.residual == "conv":
            r = new(B, Tp, V, cout)
            ops.rows_gemm(x, W["res"], r, K=cin, N=cout, tmap=(1, s, 0, 0, 1), bias=P["residual.conv.bias"])
            vec_r = _bn_vec(None, B * Tp * V, P, bufs, "residual.bn", False)
        o = new(B, Tp, V, cout)
        ops.tconv_halo_bn_relu(g_t, W["t4"], o, taps=kt, tb=1, tc=-((kt - 1) // 2), vec=vec_u, bias=P["tcn1.conv.bias"],
                               res=x if cfg.residual == "identity" else r, res_vec=vec_r)
        S.update(u=None, vec_u=vec_u, r=None, vec_r=vec_r, o=o, o_sign=None)
        return o, S
    u = torch.empty((B, Tp, V, cout), device=dev, dtype=torch.bfloat16) if pl.u_bf16 else new(B, Tp, V, cout)
    # (plan.fuse_g: the conv's first argument is the BatchNorm input y; it forms G and its sign image on the way)
    part = temporal_fwd(S["y"] if pl.fuse_g else g_t, u, W, P["tcn1.conv.bias"], kt, s, stats=train, route=pl.temporal_fwd,
                        fuse_in=(S["vec_y"], x, S["g"], S["g_sign"]) if pl.fuse_g else None, amax_out=S["amax"][1:2] if pl.g_amax else None)
    vec_u = _bn_vec(part, B * Tp * V, P, bufs, "tcn1.bn", train)
    r, vec_r = None, None
    if cfg.residual == "conv":
        hs = pl.shortcuts_bf16
        r = torch.empty((B, Tp, V, cout), device=dev, dtype=torch.bfloat16) if hs else new(B, Tp, V, cout)
        part = ops.rows_gemm(x if hs else x32(), W["res"], r, K=cin, N=cout, tmap=(1, s, 0, 0, 1), bias=P["residual.conv.bias"], stats=train)
        vec_r = _bn_vec(part, B * Tp * V, P, bufs, "residual.bn", train)
    res = x if cfg.residual == "identity" else r
    if pool_groups:
        o, o_sign = ops.bn_act_pool(u, vec_u, res, vec_r, pool_groups)
    else:
        o, o_sign = ops.bn_act(u, vec_u, res, vec_r, relu=True, sign_mask=True, out_bf16=pl.o_bf16)
    S.update(u=u, vec_u=vec_u, r=r, vec_r=vec_r, o=None if pool_groups else o, o_sign=o_sign)
    return o, S


def pool_epilogue_ok(cfg: BlockConfig, B: int, T: int, V: int, groups: int) -> bool:
    """the last block's epilogue can carry the pooling: equal groups of whole samples, a sign image exists (element count and cout in 8s)"""
    Tp = (T - 1) // cfg.stride + 1
    return ops.paths().pool_epilogue and groups > 0 and B % groups == 0 and cfg.cout % 8 == 0 and (B * Tp * V * cfg.cout) % 8 == 0


# ---- backward --------------------------------------------------------------------------------------------------------
def zero_bias_floats(cfg: BlockConfig) -> int:
    """floats of exactly-zero bias gradients a block hands out in train mode: NUM_SUBSETS slots for each of its two BatchNorm backward
    passes (conv_d x 3; the temporal conv uses the first of its three: _BiasGrads.carry writes both groups with one launch), then the
    shortcut convolutions' (residual conv, down)"""
    return (2 * NUM_SUBSETS + int(cfg.has_down) + int(cfg.residual == "conv")) * cfg.cout


class _BiasGrads:
    """Gradients of conv biases that feed a BatchNorm.  In train mode the BatchNorm subtracts the batch mean, so the
    block output does not depend on such a bias and its gradient is exactly zero (the reference's autograd produces
    ~1e-9 rounding noise there): all of a block's are disjoint slices of ONE zero-filled
    allocation (one fill launch per block; every parameter still gets memory of its own).  Only eval-mode statistics make
    them real column sums.

    A step that is not finite (include/fgcn.h, "Non-finite values in the inputs", rule 3): the reference's gradient of such a bias is the
    column sum of the BatchNorm backward's result, and that is NaN as soon as the pass's channel sum of dP * a_hat (the shortcut
    BatchNorm's: of dP * b_hat) is not a number -- a non-finite dP or a NaN a_hat makes it so.  Both passes of a block (stage 0: the temporal
    half, stage 1: the spatial half) write their sums into ONE (2, 3, C) tensor (``sums_out``), and ``carry`` writes s - s of those rows (0
    for a number, NaN otherwise) over the slots: one launch per block, one more where the block has a shortcut convolution."""

    def __init__(self, cfg: BlockConfig, device, train: bool, zeros: Optional[torch.Tensor] = None):
        self.train, self.c = train, cfg.cout
        self.sums = torch.empty((2, 3, cfg.cout), device=device, dtype=torch.float32) if train else None
        self.shortcuts: List[int] = []
        n = zero_bias_floats(cfg)
        # ``zeros``: this block's slice of a pool the MODEL filled once per step (one launch for the ten blocks instead of ten)
        if train and zeros is not None and zeros.numel() >= n:
            self.pool = zeros
        else:
            self.pool = torch.empty(n, device=device, dtype=torch.float32) if train else None      # (carry writes every slot)
        self.used = 0

    def sums_out(self, stage: int) -> Optional[torch.Tensor]:
        return self.sums[stage] if self.train else None

    def main(self, d: torch.Tensor, stage: int, j: int = 0) -> torch.Tensor:
        """the gradient of bias ``j`` in front of the BatchNorm of ``stage``"""
        if not self.train:
            return ops.col_sum(d, self.c)
        slot = NUM_SUBSETS * stage + j
        return self.pool[slot * self.c:(slot + 1) * self.c]

    def shortcut(self, d: torch.Tensor, stage: int) -> torch.Tensor:
        """the gradient of the bias of the shortcut convolution whose BatchNorm is the second one of ``stage``"""
        if not self.train:
            return ops.col_sum(d, self.c)
        self.shortcuts.append(stage)
        slot = 2 * NUM_SUBSETS + len(self.shortcuts) - 1
        return self.pool[slot * self.c:(slot + 1) * self.c]

    def carry(self) -> None:
        """after both passes: the slots become 0, or NaN where their pass's sums are not numbers"""
        if not self.train:
            return
        c, off = self.c, self.sums.storage_offset()
        src = self.sums.as_strided((2, NUM_SUBSETS, c), (3 * c, 0, 1), off + c)                  # row 1 of each stage, NUM_SUBSETS times
        torch.sub(src, src, out=self.pool[:2 * NUM_SUBSETS * c].view(2, NUM_SUBSETS, c))
        n = len(self.shortcuts)
        assert self.shortcuts in ([], [0], [1], [0, 1]), self.shortcuts       # (the view below strides from the first to the second stage)
        if n:                                                                                    # row 2 of the stages that have a shortcut BatchNorm
            src = self.sums.as_strided((n, c), (3 * c, 1), off + (3 * self.shortcuts[0] + 2) * c)
            torch.sub(src, src, out=self.pool[2 * NUM_SUBSETS * c:(2 * NUM_SUBSETS + n) * c].view(n, c))


def block_backward(d_o: torch.Tensor, S: Dict[str, Optional[torch.Tensor]], P: Dict[str, torch.Tensor],
                   W: Dict[str, torch.Tensor], cfg: BlockConfig, train: bool = True, need_dx: bool = True,
                   pool: Optional[Tuple[int, tuple]] = None, zeros: Optional[torch.Tensor] = None):
    """-> (dx (B, T, V, cx) or None, {param name: grad in the parameter's own shape}).
    The leaf reductions of the block (weight-gradient slabs, adj_b, embedding-bias partials) are collected and issued as one
    launch at the end (ops.deferred_reductions).  Weight gradients are leaves of the backward graph and run in line, on the one stream:
    launching them on a second HIP stream beside the HBM-bound chain was built in round 2, lost its A/B in rounds 3 and 4 (the matrix
    kernels fill every CU's registers and LDS, so nothing of the other stream is co-resident: DESIGN.md section 3.2 item 11) and was
    removed in round 6."""
    with ops.deferred_reductions() as batch:
        out = _block_backward(d_o, S, P, W, cfg, train, need_dx, pool, zeros)
        batch.flush()
    return out


def _block_backward(d_o, S, P, W, cfg: BlockConfig, train: bool, need_dx: bool, pool=None, zeros=None):
    """``pool`` = (groups, shape of the block's output): the block's forward returned the per-group mean of its output (pool_groups) and
    ``d_o`` is the gradient of that, (groups, cout); it is consumed as a per-group row (divided by the group's rows) where the kernels
    take one (POOL_BACKWARD_ROWS) and expanded to the output's shape otherwise."""
    x = S["x"]
    pl: BlockPlan = S["plan"]    # the forward's plan: this function evaluates no route predicate of its own
    B, T, V, cx = x.shape
    cout, ic, s = cfg.cout, cfg.ic, cfg.stride
    cin, cin_true = cx, cfg.cin  # kernels work on the padded channel count; gradients are cut back to cin_true
    Tp = d_o.shape[1] if pool is None else pool[1][1]
    dev = x.device
    new = lambda *shape: torch.empty(shape, device=dev, dtype=torch.float32)  # noqa: E731
    G: Dict[str, torch.Tensor] = {}
    d_o = d_o.contiguous()
    o_numel = B * Tp * V * cout
    kt = P["tcn1.conv.weight"].shape[2]
    # what the plan predicted of this call (the sign images exist where the element counts say so; train / pool are the forward's)
    seen = (train, pool[0] if pool is not None else 0, S["o_sign"] is not None, S["g_sign"] is not None)
    if seen != (pl.train, pl.pool_groups, pl.o_sign, pl.g_sign):
        raise ops._lib.FgcnError(f"block backward: (train, pool groups, o_sign, g_sign) = {seen} contradicts the forward's plan: {pl}")
    half, half_dy, hs, x16 = pl.g_bf16, pl.dy_bf16, pl.dshortcuts_bf16, pl.x_bf16      # (g_bf16: dU is bfloat16 as G is)
    gate_in_dagg, fuse_sums = pl.gate_in_dagg, pl.bn_sums_in_dgrad
    # run-time refinement, the one thing only the backward sees: the storage type of the incoming gradient (BlockPlan.refine_dx)
    dx16, dg16 = pl.refine_dx(d_o.dtype == torch.bfloat16)
    x_h = x                                  # the input as it arrived: the kernels with a typed form take the bfloat16 x beside a bfloat16 dy / emb / gradient
    xf = _f32_once(x)
    del x                                    # (every use below names the form it needs: x_h, or xf())
    dx = torch.empty((B, T, V, cx), device=dev, dtype=torch.bfloat16) if dx16 else new(B, T, V, cx)
    dx_live = False      # becomes True once dx holds a valid partial sum
    as_extra = lambda t: t if (dx16 or t.dtype == torch.float32) else t.float()      # noqa: E731  a gated addend has dx's storage type
    gated: List[tuple] = []
    grp_rows = grp_samples = 0
    if pool is not None:
        groups = pool[0]
        rows = o_numel // cout // groups
        d_o = d_o / rows                             # (groups, cout): every row of a group receives the group's gradient / rows
        if pl.pool_rows:
            grp_rows, grp_samples = rows, B // groups        # the BatchNorm-backward passes and the gated addend read the group's row
        else:
            d_o = d_o.unsqueeze(1).expand(groups, rows, cout).contiguous().view(B, Tp, V, cout)
    bias_grad = _BiasGrads(cfg, dev, train, zeros)

    # -- O = relu(BN(u) + res) ---------------------------------------------------------------------------------------------
    if cfg.residual != "conv":
        ident = cfg.residual == "identity"       # its gated gradient goes to dx: written here, or (gate_in_dagg) added by the spatial backward below
        du, _, sums = ops.bn_act_bwd(d_o, S["o"], S["u"], S["vec_u"], x_h if ident else None, None, res_mode=int(ident), train=train,
                                     need_db=not gate_in_dagg, db=dx if ident and not gate_in_dagg else None, sign_mask=S["o_sign"],
                                     grp_rows=grp_rows, da_bf16=half, sums_out=bias_grad.sums_out(0))
        if gate_in_dagg:
            gated.append((d_o, S["o_sign"], grp_samples) if grp_samples else (as_extra(d_o), S["o_sign"]))   # dx += d_o * [o > 0]
        dx_live = ident and not gate_in_dagg
    else:
        du, dr, sums = ops.bn_act_bwd(d_o, S["o"], S["u"], S["vec_u"], S["r"], S["vec_r"], res_mode=2, train=train,
                                      sign_mask=S["o_sign"], grp_rows=grp_rows, da_bf16=half, db_bf16=hs, sums_out=bias_grad.sums_out(0))
        G["residual.bn.weight"], G["residual.bn.bias"] = sums[2], sums[0].clone()   # own memory: sums[0] is tcn1.bn.bias too
        ops.rows_gemm(dr, W["res_t"], dx, K=cout, N=cx, tmap=(1, 1, 0, 0, s))   # frames t % s != 0 receive zeros
        dx_live = True
        G["residual.conv.weight"] = ops.rows_wgrad(x_h if dr.dtype == torch.bfloat16 else xf(), dr, K=cin, N=cout, tmap=(1, s, 0, 0, 1),
                                                   conv_param=(1, cin_true))
        G["residual.conv.bias"] = bias_grad.shortcut(dr, 0)
    G["tcn1.bn.weight"], G["tcn1.bn.bias"] = sums[1], sums[0]

    # -- temporal conv -------------------------------------------------------------------------------------------------------
    dg = torch.empty((B, T, V, cout), device=dev, dtype=torch.bfloat16) if dg16 else new(B, T, V, cout)
    # plan.bn_sums_in_dgrad (identity blocks, split-bf16 modes): the data-gradient kernel sums dg * [g > 0] and dg * [g > 0] * y_hat in its
    # epilogue, so the BatchNorm backward of the graph convolution below needs no reduction pass of its own over dg and y
    # math mode f16x2: the data-gradient kernels record the largest magnitudes of the tensors they stage (slot 0 = du, 1 = demb); with the
    # forward's slots they are the operand scales of the weight gradients, which therefore follow those kernels.  A slot only counts when
    # the kernel that ran really recorded it (plan.*_amax): a weight gradient scaled by a zero-initialised slot would leave the f16 range
    bamax = torch.zeros(4, device=dev, dtype=torch.int32) if pl.mode == "f16x2" else None
    g_partials = temporal_dgrad(du, dg, W, kt, s, bn_bwd=(S["y"], S["g_sign"], S["vec_y"]) if fuse_sums else None,
                                amax_out=bamax[0:1] if pl.du_amax else None, route=pl.temporal_dgrad)
    # weight gradients are reduced straight into the parameter's (out, in, kt, 1) layout: autograd takes them as they are
    G["tcn1.conv.weight"] = ops.tconv_wgrad(S["g_att"] if cfg.attention else S["g"], du, taps=kt, stride=s, conv_param=(1, cout), all_taps=False if pl.wide else None,
                                            amax=(S["amax"][1:2], bamax[0:1]) if pl.du_amax and pl.g_amax else None)
    G["tcn1.conv.bias"] = bias_grad.main(du, 0)
    if cfg.attention:
        # dG' -> dG in place (the plan keeps both float32 in an attention block), and the module's eight parameter gradients
        _, stc_grads = ops.stc_backward(dg, S["g"], S["stc"], [P[n] for n in stc_names()], out=dg)
        G.update(zip(stc_names(), stc_grads))

    # -- G = relu(BN(y) + down(x)) ---------------------------------------------------------------------------------------------
    if cfg.has_down:
        dy, dd, sums = ops.bn_act_bwd(dg, S["g"], S["y"], S["vec_y"], S["d"], S["vec_d"], res_mode=2, train=train,
                                      sign_mask=S["g_sign"], da_bf16=half_dy, db_bf16=hs, sums_out=bias_grad.sums_out(1))
        G["gcn1.down.1.weight"], G["gcn1.down.1.bias"] = sums[2], sums[0].clone()   # own memory: sums[0] is gcn1.bn.bias too
        pw_gemm(dd, W, "down_t", dx, K=cout, N=cx, accumulate=dx_live)
        dx_live = True
        G["gcn1.down.0.weight"] = ops.rows_wgrad(x_h if dd.dtype == torch.bfloat16 else xf(), dd, K=cin, N=cout, conv_param=(1, cin_true))
        G["gcn1.down.0.bias"] = bias_grad.shortcut(dd, 1)
    else:
        dy, _, sums = ops.bn_act_bwd(dg, S["g"], S["y"], S["vec_y"], x_h, None, res_mode=1, train=train, need_db=not gate_in_dagg,
                                     db=None if gate_in_dagg else dx, db_accumulate=dx_live, sign_mask=S["g_sign"],
                                     partials=g_partials if fuse_sums else None, da_bf16=half_dy, sums_out=bias_grad.sums_out(1))
        if gate_in_dagg:
            gated.append((as_extra(dg), S["g_sign"]))  # dx += dg * [g > 0]  (dx is still empty: both shortcuts are gated)
        dx_live = not gate_in_dagg
    G["gcn1.bn.weight"], G["gcn1.bn.bias"] = sums[1], sums[0]
    bias_grad.carry()

    # -- conv_d and the joint aggregation ------------------------------------------------------------------------------------------
    a_hat = S["a_hat"]
    c3 = 3 * cin
    dagg = None                  # (the gated list holds none or both shortcuts: gate_in_dagg needs an identity block without a down conv)
    if pl.spatial_bwd != "tile":
        # dagg = dy . Wd first: in math mode f16x2 the row GEMM records max |dy| (slot 3), the operand scale of conv_d's weight gradient
        dagg = new(B, T, V, c3)
        pw_gemm(dy, W, "d_t", dagg, K=cout, N=c3, amax_out=bamax[3:4] if pl.dy_amax else None)
    # weight gradient of conv_d: agg is recomputed (cheaper than keeping 3 activations per block) and contracted with dy
    if pl.spatial_wgrad == "tile":
        gw = ops.spatial_wgrad_tile(x_h if dy.dtype == torch.bfloat16 else xf(), dy, a_hat, conv_param=(NUM_SUBSETS, cin_true))   # agg on chip, whole frame tiles
    elif pl.spatial_wgrad == "fused":
        # agg = x . A^ is formed in registers and contracted with dy at once: never written
        gw = ops.spatial_wgrad(xf(), dy, a_hat, conv_param=(NUM_SUBSETS, cin_true))
    else:
        agg = new(B, T, V, c3)
        agg_amax = mix_agg(xf(), agg, a_hat, cin, amax_out=bamax[2:3] if pl.dy_amax else None)
        gw = ops.rows_wgrad(agg, dy, K=3 * cin, N=cout, conv_param=(NUM_SUBSETS, cin_true),   # (3, cout, cin_true, 1, 1)
                            amax=(bamax[2:3], bamax[3:4]) if agg_amax else None)
        del agg
    dbias = None if train else ops.col_sum(dy, cout)
    for k in range(NUM_SUBSETS):
        G[f"gcn1.conv_d.{k}.weight"] = gw[k]
        # three parameters, three buffers (the sum of the three biases is what the kernel adds: equal gradients)
        G[f"gcn1.conv_d.{k}.bias"] = bias_grad.main(dy, 1, k) if train else (dbias if k == 0 else dbias.clone())
    if pl.spatial_bwd == "tile":
        # dagg on chip: dx and dA^ in one launch (the bfloat16 x beside a bfloat16 dy, whatever dx is)
        part = ops.spatial_bwd_tile(dy, x_h if dy.dtype == torch.bfloat16 else xf(), a_hat, W["d_t_b3"], dx, accumulate=dx_live, gated=gated)
    elif pl.spatial_bwd == "dagg":
        part = ops.joint_dagg(xf(), dagg, a_hat, dx, accumulate=dx_live, gated=gated)   # dx and dA^ from one pass over dagg
    else:
        mix_dx(dagg, dx, a_hat, cin, accumulate=dx_live)
        part = ops.joint_gram(xf(), dagg, [(0, k * cin, cin) for k in range(NUM_SUBSETS)])
    dx_live = True
    d_a_hat, d_s = ops.adj_softmax_bwd(part, 1.0 / (ic * T), S["c_mat"], V)
    db = torch.empty_like(P["gcn1.adj_b"])
    ops.reduce_sum(d_a_hat.view(B, -1), db.view(-1), leaf=True)
    G["gcn1.adj_b"] = db

    # -- attention embeddings -----------------------------------------------------------------------------------------------------
    if not cfg.static_adjacency:
        emb = S["emb"]
        if pl.emb_bwd == "tile":
            # demb on chip: dx += demb . Wemb, then (a leaf) dWemb = demb^T . x and the bias gradient
            if x16 and not dx16 and pl.emb_bf16:
                # the last writer of this block's float32-accumulated dx hands it over as the bfloat16 tensor the bfloat16 input asks for
                dx16_out = torch.empty(dx.shape, device=dev, dtype=torch.bfloat16)
                ops.emb_dx_tile(emb, d_s, W["emb_t_b3"], dx16_out, ic=ic, accumulate=True, dx_old=dx)
                dx = dx16_out
            else:
                ops.emb_dx_tile(emb, d_s, W["emb_t_b3"], dx, ic=ic, accumulate=dx_live)
            gw, gb = ops.emb_wgrad_tile(emb, x_h if emb.dtype == torch.bfloat16 else xf(), d_s, ic=ic)
            gw = gw.view(6 * ic, cin_true, 1, 1)
        else:
            demb = new(B, T, V, 6 * ic)
            gb = mix_demb(emb, demb, d_s, ic)                                             # + column sums = bias gradient
            pw_gemm(demb, W, "emb_t", dx, K=6 * ic, N=cx, accumulate=dx_live, amax_out=bamax[1:2] if pl.demb_amax else None)
            gw = ops.rows_wgrad(xf(), demb, K=cin, N=6 * ic, conv_param=(1, cin_true),     # (6ic, cin_true, 1, 1)
                                amax=(S["amax"][0:1], bamax[1:2]) if pl.demb_amax else None)
        for k in range(NUM_SUBSETS):
            for j, grp in enumerate(("conv_a", "conv_b")):
                lo = (2 * k + j) * ic
                G[f"gcn1.{grp}.{k}.weight"] = gw[lo:lo + ic]
                G[f"gcn1.{grp}.{k}.bias"] = gb[lo:lo + ic]
    if x16 and dx.dtype != torch.bfloat16:
        dx = dx.to(torch.bfloat16)           # the gradient of a bfloat16 input (one rounding, as the bfloat16-writing kernels apply it)
    return (dx if need_dx else None), G


# ---- autograd ----------------------------------------------------------------------------------------------------------
class STBlockFunction(torch.autograd.Function):
    """y = SpatialTemporalConv(x); inputs: x, then the block's parameters in ``param_names(cfg)`` order."""

    @staticmethod
    def forward(ctx, x, cfg: BlockConfig, train: bool, bufs: Dict[str, torch.Tensor], W: Dict[str, torch.Tensor],
                holder: Optional[dict], *params):
        names = param_names(cfg)
        P = dict(zip(names, params))
        pool_groups = holder.get("pool_groups", 0) if holder is not None else 0
        inference = bool(holder.get("inference")) if holder is not None else False      # eval mode and no autograd graph (the module says)
        out_half = bool(holder.get("out_half")) if holder is not None else False        # the consumer takes a bfloat16 output (paths.half_activations)
        o, S = block_forward(x, P, bufs, W, cfg, train, pool_groups, inference=inference, out_half=out_half)
        B, T, V, _ = x.shape
        ctx.pool = (pool_groups, (B, (T - 1) // cfg.stride + 1, V, cfg.cout)) if pool_groups else None
        ctx.zeros = holder.get("zeros") if holder is not None else None      # the block's slice of the model's zero pool (or None)
        # the block's input and output go through save_for_backward (an output kept on ctx would be a reference cycle
        # o -> grad_fn -> ctx -> o that only the garbage collector frees); the other activations are private to the block
        # (the backward gates on the one-bit sign image of o, so o itself is only kept when that image does not exist;
        # nn.Dropout(inplace=True) after the block may then overwrite o freely, as in the reference's Model)
        keep_o = S["o_sign"] is None
        S["x"] = S["o"] = None
        ctx.cfg, ctx.train, ctx.names, ctx.W, ctx.S, ctx.keep_o = cfg, train, names, W, S, keep_o
        ctx.save_for_backward(x, *((o,) if keep_o else ()), *params)
        if holder is not None:
            holder["adj_c"] = S["c_mat"]
        return o

    @staticmethod
    def backward(ctx, d_o):
        if ctx.S is None:
            raise RuntimeError("STBlockFunction: backward ran twice -- the block frees its saved activations after the first "
                               "backward (retain_graph is not supported; run the forward again)")
        x, *params = ctx.saved_tensors
        o = params.pop(0) if ctx.keep_o else None
        P = dict(zip(ctx.names, params))
        S = dict(ctx.S, x=x, o=o)
        ctx.S = None
        dx, G = block_backward(d_o, S, P, ctx.W, ctx.cfg, ctx.train, need_dx=ctx.needs_input_grad[0], pool=ctx.pool, zeros=ctx.zeros)
        del S
        grads = []
        for i, n in enumerate(ctx.names):
            g = G.get(n) if ctx.needs_input_grad[6 + i] else None
            if g is None and ctx.needs_input_grad[6 + i]:
                g = torch.zeros_like(P[n])          # static-adjacency: embedding convs get no gradient
            grads.append(g)
        return (dx, None, None, None, None, None, *grads)


class LinearFunction(torch.autograd.Function):
    """logits = h . W^T + b on the row GEMM (reference: nn.Linear `fc`, mmargcn/agcn.py:177,200): keeps the classifier off
    hipBLASLt, whose `UserArgs` kernels do not survive HIP-graph replay at small row counts (the 8-clip shard of a
    strong-scaling run produced wrong logits from the second replay on)."""

    @staticmethod
    def forward(ctx, h: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor]):
        n, k = h.shape
        classes = weight.shape[0]
        npad = _r4(classes)
        wt = torch.zeros((1, k, npad), device=h.device, dtype=torch.float32)
        wt[0, :, :classes] = weight.t()
        bp = None
        if bias is not None:
            bp = torch.zeros(npad, device=h.device, dtype=torch.float32)
            bp[:classes] = bias
        hc = h.contiguous()
        out = torch.empty((n, 1, 1, npad), device=h.device, dtype=torch.float32)
        ops.rows_gemm(hc.view(n, 1, 1, k), wt, out, K=k, N=npad, bias=bp)
        ctx.save_for_backward(hc, weight)
        ctx.has_bias = bias is not None
        return out.view(n, npad)[:, :classes]

    @staticmethod
    def backward(ctx, d_out: torch.Tensor):
        hc, weight = ctx.saved_tensors
        n, k = hc.shape
        classes = weight.shape[0]
        npad = _r4(classes)
        dl = torch.zeros((n, 1, 1, npad), device=hc.device, dtype=torch.float32)
        dl.view(n, npad)[:, :classes] = d_out
        dh = dw = db = None
        if ctx.needs_input_grad[0]:
            w = torch.zeros((1, npad, k), device=hc.device, dtype=torch.float32)
            w[0, :classes] = weight
            dh = torch.empty((n, 1, 1, k), device=hc.device, dtype=torch.float32)
            ops.rows_gemm(dl, w, dh, K=npad, N=k)
            dh = dh.view(n, k)
        if ctx.needs_input_grad[1]:
            gw = ops.rows_wgrad(hc.view(n, 1, 1, k), dl, K=k, N=npad, wide=False)      # (1, k, npad)
            dw = gw[0, :, :classes].t().contiguous()
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = ops.col_sum(dl.view(n, 1, 1, npad), npad)[:classes].contiguous()
        return dh, dw, db


class GroupMeanFunction(torch.autograd.Function):
    """(G, R, C) -> (G, C) global average pooling on fgcn_group_mean (reference: x.view(N, M, c, -1).mean(3).mean(1),
    mmargcn/agcn.py:196-197 -- equal-sized groups, so one mean over all M*T'*V rows of a clip)."""

    @staticmethod
    def forward(ctx, x: torch.Tensor):
        ctx.shape = tuple(x.shape)
        return ops.group_mean(x.contiguous())

    @staticmethod
    def backward(ctx, d_out: torch.Tensor):
        G, R, C = ctx.shape
        return (d_out / R).unsqueeze(1).expand(G, R, C).contiguous()


class DataBNFunction(torch.autograd.Function):
    """data_bn (nn.BatchNorm1d over the (m, v, c) channels of the network input, statistics across (n, t); reference
    mmargcn/agcn.py:150,186-188) fused with the layout change the blocks need: (N, M, T, V, C) -> (N*M, T, V, C padded to 4).
    The nn.BatchNorm1d module is the parameter / buffer container (momentum 0.1-style exponential running statistics)."""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, train: bool, momentum: float, eps: float):
        x = x.contiguous()
        N, M, T, V, C = x.shape
        if train:
            vec = ops.bn_finalize(ops.data_bn_stats(x, centered=True), N * T, weight, bias, running_mean, running_var, momentum, eps,
                                  pivot=x)
        else:
            vec = ops.bn_eval_coeffs(weight, bias, running_mean, running_var, eps)
        ctx.save_for_backward(x, vec)
        ctx.train = train
        return ops.data_bn_apply(x, vec, _r4(C))

    @staticmethod
    def backward(ctx, d_out):
        x, vec = ctx.saved_tensors
        dgamma, dbeta, dx = ops.data_bn_bwd(d_out.contiguous(), x, vec, ctx.train, ctx.needs_input_grad[0])
        return dx, dgamma, dbeta, None, None, None, None, None


def data_bn(x: torch.Tensor, bn: torch.nn.BatchNorm1d) -> torch.Tensor:
    """The model's input stage on libfgcn: ``bn`` = the model's ``data_bn`` module; updates its running statistics and batch
    counter in train mode like the module's own forward would."""
    if bn.momentum is None or not bn.affine or not bn.track_running_stats:
        raise NotImplementedError("data_bn: affine BatchNorm1d with exponential running statistics (the reference's default) only")
    if x.shape[1] * x.shape[3] * x.shape[4] != bn.num_features:
        raise ValueError(f"data_bn: input {tuple(x.shape)} does not have {bn.num_features} (m, v, c) channels")
    out = DataBNFunction.apply(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.training, bn.momentum, bn.eps)
    if bn.training:
        bn.num_batches_tracked.add_(1)
    return out


class PatchInputFunction(torch.autograd.Function):
    """The input stage of the RGB patch-feature early-fusion modes (reference mmargcn/early_fusion_models.py:48-90, 163-210) in front of
    data_bn: reducer Linear(P, H) . Linear(H, Q), zero rows for the joints without a patch, fusion with the skeleton rows -- one
    fgcn_patch_input_fwd pass that also leaves data_bn's statistics partials -- then data_bn's finalize / apply.  Backward: data_bn's dx
    (the network input's gradient) -> fgcn_patch_input_bwd -> the reducer's four gradients.  Skeleton and patch rows are data."""

    @staticmethod
    def forward(ctx, s, p, w1, b1, w2, b2, weight, bias, running_mean, running_var, train: bool, momentum: float, eps: float, V: int,
                fusion: str):
        s = None if s is None else s.contiguous()
        p = p.contiguous()
        z, part = ops.patch_input_fwd(s, p, w1, b1, w2, b2, V=V, fusion=fusion, stats=train, centered=True)
        N, T, C = z.shape[0], z.shape[2], z.shape[4]
        if train:
            vec = ops.bn_finalize(part, N * T, weight, bias, running_mean, running_var, momentum, eps, pivot=z)
        else:
            vec = ops.bn_eval_coeffs(weight, bias, running_mean, running_var, eps)
        ctx.save_for_backward(z, vec, s, p, w1, b1, w2)
        ctx.train, ctx.fusion = train, fusion
        return ops.data_bn_apply(z, vec, _r4(C))

    @staticmethod
    def backward(ctx, d_out):
        z, vec, s, p, w1, b1, w2 = ctx.saved_tensors
        need = w1 is not None and any(ctx.needs_input_grad[2:6])
        dgamma, dbeta, dz = ops.data_bn_bwd(d_out.contiguous(), z, vec, ctx.train, need)
        dw1 = db1 = dw2 = db2 = None
        if need:
            dw1, db1, dw2, db2 = ops.patch_input_bwd(dz, s, p, w1, b1, w2, fusion=ctx.fusion)
        return None, None, dw1, db1, dw2, db2, dgamma, dbeta, None, None, None, None, None, None, None


def patch_input(s: Optional[torch.Tensor], p: torch.Tensor, reducer: Optional[Sequence[torch.nn.Linear]], bn: torch.nn.BatchNorm1d,
                V: int, fusion: str) -> torch.Tensor:
    """The patch-feature modes' network input -> what ``data_bn`` returns: s (N, M, T, V, Cs) skeleton rows or None, p (N, M, T, Vp, P)
    patch rows, ``reducer`` = the two nn.Linear of ``patch_feature_dim_reducer`` or None (identity), ``bn`` = the model's data_bn.
    ``paths.patch_input_fused`` off (this math mode's entry): the same function composed of the row GEMM (LinearFunction, twice), zero pad, the fusion's torch
    reduction and ``data_bn`` (the A/B route)."""
    if fusion not in ops.PATCH_FUSIONS:
        raise ValueError(f"unsupported fusion {fusion!r} for the patch-feature input (known: {', '.join(ops.PATCH_FUSIONS)})")
    N, M, T, Vp, P = p.shape
    if not ops.paths().get("patch_input_fused", ops.get_math_mode()) or (s is None and reducer is None):
        q = p
        if reducer is not None:
            h = LinearFunction.apply(p.reshape(-1, P), reducer[0].weight, reducer[0].bias)
            q = LinearFunction.apply(h, reducer[1].weight, reducer[1].bias).reshape(N, M, T, Vp, -1)
        if Vp < V:
            q = F.pad(q, (0, 0, 0, V - Vp))
        if s is None:
            z = q
        elif fusion == "concatenate":
            z = torch.cat((s, q), dim=-1)
        elif fusion == "sum":
            z = s + q
        elif fusion == "product":
            z = s * q
        else:
            z = torch.stack((s, q), dim=-1).mean(-1)
        return data_bn(z, bn)
    if bn.momentum is None or not bn.affine or not bn.track_running_stats:
        raise NotImplementedError("data_bn: affine BatchNorm1d with exponential running statistics (the reference's default) only")
    w = (None,) * 4 if reducer is None else (reducer[0].weight, reducer[0].bias, reducer[1].weight, reducer[1].bias)
    out = PatchInputFunction.apply(s, p, *w, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.training, bn.momentum, bn.eps,
                                   V, fusion)
    if bn.training:
        bn.num_batches_tracked.add_(1)
    return out


class CrossEntropyFunction(torch.autograd.Function):
    """nn.CrossEntropyLoss() / F.cross_entropy(logits, labels), mean reduction (reference session/session.py:53): one
    fixed-order kernel each way."""

    @staticmethod
    def forward(ctx, logits, labels):
        loss, probs = ops.cross_entropy_fwd(logits, labels)
        ctx.save_for_backward(probs, labels, loss)
        return loss[0]

    @staticmethod
    def backward(ctx, d_loss):
        probs, labels, loss = ctx.saved_tensors
        return ops.cross_entropy_bwd(probs, labels, loss, d_loss.contiguous().view(1)), None


def cross_entropy(logits: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    return CrossEntropyFunction.apply(logits, labels)


class CrossEntropyOptionsFunction(torch.autograd.Function):
    """F.cross_entropy(logits, target, weight, ignore_index=, reduction=, label_smoothing=) with int64 labels or float32 class
    probabilities (``fgcn_ce_fwd`` / ``_bwd``, include/fgcn.h): fixed-order sums each way; softmax is not stored when the logits need
    no gradient.  The target and the weight get no gradient (data)."""

    @staticmethod
    def forward(ctx, logits, target, weight, ignore_index, reduction, label_smoothing, need):
        loss, row_loss, row_scale, probs = ops.cross_entropy_opts_fwd(logits, target, weight, ignore_index=ignore_index,
                                                                      reduction=reduction, label_smoothing=label_smoothing,
                                                                      need_probs=need)
        if need:
            ctx.save_for_backward(probs, target, weight, row_scale, loss)
        ctx.options = dict(ignore_index=ignore_index, reduction=reduction, label_smoothing=label_smoothing)
        return row_loss if reduction == "none" else loss[0]

    @staticmethod
    def backward(ctx, d_loss):
        probs, target, weight, row_scale, loss = ctx.saved_tensors
        d_loss = d_loss.contiguous().view(-1)
        return ops.cross_entropy_opts_bwd(probs, target, weight, row_scale, loss, d_loss, **ctx.options), None, None, None, None, None, None


def cross_entropy_options(logits: torch.Tensor, target: torch.Tensor, weight: Optional[torch.Tensor] = None, ignore_index: int = -100,
                          reduction: str = "mean", label_smoothing: float = 0.0) -> torch.Tensor:
    need = torch.is_grad_enabled() and logits.requires_grad          # (forward() itself always runs with grad mode off)
    return CrossEntropyOptionsFunction.apply(logits, target, weight, ignore_index, reduction, label_smoothing, need)


ops.bind_all_functions(globals())     # every Function's backward runs in its forward's library context (ops.Context)
