"""Which libfgcn kernel form every stage of one AGCN block runs, and in which storage type each activation-sized tensor is kept: decided
ONCE per block call, here, as one frozen ``BlockPlan``.  block.block_forward reads the math mode and the context's PathOptions once, calls
``plan_block`` and keeps the plan in its saved dict (``S["plan"]``); block._temporal_stage and block._block_backward dispatch on its fields
and evaluate no route predicate of their own.  So the backward FOLLOWS THE PLAN ITS FORWARD MADE ("a backward sees its forward's options",
DESIGN.md section 1), and a cross-stage dependency (emb is bfloat16 only if the embedding backward takes its tile kernels, ...) is written
once, in the direction it has.  Kernel availability comes from the queries of ops.py, each asked at most once per plan.  What only the
backward sees -- the storage type of the incoming gradient -- is a run-time refinement applied there (``BlockPlan.refine_dx``)."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

from . import ops

# widest input and output of fgcn_spatial_fwd (eight 32-channel tiles each, fgcn_spatial.hip); a wider block -- the 512 / 516 input channels of
# the RGB patch-feature modes' first block, the 384 / 512 output channels of a model with start_feature_size 128 / 192 where the tile form
# is off or not built (math mode f32) -- takes the joint mixing + row GEMM form of the spatial stage
SPATIAL_FWD_MAX_C = 256


def fits32(elements: int) -> bool:
    """Whether a float32 tensor of this many elements is addressable with the 32-bit byte offsets of the tile kernels."""
    return elements * 4 < 0x7FFF0000      # BUFFER_LIMIT of csrc/fgcn_common.hpp (fits_buffer)


def pw_min_k(rows: int, mode: Optional[str] = None, o=None) -> int:
    """contraction depth from which a 1x1 convolution with a split form goes to the persistent split-bf16 row GEMM (ops.pw_gemm); below
    it, and in math mode f32, the exact-f32 row GEMM runs (paths.PathOptions.pw_min_k).  No ``mode`` / ``o``: the current context's."""
    o = o or ops.paths()
    if (mode or ops.get_math_mode()) == "f16x2":
        return o.pw_min_k_f16x2
    return min(o.pw_min_k, 64) if rows < o.pw_small_rows else o.pw_min_k


def pw_routed(forms, key: str, K: int, rows: int, mode: Optional[str] = None, o=None) -> bool:
    """Whether block.pw_gemm sends the 1x1 convolution ``key`` over ``rows`` rows of exactly K channels to the split row GEMM (it records max |x|)"""
    return (key + "_s3") in forms and K % 32 == 0 and K >= pw_min_k(rows, mode, o)


def temporal_route(forms, kt: int, s: int, T: int, wide: bool, direction: str) -> str:
    """The kernel of the (kt x 1, stride s) temporal conv over T input frames, ``direction`` "fwd" or "dgrad": "halo" (one halo-tile launch,
    stride 1), "halo_parity" (stride 2: an even-tap and an odd-tap halo pass) or "rows" (the per-tap row GEMM: a wide graph, an odd half
    padding, a form the packed set lacks).  Only the halo routes record max |input| in math mode f16x2 and take bfloat16 operands.  The
    directions differ in one term: the strided forward asks T > 1, the strided data gradient does not (temporal_dgrad skips its empty pass)."""
    key = "t4" if direction == "fwd" else "t_t4"
    if wide:
        return "rows"
    if s == 1 and key in forms:
        return "halo"
    if s == 2 and key + "_e" in forms and ((kt - 1) // 2) % 2 == 0 and (T > 1 or direction != "fwd"):
        return "halo_parity"
    return "rows"


@dataclass(frozen=True)
class BlockPlan:
    mode: str
    train: bool
    pool_groups: int
    wide: bool                  # more than 32 joints: the wide joint kernels, the joint-mix spatial form, the row-GEMM temporal conv
    half_activations: bool      # math mode bf16 training step with paths.half_activations: activation-sized tensors are bfloat16 where planned
    x_bf16: bool                # the block's input arrived as bfloat16: its gradient leaves as bfloat16
    # -- forward ---------------------------------------------------------------------------------------------------------------------
    emb_fwd: Optional[str]      # "tile" (gram on chip) | "gemm" (1x1 product + joint_gram) | None: static adjacency
    write_emb: bool             # False: inference, nothing reads the embeddings
    emb_bf16: bool
    x_amax: bool                # f16x2 slots really recorded by the forward (0 = max |x|, 1 = max |G|) ...
    g_amax: bool
    spatial_fwd: str            # "tile_bn_relu" (inference epilogue) | "tile" | "fused" | "mix"
    y_bf16: bool
    g_bf16: bool                # paths.half_storage: G, and with it dU, stored as bfloat16
    shortcuts_bf16: bool        # the down / residual conv's output, computed from the bfloat16 x
    fuse_g: bool                # G = relu(BatchNorm(y) + x) formed inside the temporal conv
    g_sign: bool                # the one-bit sign images exist (element counts in 8s; asserted by the backward)
    o_sign: bool
    temporal_fwd: str           # temporal_route(..., "fwd")
    temporal_bn_relu: bool      # inference: BatchNorm + shortcut + ReLU in the temporal conv's epilogue
    u_bf16: bool
    o_bf16: bool
    # -- backward --------------------------------------------------------------------------------------------------------------------
    temporal_dgrad: str         # temporal_route(..., "dgrad")
    du_amax: bool               # ... and by the backward (0 = max |du|, 1 = max |demb|, 3 = max |dy|; 2 = max |agg| is mix_agg's answer)
    dy_amax: bool
    demb_amax: bool
    bn_sums_in_dgrad: bool      # the graph convolution's BatchNorm-backward sums in the temporal data gradient's epilogue
    spatial_bwd: str            # "tile" (dx and dA^ in one launch) | "dagg" (row GEMM + joint_dagg) | "mix" (row GEMM + mix_dx + joint_gram)
    spatial_wgrad: str          # "tile" | "fused" (aggregation recomputed in registers) | "mix" (mix_agg + rows_wgrad)
    emb_bwd: Optional[str]      # "tile" | "chain" (mix_demb + 1x1 product + rows_wgrad) | None: static adjacency
    gate_in_dagg: bool          # both identity shortcuts' gated gradients are added to dx by the spatial backward kernel
    pool_rows: bool             # last block: the pooled gradient is read as one row per group
    dy_bf16: bool
    dshortcuts_bf16: bool       # the shortcut branches' gradients (dd / dr), their kernels on the bfloat16 x
    dg_bf16: bool               # dG / dx as bfloat16 tensors, before the run-time refinement (refine_dx)
    dx_bf16: bool

    def refine_dx(self, d_o_bf16: bool) -> Tuple[bool, bool]:
        """-> (dx, dG are bfloat16 tensors), given the incoming gradient's storage type: a gated addend has dx's storage type (the fused
        backward adds it), so a gated float32 d_o that is not read as per-group rows keeps dx float32, and dG, the other addend, follows dx."""
        dx16 = self.dx_bf16 and (not self.gate_in_dagg or d_o_bf16 or self.pool_rows)
        return dx16, self.dg_bf16 and (dx16 or not self.gate_in_dagg)


def plan_block(cfg, B: int, T: int, V: int, *, x_bf16: bool, train: bool, inference: bool, pool_groups: int, out_half: bool,
               forms, mode: str, paths, kt: int = 9) -> BlockPlan:
    """The plan of one block call: ``cfg`` the block.BlockConfig, (B, T, V) the input's samples / frames / joints, ``forms`` the packed set
    (``key in forms``), ``mode`` / ``paths`` the calling context's math mode and PathOptions, ``kt`` the temporal conv's taps.  (The inline
    code's ``x.shape[3] == cin`` terms are gone: the planner's cin IS cfg.cx, which block_forward asserts of x.)"""
    o = paths
    cin, cout, ic, s = cfg.cx, cfg.cout, cfg.ic, cfg.stride
    rows, o_numel = B * T * V, B * ((T - 1) // s + 1) * V * cfg.cout
    f16x2, split_bf16 = mode == "f16x2", mode in ("bf16x3", "bf16")
    wide = ops.wide_graph(V)

    def bf16_step(option: str) -> bool:          # a training step in math mode bf16 with this per-mode option on
        return bool(train and mode == "bf16" and o.get(option, "bf16"))
    half_storage = bf16_step("half_storage")
    ha = half_storage and bf16_step("half_activations") and not wide      # (the typed bfloat16 forms are 32-joint kernels)
    if x_bf16 and not ha:
        raise ops._lib.FgcnError("block_forward: a bfloat16 input needs math mode bf16 with paths.half_activations (a training step)")
    no_emb = bool(inference and not train and o.fused_inference)          # inference: no embeddings written, no pre-BatchNorm tensors
    infer = no_emb and ops.inference_kernels_available()
    halo_sums = ops.tconv_halo_bn_sums()
    t_fwd, t_dgrad = (temporal_route(forms, kt, s, T, wide, d) for d in ("fwd", "dgrad"))
    halo9 = s == 1 and kt > 1 and "t4" in forms                           # the stride-1 halo conv proper (not a 1x1)

    # -- attention embeddings: the backward first, because the forward stores emb as bfloat16 only for the backward's tile kernels
    emb_fwd = emb_bwd = None
    if not cfg.static_adjacency:
        emb_bwd = "tile" if (o.emb_tile and cin <= o.get("emb_tile_max_cin", mode) and "emb_t_b3" in forms and cin == cfg.cin
                             and ops.emb_tile_available(V, ic, cin) and fits32(rows * max(6 * ic, cin))) else "chain"
        # (inference: the tile form writes no embeddings at all -- it stays at every ic)
        emb_fwd = "tile" if (o.emb_fwd_tile and cin <= o.get("emb_fwd_tile_max_cin", mode) and (no_emb or ic <= o.get("emb_fwd_tile_max_ic", mode))
                             and "emb_b3" in forms and ops.emb_fwd_tile_available(V, ic, cin) and fits32(rows * max(cin, 6 * ic))) else "gemm"
    emb_bf16 = emb_fwd == "tile" and half_storage and emb_bwd == "tile"
    x_amax = emb_fwd == "gemm" and f16x2 and pw_routed(forms, "emb", cin, rows, mode, o)

    # -- spatial aggregation + conv_d, G
    tile_form = bool(cfg.fused_spatial and "d_s3" in forms and ops.spatial_fwd_tile_available(V, cin, cout))
    if infer and tile_form and (cfg.has_down or cin >= cout):
        spatial_fwd = "tile_bn_relu"
    elif tile_form and o.spatial_tile and cout >= o.get("spatial_tile_min_cout", mode):
        spatial_fwd = "tile"
    else:
        spatial_fwd = "fused" if (cfg.fused_spatial and max(cin, cout) <= SPATIAL_FWD_MAX_C and not wide) else "mix"
    staged = spatial_fwd != "tile_bn_relu"       # y, G and G's sign image exist (everything bfloat16 below needs a training step anyway)
    # (Y as bfloat16: not when the temporal data gradient is to carry the BatchNorm-backward sums -- that epilogue reads Y as float32)
    y_bf16 = bool(ha and o.half_spatial_out and not o.get("bn_sums_in_dgrad", mode) and spatial_fwd == "tile")
    # G and dU in bfloat16: their three consumers on their bfloat16-input kernels -- the halo conv forward and data gradient, and the all-taps
    # weight gradient (tap counts it is built for).  (The inline code asked the two routes without V here, a wide graph already excluded.)
    pad = (kt - 1) // 2
    per_pass = [kt] if s == 1 else [len([j for j in range(kt) if (j - pad) % s == par]) for par in range(s)]
    # An attention block (BlockConfig.attention) keeps G, G', dU and dG float32 and forms G in a pass of its own: the STC kernels between
    # the graph convolution and the temporal conv are float32, and fuse_g / bn_sums_in_dgrad fuse across the place where the gate sits
    att = bool(getattr(cfg, "attention", False))
    g_bf16 = bool(not att and half_storage and kt > 1 and not wide and t_fwd != "rows" and t_dgrad != "rows"
                  and all(n in ops.TWGRAD_TAPS_SPLIT for n in per_pass if n))
    g_sign = staged and (rows * cout) % 8 == 0
    # (the conv's fused input stage exists with the bf16x3 / bf16 products only: fgcn_tconv_halo refuses it with the f16x2 products, whose
    # BatchNorm-sums epilogue -- halo_sums -- does exist)
    fuse_g = bool(not att and staged and o.fuse_g and not f16x2 and not g_bf16 and not ha and not cfg.has_down and halo9 and halo_sums
                  and cin == cout and V <= 32 and (rows * cout) % 8 == 0)
    if g_bf16 and not g_sign:    # (no sign image: the backward would gate on g itself, which it reads as f32 -- cout % 64 == 0 rules it out)
        raise ops._lib.FgcnError("half-precision storage of G needs the sign image (element count a multiple of 8)")

    # -- temporal conv, O
    temporal_bn_relu = bool(infer and halo9 and not pool_groups and not wide and cfg.residual in ("none", "identity", "conv")
                            and (cfg.residual != "identity" or cin == cout))
    # U as bfloat16 where its conv has the form (the stride-1 halo kernel on a bfloat16 G; the strided conv's second pass accumulates: float32)
    u_bf16 = bool(ha and o.half_conv_out and g_bf16 and halo9 and not fuse_g)
    o_bf16 = bool(ha and out_half and not pool_groups)
    o_sign = not temporal_bn_relu and (pool_groups > 0 or o_numel % 8 == 0)
    if o_bf16 and not o_sign:
        raise ops._lib.FgcnError("half-precision storage of the block's output needs the sign image (element count a multiple of 8)")

    # -- backward: the spatial stage's two kernels, then the storage types in dependency order (dG, dY, dx)
    bwd_fits = fits32(rows * max(cin, cout))
    bwd_tile = bool(o.spatial_bwd_tile and cin >= o.spatial_bwd_tile_min_cin and "d_t_b3" in forms and ops.spatial_bwd_tile_available(V, cin, cout)
                    and (split_bf16 or o.spatial_bwd_tile_f16x2) and bwd_fits)
    wgrad_tile = bool(o.spatial_wgrad_tile and ops.spatial_wgrad_tile_available(V, cin, cout) and bwd_fits
                      and (split_bf16 or o.spatial_wgrad_tile_f16x2))
    wgrad_fused = o.fused_agg_wgrad and cin >= 32 and not wide and cout <= o.get("fused_agg_wgrad_max_cout", mode)
    # identity shortcuts (the graph convolution's `y += x` and the block residual) send the ReLU-gated incoming gradients straight to dx:
    # the kernel that forms the spatial term of dx adds both from their sign images
    gate_in_dagg = bool((o.gated_shortcuts_tile if bwd_tile else o.gated_shortcuts) and o.fused_dagg and not wide and not cfg.has_down
                        and cfg.residual == "identity" and cin == cfg.cin and cout % 8 == 0 and o_sign and g_sign and fits32(o_numel))
    bn_sums = bool(not att and o.get("bn_sums_in_dgrad", mode) and cout <= o.bn_sums_max_c and train and s == 1 and not cfg.has_down and g_sign
                   and "t_t4" in forms and halo_sums and not wide)
    # dG: written by the temporal data gradient's halo kernel from a bfloat16 dU; not when that kernel's epilogue carries the BatchNorm sums
    dg_bf16 = bool(ha and g_bf16 and t_dgrad != "rows" and not bn_sums and g_sign)
    # dY: both of its consumers on their tile kernels (only their staging reads it)
    dy_bf16 = bool(half_storage and wgrad_tile and bwd_tile and g_sign)
    # dx: every writer of dx must have the bfloat16 form -- the fused spatial backward first (with both gated shortcuts, or none to add),
    # then the embedding tile kernel; a residual / down conv or an ungated shortcut writes float32, and the block converts at the end.
    # (A block without a down conv always has the graph convolution's identity shortcut `y += x`: ungated -- also in a block without a
    # residual, where nothing can gate it -- bn_act_bwd writes its gradient into dx, which it takes as float32 only.)
    dx_bf16 = bool(x_bf16 and ha and bwd_tile and dy_bf16 and not cfg.has_down and cfg.residual != "conv"
                   and gate_in_dagg and (cfg.static_adjacency or (emb_bwd == "tile" and emb_bf16)) and dg_bf16)
    return BlockPlan(
        mode=mode, train=train, pool_groups=pool_groups, wide=wide, half_activations=ha, x_bf16=x_bf16,
        emb_fwd=emb_fwd, write_emb=emb_fwd == "gemm" or not no_emb, emb_bf16=emb_bf16, x_amax=x_amax, g_amax=f16x2 and t_fwd != "rows",
        spatial_fwd=spatial_fwd, y_bf16=y_bf16, g_bf16=g_bf16, shortcuts_bf16=bool(ha and o.half_shortcuts), fuse_g=fuse_g, g_sign=g_sign,
        o_sign=o_sign, temporal_fwd=t_fwd, temporal_bn_relu=temporal_bn_relu, u_bf16=u_bf16, o_bf16=o_bf16,
        temporal_dgrad=t_dgrad, du_amax=f16x2 and t_dgrad != "rows",
        dy_amax=f16x2 and not bwd_tile and pw_routed(forms, "d_t", cout, rows, mode, o),
        demb_amax=x_amax and emb_bwd == "chain" and pw_routed(forms, "emb_t", 6 * ic, rows, mode, o), bn_sums_in_dgrad=bn_sums,
        spatial_bwd="tile" if bwd_tile else ("dagg" if o.fused_dagg and not wide else "mix"), emb_bwd=emb_bwd,
        spatial_wgrad="tile" if wgrad_tile else ("fused" if wgrad_fused else "mix"),
        gate_in_dagg=gate_in_dagg, pool_rows=bool(pool_groups and o.pool_backward_rows and (not gate_in_dagg or bwd_tile)),
        dy_bf16=dy_bf16, dshortcuts_bf16=bool(x_bf16 and ha and o.half_shortcuts and cin % 32 == 0 and cout % 8 == 0),
        dg_bf16=dg_bf16, dx_bf16=dx_bf16)
