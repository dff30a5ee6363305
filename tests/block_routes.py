"""The route matrix of one AGCN block, as data, and the block-against-oracle harness that runs it (a helper module: no test, no conftest).

routes.plan_block picks a kernel chain per stage from the math mode, the phase, the block's shape and the context's PathOptions.  ``matrix``
lists, per math mode and phase, one option set per DISTINCT plan that ``CASES`` x ``option_sets`` can produce; tests/test_block_routes.py
proves on the host that the list leaves no route out, tests/test_block_routes_gpu.py executes every entry against the float64 oracle.
``WIDE_CASES`` is a second case list, the blocks of models wider than 64 / 128 / 256 channels; ``matrix(mode, phase, WIDE_CASES)`` is what
tests/test_wide_channels_gpu.py executes (deduplicated on the route tuple: ``matrix_key``).

A new PathOptions field has to be entered in ``OPTION_HANDLING`` and a new BlockPlan field in ``PLAN_CONTEXT_FIELDS`` / ``PLAN_ROUTE_FIELDS``
(the closure test fails until it is): that is how a new route or option joins the check."""
from __future__ import annotations

import dataclasses
import functools
from collections import namedtuple
from typing import Dict, Iterator, List, Tuple

import numpy as np
import torch

import guarded
from conftest import rel_l2

ALL_MODES = ("f32", "bf16x3", "f16x2", "bf16")
PHASES = ("train", "eval")       # eval = module.eval() with autograd on: block_forward(train=False, inference=False), running-statistics BatchNorm
B = 3

Case = namedtuple("Case", "name cin cout stride residual V T fused static")
# the seven blocks of test_block_model_gpu.test_block_forward_backward_vs_oracle (same shapes), a block without a residual, a down conv
# without stride and a static-adjacency block; cout % 64 == 0 everywhere, so both sign images always exist
CASES = (
    Case("first", 3, 64, 1, False, 25, 12, True, False),
    Case("identity64", 64, 64, 1, True, 25, 12, True, False),
    Case("identity64_unfused", 64, 64, 1, True, 18, 9, False, False),
    Case("down_s2", 64, 128, 2, True, 22, 13, True, False),
    Case("identity128", 128, 128, 1, True, 25, 8, True, False),
    Case("down_s2_256", 128, 256, 2, True, 27, 10, True, False),
    Case("identity256", 256, 256, 1, True, 20, 6, True, False),
    Case("noresidual64", 64, 64, 1, False, 25, 12, True, False),
    Case("down_s1", 64, 128, 1, True, 25, 12, True, False),
    Case("static64", 64, 64, 1, True, 25, 10, True, True),
)
# the same block at the channel widths of a model with start_feature_size 128 / 192, and a 320-wide one whose third 128-column tile is ragged:
# three and four column tiles in the halo conv and pw_gemm, 6 to 16 k-steps of 32 channels per tap, 3 to 5 channel groups in the spatial weight
# gradient.  The smallest shapes that still give every kernel two row tiles and a ragged last one at B = 3; from 192 channels upward behind
# the 3-channel first block.  tests/test_wide_channels_gpu.py executes ``matrix(mode, phase, WIDE_CASES)``
WIDE_CASES = (
    Case("first128", 3, 128, 1, False, 25, 8, True, False),
    Case("identity192", 192, 192, 1, True, 25, 8, True, False),
    Case("down_s2_384", 192, 384, 2, True, 22, 9, True, False),
    Case("identity320", 320, 320, 1, True, 18, 7, True, False),
    Case("down_s2_512", 256, 512, 2, True, 25, 9, True, False),
    Case("identity512", 512, 512, 1, True, 20, 6, True, False),
)

# ---- what the matrix knows of the two dataclasses (the closure test compares these tables with dataclasses.fields) ---------------------------
# PathOptions: "flip" = a boolean (per-mode boolean) flipped alone by test_block_plan.option_sets; "threshold" = an integer / tuple moved across
# the cases' sizes below; "model" = read by the model, not by a block call with pool_groups == 0 (run in the model-level leg); "other" = not read
# by an AGCN block at all
OPTION_HANDLING = {
    "pw_min_k": "threshold", "pw_min_k_f16x2": "threshold", "pw_small_rows": "threshold",
    "fuse_g": "flip", "spatial_tile": "flip", "spatial_tile_min_cout": "threshold", "spatial_bwd_tile": "flip",
    "spatial_bwd_tile_min_cin": "threshold", "spatial_bwd_tile_f16x2": "flip", "fused_dagg": "flip", "bn_sums_in_dgrad": "flip",
    "bn_sums_max_c": "threshold", "gated_shortcuts": "flip", "gated_shortcuts_tile": "flip", "spatial_wgrad_tile": "flip",
    "spatial_wgrad_tile_f16x2": "flip", "fused_agg_wgrad": "flip", "fused_agg_wgrad_max_cout": "threshold", "emb_tile": "flip",
    "emb_tile_max_cin": "threshold", "emb_fwd_tile": "flip", "emb_fwd_tile_max_cin": "threshold", "emb_fwd_tile_max_ic": "threshold",
    "half_storage": "flip", "half_activations": "flip", "half_conv_out": "flip", "half_spatial_out": "flip", "half_shortcuts": "flip",
    "fused_inference": "flip", "pool_epilogue": "model", "pool_backward_rows": "model", "mix_vw_order": "threshold",
    "patch_input_fused": "other", "graph_spmm_auto": "other", "graph_spmm_auto_density_ppm": "other",
}
# (name, FGCN_PATHS spec): the integer thresholds moved across the cases' sizes.  The cases have far fewer rows than pw_small_rows, where
# pw_min_k is capped at 64: the pw_small_rows=0 sets lift the cap so that pw_min_k decides
THRESHOLD_SETS = (
    ("pw_min_k=64", "pw_min_k=64"), ("pw_min_k=max", "pw_min_k=1073741824"),
    ("pw_small_rows=0", "pw_small_rows=0"), ("pw_small_rows=0+pw_min_k=max", "pw_small_rows=0,pw_min_k=1073741824"),
    ("pw_min_k_f16x2=128", "pw_min_k_f16x2=128"), ("pw_min_k_f16x2=max", "pw_min_k_f16x2=1073741824"),
    ("spatial_tile_min_cout=64", "spatial_tile_min_cout=64"), ("spatial_tile_min_cout=512", "spatial_tile_min_cout=512"),
    ("spatial_bwd_tile_min_cin=128", "spatial_bwd_tile_min_cin=128"),
    ("emb_tile_max_cin=64", "emb_tile_max_cin=64"), ("emb_tile_max_cin=256", "emb_tile_max_cin=256"),
    ("emb_fwd_tile_max_cin=64", "emb_fwd_tile_max_cin=64"), ("emb_fwd_tile_max_cin=256", "emb_fwd_tile_max_cin=256"),
    ("emb_fwd_tile_max_ic=16", "emb_fwd_tile_max_ic=16"), ("emb_fwd_tile_max_ic=64", "emb_fwd_tile_max_ic=64"),
    ("fused_agg_wgrad_max_cout=64", "fused_agg_wgrad_max_cout=64"), ("fused_agg_wgrad_max_cout=256", "fused_agg_wgrad_max_cout=256"),
    ("bn_sums_max_c=64", "bn_sums_max_c=64"), ("mix_vw_order=1:2", "mix_vw_order=1:2"),
)
ALL_UNFUSED = "emb_tile=0,emb_fwd_tile=0,spatial_bwd_tile=0,spatial_wgrad_tile=0,bn_sums_in_dgrad=0"      # the set of tests/test_context_gpu.py
# what a single flip cannot express, because the fused form shadows the older one
COMPOSITE_SETS = (
    ("spatial_bwd_tile=0+fused_dagg=0", "spatial_bwd_tile=0,fused_dagg=0"),                      # -> spatial_bwd "mix" (mix_dx + joint_gram)
    ("spatial_bwd_tile=0+gated_shortcuts=1", "spatial_bwd_tile=0,gated_shortcuts=1"),            # -> joint_dagg with gated addends
    ("spatial_wgrad_tile=0+fused_agg_wgrad=1", "spatial_wgrad_tile=0,fused_agg_wgrad=1,fused_agg_wgrad_max_cout=256"),   # -> "fused"
    ("spatial_wgrad_tile=0+fused_agg_wgrad=0", "spatial_wgrad_tile=0,fused_agg_wgrad=0"),        # -> "mix" (mix_agg + rows_wgrad)
    ("spatial_tile=0", "spatial_tile=0"),
    ("all_unfused", ALL_UNFUSED),
    ("all_unfused+mix_vw_order=1:2", ALL_UNFUSED + ",fused_dagg=0,fused_agg_wgrad=0,mix_vw_order=1:2"),
    ("fuse_g=1", "fuse_g=1"),
    ("fuse_g=1+half_storage=0", "fuse_g=1,half_storage=0"),                                     # math mode bf16: G formed in the conv is float32
    ("fuse_g=1+half_storage=0+bn_sums_in_dgrad=1", "fuse_g=1,half_storage=0,bn_sums_in_dgrad=1"),
)

# BlockPlan: what a plan is OF (not a route) ...
PLAN_CONTEXT_FIELDS = ("mode", "train", "pool_groups", "wide", "half_activations", "x_bf16")
# ... and what it decides.  ROUTE_TUPLE is the part the issue calls a route combination; the rest are storage types and by-products
ROUTE_TUPLE = ("emb_fwd", "spatial_fwd", "temporal_fwd", "temporal_dgrad", "spatial_bwd", "spatial_wgrad", "emb_bwd", "fuse_g", "gate_in_dagg",
               "bn_sums_in_dgrad", "x_amax", "g_amax", "du_amax", "dy_amax", "demb_amax")
PLAN_ROUTE_FIELDS = ROUTE_TUPLE + ("write_emb", "emb_bf16", "y_bf16", "g_bf16", "shortcuts_bf16", "g_sign", "o_sign", "temporal_bn_relu", "u_bf16",
                                   "o_bf16", "pool_rows", "dy_bf16", "dshortcuts_bf16", "dg_bf16", "dx_bf16")
# field values that no default-option run reaches at <= 32 joints, by math mode: the matrix must hold them.  (fuse_g and bn_sums_in_dgrad are
# epilogues of the split-bf16 halo kernel, ops.tconv_halo_bn_sums: math mode f32 has neither under any option, and the fused input stage is
# not built for the f16x2 products -- UNREACHABLE says so.)
SPLIT_MODES = ("bf16x3", "f16x2", "bf16")
MUST_REACH = (      # ({field: value, ...} met by ONE plan, math modes, phases)
    ({"spatial_bwd": "mix"}, ALL_MODES, PHASES),                                     # mix_dx + joint_gram at <= 32 joints
    ({"spatial_bwd": "dagg", "gate_in_dagg": True}, ALL_MODES, PHASES),              # joint_dagg with gated addends inside a block
    ({"spatial_wgrad": "fused"}, SPLIT_MODES, PHASES), ({"spatial_wgrad": "mix"}, ALL_MODES, PHASES),
    ({"fuse_g": True, "bn_sums_in_dgrad": True}, ("bf16x3", "bf16"), ("train",)), ({"fuse_g": True, "bn_sums_in_dgrad": False}, ("bf16x3", "bf16"), PHASES),
    ({"bn_sums_in_dgrad": True}, ("f16x2", "bf16"), ("train",)),                     # (batch-statistics BatchNorm's sums: train only)
    ({"gate_in_dagg": True}, ("f32",), PHASES),
)
UNREACHABLE = (("fuse_g", True, ("f32", "f16x2")), ("bn_sums_in_dgrad", True, ("f32",)))


def route_tuple(pl) -> tuple:
    return tuple(getattr(pl, f) for f in ROUTE_TUPLE)


def option_sets(mode: str) -> Iterator[Tuple[str, object]]:
    """(name, PathOptions): the default and every boolean flipped alone (test_block_plan.option_sets), the thresholds, the composites"""
    from fusion_gcn_amd.paths import PathOptions
    from test_block_plan import option_sets as flips
    for name, o in flips(mode):
        yield (name if name == "default" else f"flip:{name}"), o
    for name, spec in THRESHOLD_SETS + COMPOSITE_SETS:
        yield name, PathOptions().update_from(spec)
    o = PathOptions().update_from("fuse_g=1")                # fuse_g with this mode's bn_sums_in_dgrad flipped
    o.bn_sums_in_dgrad[mode] = not o.bn_sums_in_dgrad[mode]
    yield "fuse_g=1+flip:bn_sums_in_dgrad", o


def make_block(case: Case):
    """The case's module with filler parameters (on the host)"""
    from fusion_gcn_amd.models.mmargcn.agcn import SpatialTemporalConv
    from oracle import filler
    from test_block_model_gpu import adj_for          # the skeleton graphs of the existing block tests, by joint count
    blk = SpatialTemporalConv(case.cin, case.cout, adj_for(case.V), stride=case.stride, residual=case.residual,
                              static_adjacency=case.static, fused_spatial=case.fused)
    filler.fill_state_dict(blk.state_dict(), prefix="l0.")
    return blk


# ---- the matrix ---------------------------------------------------------------------------------------------------------------------------
Entry = namedtuple("Entry", "case half option_name options plan key")      # half: bfloat16 input and out_half=True (math mode bf16)


def runs_a_mix_kernel(pl) -> bool:
    return pl.spatial_fwd == "mix" or pl.spatial_bwd == "mix" or pl.spatial_wgrad == "mix" or pl.emb_bwd == "chain"


def dedupe_key(pl, case: Case, cfg, forms, mode: str, o) -> tuple:
    """The whole frozen plan plus the two kernel choices block.py makes at run time from the context's options: pw_routed per 1x1 convolution
    the plan really sends through block.pw_gemm, and mix_vw_order where the plan runs a mix kernel"""
    from fusion_gcn_amd import routes
    rows = B * case.T * case.V
    pw = {"emb": (cfg.cx, pl.emb_fwd == "gemm"), "emb_t": (6 * cfg.ic, pl.emb_bwd == "chain"), "d_t": (cfg.cout, pl.spatial_bwd != "tile"),
          "down": (cfg.cx, cfg.has_down), "down_t": (cfg.cout, cfg.has_down)}
    routed = tuple(bool(called and routes.pw_routed(forms, key, K, rows, mode, o)) for key, (K, called) in pw.items())
    return (pl, routed, tuple(o.mix_vw_order) if runs_a_mix_kernel(pl) else None)


def plan_all(mode: str, phase: str, cases: Tuple[Case, ...] = CASES) -> List[Entry]:
    """Every (case, input type, option set) the planner accepts for ``cases``, planned on the host: no dedupe"""
    from fusion_gcn_amd import block, ops, routes
    train = phase == "train"
    out = []
    with ops.context(mode):
        for case in cases:
            blk = make_block(case)
            cfg = blk.cfg
            forms = block.pack_weights({n: blk._tensor(n) for n in block.param_names(cfg)}, cfg)
            for name, o in option_sets(mode):
                for half in (False, True):
                    if half and not (train and mode == "bf16" and o.half_storage["bf16"] and o.half_activations["bf16"]):
                        continue            # (plan_block refuses a bfloat16 input outside the half-precision activation step)
                    pl = routes.plan_block(cfg, B, case.T, case.V, x_bf16=half, train=train, inference=False, pool_groups=0, out_half=half,
                                           forms=forms, mode=mode, paths=o, kt=9)
                    out.append(Entry(case, half, name, o, pl, dedupe_key(pl, case, cfg, forms, mode, o)))
    return out


def matrix_key(e: Entry) -> tuple:
    """What makes an entry a distinct run of its case.  CASES: the whole plan (``dedupe_key``).  WIDE_CASES: the kernels the plan runs and the
    input type -- ROUTE_TUPLE, the pw routing, mix_vw_order, ``half`` -- and not the storage-type fields: which tensors a bf16 step stores as
    bfloat16 does not depend on the width and is CASES' to cover, the tile and k-loop geometry is what a wide case adds"""
    if e.case in WIDE_CASES:
        return (route_tuple(e.plan),) + tuple(e.key[1:]) + (e.half,)
    return e.key


@functools.lru_cache(maxsize=None)
def matrix(mode: str, phase: str, cases: Tuple[Case, ...] = CASES) -> Tuple[Entry, ...]:
    """One option set per distinct ``matrix_key`` of every case, and every entry of the default option set: what the GPU modules execute"""
    seen, out = set(), []
    for e in plan_all(mode, phase, cases):
        k = (e.case.name, matrix_key(e))
        if k not in seen or e.option_name == "default":
            seen.add(k)
            out.append(e)
    return tuple(out)


# ---- the oracle's side of a case: depends on case and phase only ----------------------------------------------------------------------------
# eval phase: the biases in front of a running-statistics BatchNorm have real gradients.  Only theta's bias stays analytically zero: it adds a
# constant along the softmax's dimension (agcn_oracle.effective_adjacency, softmax over dim -2); ``oracle_case`` asserts that of the reference
ZERO_IN_EVAL = ("conv_a.0.bias", "conv_a.1.bias", "conv_a.2.bias")


@functools.lru_cache(maxsize=None)
def oracle_case(case: Case, phase: str) -> dict:
    from oracle import agcn_oracle as O
    from oracle import filler
    from oracle import relu_masks as RM
    from test_block_model_gpu import ZERO_GRAD_SUFFIXES       # train mode's analytically-zero bias gradients, as the existing block tests list them
    train = phase == "train"
    blk = make_block(case)
    sd = {"l0." + k: (v.detach().double() if v.is_floating_point() else v.detach().clone()) for k, v in blk.state_dict().items()}
    x = torch.from_numpy(filler.bellish(f"x.blk.{case.name}", (B, case.cin, case.T, case.V))).double()
    Tp = (case.T - 1) // case.stride + 1
    probe = torch.from_numpy(filler.uniform(f"probe.blk.{case.name}", (B, case.cout, Tp, case.V), -1, 1)).double()
    params = {k: v.clone().requires_grad_(True) for k, v in sd.items()
              if v.is_floating_point() and not k.endswith(("running_mean", "running_var", "adj_a"))}
    live = dict(sd)
    live.update(params)
    xo = x.clone().requires_grad_(True)
    stats, cap = O.Stats(), {}
    out, adj_c = O.st_block(xo, live, "l0", case.stride, case.residual, train, stats if train else None, static_adjacency=case.static, capture=cap)
    grads = torch.autograd.grad((out * probe).sum(), [xo] + list(params.values()), allow_unused=True)
    want = {k[3:]: g.numpy() for k, g in zip(params.keys(), grads[1:]) if g is not None}
    scale_ref = max(float(np.abs(v).max()) for v in want.values())
    zero = tuple(k for k in want if k.endswith(ZERO_GRAD_SUFFIXES if train else ZERO_IN_EVAL))
    for k in zero:                   # the exemption is the reference's own statement, not a list of names
        assert float(np.abs(want[k]).max()) <= 1e-9 * scale_ref, (k, float(np.abs(want[k]).max()), scale_ref)
    return dict(x=x, probe=probe, out=out.detach(), adj_c=None if case.static else torch.stack(adj_c, 1).detach(), dx=grads[0], want=want,
                zero=zero, scale_ref=scale_ref, unused=tuple(k[3:] for k, g in zip(params.keys(), grads[1:]) if g is None),
                images={n: RM.pack_sign_image(cap[f"l0.{n}"]) for n in RM.RELU_NAMES}, stats={k[3:]: v for k, v in stats.updates.items()})


# ---- the HIP side ---------------------------------------------------------------------------------------------------------------------------
def cosine(a, b) -> float:
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    return float(np.dot(a, b) / (np.linalg.norm(a) * np.linalg.norm(b) + 1e-300))


def poison(device) -> None:
    """NaN into whatever the caching allocator will hand out next: a ``torch.empty`` that a kernel reads before writing then returns NaN instead
    of a lucky zero.  64 x 4 MB is tests/test_session_gpu.py's figure (the large pool); the blocks of ``CASES`` are smaller than 1 MB per tensor
    and come from the allocator's small pool, so the same is done there in two sizes."""
    junk = [torch.full((1 << 20,), float("nan"), device=device) for _ in range(64)]
    junk += [torch.full((1 << 17,), float("nan"), device=device) for _ in range(64)]
    junk += [torch.full((1 << 12,), float("nan"), device=device) for _ in range(128)]
    del junk


class BlockRun:
    """One case's module on the device; ``run`` = one poisoned forward + backward under an entry's options, with the plan really used captured.
    The run is made on guarded allocations (tests/guarded.py) and ends with the check of their margins: a route that stores outside a tensor
    the host layer allocated fails the entry.  ``poison`` stays: it reaches what autograd allocates in C++, the guard does not."""

    def __init__(self, case: Case, device, margin: int = guarded.MARGIN):
        self.case, self.device, self.margin = case, device, margin
        self.blk = make_block(case).to(device)
        self.buffers0 = {k: v.detach().clone() for k, v in self.blk.named_buffers()}
        ora = oracle_case(case, "train")
        xc = ora["x"].float().permute(0, 2, 3, 1)
        pad = self.blk.cfg.cx - case.cin
        self.x_host = (torch.nn.functional.pad(xc, (0, pad)) if pad else xc).contiguous()      # (the three lines of forward_nchw)
        self.probe_host = ora["probe"].float().permute(0, 2, 3, 1).contiguous()

    def run(self, entry: Entry, phase: str, inject=None, guard: bool = True) -> dict:
        """``guard=False``: the same run on the allocator's own tensors (for the test that the guard changes no bit)"""
        if not guard:
            return self._run(entry, phase, inject)
        with guarded.Guard(margin=self.margin) as g:
            res = self._run(entry, phase, inject)
            g.check()
        return res

    def _run(self, entry: Entry, phase: str, inject) -> dict:
        from fusion_gcn_amd import block, ops
        from oracle import relu_masks as RM
        blk, dev = self.blk, self.device
        blk.train(phase == "train")
        with torch.no_grad():
            for k, v in blk.named_buffers():
                v.copy_(self.buffers0[k])
        blk.zero_grad(set_to_none=True)
        plans, real = [], block.plan_block

        def spy(*a, **kw):
            plans.append(real(*a, **kw))
            return plans[-1]
        taps = RM.BlockTaps(blk)
        block.plan_block = spy
        try:
            with ops.context(entry.plan.mode) as ctx:
                ctx.paths = entry.options.copy()
                x_cl = guarded.put(self.x_host, torch.bfloat16 if entry.half else None, device=dev)       # NaN on both sides of the inputs too
                probe_cl = guarded.put(self.probe_host, device=dev)
                poison(dev)
                xg = x_cl.requires_grad_(True)
                out = blk(xg, out_half=entry.half)          # the module itself: the forward hook sees the STBlockFunction node
                signs = taps.sign_images()[0]
                if inject is not None:
                    taps.inject([inject])
                poison(dev)
                (out.float() * probe_cl).sum().backward()
                torch.cuda.synchronize()
        finally:
            block.plan_block = real
            taps.close()
        c = self.case
        return dict(plans=plans, out=out.detach().float().permute(0, 3, 1, 2), out_dtype=out.dtype, signs=signs,
                    adj_c=None if c.static else torch.stack(blk.gcn1.adj_c, 1).detach(),
                    dx=xg.grad.detach().float()[..., :c.cin].permute(0, 3, 1, 2), dx_dtype=xg.grad.dtype,
                    grads={n: p.grad.detach().clone() for n, p in blk.named_parameters()},
                    buffers={k: v.detach().clone() for k, v in blk.named_buffers()})


def flips_of(signs: Dict[str, np.ndarray], ora: dict) -> int:
    from oracle import relu_masks as RM
    return RM.count_flips([signs], [ora["images"]])[1]


def compare_grads(res: dict, ora: dict, tol: float, fails: List[str], tag: str):
    """dx and EVERY parameter gradient separately against the oracle at ``tol`` (rel-L2); analytically-zero ones <= 1e-4 x the largest reference
    gradient entry; a parameter without a gradient in the oracle (static adjacency: the embedding convs) exactly zero.  -> (worst name, error)"""
    worst = ("dx", rel_l2(res["dx"].cpu().numpy(), ora["dx"].numpy()))
    if not worst[1] < tol:
        fails.append(f"{tag}: dx {worst[1]:.3e} >= {tol:g}")
    for k, g in res["grads"].items():
        g = g.double().cpu().numpy()
        if k in ora["unused"]:
            if float(np.abs(g).max()) != 0.0:
                fails.append(f"{tag}: {k} has no gradient in the oracle, max |g| = {float(np.abs(g).max()):.3e}")
        elif k in ora["zero"]:
            if not float(np.abs(g).max()) <= 1e-4 * ora["scale_ref"]:
                fails.append(f"{tag}: {k} analytically zero, max |g| = {float(np.abs(g).max()):.3e} (scale {ora['scale_ref']:.3e})")
        else:
            err = rel_l2(g.reshape(ora["want"][k].shape), ora["want"][k])
            if err > worst[1] or not err == err:
                worst = (k, err)
            if not err < tol:
                fails.append(f"{tag}: {k} {err:.3e} >= {tol:g}")
    return worst


def compare_grads_bf16(res: dict, ora: dict, fails: List[str], tag: str):
    """the bf16 contract (tests/test_bf16_gpu.py, test_wide_graph_gpu._check_block): cosine >= 0.98 for dx and per parameter, all finite"""
    worst = ("dx", cosine(res["dx"].cpu().numpy(), ora["dx"].numpy()))
    if not (worst[1] >= 0.98 and bool(torch.isfinite(res["dx"]).all())):
        fails.append(f"{tag}: dx cosine {worst[1]:.4f}")
    for k, g in res["grads"].items():
        if not bool(torch.isfinite(g).all()):
            fails.append(f"{tag}: {k} is not finite")
            continue
        g = g.double().cpu().numpy()
        if k in ora["unused"]:
            if float(np.abs(g).max()) != 0.0:
                fails.append(f"{tag}: {k} has no gradient in the oracle, max |g| = {float(np.abs(g).max()):.3e}")
        elif k in ora["zero"]:
            if not float(np.abs(g).max()) <= 1e-4 * ora["scale_ref"]:
                fails.append(f"{tag}: {k} analytically zero, max |g| = {float(np.abs(g).max()):.3e}")
        elif np.linalg.norm(ora["want"][k]) > 1e-9 * ora["scale_ref"]:
            cs = cosine(g, ora["want"][k])
            if cs < worst[1] or not cs == cs:
                worst = (k, cs)
            if not cs >= 0.98:
                fails.append(f"{tag}: {k} cosine {cs:.4f} < 0.98")
    return worst
