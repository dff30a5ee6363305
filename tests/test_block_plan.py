"""routes.plan_block: one plan per block call, and the cross-stage invariants the block used to re-check at run time (an emb stored as
bfloat16 whose backward is not the tile form, a bfloat16 dy without the fused spatial backward).  The planner and the availability
queries it asks are host functions of the built library: no GPU needed."""
import dataclasses
import itertools

import numpy as np
import pytest

MODES = ("f32", "bf16x3", "f16x2", "bf16")
JOINTS = (25, 27, 22, 33, 64)
PHASES = {"train": (True, False), "eval": (False, False), "inference": (False, True)}       # -> (train, inference)
# (cin, cout, stride, residual, static adjacency, input frames): the ten blocks of the headline model (64 clips x 2 bodies, T = 300), a
# static-adjacency block, the 512-channel first block of the RGB patch-feature modes
HEADLINE = [(3, 64, 1, False, False, 300)] + [(64, 64, 1, True, False, 300)] * 3 + [(64, 128, 2, True, False, 300)] + \
           [(128, 128, 1, True, False, 150)] * 2 + [(128, 256, 2, True, False, 150)] + [(256, 256, 1, True, False, 75)] * 2
# ... and the blocks of a 128- / 192-wide model (start_feature_size=128: 256 -> 512 and 512 -> 512; 192: 192 -> 384) and a 320-wide one
WIDE = [(256, 512, 2, True, False, 150), (512, 512, 1, True, False, 75), (320, 320, 1, True, False, 75), (192, 384, 2, True, False, 150)]
BLOCKS = HEADLINE + [(64, 64, 1, True, True, 300), (512, 64, 1, False, False, 128)] + WIDE
TILE_OR_BF16 = ("emb_bf16", "y_bf16", "g_bf16", "shortcuts_bf16", "u_bf16", "o_bf16", "dy_bf16", "dshortcuts_bf16", "dg_bf16", "dx_bf16",
                "half_activations", "x_bf16")


def option_sets(mode):
    """default options, then each boolean field (a per-mode boolean: this mode's entry) flipped"""
    from fusion_gcn_amd.paths import PathOptions
    yield "default", PathOptions()
    for f in dataclasses.fields(PathOptions):
        o = PathOptions()
        v = getattr(o, f.name)
        if isinstance(v, bool):
            setattr(o, f.name, not v)
        elif isinstance(v, dict) and isinstance(v[mode], bool):
            v[mode] = not v[mode]
        else:
            continue
        yield f.name, o


def check(pl, cfg, mode, train):
    bf16 = [n for n in TILE_OR_BF16 if getattr(pl, n)]
    assert not bf16 or (mode == "bf16" and train), bf16              # nothing is bfloat16 outside a bf16 training step
    assert not pl.emb_bf16 or (pl.emb_fwd == "tile" and pl.emb_bwd == "tile")
    assert not pl.dy_bf16 or (pl.spatial_bwd == "tile" and pl.spatial_wgrad == "tile")
    assert not pl.g_bf16 or ("rows" not in (pl.temporal_fwd, pl.temporal_dgrad) and pl.g_sign)
    assert not pl.u_bf16 or (pl.g_bf16 and pl.temporal_fwd == "halo" and not pl.fuse_g)
    assert not pl.y_bf16 or (pl.spatial_fwd == "tile" and not pl.bn_sums_in_dgrad)
    assert not pl.o_bf16 or pl.o_sign
    for d_o_bf16 in (False, True):                                   # the backward's run-time refinement
        dx16, dg16 = pl.refine_dx(d_o_bf16)
        assert (not dx16 or pl.dx_bf16) and (not dg16 or pl.dg_bf16)
        if dx16:     # every writer of dx has the bfloat16 form
            assert pl.x_bf16 and pl.spatial_bwd == "tile" and pl.dy_bf16 and not cfg.has_down and cfg.residual != "conv"
            assert pl.gate_in_dagg      # (the graph convolution's own identity shortcut, ungated, is written by bn_act_bwd: float32 only)
            assert cfg.static_adjacency or (pl.emb_bwd == "tile" and pl.emb_bf16)
            assert dg16 and (d_o_bf16 or pl.pool_rows)
        assert not (dg16 and pl.gate_in_dagg) or dx16                # a gated addend has dx's storage type
        assert not dg16 or (pl.g_bf16 and pl.temporal_dgrad != "rows" and not pl.bn_sums_in_dgrad)
    assert not pl.gate_in_dagg or (pl.o_sign and pl.g_sign and pl.spatial_bwd in ("tile", "dagg") and cfg.residual == "identity" and not cfg.has_down)
    assert not pl.bn_sums_in_dgrad or (pl.temporal_dgrad == "halo" and pl.g_sign and train)
    assert not pl.fuse_g or (pl.temporal_fwd == "halo" and pl.g_sign and not cfg.has_down)
    assert not pl.temporal_bn_relu or (not train and pl.temporal_fwd == "halo" and not pl.o_sign and not pl.pool_groups)
    assert (pl.spatial_fwd == "tile_bn_relu") <= (not train) and (pl.spatial_fwd == "tile_bn_relu") == (not pl.g_sign)
    assert (pl.emb_fwd is None) == (pl.emb_bwd is None) == cfg.static_adjacency
    assert pl.write_emb or (not train and pl.emb_fwd != "gemm")
    assert mode == "f16x2" or not (pl.x_amax or pl.g_amax or pl.du_amax or pl.dy_amax or pl.demb_amax)
    assert not pl.demb_amax or (pl.x_amax and pl.emb_bwd == "chain")
    assert not pl.dy_amax or pl.spatial_bwd != "tile"
    assert not pl.pool_rows or pl.pool_groups
    if pl.wide:      # no tile form, no halo route, no bfloat16 storage
        assert pl.emb_fwd != "tile" and pl.emb_bwd != "tile" and pl.spatial_fwd == "mix" and pl.spatial_bwd == "mix" and pl.spatial_wgrad == "mix"
        assert pl.temporal_fwd == pl.temporal_dgrad == "rows" and not pl.temporal_bn_relu and not pl.fuse_g and not pl.bn_sums_in_dgrad
        assert not bf16 and not pl.gate_in_dagg


@pytest.mark.parametrize("mode", MODES)
def test_plan_block_returns_and_keeps_its_invariants(mode):
    from fusion_gcn_amd import block, ops, routes
    from fusion_gcn_amd.models.mmargcn.agcn import SpatialTemporalConv
    plans, seen = 0, set()
    with ops.context(mode):
        assert ops.get_math_mode() == mode
        for i, (cin, cout, stride, residual, static, T) in enumerate(BLOCKS):
            mod = SpatialTemporalConv(cin, cout, np.zeros((3, 25, 25), np.float32), stride=stride, residual=residual, static_adjacency=static)
            cfg = mod.cfg
            forms = block.pack_weights({n: mod._tensor(n) for n in block.param_names(cfg)}, cfg)
            pools = (0, 64) if i == len(HEADLINE) - 1 else (0,)      # the model's last block: pooling on and off
            for (phase, (train, inference)), V, pool, (name, o) in itertools.product(PHASES.items(), JOINTS, pools, option_sets(mode)):
                half = bool(train and mode == "bf16" and o.half_storage["bf16"] and o.half_activations["bf16"] and V <= 32)
                for x_bf16, out_half in ((False, False), (True, True)):
                    kw = dict(x_bf16=x_bf16, train=train, inference=inference, pool_groups=pool, out_half=out_half, forms=forms, mode=mode,
                              paths=o, kt=9)
                    if x_bf16 and not half:                           # a bfloat16 input needs the half-precision activation step
                        with pytest.raises(ops._lib.FgcnError):
                            routes.plan_block(cfg, 128, T, V, **kw)
                        continue
                    pl = routes.plan_block(cfg, 128, T, V, **kw)
                    assert (pl.mode, pl.train, pl.pool_groups, pl.x_bf16, pl.wide) == (mode, train, pool, x_bf16, V > 32)
                    assert pl.half_activations == half
                    check(pl, cfg, mode, train)
                    plans += 1
                    seen.add((pl.emb_fwd, pl.spatial_fwd, pl.temporal_fwd, pl.spatial_bwd, pl.spatial_wgrad, pl.emb_bwd))
    print(f"{mode}: {plans} plans, {len(seen)} distinct route combinations")
    assert len(seen) > 8, seen      # the sweep really reaches the routes (tile and unfused forms, halo and row-GEMM convs)


def test_temporal_route_directions():
    """the strided forward asks T > 1, the strided data gradient does not (block.temporal_dgrad skips the empty odd pass itself)"""
    from fusion_gcn_amd.routes import temporal_route
    forms = {"t4_e", "t4_o", "t_t4_e", "t_t4_o"}
    assert temporal_route(forms, 9, 2, 1, False, "fwd") == "rows" and temporal_route(forms, 9, 2, 1, False, "dgrad") == "halo_parity"
    assert temporal_route(forms, 9, 2, 8, False, "fwd") == "halo_parity" and temporal_route(forms, 9, 2, 8, True, "fwd") == "rows"
    assert temporal_route(forms, 7, 2, 8, False, "fwd") == "rows"     # odd half padding
    assert temporal_route({"t4", "t_t4"}, 9, 1, 8, False, "fwd") == temporal_route({"t4", "t_t4"}, 9, 1, 8, False, "dgrad") == "halo"
    assert temporal_route({"t"}, 9, 1, 8, False, "fwd") == "rows"
