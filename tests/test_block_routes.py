"""The route matrix of tests/block_routes.py is closed: every route the planner can produce for an AGCN block at <= 32 joints is an entry of the
matrix that tests/test_block_routes_gpu.py executes against the float64 oracle, and the same for the blocks of 128 .. 512 channels
(block_routes.WIDE_CASES) and the matrix that tests/test_wide_channels_gpu.py executes.  Host only (routes.plan_block and the availability queries are
host functions of the built library)."""
import dataclasses
import inspect
import itertools
import re

import numpy as np
import pytest

import block_routes as R


def test_every_field_of_the_two_dataclasses_is_handled():
    """A new PathOptions or BlockPlan field has to be entered in the matrix's tables, and every option the planner reads is one the matrix moves"""
    from fusion_gcn_amd import routes
    from fusion_gcn_amd.paths import PathOptions
    opts = {f.name for f in dataclasses.fields(PathOptions)}
    assert opts == set(R.OPTION_HANDLING), opts ^ set(R.OPTION_HANDLING)
    plan_fields = [f.name for f in dataclasses.fields(routes.BlockPlan)]
    assert len(set(R.PLAN_CONTEXT_FIELDS + R.PLAN_ROUTE_FIELDS)) == len(R.PLAN_CONTEXT_FIELDS + R.PLAN_ROUTE_FIELDS)
    assert set(plan_fields) == set(R.PLAN_CONTEXT_FIELDS + R.PLAN_ROUTE_FIELDS), set(plan_fields) ^ set(R.PLAN_CONTEXT_FIELDS + R.PLAN_ROUTE_FIELDS)
    for f in dataclasses.fields(PathOptions):       # a "flip" is a boolean (per-mode boolean), a "threshold" is not
        v = getattr(PathOptions(), f.name)
        is_bool = isinstance(v, bool) or (isinstance(v, dict) and isinstance(next(iter(v.values())), bool))
        how = R.OPTION_HANDLING[f.name]
        assert how in ("flip", "threshold", "model", "other") and (how != "flip" or is_bool) and (how != "threshold" or not is_bool), f.name
    src = inspect.getsource(routes)
    read = set(re.findall(r"\bo\.([a-z_0-9]+)\b", src)) | set(re.findall(r"""\bo\.get\(\s*["']([a-z_0-9]+)["']""", src))
    read |= set(re.findall(r"""bf16_step\(\s*["']([a-z_0-9]+)["']""", src))
    read -= {"get"}
    assert {"spatial_bwd_tile", "fuse_g", "emb_tile_max_cin", "half_storage"} <= read, read     # (the patterns still match how the planner reads its options)
    assert read <= opts, read - opts
    not_moved = {n for n in read if R.OPTION_HANDLING[n] == "other"}
    assert not not_moved, not_moved
    moved = " ".join(spec for _, spec in R.THRESHOLD_SETS)
    for name, how in R.OPTION_HANDLING.items():
        assert how != "threshold" or re.search(rf"\b{name}=", moved), name


def _sweep_values(mode, phase):
    """field -> values over the sweep of tests/test_block_plan.py (its blocks, joint counts and option sets; B = 128) at <= 32 joints, pool_groups 0"""
    import test_block_plan as TP
    from fusion_gcn_amd import block, ops, routes
    from fusion_gcn_amd.models.mmargcn.agcn import SpatialTemporalConv
    train, inference = TP.PHASES[phase]
    values = {f: set() for f in R.PLAN_ROUTE_FIELDS}
    with ops.context(mode):
        for cin, cout, stride, residual, static, T in TP.BLOCKS:
            mod = SpatialTemporalConv(cin, cout, np.zeros((3, 25, 25), np.float32), stride=stride, residual=residual, static_adjacency=static)
            forms = block.pack_weights({n: mod._tensor(n) for n in block.param_names(mod.cfg)}, mod.cfg)
            for V, (name, o) in itertools.product([v for v in TP.JOINTS if v <= 32], TP.option_sets(mode)):
                half = bool(train and mode == "bf16" and o.half_storage["bf16"] and o.half_activations["bf16"])
                for x_bf16 in ((False, True) if half else (False,)):
                    pl = routes.plan_block(mod.cfg, 128, T, V, x_bf16=x_bf16, train=train, inference=inference, pool_groups=0, out_half=x_bf16,
                                           forms=forms, mode=mode, paths=o, kt=9)
                    for f in R.PLAN_ROUTE_FIELDS:
                        values[f].add(getattr(pl, f))
    return values


@pytest.mark.parametrize("phase", R.PHASES)
@pytest.mark.parametrize("mode", R.ALL_MODES)
def test_the_matrix_leaves_no_route_out(mode, phase):
    entries = R.matrix(mode, phase)
    everything = R.plan_all(mode, phase)
    assert entries and all(e.plan.mode == mode and e.plan.train == (phase == "train") and not e.plan.wide and not e.plan.pool_groups for e in entries)
    in_matrix = {f: {getattr(e.plan, f) for e in entries} for f in R.PLAN_ROUTE_FIELDS}
    # (1) every value of every route field that the planner sweep of test_block_plan.py produces appears in the matrix
    for f, vals in _sweep_values(mode, phase).items():
        # the 512-channel first block of the RGB patch-feature modes and the blocks of 320 .. 512 channels are the sweep's blocks beyond the fused
        # spatial kernel's width: their forward "mix" at <= 32 joints is reached here by fused_spatial=False (identity64_unfused), checked like
        # every other value
        assert vals <= in_matrix[f], (mode, phase, f, vals - in_matrix[f])
    # (2) the values no default-option run reaches
    for want, modes, phases in R.MUST_REACH:
        if mode in modes and phase in phases:
            assert any(all(getattr(e.plan, f) == v for f, v in want.items()) for e in entries), ("no entry of the matrix runs", mode, phase, want)
    for f, v, modes in R.UNREACHABLE:               # what no option and no case produces in this mode (if that changes, it joins MUST_REACH)
        if mode in modes:
            assert v not in {getattr(e.plan, f) for e in everything}, (mode, phase, f, v)
    # (3) every route combination reachable from CASES x option_sets is in the matrix, per case: the dedupe drops none
    reach = {(e.case.name, e.half, R.route_tuple(e.plan)) for e in everything}
    kept = {(e.case.name, e.half, R.route_tuple(e.plan)) for e in entries}
    lost = reach - kept
    assert not lost, [(c, h, dict(zip(R.ROUTE_TUPLE, t))) for c, h, t in sorted(lost, key=str)]
    assert {(e.case.name, e.key) for e in everything} == {(e.case.name, e.key) for e in entries}
    assert len({(e.case.name, e.key) for e in entries}) == len(entries)              # ... and runs none twice
    default = {R.route_tuple(e.plan) for e in everything if e.option_name == "default"}
    combos = {R.route_tuple(e.plan) for e in entries}
    print(f"{mode} {phase}: {len(entries)} entries of {len(everything)} planned; {len(default)} route combinations under the default options + "
          f"{len(combos - default)} by option sets")
    # the counts of the issue's table (default + further combinations); they only grow with cases and option sets
    floor = {"f32": (4, 8), "bf16x3": (9, 68), "f16x2": (7, 45), "bf16": (5, 37)}[mode]
    if phase == "train":
        assert len(default) >= floor[0] and len(combos - default) >= floor[1], (len(default), len(combos - default), floor)


# entries of the wide matrix per mode, (train, eval): what tests/test_wide_channels_gpu.py runs.  Under the whole-plan dedupe of CASES math mode
# bf16's train phase would hold 168; on the route tuple (block_routes.matrix_key) it is 126
WIDE_ENTRIES = {"f32": (28, 28), "bf16x3": (69, 63), "f16x2": (58, 55), "bf16": (126, 60)}


@pytest.mark.parametrize("phase", R.PHASES)
@pytest.mark.parametrize("mode", R.ALL_MODES)
def test_the_wide_matrix_leaves_no_route_out(mode, phase):
    """WIDE_CASES (128 .. 512 channels): every route combination the planner produces for a wide case under ``option_sets``, per case, input
    type, pw routing and mix order, is an entry of the wide matrix; every default-option entry is kept; no wide case is planned onto the
    > 32-joint path; and the tile forms are really what the wide blocks run"""
    entries = R.matrix(mode, phase, R.WIDE_CASES)
    everything = R.plan_all(mode, phase, R.WIDE_CASES)
    assert entries and all(e.plan.mode == mode and e.plan.train == (phase == "train") and not e.plan.wide and not e.plan.pool_groups for e in entries)
    assert {e.case for e in entries} == set(R.WIDE_CASES)
    reach = {(e.case.name, e.half, R.route_tuple(e.plan)) for e in everything}
    kept = {(e.case.name, e.half, R.route_tuple(e.plan)) for e in entries}
    lost = reach - kept
    assert not lost, [(c, h, dict(zip(R.ROUTE_TUPLE, t))) for c, h, t in sorted(lost, key=str)]
    assert {(e.case.name, R.matrix_key(e)) for e in everything} == {(e.case.name, R.matrix_key(e)) for e in entries}
    kept_default = [e for e in entries if e.option_name == "default"]
    assert kept_default == [e for e in everything if e.option_name == "default"]
    assert len({(e.case.name, R.matrix_key(e)) for e in entries}) == len(entries)    # the default set comes first: no key runs twice
    for f, v, modes in R.UNREACHABLE:
        if mode in modes:
            assert v not in {getattr(e.plan, f) for e in everything}, (mode, phase, f, v)
    # the dedupe on the route tuple drops storage-type variants only: every plan it drops differs from the kept entry of its key in fields
    # outside ROUTE_TUPLE alone (by construction of the key), and CASES' matrix holds every value of those fields that a wide case takes
    narrow = {f: {getattr(e.plan, f) for e in R.matrix(mode, phase)} for f in R.PLAN_ROUTE_FIELDS if f not in R.ROUTE_TUPLE}
    for f, vals in narrow.items():
        assert {getattr(e.plan, f) for e in everything} <= vals, (mode, phase, f)
    print(f"{mode} {phase}: {len(entries)} wide entries of {len(everything)} planned")
    assert len(entries) >= WIDE_ENTRIES[mode][phase == "eval"], (len(entries), WIDE_ENTRIES[mode])      # (they only grow with option sets)
    if mode != "f32":                # the default options send 192 .. 512 channels to the tile forms and the halo conv, as a wide model runs them
        for c in R.WIDE_CASES[1:]:
            pl = next(e.plan for e in kept_default if e.case == c and not e.half)
            assert pl.spatial_bwd == "tile" and pl.spatial_wgrad == "tile" and pl.temporal_fwd in ("halo", "halo_parity"), (c.name, pl)
