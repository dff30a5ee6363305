"""The table of kernel variants (tests/variants.py) against the library, without a GPU: every ``tuning(N)`` the launchers read is a key of the
table and of the header's list and the other way round; the variants a host query can see move it as their row says; and the shapes that
tests/test_variants_gpu.py runs the workgroup orders at meet the launchers' conditions with tile totals below 8, one past a multiple of 8 and
on a multiple of 8 (an XCD-aware grid is rounded up to a multiple of 8 workgroups: the ids past the last tile must be dropped)."""
import glob
import os
import re

import pytest

import variants as VT
from variants import tuned

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = {"f32": 0, "bf16": 1, "bf16x3": 2, "f16x2": 2}


@pytest.fixture()
def lib():
    from fusion_gcn_amd import _lib
    return _lib.load()


@pytest.fixture()
def mode():
    """-> a context manager that selects a math mode on the host (no device call)"""
    from fusion_gcn_amd import ops
    return ops.math_mode


def keys_read_by_the_launchers():
    found = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "fusion_gcn_amd", "csrc", "*.hip")) + glob.glob(os.path.join(ROOT, "fusion_gcn_amd", "csrc", "*.hpp"))):
        for m in re.finditer(r"\btuning\(\s*(\d+)\s*\)", open(path).read()):
            found.setdefault(int(m.group(1)), set()).add(os.path.basename(path))
    return found


def keys_of_the_header(text=None):
    """the keys listed in the comment in front of fgcn_set_tuning: its lines that begin with a key number"""
    text = open(os.path.join(ROOT, "include", "fgcn.h")).read() if text is None else text
    end = text.index("int fgcn_set_tuning(")
    start = text.rindex("/*", 0, end)
    return [int(m.group(1)) for m in re.finditer(r"^ \*   (\d+) ", text[start:end], flags=re.M)]


def test_every_key_the_launchers_read_has_a_row_and_a_line_in_the_header():
    read = keys_read_by_the_launchers()
    assert len(read) >= 15, read                                       # (the scan found the launchers)
    assert sorted(read) == VT.KEYS, (sorted(set(read) ^ set(VT.KEYS)), read)
    listed = keys_of_the_header()
    assert len(listed) == len(set(listed)), listed
    assert sorted(listed) == VT.KEYS, sorted(set(listed) ^ set(VT.KEYS))


def test_the_scan_and_the_header_parser_see_what_they_are_for():
    """the two parsers on small texts: a read with blanks inside the parentheses, a name that only ends in `tuning`, continuation lines of the
    header comment that begin with a number"""
    assert [int(m.group(1)) for m in re.finditer(r"\btuning\(\s*(\d+)\s*\)", "fgcn::tuning(7) & 1; tuning( 12 ); set_tuning(3); retuning(9); tuning(k)")] == [7, 12]
    text = "/* other */\n/* Select:\n *   0  tiles\n *      16: not a key\n *   13 target\n *   7  bits\n */\nint fgcn_set_tuning(int key, int value);\n"
    assert keys_of_the_header(text) == [0, 13, 7]


def test_rows_are_well_formed_and_point_at_tests_that_exist():
    seen = set()
    for r in VT.TABLE:
        assert (r.key, r.value) not in seen, (r.key, r.value)
        seen.add((r.key, r.value))
        assert 0 <= r.key <= 31 and r.modes and set(r.modes) <= set(MODES) and r.engage and r.proof in ("query", "mutant", "reasoning"), r
        assert not (r.sums_bitwise and not r.order_only), r
        path, _, name = r.test.partition("::")
        src = open(os.path.join(ROOT, path)).read()
        assert re.search(rf"^def {name}\(", src, flags=re.M), r.test
        if r.test == VT.NEW:
            assert r.case and r.shapes and r.proof != "reasoning", r      # a row of the new module is reached provably
        else:
            assert r.case is None, r
            assert re.search(rf"set_tuning\({r.key}, |tuned\({r.key}, ", src), r.test    # the test it points at sets the key
    gpu_src = open(os.path.join(ROOT, "tests", "test_variants_gpu.py")).read()
    for case in {r.case for r in VT.gpu_rows()}:
        assert re.search(rf"^def run_{case}\(", gpu_src, flags=re.M), case


def test_tuned_restores_the_previous_value_in_the_current_context(lib):
    from fusion_gcn_amd import ops
    assert lib.fgcn_get_tuning(6) == 0
    with tuned(6, 32):
        assert lib.fgcn_get_tuning(6) == 32
        with tuned(6, 64, (10, 2)):
            assert (lib.fgcn_get_tuning(6), lib.fgcn_get_tuning(10)) == (64, 2)
        assert (lib.fgcn_get_tuning(6), lib.fgcn_get_tuning(10)) == (32, 0)
        with ops.context() as ctx:                                     # a fresh context copies the settings; tuned() writes the current one only
            with tuned(6, 256):
                assert lib.fgcn_get_tuning(6) == 256
            assert lib.fgcn_get_tuning(6) == 32 and ctx is not None
        assert lib.fgcn_get_tuning(6) == 32
    with pytest.raises(RuntimeError):
        with tuned(6, 1):
            raise RuntimeError("the body fails")
    assert lib.fgcn_get_tuning(6) == 0
    from fusion_gcn_amd import _lib
    with pytest.raises(_lib.FgcnError):
        with tuned(32, 1):
            pass


# ---- variants a host query can see -----------------------------------------------------------------------------------------------------------
def test_weight_gradient_slab_counts_follow_key_6(lib, mode):
    """fgcn_tconv_wgrad_slabs / fgcn_pw_wgrad_slabs = row splits x row parts of a stage (waves / 2 at <= 64 columns, waves / 4 above, on the
    split kernel); bit 5: 1x1 on 8 waves, bit 6: all taps above 64 columns on 8 waves -- 4 in math mode bf16, whose default is 8 --, bit 8: all
    taps at 64 columns on 4 waves; the limits of resident workgroups follow (256 for an 8-wave form)."""
    for name in ("bf16x3", "f16x2", "bf16"):
        with mode(name):
            wide_default = 2 if name == "bf16" else 1                  # all taps above 64 columns: 8 waves in bf16, 4 in bf16x3
            assert (lib.fgcn_tconv_wgrad_slabs(64, 3), lib.fgcn_tconv_wgrad_slabs(128, 3)) == (12, 3 * wide_default)
            assert (lib.fgcn_pw_wgrad_slabs(64, 3), lib.fgcn_pw_wgrad_slabs(128, 3)) == (6, 3)
            assert (lib.fgcn_tconv_wgrad_resident(64), lib.fgcn_tconv_wgrad_resident(128)) == (256, 256 if name == "bf16" else 512)
            assert (lib.fgcn_pw_wgrad_resident(64), lib.fgcn_pw_wgrad_resident(128)) == (512, 512)
            with tuned(6, 32):
                assert (lib.fgcn_pw_wgrad_slabs(64, 3), lib.fgcn_pw_wgrad_slabs(128, 3)) == (12, 6)
                assert (lib.fgcn_pw_wgrad_resident(64), lib.fgcn_pw_wgrad_resident(128)) == (256, 256)
                assert lib.fgcn_tconv_wgrad_slabs(128, 3) == 3 * wide_default
            with tuned(6, 64):
                assert lib.fgcn_tconv_wgrad_slabs(128, 3) == 3 * (3 - wide_default)            # the other wave count
                assert lib.fgcn_tconv_wgrad_resident(128) == (512 if name == "bf16" else 256)
                assert lib.fgcn_tconv_wgrad_slabs(64, 3) == 12 and lib.fgcn_pw_wgrad_slabs(128, 3) == 3
            with tuned(6, 256):
                assert lib.fgcn_tconv_wgrad_slabs(64, 3) == 6 and lib.fgcn_tconv_wgrad_resident(64) == 512
                assert lib.fgcn_tconv_wgrad_slabs(128, 3) == 3 * wide_default
            with tuned(6, 1):                                           # 1x1 on the per-tap kernel's relative: the same partition, not visible here
                assert (lib.fgcn_pw_wgrad_slabs(64, 3), lib.fgcn_pw_wgrad_slabs(128, 3)) == (6, 3)
    with mode("f32"):                                                   # no split kernel: key 6 selects nothing
        for value in (0, 1, 32, 64, 256):
            with tuned(6, value):
                assert (lib.fgcn_tconv_wgrad_slabs(64, 3), lib.fgcn_tconv_wgrad_slabs(128, 3), lib.fgcn_pw_wgrad_slabs(64, 3)) == (6, 3, 6)


def test_segment_and_chunk_counts_follow_keys_15_and_13(lib):
    """fgcn_spatial_bwd_tile_segments: cdiv(target, B) segments per sample at most, the tiles spread evenly (5 frames per tile at V = 25);
    fgcn_spatial_wgrad_chunks: target / (tiles x B) chunks, at least 4 frames each"""
    B, T, V = 2, 13, 25
    assert lib.fgcn_spatial_bwd_tile_segments(B, T, V) == 3             # default target 256: one tile per workgroup
    for target, segs in ((1, 1), (2, 1), (3, 2), (4, 2), (6, 3), (100000, 3)):
        with tuned(15, target):
            assert lib.fgcn_spatial_bwd_tile_segments(B, T, V) == segs, target
    assert lib.fgcn_spatial_bwd_tile_segments(B, T, V) == 3
    assert lib.fgcn_spatial_wgrad_chunks(B, T, 64, 64) == 4             # 13 frames: chunks of 4, 4, 4, 1
    for target, chunks in ((1, 1), (2 * 2 * B, 2), (100000, 4)):
        with tuned(13, target):
            assert lib.fgcn_spatial_wgrad_chunks(B, T, 64, 64) == chunks, target


def test_the_rows_with_a_query_as_proof_move_it(lib, mode):
    """every row whose proof is "query", at the shapes its GPU test runs: the count the host sizes the partial buffer with differs from the
    default's in at least one of the row's modes and shapes (so the GPU test cannot be running the default partition everywhere)"""
    for r in VT.TABLE:
        if r.proof != "query" or r.case is None:
            continue
        moved = False
        for name in r.modes:
            with mode(name):
                for shape in r.shapes:
                    def count():
                        if r.case == "pw_wgrad":
                            return lib.fgcn_pw_wgrad_slabs(shape[4], 1)
                        if r.case == "tconv_wgrad":
                            return lib.fgcn_tconv_wgrad_slabs(shape[4], 1)
                        V, T, _, _, B = shape
                        return lib.fgcn_spatial_bwd_tile_segments(B, T, V)
                    base = count()
                    for value in ([1, 2 * shape[4]] if r.value == "target" else [r.value]):
                        with tuned(r.key, value):
                            moved |= count() != base
        assert moved, (r.key, r.value)


# ---- the workgroup orders of key 5 -----------------------------------------------------------------------------------------------------------
def order_totals(lib, mode, r):
    """-> the tile totals of a key-5 row's shapes, each checked against the launcher's condition for the order the bit selects"""
    totals = []
    for name in r.modes:
        with mode(name):
            for shape in r.shapes:
                if r.case == "rows_gemm":
                    tiles_m, tiles_n = VT.rows_gemm_tiles(lib, shape)
                    assert tiles_n > 1 and tiles_m < 65536, shape
                    totals.append(tiles_m * tiles_n)
                elif r.case == "rows_wgrad":
                    totals.append(VT.rows_wgrad_total(shape))
                elif r.case == "tconv_halo":
                    tiles_m, tiles_n = VT.halo_tiles(lib, shape)
                    totals.append(tiles_m * tiles_n)
                elif r.case == "spatial_fwd":
                    tiles, ncol = VT.spatial_fwd_tiles(lib, shape)
                    assert ncol > 1 and shape[2] % 32 == 0, shape
                    totals.append(tiles * ncol)
                else:
                    assert r.case == "tconv_wgrad"
                    tiles_xy, nsplit = VT.twgrad_tiles(lib, shape)
                    assert tiles_xy > 1, shape
                    totals.append(tiles_xy * nsplit)
    return totals


@pytest.mark.parametrize("bit", [1, 2, 4, 8, 16, 32, 64])
def test_the_shapes_of_each_workgroup_order_meet_its_condition(lib, mode, bit):
    (r,) = [r for r in VT.TABLE if r.key == 5 and r.value == bit]
    totals = order_totals(lib, mode, r)
    assert all(0 < t < (1 << 30) for t in totals)
    assert any(t < 8 for t in totals), totals
    assert any(t > 8 and t % 8 == 1 for t in totals), totals
    assert any(t % 8 == 0 for t in totals), totals


def test_the_tile_rules_restated_for_the_orders_agree_with_the_queries(lib, mode):
    """the restated rules of tests/variants.py at known points: a row GEMM of fewer than 256 workgroups runs 128-row, 32-column tiles (nt = 3
    falls to 1); with key 24 the large-problem tiles; the halo conv's and the spatial forward's tile queries"""
    with mode("f32"):
        assert VT.rows_gemm_tiles(lib, (1, 5, 20, 64, 128, 1, 1)) == (1, 4)
        assert VT.rows_gemm_tiles(lib, (1, 13, 25, 32, 96, 1, 1)) == (3, 3)
        assert VT.rows_gemm_tiles(lib, (2, 20, 25, 64, 64, 9, 1), key24=1) == (4, 1)        # 1000 rows: four 256-row tiles, one 64-column tile
        assert VT.rows_gemm_tiles(lib, (2, 12, 22, 256, 384, 1, 1), key24=1) == (5, 3)
        assert VT.halo_tiles(lib, (3, 15, 25, 64, 64)) == (9, 1) and VT.halo_tiles(lib, (2, 20, 25, 128, 256)) == (8, 2)
        assert VT.spatial_fwd_tiles(lib, (20, 20, 64, 192, 1)) == (3, 3)
    with mode("bf16x3"):
        assert VT.twgrad_tiles(lib, (3, 5, 25, 96, 64, 3, 1)) == (3, 3) and VT.twgrad_tiles(lib, (2, 10, 25, 64, 64, 9, 1)) == (2, 4)
