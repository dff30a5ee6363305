"""The kernel variants that fgcn_set_tuning selects, as one table (a helper module: no test, no conftest), shared by tests/test_variants.py
(host: the table against the source and the header, the variants a host query can see, the shapes of the workgroup orders) and
tests/test_variants_gpu.py (every variant no other test launches, against float64 and against the default variant).

One ``Row`` per (key, value or bit) that changes which kernel, instantiation, workgroup order, store form or partition runs:

  entry       the entry point(s) of include/fgcn.h it affects
  modes       the math modes in which it has any effect (names of fusion_gcn_amd.ops.math_mode)
  engage      the launcher's own condition under which the variant branch is taken, at the smallest shapes the tests use
  order_only  every OUTPUT element is the same sum in the same order as under the default: the GPU test requires torch.equal with the
              default's output.  Partial sums (BatchNorm statistics, gram / weight-gradient slabs) are compared in total, within the
              tolerance, unless ``sums_bitwise`` says the partials themselves are the same sums too.
  proof       how it is known that the row's test reaches the variant: "query" (a host query moves: tests/test_variants.py), "mutant" (a
              value-only mutant inside the variant's code failed the row's test on a scratch build: DESIGN.md section 8m), "reasoning" (the
              launcher's condition, read; no query and no mutant)
  test        the test that launches it
  with_keys   other keys the row's test sets so that the launcher takes the branch at a small shape
  case        the runner of tests/test_variants_gpu.py and its shapes (rows of this module's tests only)

``tuned(key, value)`` sets a key in the calling thread's current context and restores the previous value."""
import contextlib
from collections import namedtuple

Row = namedtuple("Row", "key value entry modes engage order_only sums_bitwise proof test with_keys case shapes")

X3 = ("bf16x3", "f16x2")
SPLIT = ("bf16x3", "f16x2", "bf16")
ALL = ("f32", "bf16x3", "f16x2", "bf16")
OLD = "tests/test_kernels_gpu.py::"
NEW = "tests/test_variants_gpu.py::test_variant_against_float64_and_the_default"


def _row(key, value, entry, modes, engage, *, order_only=False, sums_bitwise=False, proof="mutant", test=NEW, with_keys=(), case=None, shapes=()):
    return Row(key, value, entry, tuple(modes), engage, order_only, sums_bitwise, proof, test, tuple(with_keys), case, tuple(shapes))


# ---- shapes ---------------------------------------------------------------------------------------------------------------------------------
# rows_gemm (B, T, V, K, N, taps, stride).  Key 24 = 1 keeps the large-problem tiles at these sizes (otherwise fewer than 256 workgroups fall
# back to 128-row tiles and the narrowest column tiles, and keys 0 / 1 select nothing).
GEMM_NARROW = [(2, 20, 25, 64, 64, 9, 1), (1, 7, 5, 40, 36, 3, 1), (2, 9, 27, 4, 64, 1, 1), (3, 11, 20, 64, 32, 1, 1)]     # nt <= 2
GEMM_WIDE = [(2, 21, 25, 64, 128, 9, 2), (3, 10, 18, 128, 96, 1, 1), (2, 12, 22, 256, 384, 1, 1)]                             # nt = 4, 3, 4
# ... for the workgroup orders (no key 24: 128-row tiles, 32-column tiles): row tiles x column tiles = 1 x 4 = 4, 3 x 3 = 9, 2 x 4 = 8, 5 x 12 = 60
GEMM_ORDER = [(1, 5, 20, 64, 128, 1, 1), (1, 13, 25, 32, 96, 1, 1), (2, 5, 25, 64, 128, 3, 1), (2, 12, 22, 64, 384, 1, 1)]
# rows_wgrad, the per-tap kernel (B, T, V, K, N, taps, stride): tiles x taps x row splits = 1, 3 x 3 x 1 = 9, 2 x 1 x 4 = 8, 2 x 1 x 2 = 4
ROWS_WGRAD = [(1, 5, 25, 64, 64, 1, 1), (2, 10, 25, 64, 192, 3, 1), (3, 25, 25, 64, 128, 1, 1), (2, 33, 25, 64, 128, 1, 2)]
# tconv_halo, nine taps, stride 1 (B, T, V, K, N): row tiles x column tiles = 1, 9 x 1 = 9, 8 x 2 = 16, 3 x 2 = 6
HALO = [(1, 5, 25, 64, 64), (3, 15, 25, 64, 64), (2, 20, 25, 128, 256), (1, 13, 27, 64, 160)]
HALO_WIDE = [(2, 13, 25, 128, 256), (3, 17, 20, 64, 64), (1, 5, 27, 64, 192)]          # key 7 bit 4: two 128-column tiles; 64 columns; a ragged second tile
HALO_BF16_OUT = [(2, 20, 25, 64, 64), (3, 13, 18, 256, 256), (1, 9, 27, 128, 64)]
# spatial_fwd (V, T, Cin, Cout, B): frame chunks x samples x column blocks = 1 x 1 x 2 = 2, 3 x 1 x 3 = 9, 2 x 2 x 2 = 8
SPATIAL_FWD = [(25, 5, 64, 128, 1), (20, 20, 64, 192, 1), (25, 13, 128, 128, 2)]
SPATIAL_FWD_OLD = [(25, 13, 64, 64, 2), (27, 9, 64, 128, 1), (20, 7, 128, 256, 2)]
# all-taps / 1x1 weight gradients of the split kernels (B, T, V, K, N, taps, stride): (channel group, column tile) pairs x row splits =
# 2 x 1 = 2, 3 x 3 = 9, 2 x 4 = 8
TWGRAD_ORDER = [(1, 5, 25, 64, 64, 9, 1), (3, 5, 25, 96, 64, 3, 1), (2, 10, 25, 64, 64, 9, 1)]
TWGRAD = [(3, 20, 25, 64, 64, 9, 1), (2, 21, 25, 64, 128, 9, 2), (2, 13, 27, 128, 256, 9, 1), (2, 9, 20, 64, 96, 3, 1)]
PWGRAD = [(2, 30, 25, 192, 64, 1, 1), (3, 20, 18, 64, 96, 1, 1), (2, 21, 27, 64, 128, 1, 2), (1, 12, 25, 256, 256, 1, 1)]
# joint_dagg (V, T, C, B)
DAGG = [(25, 30, 64, 3), (27, 12, 256, 2), (20, 9, 128, 2)]
SPATIAL_WGRAD = [(25, 13, 64, 64, 2), (27, 12, 128, 128, 2), (20, 5, 64, 256, 1)]      # (V, T, Cin, Cout, B)
GRAM = [(25, 30, 16), (18, 33, 32), (27, 12, 64)]                                      # (V, T, ic), B = 3
SPATIAL_TILE = [(25, 13, 64, 64, 2), (27, 9, 64, 128, 1), (20, 37, 128, 128, 3)]       # (V, T, Cin, Cout, B)
EMB_TILE = [(25, 13, 16, 128, 2), (27, 9, 32, 128, 1), (20, 7, 64, 256, 2)]            # (V, T, ic, cx, B): cx > 64, the 128-column tiles
BN_REDUCE = [(1000, 64, 0), (777, 128, 1), (2048, 256, 2), (50, 8, 1)]                 # (rows, C, res_mode)

TABLE = [
    # ---- key 0 / 1 / 24: tiles of the row GEMM ----------------------------------------------------------------------------------------------
    _row(0, 0, "fgcn_rows_gemm*", ALL, "nt <= 2 and (key 24 == 1 or cdiv(M, 256) * tiles_n * batch >= 256): mt = 1", order_only=True,
         with_keys=[(24, 1)], case="rows_gemm", shapes=GEMM_NARROW),
    _row(0, 2, "fgcn_rows_gemm*", ALL, "nt <= 2 and (key 24 == 1 or cdiv(M, 256) * tiles_n * batch >= 256): mt = 2, double-buffered", order_only=True,
         sums_bitwise=True, with_keys=[(24, 1)], case="rows_gemm", shapes=GEMM_NARROW),
    _row(1, 1, "fgcn_rows_gemm*", ALL, "nt >= 3 (key 24 == 1 or cdiv(M, 128) * tiles_n * batch >= 256): double-buffered", order_only=True,
         sums_bitwise=True, with_keys=[(24, 1)], case="rows_gemm", shapes=GEMM_WIDE),
    _row(24, 1, "fgcn_rows_gemm*", ALL, "fewer than 256 workgroups with the large-problem tiles", proof="reasoning",
         test=OLD + "test_batched_row_gemms_one_and_two_levels"),
    # ---- key 4: the f32 halo conv's register budget -----------------------------------------------------------------------------------------
    _row(4, 1, "fgcn_tconv_halo", ("f32",), "math mode f32 (conv_halo_kernel<NT, 2, BF>)", order_only=True, sums_bitwise=True, case="tconv_halo",
         shapes=HALO),
    # ---- key 5: workgroup orders ------------------------------------------------------------------------------------------------------------
    _row(5, 1, "fgcn_rows_gemm*", ALL, "tiles_n > 1 and tiles_m * tiles_n < 2^30", order_only=True, sums_bitwise=True, case="rows_gemm",
         shapes=GEMM_ORDER),
    _row(5, 8, "fgcn_rows_gemm*", ALL, "tiles_n > 1 and tiles_m < 65536 and not key 5 bit 0", order_only=True, sums_bitwise=True, case="rows_gemm",
         shapes=GEMM_ORDER),
    _row(5, 4, "fgcn_rows_wgrad", ALL, "always (the default is the XCD-aware order; the bit selects the 3-D grid)", order_only=True,
         case="rows_wgrad", shapes=ROWS_WGRAD),
    _row(5, 16, "fgcn_spatial_fwd", X3, "split kernel (Cin % 32 == 0) and ncol = cdiv(Cout, 64) > 1", order_only=True, sums_bitwise=True,
         case="spatial_fwd", shapes=SPATIAL_FWD),
    _row(5, 32, "fgcn_tconv_halo", SPLIT, "split kernel, tiles * tiles_n < 2^30 (the default is the XCD-aware order; the bit selects the 2-D grid)",
         order_only=True, sums_bitwise=True, case="tconv_halo", shapes=HALO),
    _row(5, 2, "fgcn_tconv_halo", ("f32",), "math mode f32 and tiles * tiles_n < 2^30", order_only=True, sums_bitwise=True, case="tconv_halo",
         shapes=HALO),
    _row(5, 64, "fgcn_tconv_wgrad / fgcn_pw_wgrad", SPLIT, "split kernel and tiles_xy = tiles_k * tiles_n > 1 (the bit selects the 2-D grid)",
         order_only=True, case="tconv_wgrad", shapes=TWGRAD_ORDER),
    # ---- key 6: weight-gradient forms, joint_dagg forms -------------------------------------------------------------------------------------
    _row(6, 1, "fgcn_pw_wgrad", SPLIT, "chunk mode (1x1) in a split math mode: tconv_wgrad_kernel<NTAP, TN, BF> instead of the split kernel",
         case="pw_wgrad", shapes=PWGRAD),
    _row(6, 32, "fgcn_pw_wgrad", SPLIT, "chunk mode (1x1) on the split kernel: 8 waves", proof="query", case="pw_wgrad", shapes=PWGRAD),
    _row(6, 64, "fgcn_tconv_wgrad", SPLIT, "tap mode on the split kernel and N > 64: 8 waves (bf16x3) / 4 waves (bf16)", proof="query",
         case="tconv_wgrad", shapes=TWGRAD),
    _row(6, 256, "fgcn_tconv_wgrad", SPLIT, "tap mode on the split kernel and N <= 64: 4 waves", proof="query", case="tconv_wgrad", shapes=TWGRAD),
    _row(6, 128, "fgcn_tconv_wgrad", SPLIT, "tap mode on the split kernel, more than one tap per pass and N > 64 (at 64 columns the circular window "
         "does not fit beside the 128-row stage and is off by default): ring_rows = 0", case="tconv_wgrad", shapes=TWGRAD),
    _row(6, 8, "fgcn_joint_dagg", ("f32",) + X3, "n_extra == 2 (any mode), or n_extra == 0 outside math mode f32: two / three workgroups per CU",
         order_only=True, sums_bitwise=True, case="joint_dagg", shapes=DAGG),
    _row(6, 16, "fgcn_joint_dagg", X3, "n_extra == 0 outside math mode f32: the gram on the f32 MFMA", order_only=True, case="joint_dagg",
         shapes=DAGG),
    _row(6, 1024, "fgcn_joint_dagg", X3, "n_extra == 0 and n_subsets == 3 outside math mode f32, key 6 bit 3 clear: run-time subset count",
         order_only=True, sums_bitwise=True, case="joint_dagg", shapes=DAGG),
    _row(6, 2048, "fgcn_joint_dagg", X3, "n_extra == 0 and n_subsets == 3 outside math mode f32, key 6 bits 3 and 10 clear: one tile register set",
         order_only=True, sums_bitwise=True, case="joint_dagg", shapes=DAGG),
    _row(6, 512, "fgcn_spatial_wgrad", X3, "math mode bf16x3: spatial_wgrad_kernel<KS, 0>, the exact-f32 form", case="spatial_wgrad",
         shapes=SPATIAL_WGRAD),
    # ---- key 7: split-bf16 forward kernels --------------------------------------------------------------------------------------------------
    _row(7, 1, "fgcn_spatial_fwd", ("bf16x3",), "math mode bf16x3 with the bf16x3 products and Cin % 32 == 0: spatial_fwd_kernel<CI, CO, 2>",
         case="spatial_fwd", shapes=SPATIAL_FWD_OLD),
    _row(7, 8 | 32, "fgcn_tconv_halo", X3, "split kernel: the 2 x 2 wave arrangement over 128-row tiles", order_only=True, proof="reasoning",
         test=OLD + "test_halo_conv_wave_arrangements_agree"),
    _row(7, 64, "fgcn_tconv_halo", X3, "split kernel, 32 < N <= 128, tap form: the 4 x 1 arrangement whatever the tile count", order_only=True,
         proof="reasoning", test=OLD + "test_halo_conv_wave_arrangements_agree"),
    _row(7, 16 | 64, "fgcn_tconv_halo", SPLIT, "N > 128 (bf16: N > 32), tap form, no BatchNorm-backward sums, no fused stages, halo of at most "
         "426 rows, and (cdiv(Mv, 192) >= 1536 or key 7 bit 6): the 4 x 1 arrangement with a 128-column tile", order_only=True, with_keys=(),
         case="tconv_halo", shapes=HALO_WIDE),
    # ---- keys 8 .. 24 -----------------------------------------------------------------------------------------------------------------------
    _row(8, 1, "fgcn_pw_gemm", SPLIT, "always: one tile per workgroup", order_only=True, sums_bitwise=True, proof="reasoning",
         test=OLD + "test_persistent_pointwise_gemm"),
    _row(10, 1, "the activation-writing kernels", ALL, "a call that writes 96 MiB or more", order_only=True, sums_bitwise=True, proof="reasoning",
         test="tests/test_block_model_gpu.py::test_streamed_output_stores_change_no_bit"),
    _row(10, 2, "the activation-writing kernels", ALL, "a call that writes less than 96 MiB", order_only=True, sums_bitwise=True, proof="reasoning",
         test="tests/test_block_model_gpu.py::test_streamed_output_stores_change_no_bit"),
    _row(12, 1, "fgcn_joint_gram", ("f32", "bf16x3"), "n_items == 3 and equal widths of 16 / 32 / 64 and not share1: joint_gram_kernel",
         case="joint_gram", shapes=GRAM),
    _row(13, "target", "fgcn_spatial_wgrad", ALL, "always: workgroups to aim for", proof="query",
         test=OLD + "test_spatial_wgrad_with_many_frames_per_workgroup"),
    _row(15, "target", "fgcn_spatial_bwd_tile", SPLIT, "always: cdiv(target, B) segments per sample at most", proof="query", case="spatial_bwd_tile",
         shapes=SPATIAL_TILE),
    _row(16, "target", "fgcn_spatial_wgrad_tile", SPLIT, "always: workgroups to aim for", proof="query",
         test=OLD + "test_spatial_weight_gradient_tile_form"),
    _row(17, "target", "fgcn_emb_wgrad_tile", SPLIT, "always: workgroups to aim for", proof="query", test=OLD + "test_embedding_backward_tile_form"),
    _row(18, 1, "fgcn_emb_dx_tile", SPLIT, "Cx > 64 (128-column tiles): a two-slot weight ring", order_only=True, case="emb_dx_tile", shapes=EMB_TILE),
    _row(19, 1, "fgcn_emb_wgrad_tile", SPLIT, "always: emb values requested one frame slot ahead", order_only=True, case="emb_wgrad_tile",
         shapes=EMB_TILE),
    _row(21, 2, "fgcn_spatial_wgrad_tile / fgcn_emb_wgrad_tile", SPLIT, "always (emb: ic >= 32): 64 x 64 tiles", proof="reasoning",
         test=OLD + "test_spatial_weight_gradient_tile_form"),
    _row(22, "target", "fgcn_emb_fwd_tile", SPLIT, "always: resident workgroups to aim for", proof="reasoning",
         test=OLD + "test_embedding_forward_tile_form"),
    # ---- keys 25 / 26: bfloat16 tensors (math mode bf16) ------------------------------------------------------------------------------------
    _row(25, 1, "fgcn_tconv_halo", ("bf16",), "a bfloat16 output (half_mask 3), not accumulating, and stream_out(bytes): key 10 == 2 at small "
         "sizes", order_only=True, sums_bitwise=True, with_keys=[(10, 2)], case="tconv_halo_bf16_out", shapes=HALO_BF16_OUT),
    _row(25, 2, "fgcn_spatial_fwd_tile", ("bf16",), "a bfloat16 y (half_mask bit 1) and stream_out(bytes): key 10 == 2 at small sizes",
         order_only=True, sums_bitwise=True, with_keys=[(10, 2)], case="spatial_fwd_tile_bf16_out", shapes=SPATIAL_TILE),
    _row(26, 1, "fgcn_bn_act_bwd_reduce", ("bf16",), "half_mask != 0 and C % 8 == 0 and ld_dout == C: 256 threads, twice the LDS", case="bn_reduce_bf16",
         shapes=BN_REDUCE),
]

KEYS = sorted({r.key for r in TABLE})


def gpu_rows():
    """the rows tests/test_variants_gpu.py launches"""
    return [r for r in TABLE if r.case is not None]


@contextlib.contextmanager
def tuned(key, value, *more):
    """with tuned(5, 1): ... -- fgcn_set_tuning(key, value) (and further (key, value) pairs) in the calling thread's CURRENT context; the
    previous values come back in ``finally``, in that same context."""
    from fusion_gcn_amd import _lib
    lib = _lib.load()
    pairs = [(key, value)] + list(more)
    prev = [(k, lib.fgcn_get_tuning(k)) for k, _ in pairs]
    try:
        for k, v in pairs:
            _lib.check(lib.fgcn_set_tuning(k, v), "fgcn_set_tuning")
        yield
    finally:
        for k, v in reversed(prev):
            _lib.check(lib.fgcn_set_tuning(k, v), "fgcn_set_tuning")


# ---- the launchers' tile counts, from the public queries (tests/test_variants.py: the shapes of the workgroup orders) ----------------------
def cdiv(a, b):
    return -(-a // b)


def rows_gemm_tiles(lib, shape, key24=0):
    """-> (row tiles, column tiles) of fgcn_rows_gemm at the default tile keys.  The row tiles are fgcn_rows_gemm_tiles (128-row tiles: what a
    launch of fewer than 256 workgroups runs); the column tile is the launcher's rule restated (fgcn_gemm.hip, rows_gemm_launch): the width
    32 * nt with the fewest padded columns, halved while that leaves fewer than 256 workgroups."""
    B, T, V, K, N, kt, s = shape
    M = B * ((T - 1) // s + 1) * V
    nt, best = 4, None
    for c in (4, 3, 2, 1):
        padded = cdiv(N, 32 * c) * 32 * c
        if best is None or padded < best:
            best, nt = padded, c
    mt = 2 if nt <= 2 else 1
    if key24 != 1:
        wgs = lambda mt_, nt_: cdiv(M, 128 * mt_) * cdiv(N, 32 * nt_)      # noqa: E731
        if mt == 2 and wgs(mt, nt) < 256:
            mt = 1
        while nt % 2 == 0 and wgs(mt, nt) < 256:
            nt //= 2
        if nt == 3 and wgs(mt, nt) < 256:
            nt = 1
    tiles_m = lib.fgcn_rows_gemm_tiles(M)
    assert mt == 1 or key24 == 1
    return (tiles_m if mt == 1 else cdiv(tiles_m, 2)), cdiv(N, 32 * nt)


def rows_wgrad_total(shape):
    """tiles x taps x row splits of fgcn_rows_wgrad as ops.rows_wgrad(wide=False) launches it (ops._pick_nsplit)"""
    from fusion_gcn_amd import ops
    B, T, V, K, N, kt, s = shape
    return cdiv(K, 64) * cdiv(N, 64) * kt * ops._pick_nsplit(B * ((T - 1) // s + 1) * V, K, N, kt)


def halo_tiles(lib, shape):
    B, T, V, K, N = shape
    return lib.fgcn_tconv_halo_tiles(B, T, T, V), cdiv(N, 64 if N <= 64 else 128)


def spatial_fwd_tiles(lib, shape):
    V, T, cin, cout, B = shape
    return lib.fgcn_spatial_tiles(B, T), cdiv(cout, 64)


def twgrad_tiles(lib, shape):
    """-> ((channel group, column tile) pairs, row splits) of the all-taps weight gradient on the split kernel, the row splits as
    ops.tconv_wgrad picks them (restated: its rule reads the two exported limits)"""
    from fusion_gcn_amd import ops
    B, T, V, K, N, kt, s = shape
    T_g = (T - 1) // s + 1
    tiles = cdiv(K, 32) * (cdiv(N, 128) if N > 64 else 1)
    stages = B * cdiv(T_g * V, 64) if N > 64 else B * cdiv(T_g * V, 128)
    cap = max(1, lib.fgcn_tconv_wgrad_resident(N) // max(tiles, 1))
    nsplit = max(1, min(cap, max(stages // ops.WGRAD_MIN_STAGES, min(stages, max(1, 256 // max(tiles, 1))))))
    return tiles, nsplit
