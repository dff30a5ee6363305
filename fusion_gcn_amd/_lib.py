"""ctypes binding of libfgcn.so (the C ABI declared in include/fgcn.h).

No fallback: if the library is missing or the device is not gfx950 every entry point raises.  Build it with
``python -m fusion_gcn_amd.build`` (or ``__graft_entry__.build()``).
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FGCN_LIB") or os.path.join(_HERE, "libfgcn.so")   # FGCN_LIB: timing-probe builds (tools/probes)

c_float_p = C.c_void_p  # device pointers travel as integers (tensor.data_ptr())


class TMap(C.Structure):
    """fgcn_tmap: ti = (to*ta + j*tb + tc) / td."""
    _fields_ = [("taps", C.c_int), ("ta", C.c_int), ("tb", C.c_int), ("tc", C.c_int), ("td", C.c_int)]


class MixTerm(C.Structure):
    _fields_ = [("mat", C.c_short), ("transpose", C.c_short), ("in_c_lo", C.c_short), ("in_c_hi", C.c_short),
                ("mask", C.c_short)]


class MixItem(C.Structure):
    _fields_ = [("out_c", C.c_short), ("width", C.c_short), ("nterms", C.c_short), ("term", MixTerm * 3)]


class MixVTerm(C.Structure):
    _fields_ = [("mat", C.c_short), ("transpose", C.c_short), ("in_c", C.c_short)]


class MixVItem(C.Structure):
    _fields_ = [("out_c", C.c_short), ("nch", C.c_short), ("nterms", C.c_short), ("term", MixVTerm * 3)]


class GramItem(C.Structure):
    _fields_ = [("c1", C.c_short), ("c2", C.c_short), ("width", C.c_short), ("mat", C.c_short)]


class PackSeg(C.Structure):
    """fgcn_pack_seg: one strided window of a parameter tensor inside a packed form."""
    _fields_ = [("src", C.c_void_p), ("st_tap", C.c_longlong), ("st_k", C.c_longlong), ("st_n", C.c_longlong),
                ("t0", C.c_int), ("tlen", C.c_int), ("k0", C.c_int), ("klen", C.c_int), ("n0", C.c_int), ("nlen", C.c_int),
                ("tap0", C.c_int), ("tap_step", C.c_int)]


PACK_MAX_SEG = 6            # FGCN_PACK_MAX_SEG
PACK_MODES = {"plain": 0, "k4": 1, "split3": 2, "split3_acc": 3, "split2h": 4, "split2h_acc": 5}       # FGCN_PACK_*


class PackItem(C.Structure):
    """fgcn_pack_item: one packed / split weight form = a sum of segments + the layout its consumer streams."""
    _fields_ = [("dst", C.c_void_p), ("mode", C.c_int), ("taps", C.c_int), ("K", C.c_int), ("N", C.c_int),
                ("kgroups", C.c_int), ("nseg", C.c_int), ("seg", PackSeg * PACK_MAX_SEG)]


class ReduceItem(C.Structure):
    """fgcn_reduce_item: one slab sum of a batched fgcn_reduce_multi launch."""
    _fields_ = [("dst", C.c_void_p), ("src", C.c_void_p), ("st_tap", C.c_longlong), ("st_k", C.c_longlong), ("st_n", C.c_longlong),
                ("S", C.c_int), ("taps", C.c_int), ("K", C.c_int), ("N", C.c_int), ("K_dst", C.c_int), ("accumulate", C.c_int)]


REDUCE_MAX_ITEMS = 8        # FGCN_REDUCE_MAX_ITEMS


class OptimGroup(C.Structure):
    """fgcn_optim_group: the scalars of one parameter group of the optimizer step."""
    _fields_ = [("lr", C.c_float), ("weight_decay", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float),
                ("momentum", C.c_float), ("dampening", C.c_float), ("nesterov", C.c_int)]


class OptimGuard(C.Structure):
    """fgcn_optim_guard: the guard of the optimizer step (clip by global norm, skip non-finite steps) and its device state."""
    _fields_ = [("max_norm", C.c_double), ("skip_nonfinite", C.c_int), ("n_partials", C.c_int), ("partials", C.c_void_p),
                ("state", C.c_void_p), ("group_sched", C.c_void_p)]


OPT_MAX_GROUPS = 8          # FGCN_OPT_MAX_GROUPS
OPT_TILE4 = 1024            # FGCN_OPT_TILE4: 16-byte groups per row of the tile table, at most

FUSE_MAX_STREAMS = 8        # FGCN_FUSE_MAX_STREAMS
FUSE_PASS = 2048            # FGCN_FUSE_PASS
FUSE_MAX_CANDIDATES = 1 << 20      # FGCN_FUSE_MAX_CANDIDATES
FUSE_TRANSFORMS = {"none": 0, "softmax": 1}            # enum fgcn_fuse_transform
FUSE_EXAMPLES, FUSE_IGNORED, FUSE_INVALID, FUSE_HEADER = range(4)      # enum fgcn_fuse_word: the words at the head of fgcn_fuse_sweep's counts


class FuseIn(C.Structure):
    """FgcnFuseIn: the score tensors of the stream models (device pointers, row strides in floats) and, for fgcn_score_fuse, their weights."""
    _fields_ = [("scores", C.c_void_p * FUSE_MAX_STREAMS), ("ld", C.c_int * FUSE_MAX_STREAMS), ("weight", C.c_float * FUSE_MAX_STREAMS)]


_I, _LL, _F, _D, _P = C.c_int, C.c_longlong, C.c_float, C.c_double, C.c_void_p

# name -> (restype, argtypes); mirrors include/fgcn.h one to one.  The fifteen kernels that take bfloat16 activation tensors carry `half_mask`
# (an int) immediately before the stream (include/fgcn.h, "storage types and half_mask")
SIGNATURES = {
    "fgcn_version": (_I, []),
    "fgcn_last_error": (C.c_char_p, []),
    "fgcn_check_device": (_I, []),
    "fgcn_ctx_create": (_I, [C.POINTER(C.c_void_p)]),
    "fgcn_ctx_destroy": (_I, [_P]),
    "fgcn_ctx_set_current": (_I, [_P]),
    "fgcn_ctx_get_current": (_P, []),
    "fgcn_set_tuning": (_I, [_I, _I]),
    "fgcn_get_tuning": (_I, [_I]),
    "fgcn_set_math_mode": (_I, [_I]),
    "fgcn_get_math_mode": (_I, []),
    "fgcn_set_products": (_I, [_I]),
    "fgcn_get_products": (_I, []),
    "fgcn_rows_gemm": (_I, [_P] * 5 + [_I] * 8 + [TMap, _I, _I, _P]),
    "fgcn_rows_gemm_batched": (_I, [_P, _P, _P, _I, _LL, _LL, _LL, _I, _I, _I, _I, _I, _I, _P]),
    "fgcn_rows_gemm_batched2": (_I, [_P, _P, _P, _I, _LL, _LL, _LL, _I, _LL, _LL, _LL, _I, _I, _I, _I, _I, _I, _P]),
    "fgcn_rows_gemm_tiles": (_I, [_LL]),
    "fgcn_tconv_halo_tiles": (_I, [_I, _I, _I, _I]),
    "fgcn_tconv_halo": (_I, [_P] * 3 + [_I] + [_P] * 2 + [_I] * 18 + [_P] * 8 + [_I, _P]),
    "fgcn_tconv_halo_bn_sums": (_I, []),
    "fgcn_rows_wgrad": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, TMap, _I, _P]),
    "fgcn_tconv_wgrad_slabs": (_I, [_I, _I]),
    "fgcn_pw_wgrad_slabs": (_I, [_I, _I]),
    "fgcn_tconv_wgrad_resident": (_I, [_I]),
    "fgcn_pw_wgrad_resident": (_I, [_I]),
    "fgcn_tconv_wgrad": (_I, [_P] * 3 + [_I] * 17 + [_P, _P, _I, _P]),
    "fgcn_pw_wgrad_chunks": (_I, [_I, _I]),
    "fgcn_pw_wgrad": (_I, [_P] * 3 + [_I] * 11 + [_P, _P, _I, _P]),
    "fgcn_reduce_sum": (_I, [_P, _P, _I, _LL, _I, _P]),
    "fgcn_reduce_sum_strided": (_I, [_P, _P, _I, _I, _I, _I, _I, _LL, _LL, _LL, _I, _P]),
    "fgcn_reduce_multi": (_I, [C.POINTER(ReduceItem), _I, _P]),
    "fgcn_group_mean_splits": (_I, [_I, _I]),
    "fgcn_group_mean": (_I, [_P, _P, _P, _I, _I, _I, _I, _P]),
    "fgcn_pack_split3": (_I, [_P, _P, _I, _I, _I, _I, _P]),
    "fgcn_pack_weight": (_I, [_P, _P, _I, _I, _I, _I, _LL, _LL, _LL, _I, _P]),
    "fgcn_pack_kgroups": (_I, [_I, _I]),
    "fgcn_pack_units": (_LL, [_I, _I, _I, _I]),
    "fgcn_pack_run": (_I, [_P, _P, _I, _P]),
    "fgcn_pack_run_scaled": (_I, [_P, _P, _I, _I, _P]),
    "fgcn_joint_mix": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, C.POINTER(MixItem), _I, _I, _P]),
    "fgcn_joint_mix_vec": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, C.POINTER(MixVItem), _I, _I, _I, _P, _P, _P]),
    "fgcn_joint_mix_chunks": (_I, [_I, _I]),
    "fgcn_joint_gram": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, C.POINTER(GramItem), _I, _P]),
    "fgcn_spatial_wgrad_chunks": (_I, [_I, _I, _I, _I]),
    "fgcn_spatial_wgrad": (_I, [_P] * 4 + [_I] * 9 + [_P]),
    "fgcn_spatial_wgrad_tile": (_I, [_P] * 4 + [_I] * 9 + [_P]),
    "fgcn_spatial_wgrad_tile_slabs": (_I, [_I] * 5),
    "fgcn_spatial_wgrad_tile_available": (_I, [_I] * 3),
    "fgcn_emb_fwd_tile": (_I, [_P] * 5 + [_I] * 8 + [_P]),
    "fgcn_emb_fwd_tile_segments": (_I, [_I] * 4),
    "fgcn_emb_fwd_tile_available": (_I, [_I] * 3),
    "fgcn_emb_dx_tile": (_I, [_P] * 5 + [_I] * 9 + [_P, _I, _P]),
    "fgcn_emb_dx_tile_workspace": (_LL, [_I, _I]),
    "fgcn_emb_wgrad_tile": (_I, [_P] * 5 + [_I] * 9 + [_P]),
    "fgcn_emb_wgrad_tile_slabs": (_I, [_I] * 5),
    "fgcn_emb_tile_available": (_I, [_I] * 3),
    "fgcn_joint_dagg": (_I, [_P] * 5 + [_I] * 11 + [_P] * 5),
    "fgcn_adj_softmax_fwd": (_I, [_P, _I, _F, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "fgcn_adj_softmax_bwd": (_I, [_P, _I, _F, _P, _P, _P, _I, _I, _I, _P]),
    "fgcn_joint_mix_wide": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, C.POINTER(MixVItem), _I, _I, _P]),
    "fgcn_joint_gram_wide": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, C.POINTER(GramItem), _I, _P]),
    "fgcn_adj_softmax_fwd_wide": (_I, [_P, _I, _F, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "fgcn_adj_softmax_bwd_wide": (_I, [_P, _I, _F, _P, _P, _P, _I, _I, _I, _P]),
    "fgcn_bn_finalize": (_I, [_P, _I, _LL, _P, _P, _P, _P, _F, _F, _P, _I, _P, _I, _LL, _P]),
    "fgcn_bn_eval_coeffs": (_I, [_P, _P, _P, _P, _F, _P, _I, _P]),
    "fgcn_bn_act": (_I, [_P] * 6 + [_LL, _I, _I, _I, _I, _P]),
    "fgcn_tconv_halo_bn_relu": (_I, [_P] * 7 + [_I] * 10 + [_P]),
    "fgcn_spatial_fwd_tile_bn_relu": (_I, [_P] * 7 + [_I] + [_P] + [_I] * 8 + [_P]),
    "fgcn_bn_act_pool_splits": (_I, [_I, _I]),
    "fgcn_bn_act_pool": (_I, [_P] * 7 + [_I] * 5 + [_P]),
    "fgcn_bn_act_bwd_reduce": (_I, [_P, _I] + [_P] * 7 + [_I, _LL, _I, _I, _I, _I, _P]),
    "fgcn_bn_act_bwd_apply": (_I, [_P, _I] + [_P] * 9 + [_LL] + [_I] * 6 + [_P]),
    "fgcn_elem_tiles": (_I, [_LL]),
    "fgcn_bn_apply_ld": (_I, [_P, _P, _P, _LL, _I, _I, _P]),
    "fgcn_bn_bwd_reduce_ld": (_I, [_P, _I, _P, _P, _P, _I, _LL, _I, _P]),
    "fgcn_bn_bwd_apply_ld": (_I, [_P, _I, _P, _P, _P, _P, _LL, _I, _I, _P]),
    "fgcn_col_sum": (_I, [_P, _P, _LL, _I, _I, _P]),
    "fgcn_spatial_fwd": (_I, [_P, _P, _P, _I, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "fgcn_spatial_tiles": (_I, [_I, _I]),
    "fgcn_spatial_fwd_tile": (_I, [_P] * 6 + [_I] * 9 + [_P]),
    "fgcn_spatial_fwd_tile_tiles": (_I, [_I, _I, _I]),
    "fgcn_spatial_fwd_tile_available": (_I, [_I, _I, _I]),
    "fgcn_spatial_bwd_tile": (_I, [_P] * 6 + [_I] * 10 + [_P, _I, _P, _P, _P, _I, _P]),
    "fgcn_spatial_bwd_tile_segments": (_I, [_I, _I, _I]),
    "fgcn_spatial_bwd_tile_available": (_I, [_I, _I, _I]),
    "fgcn_transpose": (_I, [_P, _P, _I, _I, _I, _I, _I, _P]),
    "fgcn_graph_spmm": (_I, [_P] * 8 + [_I] * 8 + [_P]),
    "fgcn_row_softmax_fwd": (_I, [_P, _P, _P, _P, _LL, _I, _I, _I, _F, _P]),
    "fgcn_row_softmax_bwd": (_I, [_P, _P, _P, _LL, _I, _I, _F, _P]),
    "fgcn_tmaxpool3_fwd": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "fgcn_tmaxpool3_bwd": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "fgcn_unfold_windows": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "fgcn_pw_gemm_available": (_I, []),
    "fgcn_pw_gemm_tiles": (_I, [_LL]),
    "fgcn_pw_gemm": (_I, [_P] * 3 + [_I] + [_P] * 2 + [_LL] + [_I] * 5 + [_P, _I, _P]),
    "fgcn_data_bn_tiles": (_I, [_I, _I]),
    "fgcn_data_bn_stats": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "fgcn_data_bn_apply": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "fgcn_data_bn_bwd_reduce": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "fgcn_data_bn_bwd_apply": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "fgcn_patch_input_slabs": (_I, [_I, _I, _I, _I, _I]),
    "fgcn_patch_input_fwd": (_I, [_P] * 8 + [_I] * 11 + [_P]),
    "fgcn_patch_input_bwd": (_I, [_P] * 10 + [_I] * 10 + [_P]),
    "fgcn_cross_entropy_fwd": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "fgcn_cross_entropy_bwd": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "fgcn_ce_workspace_bytes": (_LL, [_I]),
    "fgcn_ce_fwd": (_I, [_P] * 9 + [_I, _I, _I, _I, _LL, _F, _I, _P]),
    "fgcn_ce_bwd": (_I, [_P] * 8 + [_I, _I, _I, _I, _LL, _F, _I, _P]),
    "fgcn_optim_step": (_I, [_P, _P, _P, _P, _LL, _I, C.POINTER(OptimGroup), _I, _P, _I, _F, _LL, C.POINTER(OptimGuard), _P]),
    "fgcn_grad_norm_tiles": (_I, [_LL]),
    "fgcn_optim_guard_bytes": (_LL, []),
    "fgcn_classify_state_bytes": (_LL, [_I]),
    "fgcn_classify_update": (_I, [_P, _P, _P, _P, _P, _LL, _LL, _I, _I, _I, _I, _P]),
    "fgcn_philox4x32_10": (_I, [C.POINTER(C.c_uint), C.POINTER(C.c_uint), C.POINTER(C.c_uint)]),
    "fgcn_dropout_fwd": (_I, [_P, _P, _P, _LL, _F, C.c_ulonglong, C.c_uint, _P, _P]),
    "fgcn_dropout_bwd": (_I, [_P, _P, _P, _LL, _F, _P]),
    "fgcn_rng_advance": (_I, [_P, _P]),
    "fgcn_clip_augment": (_I, [_P] * 6 + [_I] * 7 + [C.POINTER(C.c_float), _F, _F, C.c_ulonglong, C.c_uint, C.c_uint, _P]),
    "fgcn_augment_params": (_I, [C.c_uint, C.c_uint, C.c_uint, C.c_ulonglong, C.POINTER(C.c_float), _F, _F, C.POINTER(C.c_float)]),
    "fgcn_clip_normalize": (_I, [_P] * 5 + [_I] * 10 + [_P]),
    "fgcn_clip_bodies": (_I, [_P] * 5 + [_I] * 6 + [_P]),
    "fgcn_resample_index": (_I, [_I, _I, _I, C.POINTER(C.c_int)]),
    "fgcn_signal_prepare": (_I, [_P] * 6 + [_I] * 5 + [_P]),
    "fgcn_imu_enhance": (_I, [_P] * 7 + [_I] * 7 + [_P]),
    "fgcn_clip_streams": (_I, [_P] * 8 + [_I] * 5 + [_P]),
    "fgcn_clip_window": (_I, [_P] * 6 + [_I] * 5 + [_F, _F, _I, C.c_ulonglong, C.c_uint, C.c_uint, _P]),
    "fgcn_window_params": (_I, [C.c_uint, C.c_uint, C.c_uint, C.c_ulonglong, _F, _F, _I, C.POINTER(C.c_float)]),
    "fgcn_clip_valid_frames": (_I, [_P, _P, _P, _I, _I, _I, _I, _P]),
    "fgcn_clip_sensors": (_I, [_P] * 7 + [_I] * 6 + [C.POINTER(C.c_float), _F, _F, _I, C.POINTER(C.c_float), _F, _I, C.c_ulonglong, C.c_uint,
                               C.c_uint, _P]),
    "fgcn_sensors_params": (_I, [C.c_uint, C.c_uint, C.c_uint, C.c_ulonglong, C.POINTER(C.c_float), _F, _F, _I, _F, _I, C.POINTER(C.c_float)]),
    "fgcn_score_fuse": (_I, [C.POINTER(FuseIn), _I, _I, _P, _I, _I, _I, _P]),
    "fgcn_fuse_sweep": (_I, [C.POINTER(FuseIn), _I, _I, _P, _I, _P, _I, _I, _I, _P, _P]),
    "fgcn_stc_splits": (_I, [_I, _I]),
    "fgcn_stc_mean_t": (_I, [_P] * 2 + [_I] * 4 + [_P]),
    "fgcn_stc_gate_s": (_I, [_P] * 4 + [_I] * 3 + [_P]),
    "fgcn_stc_mean_v": (_I, [_P] * 3 + [_I] * 4 + [_P]),
    "fgcn_stc_gates_tc": (_I, [_P] * 11 + [_I] * 3 + [_P]),
    "fgcn_stc_apply": (_I, [_P] * 5 + [_I] * 4 + [_P]),
    "fgcn_stc_bwd_qr": (_I, [_P] * 6 + [_I] * 4 + [_P]),
    "fgcn_stc_bwd_tc": (_I, [_P] * 16 + [_I] * 3 + [_P]),
    "fgcn_stc_bwd_ds": (_I, [_P] * 3 + [_I] * 4 + [_P]),
    "fgcn_stc_bwd_s": (_I, [_P] * 10 + [_I] * 4 + [_P]),
    "fgcn_stc_bwd_apply": (_I, [_P] * 7 + [_I] * 4 + [_P]),
    "fgcn_stc_param_grads": (_I, [_P] * 16 + [_I] * 3 + [_P]),
    "fgcn_ctr_chunk": (_I, []),
    "fgcn_ctr_split_frames": (_I, [_I] * 4),
    "fgcn_ctr_mean_t": (_I, [_P] * 2 + [_I] * 4 + [_P]),
    "fgcn_ctr_mean_t_bwd": (_I, [_P] * 2 + [_I] * 5 + [_P]),
    "fgcn_ctr_tanh": (_I, [_P] * 2 + [_I] * 3 + [_P]),
    "fgcn_ctr_aggregate": (_I, [_P] * 7 + [_I] * 5 + [_P]),
    "fgcn_ctr_bwd_dx3": (_I, [_P] * 7 + [_I] * 5 + [_P]),
    "fgcn_ctr_bwd_da": (_I, [_P] * 3 + [_I] * 4 + [_P]),
    "fgcn_ctr_bwd_small": (_I, [_P] * 11 + [_I] * 4 + [_P]),
    "fgcn_ctr_param_grads": (_I, [_P] * 9 + [_I] * 4 + [_P]),
    "fgcn_shift_joint_rows": (_I, [_LL, _I, _I]),
    "fgcn_shift_joint_stage": (_I, [_I]),
    "fgcn_shift_frame_split": (_I, [_I] * 5),
    "fgcn_shift_joint": (_I, [_P] * 5 + [_LL] + [_I] * 5 + [_P]),
    "fgcn_shift_dmask": (_I, [_P] * 3 + [_I] * 4 + [_P]),
    "fgcn_shift_frame": (_I, [_P] * 4 + [_I] * 6 + [_P]),
    "fgcn_shift_frame_bwd": (_I, [_P] * 5 + [_I] * 6 + [_P]),
}

# enum fgcn_cls_word: the 8-byte words at the head of a classify state (include/fgcn.h)
CLS_EXAMPLES, CLS_TOP1, CLS_TOPK, CLS_IGNORED, CLS_INVALID, CLS_DROPPED, CLS_LOSS_ITEMS, CLS_LOSS_SUM, CLS_WORDS = range(9)
CLS_MAX_CLASSES = 1024      # FGCN_CLS_MAX_CLASSES
CE_REDUCTIONS = {"mean": 0, "sum": 1, "none": 2}       # enum fgcn_ce_reduction
# enum fgcn_guard_word: the 8-byte words of the guarded optimizer step's state (include/fgcn.h)
GUARD_STEP, GUARD_SKIPPED, GUARD_CLIPPED, GUARD_NORM, GUARD_COEF, GUARD_APPLY, GUARD_FIRST_STEP, GUARD_WORDS = range(8)
GRAD_NORM_MAX_TILES = 512   # FGCN_GRAD_NORM_MAX_TILES
NORMALIZE_MAX_T = 4096      # FGCN_NORMALIZE_MAX_T
BODIES_MAX = 16             # FGCN_BODIES_MAX
BODIES_MAX_T = 524288       # FGCN_BODIES_MAX_T
WINDOW_MODES = {"random": 0, "centre": 1}              # enum fgcn_window_mode
SENSORS_MAX = 16            # FGCN_SENSORS_MAX
SENSORS_MAX_KNOTS = 8       # FGCN_SENSORS_MAX_KNOTS

_lib = None


class FgcnError(RuntimeError):
    pass


def load() -> C.CDLL:
    """Load libfgcn.so once; raises (never falls back) when it is absent."""
    global _lib
    if _lib is None:
        # torch ships its own HIP runtime (torch/lib/libamdhip64.so); it must be the one already mapped when
        # libfgcn.so resolves its HIP symbols, otherwise two runtimes coexist and ours sees no device.
        import torch  # noqa: F401
        if not os.path.exists(LIB_PATH):
            raise FgcnError(f"{LIB_PATH} not found: build the HIP extension first (python -m fusion_gcn_amd.build). "
                            "There is no CPU / eager fallback for the AGCN block.")
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)          # AttributeError if the library does not export a declared symbol
            fn.restype, fn.argtypes = res, args
        _lib = lib
    return _lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().fgcn_last_error()
        raise FgcnError(f"{what} failed ({rc}): {msg.decode(errors='replace') if msg else ''}")
