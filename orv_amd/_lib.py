"""ctypes binding of liborv_mi355.so (the C ABI declared in include/orv_mi355.h).

The product path has NO fallback: if the shared library is missing or a call fails, a RuntimeError is raised.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, Structure, c_char_p, c_double, c_float, c_int, c_long, c_uint, c_ulong, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
# ORV_LIB: another build of the same library (developer A/B runs: tools/*.sh); the default is the in-tree build
LIB_PATH = os.environ.get("ORV_LIB") or os.path.join(_HERE, "liborv_mi355.so")


class Groups(Structure):
    _fields_ = [("seq", c_int), ("n_text", c_int), ("per_group", c_int)]


class RowMap(Structure):
    _fields_ = [("rows", c_int), ("bstride", c_int), ("off", c_int)]


class Gemm(Structure):
    _fields_ = [("A", c_void_p), ("lda", c_int), ("W", c_void_p), ("ldw", c_int), ("bias", c_void_p),
                ("C", c_void_p), ("ldc", c_int), ("M", c_int), ("N", c_int), ("K", c_int), ("epilogue", c_int),
                ("R", c_void_p), ("ldr", c_int), ("r_mod", c_int), ("gate", c_void_p), ("gate_b", c_long),
                ("gate_g", c_long), ("grp", Groups), ("cmap", RowMap), ("Y", c_void_p), ("ldy", c_int),
                ("qn_gamma_q", c_void_p), ("qn_beta_q", c_void_p), ("qn_gamma_k", c_void_p), ("qn_beta_k", c_void_p),
                ("qn_eps", c_float), ("qn_premul", c_float), ("qn_heads", c_int), ("a_packed", c_int), ("c_packed", c_int)]


class Conv(Structure):
    _fields_ = [("src", c_void_p)] + [(n, c_int) for n in ("B", "Ts", "Hs", "Ws", "C", "T", "H", "W", "kt", "kh", "kw", "stride",
                                                             "pad_lo", "ups_s", "ups_t", "t_shift")]


class Frames(Structure):
    _fields_ = [("data", c_void_p), ("kind", c_int), ("h", c_int), ("w", c_int), ("extent", c_long), ("offset", c_long), ("stride", c_long * 4)]


class SnapshotEntry(Structure):      # orv_snapshot_entry_t
    _fields_ = [("src", c_void_p), ("dst", c_void_p), ("bytes", c_long)]


ADAMW_MAX_GROUPS = 8        # ORV_ADAMW_MAX_GROUPS


class AdamwGroups(Structure):      # orv_adamw_groups_t, passed by value
    _fields_ = [("ngroups", c_int), ("lr", c_float * ADAMW_MAX_GROUPS), ("weight_decay", c_float * ADAMW_MAX_GROUPS)]


class Came(Structure):      # orv_came_t
    _fields_ = ([(n, c_void_p) for n in ("p", "lo", "g", "m", "r", "c", "res_r", "res_c", "v")]
                + [(n, c_long) for n in ("n", "n_rows", "n_cols", "n_v")]
                + [("seg_start", c_void_p), ("seg_active", c_void_p), ("nseg", c_int), ("geom", c_void_p)]
                + [(n, c_long) for n in ("n_tiles", "n_mats", "n_rowp", "n_colp")]
                + [("scratch", c_void_p), ("n_scratch", c_long), ("clip_coef", c_void_p)]
                + [(n, c_float) for n in ("lr", "beta1", "beta2", "beta3", "eps1", "eps2", "clip_threshold", "weight_decay")]
                + [("mode", c_int)])


# name -> (restype, argtypes); every symbol include/orv_mi355.h declares
SIGNATURES = {
    "orv_version": (c_int, []),
    "orv_last_error": (c_char_p, []),
    "orv_device_check": (c_int, [c_int]),
    "orv_timestep_embedding": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_void_p]),
    "orv_skinny_linear": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                  c_int, c_int, c_int, RowMap, c_void_p]),
    "orv_patchify": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int,
                             c_void_p]),
    "orv_unpatchify": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "orv_gather_rows": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "orv_scatter_gated_rows": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_long, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                       c_void_p]),
    "orv_add_rows": (c_int, [c_void_p, c_int, RowMap, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "orv_layernorm_modulate": (c_int, [c_void_p, c_int, RowMap, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                       c_void_p, c_long, c_long, Groups, c_int, c_int, c_float, c_void_p]),
    "orv_layernorm_modulate_packed": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_long, Groups,
                                              c_int, c_int, c_float, c_void_p]),
    "orv_modulation_tables": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                      c_int, c_void_p]),
    "orv_qkv_prep": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                             c_int, c_int, c_int, c_int, c_float, c_float, c_void_p]),
    "orv_qkv_prep_from": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                  c_int, c_int, c_int, c_int, c_int, c_float, c_float, c_void_p]),
    "orv_gemm_kernel_name": (c_int, [c_int, c_int, c_int, c_int, ctypes.c_char_p, c_int]),
    "orv_gemm_kernel_name_packed": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, ctypes.c_char_p, c_int]),
    "orv_gemm_force_tile": (c_int, [c_int, c_int, c_int]),
    "orv_gemm_force_epoch": (c_int, []),
    "orv_gemm_tn_bf16": (c_int, [c_void_p, c_long, c_void_p, c_long, c_void_p, c_long, c_int, c_int, c_int, c_int, c_void_p]),
    "orv_gemm_tn_skinny_scratch": (c_long, [c_int, c_int, c_int]),
    "orv_gemm_tn_skinny_bf16": (c_int, [c_void_p, c_long, c_void_p, c_long, c_void_p, c_long, c_int, c_int, c_int, c_float, c_int, c_void_p,
                                        c_void_p]),
    "orv_gemm_bf16": (c_int, [POINTER(Gemm), c_void_p]),
    "orv_packed_rows": (c_long, [c_long]),
    "orv_mxfp8_quantize": (c_int, [c_void_p, c_long, c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "orv_gemm_mxfp8": (c_int, [POINTER(Gemm), c_void_p, c_void_p, c_void_p]),
    "orv_layernorm_modulate_mxfp8": (c_int, [c_void_p, c_int, RowMap, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                             c_long, c_long, Groups, c_int, c_int, c_float, c_void_p]),
    "orv_pack_rows16": (c_int, [c_void_p, c_long, c_void_p, c_int, c_int, c_void_p]),
    "orv_unpack_rows16": (c_int, [c_void_p, c_void_p, c_long, c_int, c_int, c_void_p]),
    "orv_attention_fwd": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int,
                                  c_float, c_void_p]),
    "orv_attention_fwd_bounded": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_float, c_float, c_void_p]),
    "orv_attention_fwd_packed": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_float, c_void_p]),
    "orv_attention_static_limit": (c_float, [c_int]),
    "orv_attention_ws_bytes": (ctypes.c_size_t, [c_int, c_int, c_int]),
    "orv_attention_fwd_bounded_ws": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_float, c_float, c_void_p,
                                             ctypes.c_size_t, c_void_p]),
    "orv_attention_fwd_bounded_dev": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_float, c_void_p, c_void_p]),
    "orv_attention_kernel_name": (c_int, [c_int, c_int, c_int, c_int, c_float, c_float, c_int, ctypes.c_char_p, c_int]),
    "orv_transpose_bf16": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p]),
    "orv_transpose_colsum_bf16": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "orv_colsum": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_void_p]),
    "orv_gated_residual_bwd_scratch": (c_long, [Groups, c_int, c_int]),
    "orv_gated_residual_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_long, Groups, c_int,
                                       c_int, c_void_p]),
    "orv_layernorm_modulate_bwd_scratch": (c_long, [Groups, c_int, c_int]),
    "orv_layernorm_modulate_bwd": (c_int, [c_void_p, c_void_p, RowMap, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                           c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_long, Groups, c_int,
                                           c_int, c_float, c_void_p]),
    "orv_modulation_tables_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                          c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "orv_small_linear_bwd": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                     c_int, c_int, c_int, c_void_p]),
    "orv_adamw": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_float, c_float, c_float, c_float, c_float, c_int,
                          c_void_p, c_void_p]),
    "orv_adamw_flat": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_void_p, c_void_p, c_int, c_float, c_float,
                               c_float, c_float, c_float, c_int, c_void_p, c_void_p]),
    "orv_adamw_flat_steps": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_void_p, c_void_p, c_void_p, c_int,
                                     c_float, c_float, c_float, c_float, c_float, c_int, c_void_p, c_void_p]),
    "orv_adamw_flat_ex": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_void_p, c_void_p, c_void_p, c_int,
                                  c_float, c_float, c_float, c_float, c_float, c_int, c_void_p, c_void_p, c_int, c_uint, c_void_p]),
    "orv_adamw_flat_s8": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_void_p, c_void_p, c_void_p, c_int,
                                  c_float, c_float, c_float, c_float, c_float, c_int, c_void_p, c_void_p, c_int, c_uint, c_void_p]),
    "orv_adamw_flat_groups": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                                      AdamwGroups, c_float, c_float, c_float, c_int, c_void_p, c_void_p, c_int, c_uint, c_void_p]),
    "orv_adamw_flat_s8_groups": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_void_p, c_void_p, c_void_p,
                                         c_int, c_void_p, AdamwGroups, c_float, c_float, c_float, c_int, c_int, c_void_p, c_void_p, c_int,
                                         c_uint, c_void_p]),
    "orv_segment_sumsq": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "orv_step_guard": (c_int, [c_void_p, c_void_p, c_int, c_float, c_float, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "orv_state8_quantize": (c_int, [c_void_p, c_void_p, c_void_p, c_long, c_int, c_uint, c_int, c_void_p]),
    "orv_state8_dequantize": (c_int, [c_void_p, c_void_p, c_void_p, c_long, c_int, c_void_p]),
    "orv_prodigy_moments": (c_int, [c_void_p] * 7 + [c_long, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_float, c_float,
                                    c_float, c_float, c_float, c_int, c_int, c_int, c_double, c_void_p, c_void_p]),
    "orv_prodigy_recurrence": (c_int, [c_void_p, c_void_p, c_long, c_float, c_float, c_float, c_float, c_int, c_double, c_double, c_double,
                                       c_void_p]),
    "orv_prodigy_update": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_void_p, c_void_p, c_int, c_void_p, c_float, c_float,
                                   c_int, c_void_p]),
    "orv_came_launch": (c_int, [POINTER(Came), c_int, c_void_p]),
    "orv_came_step": (c_int, [POINTER(Came), c_void_p]),
    "orv_ema_update": (c_int, [c_void_p, c_void_p, c_void_p, c_long, c_float, c_void_p]),
    "orv_ema_swap_in": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_int, c_void_p]),
    "orv_scatter_f32_to_bf16": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "orv_sumsq": (c_int, [c_void_p, c_long, c_void_p, c_void_p]),
    "orv_head_transpose": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "orv_attention_bwd": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                  c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_float, c_void_p]),
    "orv_qkv_prep_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                 c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float, c_void_p]),
    "orv_sched_step": (c_int, [c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_float,
                               c_float, c_float, c_float, c_float, c_float, c_float, c_long, c_void_p]),
    "orv_gaussian_sample": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float, c_void_p]),
    "orv_vae_im2col": (c_int, [c_void_p, c_void_p] + [c_int] * 17 + [c_long, c_long, c_void_p]),
    "orv_conv_gemm_bf16": (c_int, [POINTER(Gemm), POINTER(Conv), c_void_p]),
    "orv_vae_groupnorm_scratch": (c_long, [c_int, c_long, c_int, c_int]),
    "orv_vae_groupnorm_stats": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_long, c_int, c_int, c_void_p]),
    "orv_vae_norm_apply": (c_int, [c_void_p] * 7 + [c_int] * 9 + [c_float, c_int, c_int, c_void_p]),
    "orv_vae_blend": (c_int, [c_void_p, c_void_p] + [c_int] * 8 + [c_void_p]),
    "orv_t5_attention_max_seq": (c_int, []),
    "orv_t5_attention_fwd": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "orv_t5_rmsnorm": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_void_p]),
    "orv_geglu": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p]),
    "orv_gs_preprocess": (c_int, [c_void_p] * 6 + [c_int, c_int, c_int, c_float, c_float, c_float] + [c_void_p] * 7),
    "orv_gs_tile_keys": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_long, c_void_p, c_void_p, c_void_p]),
    "orv_gs_tile_ranges": (c_int, [c_void_p, c_long, c_int, c_int, c_void_p, c_void_p]),
    "orv_gs_render": (c_int, [c_void_p, c_void_p, c_long] + [c_void_p] * 5 + [c_int, c_int, c_void_p, c_int, c_int] + [c_void_p] * 5),
    "orv_voxel_grid_size": (c_int, [c_float] * 9 + [c_void_p]),
    "orv_voxel_coors": (c_int, [c_void_p, c_int, c_int] + [c_float] * 9 + [c_void_p, c_void_p, c_void_p]),
    "orv_voxel_segments": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "orv_voxel_scatter": (c_int, [c_void_p] * 6 + [c_int] * 4 + [c_void_p] * 4),
    "orv_voxel_vote": (c_int, [c_void_p] * 6 + [c_int] * 4 + [c_void_p] * 3),
    "orv_occ_project_labels": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "orv_occ_cell_keys": (c_int, [c_void_p] + [c_int] * 4 + [c_void_p] * 3),
    "orv_occ_mark_cells": (c_int, [c_void_p] * 3 + [c_int] + [c_void_p] * 3),
    "orv_occ_write_gaussians": (c_int, [c_void_p] * 4 + [c_int] * 5 + [c_void_p] * 4 + [c_ulong, c_int] + [c_void_p] * 7),
    "orv_cond_prepare": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, POINTER(c_int), c_int, c_int, c_int,
                                 c_void_p, c_int, c_void_p]),
    "orv_frame_metrics_workspace": (c_long, [c_int, c_int, c_int]),
    "orv_frame_metrics": (c_int, [POINTER(Frames), POINTER(Frames), c_int, c_int, c_int, c_double, c_void_p, c_void_p, c_void_p, c_long, c_void_p]),
    "orv_pc_cells": (c_int, [c_void_p, c_int] + [c_float] * 3 + [c_double] + [c_int] * 3 + [c_void_p, c_void_p]),
    "orv_pc_cell_table": (c_int, [c_void_p] * 3 + [c_int, c_int] + [c_void_p] * 3),
    "orv_pc_knn": (c_int, [c_void_p] * 3 + [c_int, c_int] + [c_float] * 3 + [c_double] + [c_int] * 3 + [c_void_p] * 4),
    "orv_pc_knn_brute": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int] + [c_void_p] * 3),
    "orv_pc_outlier_workspace": (c_long, [c_int]),
    "orv_pc_outlier": (c_int, [c_void_p, c_int, c_int, c_double] + [c_void_p] * 4 + [c_long, c_void_p]),
    "orv_pc_normals": (c_int, [c_void_p, c_void_p, c_int, c_int] + [c_double] * 3 + [c_void_p, c_void_p]),
    "orv_pc_orient": (c_int, [c_void_p, c_void_p, c_int] + [c_double] * 3 + [c_void_p, c_void_p]),
    "orv_lm_mask_stats": (c_int, [c_void_p] + [c_int] * 5 + [c_long, c_long, c_float, c_int] + [c_void_p] * 4),
    "orv_lm_compose": (c_int, [c_void_p] + [c_int] * 5 + [c_long, c_long, c_float, c_void_p, c_int] + [c_void_p] * 6),
    "orv_frames_quantize": (c_int, [c_void_p, c_int, c_long, c_void_p] + [c_int] * 5 + [c_void_p, c_long, c_long, c_long, c_int, c_void_p]),
    "orv_frames_handoff": (c_int, [c_void_p, c_long, c_void_p] + [c_int] * 5 + [c_void_p, c_void_p, c_void_p]),
    "orv_step_cache_scratch": (c_long, [c_int, c_int, c_int]),
    "orv_step_cache_probe": (c_int, [c_void_p] * 6 + [c_long, c_void_p] + [c_int] * 4 + [c_void_p]),
    "orv_step_cache_store": (c_int, [c_void_p] * 5 + [c_int] * 4 + [c_void_p]),
    "orv_step_cache_apply": (c_int, [c_void_p, c_void_p] + [c_int] * 4 + [c_void_p]),
    "orv_snapshot_chunk_bytes": (c_int, []),
    "orv_snapshot_scratch_bytes": (c_long, [c_int, c_long]),
    "orv_snapshot": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_long, c_void_p]),
    "orv_checksum": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_long, c_void_p]),
}

_lib = None


def lib() -> ctypes.CDLL:
    """Load liborv_mi355.so once; raise loudly if it has not been built (``python -c 'import __graft_entry__ as g; g.build()'``)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: build it with `make -C orv_amd/csrc` "
                               "(hipcc --offload-arch=gfx950). orv_amd has no CPU/PyTorch fallback.")
        handle = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)  # AttributeError if a declared symbol is not exported
            fn.restype, fn.argtypes = res, args
        _lib = handle
    return _lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = lib().orv_last_error()
        raise RuntimeError(f"liborv_mi355 {what} failed (rc={rc}): {msg.decode() if msg else ''}")
