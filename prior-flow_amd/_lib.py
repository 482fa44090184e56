"""ctypes binding of ``libpriorflow_hip.so`` (C-ABI declared in ``include/priorflow_hip.h``).

``load()`` fails loudly when the HIP library has not been built: there is no CPU or
PyTorch fallback anywhere in the product path.  torch is plumbing only (device memory,
streams): every wrapper passes ``tensor.data_ptr()`` and the current HIP stream.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PRIORFLOW_LIB") or os.path.join(_HERE, "lib", "libpriorflow_hip.so")

EPI_LINEAR, EPI_RELU, EPI_GRU_ZR, EPI_GRU_Q, EPI_TANH_RELU, EPI_RELU_RES, EPI_MASK, EPI_ADD = 0, 1, 2, 3, 4, 5, 6, 7
PREC_F32, PREC_BF16X3, PREC_F16 = 0, 1, 2
ACT_NONE, ACT_RELU, ACT_TANH = 0, 1, 2

_fp = C.c_void_p
_i = C.c_int


def _norm_bwd_blocks(Np: int) -> int:
    """Pixel chunks of pf_norm_bwd's two-stage reduction: >= 16 pixels per partial sum, at most 1024 chunks per image (the
    partial pass runs one thread per chunk and channel; the final pass sums the chunks of one (image, channel) with one wave)."""
    return max(1, min(Np // 16, 1024))


class UnpackJob(C.Structure):
    """Mirror of ``pf_unpack_job`` (include/priorflow_hip.h)."""
    _fields_ = [("dw", _fp), ("db", _fp), ("gw", _fp), ("gb", _fp),
                ("cout", _i), ("cin", _i), ("taps", _i), ("cin_pad", _i), ("o_off", _i), ("scale", C.c_float)]


class PackJob(C.Structure):
    """Mirror of ``pf_pack_job`` (include/priorflow_hip.h)."""
    _fields_ = [("w0", _fp), ("w1", _fp), ("b0", _fp), ("b1", _fp), ("dst_w", _fp), ("dst_b", _fp),
                ("cout0", _i), ("cout1", _i), ("cin", _i), ("kh", _i), ("kw", _i), ("mode", _i), ("cin_rot", _i),
                ("cout_pad", _i), ("cin_pad", _i)]


class ComposeJob(C.Structure):
    """Mirror of ``pf_compose_job`` (include/priorflow_hip.h)."""
    _fields_ = [("f", _fp), ("state_f", _fp), ("g", _fp), ("occ_g", _fp), ("out", _fp), ("state_out", _fp)]


class SplatJob(C.Structure):
    """Mirror of ``pf_splat_job`` (include/priorflow_hip.h)."""
    _fields_ = [("src", _fp), ("flow", _fp), ("metric", _fp), ("mask", _fp), ("cm", _i), ("tau", C.c_float), ("beta", C.c_float)]


class ConvDesc(C.Structure):
    """Mirror of ``pf_conv_desc`` (include/priorflow_hip.h)."""
    _fields_ = [
        ("in0", _fp), ("ld0", _i), ("off0", _i), ("c0", _i),
        ("in1", _fp), ("ld1", _i), ("off1", _i), ("c1", _i),
        ("weight", _fp), ("bias", _fp),
        ("out", _fp), ("ld_out", _i), ("off_out", _i), ("cout", _i),
        ("kh", _i), ("kw", _i),
        ("epilogue", _i), ("scale", C.c_float),
        ("h", _fp), ("ld_h", _i),
        ("z", _fp), ("ld_z", _i),
        ("aux_out", _fp), ("ld_aux", _i),
        ("precision", _i), ("stride", _i),
        ("in_scale", _fp), ("in_shift", _fp), ("in_relu", _i),
        ("stats_out", _fp),
        ("in0_split", _fp), ("lds0", _i),
        ("in1_split", _fp), ("lds1", _i),
        ("out_split", _fp), ("lds_out", _i),
        ("aux_split", _fp), ("lds_aux", _i),
        ("zeros", _fp), ("zeros_bytes", _i),
        ("pre", _fp), ("ld_pre", _i), ("off_pre", _i),
        ("save_gates", _i),
        ("co_groups", _i),
    ]


class CombineConvDesc(C.Structure):
    """Mirror of ``pf_combine_conv_desc`` (include/priorflow_hip.h)."""
    _fields_ = [("own", _fp), ("raw", _fp), ("ld", _i), ("g_back", _fp), ("weight", _fp), ("bias", _fp),
                ("out", _fp), ("ld_out", _i), ("off_out", _i), ("cout", _i), ("out_split", _fp), ("lds_out", _i)]


class DirectDesc(C.Structure):
    """Mirror of ``pf_direct_desc`` (include/priorflow_hip.h)."""
    _fields_ = [("in_", _fp), ("ld_in", _i), ("off_in", _i), ("weight", _fp), ("bias", _fp),
                ("out", _fp), ("ld_out", _i), ("off_out", _i), ("out_split", _fp), ("lds_out", _i)]


_SIGNATURES = {
    "pf_sample_grid": [_fp, _i, _i, C.POINTER(C.c_float), _fp],
    "pf_img_rotate": [_fp, _fp, _fp, _i, _i, _i, _i, _fp],
    "pf_normalise_images": [_fp, _fp, _fp, _fp, _fp, C.c_long, _fp],
    "pf_prepare_images": [_fp, _fp, _fp, _fp, _fp, _i, _i, _i, _fp],
    "pf_prepare_frame": [_fp, _fp, _fp, _i, _i, _i, _fp],
    "pf_forward_interpolate": [_fp, _fp, _fp, C.c_long, _i, _i, _i, _i, _fp],
    "pf_fb_check": [_fp] * 6 + [_i, _i, _i, _i, C.c_float, C.c_float, _fp],
    "pf_flow_compose": [C.POINTER(ComposeJob), _i, _i, _i, _i, _fp],
    "pf_track_points": [_fp, _fp, _fp, _fp, _i, _i, _i, _i, _fp],
    "pf_track_grid": [_fp, _i, _i, _i, _fp],
    "pf_flow_prep": [_fp, _fp, _fp, _i, _i, _fp, _i, _i, _i, _i, _i, _fp],
    "pf_flo_rotate": [_fp, _fp, _fp, _fp, _fp, _i, _i, _fp, _i, _i, _i, _i, _i, _fp],
    "pf_corr_pyramid": [_fp, _fp, _fp, _fp, _fp, _fp, _i, _i, _i, _i, _fp],
    "pf_corr_pyramid_bf16x3": [_fp, _fp, _fp, _fp, _fp, _fp, _i, _i, _i, _i, _fp],
    "pf_split_bf16": [_fp, _fp, C.c_long, _i, _fp],
    "pf_split_f16": [_fp, _i, _fp, _i, C.c_long, _i, _fp],
    "pf_enc_stem": [_fp, _fp, _fp, _fp, _fp, _i, _fp, _i, _i, _i, _fp],
    "pf_debug_dirty_lds": [C.c_uint, _fp],
    "pf_gru_dx_finish": [_fp, _i, _fp, _i, _fp, _i, _fp, _i, _fp, _i, C.c_long, _i, _i, _fp],
    "pf_pack_conv_weights": [_fp, _i, _fp, _i, _fp, _fp, _i, _i, _i, _i, _i, _fp, _fp, _i, _i, _fp],
    "pf_unpack_wgrads": [C.POINTER(UnpackJob), _i, _fp],
    "pf_pack_conv_weights_batch": [C.POINTER(PackJob), _i, _fp],
    "pf_add_relu": [_fp, _fp, _fp, C.c_long, _fp],
    "pf_relu_mask": [_fp, _fp, _fp, C.c_long, _fp],
    "pf_bn_frozen_fwd": [_fp, _fp, _fp, _fp, _fp, C.c_float, _i, _fp, C.c_long, _i, _fp],
    "pf_bn_frozen_bwd": [_fp, _fp, _fp, _fp, _fp, _fp, C.c_float, _i, _fp, _i, _fp, _fp, _fp, _i, C.c_long, _i, _fp],
    "pf_dccl_lookup": [_fp] * 12 + [_i, _i, _i, _i, _fp],
    "pf_dccl_lookup_il": [_fp] * 13 + [_i, _i, _i, _i, _fp],
    "pf_feature_pyramid": [_fp] * 4 + [_i, _i, _i, _i, _fp],
    "pf_dccl_lookup_feat": [_fp] * 15 + [_i, _i, _i, _i, _i, _fp],
    "pf_dccl_combine": [_fp, _fp, _fp, _fp, _i, _i, _i, _i, _i, _fp],
    "pf_warp_gcorr": [_fp, _fp, _fp, _i, _fp, _i, _i, _i, _i, _i, _i, _fp],
    "pf_conf_stem": [_fp, _i, _i, _fp, _fp, _fp, _fp, _fp, _i, _i, _fp, _i, _i, _i, _i, _fp],
    "pf_conf_stem_f16": [_fp, _i, _i, _fp, _fp, _fp, _fp, _fp, _i, _i, _fp, _i, _i, _i, _i, _fp],
    "pf_motion_prep": [_fp] * 9 + [_i, _i, _fp, _i, _i, _fp, _i, _fp, _i, _fp, _i, _i, _i, _i, _i, _fp],
    "pf_motion_prep_f16": [_fp] * 9 + [_i, _i, _fp, _i, _i, _fp, _i, _fp, _i, _fp, _i, _i, _i, _i, _i, _fp],
    "pf_conv2d": [C.POINTER(ConvDesc), _i, _i, _i, _i, _fp],
    "pf_dccl_combine_conv1x1": [C.POINTER(CombineConvDesc), _i, _i, _i, _i, _fp],
    "pf_dccl_combine_conv1x1_f16": [C.POINTER(CombineConvDesc), _i, _i, _i, _i, _fp],
    "pf_conv2d_tile": [C.POINTER(ConvDesc), _i, _i, _i, _i],
    "pf_conv2d_stats_blocks": [C.POINTER(ConvDesc), _i, _i, _i, _i],
    "pf_conv2d_roles": [C.POINTER(ConvDesc), _i, _i, _i, _i],
    "pf_conv2d_direct": [_fp, _i, _i, _i, _fp, _fp, _fp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _fp],
    "pf_conv2d_direct_group": [C.POINTER(DirectDesc), _i, _i, _i, _i, _i, _i, _i, _i, _i, _fp],
    "pf_conv2d_direct_group_f16": [C.POINTER(DirectDesc), _i, _i, _i, _i, _i, _i, _i, _i, _i, _fp],
    "pf_conv2d_small": [_fp, _i, _i, _i, _i, _fp, _fp, _fp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _fp],
    "pf_channel_stats": [_fp, _i, _i, _i, C.c_float, _fp, _fp, _fp, _i, _fp],
    "pf_channel_stats_final": [_fp, _i, _i, _i, _i, C.c_float, _fp, _fp, _fp],
    "pf_norm_act": [_fp, _fp, _fp, _fp, _fp, _fp, _i, _fp, _i, _i, _i, _fp],
    "pf_flow_head_out": [_fp, _i, _i, _fp, _fp, _fp, _fp, _i, _i, _i, _i, _fp],
    "pf_coords_add": [_fp, _fp, _i, _i, _i, _i, _fp],
    "pf_coords_add_to": [_fp, _fp, _i, _fp, _i, _i, _i, _fp],
    "pf_upsample_flow": [_fp, _fp, _i, _fp, _i, _i, _i, _fp],
    "pf_to_channel_last": [_fp, _i, _i, _i, _fp, _i, _i, _i, _i, _i, _fp],
    "pf_space_to_depth2": [_fp, _i, _fp, _i, _i, _i, _i, _fp],
    "pf_conv2d_wgrad_small": [_fp, _i, _i, _i, _i, _fp, _i, _i, _i, _fp, _fp, _i, _i, _i, _i, _i, _i, _fp],
    "pf_conv2d_wgrad_small_ws": [_fp, _i, _i, _i, _i, _fp, _i, _i, _i, _fp, _fp, _i, _i, _i, _i, _i, _i, _fp, C.c_long, _fp],
    "pf_conv2d_wgrad_small_ws_floats": [_i, _i, _i, _i, _i, _i, _i],
    "pf_to_nchw": [_fp, _i, _i, _i, _fp, _i, _i, _fp],
    "pf_warp_gcorr_bwd": [_fp, _fp, _fp, _i, _fp, _i, _i, _fp, _fp, _i, _i, _i, _i, _fp],
    "pf_upsample_flow_bwd": [_fp, _fp, _i, _fp, _fp, _i, _fp, _i, _i, _i, _fp],
    "pf_pyramid_bwd": [_fp, _fp, _fp, _fp, _i, _i, _i, _fp],
    "pf_norm_bwd": [_fp, _fp, _fp, _fp, _i, _i, _fp, _i, _fp, _fp, _i, _i, _i, _fp],
    "pf_gru_q_bwd": [_fp, _i] * 7 + [C.c_long, _i, _fp],
    "pf_gru_zr_bwd": [_fp, _i] * 7 + [C.c_long, _i, _fp],
    "pf_dccl_combine_bwd": [_fp, _i, _fp, _fp, _i, _i, _i, _i, _fp],
    "pf_dccl_lookup_bwd": [_fp, _fp, _fp, _fp, _i, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _i, _i, _i, _i, _fp],
    "pf_conv2d_wgrad": [_fp, _i, _i, _i, _fp, _i, _i, _i, _fp, _i, _i, _i, _fp, _fp, _i, _i, _i, _i, _i, _fp],
    "pf_seq_loss": [_fp, _fp, _fp, _fp, C.c_float, C.c_float, _fp, _fp, _i, _i, _i, _fp],
    "pf_seq_loss_batch": [_fp, _fp, _fp, _fp, _fp, C.c_float, _fp, _fp, _i, _i, _i, _i, _fp],
    "pf_sum_squares": [_fp, C.c_long, _fp, _i, _fp],
    "pf_adamw_step": [_fp, _fp, _fp, _fp, C.c_long, C.c_double, C.c_float, C.c_float, C.c_float, C.c_double, _i,
                      C.c_float, _fp],
    "pf_adamw_step_dev": [_fp, _fp, _fp, _fp, C.c_long, C.c_float, C.c_float, C.c_float, _fp, _fp],
    "pf_flow_metrics": [_fp, _fp, _fp, _fp, _i, _i, _i, _i, _fp],
    "pf_region_sums": [_fp, _fp, _fp, _fp, _i, _fp, _i, _i, _i, _fp],
    "pf_order_stat_scratch_bytes": [_i, C.c_long],
    "pf_order_stat": [_fp, _fp, _fp, C.c_long, _i, C.c_long, C.c_long, _fp],
    "pf_flow_render_scratch_bytes": [_i, _i, _i],
    "pf_flow_render": [_fp, _fp, _fp, C.c_long, _i, _i, _i, _i, C.c_double, _i, _i, _fp],
    "pf_cycle_warp": [_fp, _fp, _fp, _fp, _fp, _i, _i, _i, _i, _fp],
    "pf_masked_mean": [_fp, _fp, _fp, _fp, C.c_long, _i, _i, _fp],
    "pf_augment_scratch_bytes": [_i],
    "pf_augment_360": [_fp] * 9 + [C.c_long, _i, _i, _i, _fp],
    "pf_augment_convert": [_fp, _fp, C.c_long, _i, _fp],
    "pf_viewport_image": [_fp, _fp, C.POINTER(C.c_float), _i, _i, _i, _i, _i, _i, _fp],
    "pf_viewport_flow": [_fp, C.POINTER(C.c_float), _i, _fp, _fp, _i, _i, _i, C.c_float, _fp],
    "pf_cubemap_to_erp": [_fp, _fp, _i, _i, _i, _i, _i, _fp],
    "pf_splat_scratch_bytes": [_i, _i, _i, _i],
    "pf_splat_accumulate": [C.POINTER(SplatJob), _i, _fp, _i, _i, _i, _i, C.c_float, C.c_float, C.c_float, _fp],
    "pf_splat_resolve": [_fp, _fp, _fp, _fp, _fp, C.c_float, C.c_float, _i, _i, _i, _i, _i, C.c_float, _fp],
    "pf_ego_scratch_bytes": [_i, _i, _i],
    "pf_ego_accumulate": [_fp, _fp, _fp, _fp, _i, _i, _i, _i, C.c_float, _i, _fp],
    "pf_ego_solve": [_fp, _fp, _fp, _fp, _i, _i, _i, C.c_float, _fp],
    "pf_ego_track": [_fp, _fp, _fp, _fp, _i, C.c_float, _fp],
    "pf_erp_rotate": [_fp, _fp, _fp, _i, _i, _i, _i, _i, _fp],
    "pf_ego_derotate": [_fp, _fp, _fp, _fp, _fp, _i, _i, _i, _fp],
    "pf_epi_sums_bytes": [_i, _i, _i],
    "pf_epi_accumulate": [_fp, _fp, _fp, _fp, _fp, _i, _i, _i, _i, C.c_float, C.c_float, _i, _fp],
    "pf_epi_solve": [_fp, _fp, _fp, _fp, _fp, _i, _i, _i, _i, C.c_float, C.c_float, _fp],
    "pf_epi_map": [_fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _i, _i, _i, C.c_float, C.c_float, C.c_float, _fp],
    "pf_odo_hist_bytes": [_i, _i, _i, _i],
    "pf_odo_accumulate": [_fp] * 7 + [_i] * 4 + [C.c_float, C.c_float, _i, _fp],
    "pf_odo_solve": [_fp, _fp, _fp, _i, _i, _i, _i, C.c_float, _i, C.c_float, C.c_float, _fp],
    "pf_odo_reverse_pose": [_fp, _fp, _fp, _fp, _i, _fp],
    "pf_odo_track": [_fp] * 10 + [_i, _fp],
    "pf_odo_fuse": [_fp] * 12 + [_i, _i, _i, C.c_float, C.c_float, C.c_float, _fp],
    "pf_reproj_project": [_fp] * 8 + [_i, _i, _i, C.c_float, _fp],
    "pf_zsplat_bytes": [_i, _i, _i, _i],
    "pf_zsplat_front": [_fp] * 6 + [_i, _i, _i, _i, C.c_float, _fp],
    "pf_zsplat_accumulate": [_fp] * 7 + [_i, _i, _i, _i] + [C.c_float] * 5 + [_fp],
    "pf_zsplat_resolve": [_fp] * 6 + [_i, _i, _i, _i] + [C.c_float] * 4 + [_fp],
    "pf_depth_update": [_fp] * 7 + [_i, _i, _i, C.c_float, C.c_float, C.c_float, _fp],
    "pf_selfsup_loss_batch": [_fp] * 8 + [_i] * 5 + [C.c_float] * 7 + [_i, _fp],
    "pf_seg_scratch_bytes": [_i, _i, _i],
    "pf_seg_tables": [_fp, _fp, _i, _i, _fp],
    "pf_seg_label": [_fp, _fp, _fp, _fp, C.c_long, _i, _i, _i, _i, _i, _fp],
    "pf_seg_objects": [_fp] * 5 + [C.c_long] + [_fp] * 6 + [_i] * 5 + [C.c_float, _fp],
    "pf_trk_begin": [_fp, _i, _i, _fp],
    "pf_trk_vote": [_fp] * 8 + [_i] * 4 + [_fp],
    "pf_trk_match": [_fp] * 15 + [_i] * 3 + [C.c_float, _fp],
    "pf_trk_paint": [_fp] * 4 + [_i] * 4 + [_fp],
    "pf_fill_levels": [_i, _i],
    "pf_fill_bytes": [_i, _i, _i, _i],
    "pf_fill_pushpull": [_fp] * 6 + [_i] * 4 + [_fp],
    "pf_fill_stage": [_fp] * 6 + [_i] * 5 + [_fp],
    "pf_fill_prepare": [_fp] * 4 + [_i] * 4 + [_fp],
    "pf_fill_pull_level": [_fp] * 4 + [_i] * 4 + [_fp],
    "pf_fill_push_level": [_fp] * 5 + [_i] * 4 + [_fp],
}
EXPORTS = ["pf_version"] + list(_SIGNATURES)
# entry points whose host emulation is a library of its own (tests/emu/pf_emu_augment.cpp, pf_emu_viewport.cpp,
# pf_emu_splat.cpp, pf_emu_egomotion.cpp, pf_emu_epipolar.cpp, pf_emu_selfsup.cpp, pf_emu_odometry.cpp, pf_emu_reproject.cpp, pf_emu_segments.cpp, pf_emu_tracker.cpp, pf_emu_fill.cpp): a host-only handle (require_cuda=False) may lack them and then refuses the call; the product's handle never may
_OWN_EMULATION = ("pf_augment_scratch_bytes", "pf_augment_360", "pf_augment_convert",
                  "pf_viewport_image", "pf_viewport_flow", "pf_cubemap_to_erp",
                  "pf_splat_scratch_bytes", "pf_splat_accumulate", "pf_splat_resolve",
                  "pf_ego_scratch_bytes", "pf_ego_accumulate", "pf_ego_solve", "pf_ego_track", "pf_erp_rotate", "pf_ego_derotate",
                  "pf_epi_sums_bytes", "pf_epi_accumulate", "pf_epi_solve", "pf_epi_map", "pf_selfsup_loss_batch",
                  "pf_odo_hist_bytes", "pf_odo_accumulate", "pf_odo_solve", "pf_odo_reverse_pose", "pf_odo_track", "pf_odo_fuse",
                  "pf_reproj_project", "pf_zsplat_bytes", "pf_zsplat_front", "pf_zsplat_accumulate", "pf_zsplat_resolve", "pf_depth_update",
                  "pf_seg_scratch_bytes", "pf_seg_tables", "pf_seg_label", "pf_seg_objects",
                  "pf_trk_begin", "pf_trk_vote", "pf_trk_match", "pf_trk_paint",
                  "pf_fill_levels", "pf_fill_bytes", "pf_fill_pushpull", "pf_fill_stage", "pf_fill_prepare", "pf_fill_pull_level",
                  "pf_fill_push_level")
EGO_SUMS, EGO_STATS, EGO_STATE = 12, 5, 8           # PF_EGO_SUMS, PF_EGO_STATS, PF_EGO_STATE
EPI_SUMS, EPI_STATS = 22, 6                         # PF_EPI_SUMS, PF_EPI_STATS
EPI_T, EPI_R = 0, 1                                 # PF_EPI_T / PF_EPI_R
ODO_STATS, ODO_STATE, ODO_FLAGS = 6, 12, 4          # PF_ODO_STATS, PF_ODO_STATE, PF_ODO_FLAGS
SEG_SUMS, SEG_COLS, SEG_MAX_OBJECTS = 10, 6, 4096   # PF_SEG_SUMS, PF_SEG_COLS, PF_SEG_MAX_OBJECTS
TRK_MAX_OBJECTS = 256                               # PF_TRK_MAX_OBJECTS
SS_MAX, SS_SUMS = 32, 4                             # PF_SS_MAX, PF_SS_SUMS
SPLAT_MAX = 4                                       # PF_SPLAT_MAX
AUG_ROW_WORDS = 32                                  # PF_AUG_ROW_WORDS
VIEW_MAX, VIEW_WORDS = 16, 12                       # PF_VIEW_MAX, PF_VIEW_WORDS
VIEW_F32, VIEW_U8 = 0, 1                            # PF_VIEW_F32 / PF_VIEW_U8


class PfError(RuntimeError):
    pass


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _twin(t: Optional[torch.Tensor]):
    """(pointer, chunks per row) of a split twin [rows, chunks, 2, 32] bfloat16 (``engine.split_twin``), or (None, 0)."""
    if t is None:
        return None, 0
    if t.dtype != torch.bfloat16 or t.dim() != 4 or tuple(t.shape[2:]) != (2, 32) or not t.is_contiguous():
        raise PfError("a split twin is a contiguous bfloat16 tensor [rows, chunks, 2, 32]")
    return C.c_void_p(t.data_ptr()), t.shape[1]


def is_f16_map(t: Optional[torch.Tensor]) -> bool:
    """An f16 map (PF_PREC_F16 operand, include/priorflow_hip.h): contiguous float16 [rows, lds * 64] (``engine.f16_map``)."""
    return t is not None and t.dtype == torch.float16


def _opmap(t: Optional[torch.Tensor]):
    """(pointer, 128-byte units per row, is_f16) of a split twin or an f16 map, or (None, 0, False)."""
    if t is None:
        return None, 0, False
    if is_f16_map(t):
        if t.dim() != 2 or t.shape[1] % 64 or not t.is_contiguous():
            raise PfError("an f16 map is a contiguous float16 tensor [rows, lds * 64]")
        return C.c_void_p(t.data_ptr()), t.shape[1] // 64, True
    p, n = _twin(t)
    return p, n, False


def _one_form(*maps) -> bool:
    """True when the given operand buffers are f16 maps, False for split twins; a mix is an error."""
    kinds = {f for p, _, f in maps if p is not None}
    if len(kinds) > 1:
        raise PfError("split twins and f16 maps mixed in one launch")
    return kinds == {True}


def _feat_shapes(levels, B, H8, W8, C, what):
    """alternate_corr: feature level i is channel-last [B*(H8>>i)*(W8>>i), C] (the kernels read that many rows)."""
    for i, t in enumerate(levels):
        want = (B * (H8 >> i) * (W8 >> i), C)
        if t.dim() != 2 or tuple(t.shape) != want:
            raise PfError(f"{what}: feature level {i} is {tuple(t.shape)}, expected {want}")


class PfLib:
    """Typed wrappers; one instance per loaded shared object."""

    def __init__(self, path: str, require_cuda: bool = True, optional: Sequence[str] = ()):
        if not os.path.exists(path):
            raise PfError(
                f"HIP library not found: {path}\n"
                "Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
        if require_cuda:
            # bind against the HIP runtime torch already loaded (same SONAME libamdhip64.so.7)
            torch_hip = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
            if os.path.exists(torch_hip):
                C.CDLL(torch_hip, mode=C.RTLD_GLOBAL)
        self.path = path
        self.require_cuda = require_cuda
        self._dll = C.CDLL(path)
        self._dll.pf_version.restype = C.c_char_p
        self.missing = []
        self.pack_queue = None
        for name, args in _SIGNATURES.items():
            try:
                fn = getattr(self._dll, name)
            except AttributeError:
                if name in optional or (not require_cuda and name in _OWN_EMULATION):
                    self.missing.append(name)
                    continue
                raise PfError(f"{path} does not export {name}")
            fn.argtypes = args
            fn.restype = C.c_long if name.endswith(("_ws_floats", "_scratch_bytes", "_sums_bytes", "_hist_bytes", "_zsplat_bytes", "_fill_bytes")) else _i

    # ---- helpers -----------------------------------------------------------------------------
    def version(self) -> str:
        return self._dll.pf_version().decode()

    def _chk(self, *tensors: Optional[torch.Tensor]):
        for t in tensors:
            if t is None:
                continue
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise PfError(f"expected contiguous fp32 tensor, got {t.dtype} contiguous={t.is_contiguous()}")
            if self.require_cuda and not t.is_cuda:
                raise PfError("the HIP path needs tensors on a cuda (ROCm) device; there is no CPU fallback")

    def _chk_rows(self, *tensors: torch.Tensor):
        """2-D fp32 row views: unit stride along the channels, any leading dimension (column slices are fine)."""
        for t in tensors:
            if t.dtype != torch.float32 or t.dim() != 2 or t.stride(1) != 1:
                raise PfError(f"expected a 2-D fp32 view with unit channel stride, got {t.dtype} {tuple(t.shape)} {t.stride()}")
            if self.require_cuda and not t.is_cuda:
                raise PfError("the HIP path needs tensors on a cuda (ROCm) device; there is no CPU fallback")

    def _stream(self, t: torch.Tensor):
        if t.is_cuda:
            return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)
        return None

    @staticmethod
    def _rc(rc: int, what: str):
        if rc != 0:
            kind = "bad argument/shape" if rc < 0 else "hipError_t"
            raise PfError(f"{what} failed: {kind} {rc}")

    # ---- geometry ----------------------------------------------------------------------------
    def sample_grid(self, grid: torch.Tensor, R: torch.Tensor):
        self._chk(grid)
        H, W = grid.shape[-2:]
        r = (C.c_float * 9)(*[float(v) for v in R.reshape(-1).tolist()])
        self._rc(self._dll.pf_sample_grid(_ptr(grid), H, W, r, self._stream(grid)), "pf_sample_grid")
        return grid

    def img_rotate(self, img, grid, out):
        self._chk(img, grid, out)
        B, Cc, H, W = img.shape
        self._rc(self._dll.pf_img_rotate(_ptr(img), _ptr(grid), _ptr(out), B, Cc, H, W,
                                         self._stream(img)), "pf_img_rotate")
        return out

    def normalise_images(self, image1, image2, f1, f2, c1=None):
        """2 * (image / 255.0) - 1.0 of both images into the encoders' batches (image1 -> f1 and c1, image2 -> f2)."""
        self._chk(image1, image2, f1, f2, c1)
        n = image1.numel()
        if not (image2.numel() == f1.numel() == f2.numel() == n and (c1 is None or c1.numel() == n)):
            raise PfError("normalise_images: operand sizes differ")
        self._rc(self._dll.pf_normalise_images(_ptr(image1), _ptr(image2), _ptr(f1), _ptr(f2), _ptr(c1), n,
                                               self._stream(image1)), "pf_normalise_images")

    def prepare_images(self, image1, image2, grid, img_f, img_c=None):
        """Normalise + rotate into view B in one launch: img_f = [im1 | im2 | im1_B | im2_B], img_c = [im1 | im1_B] (optional)."""
        self._chk(image1, image2, grid, img_f, img_c)
        B, Cc, H, W = image1.shape
        if not (Cc == 3 and image2.shape == image1.shape and tuple(grid.shape) == (2, H, W) and
                tuple(img_f.shape) == (4 * B, 3, H, W) and (img_c is None or tuple(img_c.shape) == (2 * B, 3, H, W))):
            raise PfError("prepare_images: operand shapes do not fit")
        self._rc(self._dll.pf_prepare_images(_ptr(image1), _ptr(image2), _ptr(grid), _ptr(img_f), _ptr(img_c), B, H, W,
                                             self._stream(image1)), "pf_prepare_images")

    def prepare_frame(self, image, grid, out):
        """The input stage of one frame: out = [im | im_B] ([2B,3,H,W]), bit-identical to prepare_images' img_c for image1 = image."""
        self._chk(image, grid, out)
        B, Cc, H, W = image.shape
        if not (Cc == 3 and tuple(grid.shape) == (2, H, W) and tuple(out.shape) == (2 * B, 3, H, W)):
            raise PfError("prepare_frame: operand shapes do not fit")
        self._rc(self._dll.pf_prepare_frame(_ptr(image), _ptr(grid), _ptr(out), B, H, W, self._stream(image)), "pf_prepare_frame")
        return out

    @staticmethod
    def forward_interpolate_scratch_bytes(B: int, h: int, w: int) -> int:
        """Scratch of pf_forward_interpolate: cell counts / offsets, ranks and the sorted points (int32)."""
        return 4 * B * (3 * h * w + 1)

    def forward_interpolate(self, flow, out, scratch, wrap: bool = False):
        """forward_interpolate (core/utils/utils.py:30-58) of planar flows [B,2,h,w] into out; scratch: a device tensor of at least
        forward_interpolate_scratch_bytes(B, h, w) bytes (any dtype; overwritten)."""
        self._chk(flow, out)
        if flow.dim() != 4 or flow.shape[1] != 2 or tuple(out.shape) != tuple(flow.shape):
            raise PfError(f"forward_interpolate: flow {tuple(flow.shape)} / out {tuple(out.shape)}: expected two [B,2,h,w] tensors")
        if not scratch.is_contiguous() or (self.require_cuda and not scratch.is_cuda):
            raise PfError("forward_interpolate: scratch must be a contiguous device tensor")
        B, _, h, w = flow.shape
        self._rc(self._dll.pf_forward_interpolate(_ptr(flow), _ptr(out), _ptr(scratch), scratch.numel() * scratch.element_size(),
                                                  B, h, w, int(bool(wrap)), self._stream(flow)), "pf_forward_interpolate")
        return out

    def flow_prep(self, coords1, flow_out=None, d0=None, d0_off=0, d1=None, d1_off=0):
        self._chk(coords1, flow_out, d0, d1)
        B, _, H, W = coords1.shape
        self._rc(self._dll.pf_flow_prep(
            _ptr(coords1), _ptr(flow_out),
            _ptr(d0), 0 if d0 is None else d0.shape[-1], d0_off,
            _ptr(d1), 0 if d1 is None else d1.shape[-1], d1_off,
            B, H, W, self._stream(coords1)), "pf_flow_prep")

    def flo_rotate(self, flow, g_w2c, g_c2w, out=None, d0=None, d0_off=0, d1=None, d1_off=0):
        self._chk(flow, g_w2c, g_c2w, out, d0, d1)
        B, _, H, W = flow.shape
        self._rc(self._dll.pf_flo_rotate(
            _ptr(flow), _ptr(g_w2c), _ptr(g_c2w), _ptr(out),
            _ptr(d0), 0 if d0 is None else d0.shape[-1], d0_off,
            _ptr(d1), 0 if d1 is None else d1.shape[-1], d1_off,
            B, H, W, self._stream(flow)), "pf_flo_rotate")
        return out

    def conf_stem(self, x, off_in, w1, b1, w2, b2, out, off_out, B, H8, W8, out_split=None):
        """relu(conv3x3 32->16(relu(conv3x3 8->32(x)))) in one launch (core/update.py:193-194); w*: [9*Cin][Cout].
        out_split: optional split twin -- or f16 map (pf_conf_stem_f16) -- of `out` written at the same channel offset (`out` may
        then be None)."""
        self._chk(x, w1, b1, w2, b2, out)
        o = _opmap(out_split)
        fn = "pf_conf_stem_f16" if _one_form(o) else "pf_conf_stem"
        self._rc(getattr(self._dll, fn)(_ptr(x), x.shape[-1], off_in, _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2),
                                        _ptr(out), 0 if out is None else out.shape[-1], off_out, o[0], o[1],
                                        B, H8, W8, self._stream(x)), fn)

    def motion_prep(self, c1a, c1b, g_w2c, g_c2w, f1a, f2a, flow4_a, flow2_b, conf, xa=None, xa_off=0, xb=None, xb_off=0,
                    xa_split=None, xb_split=None):
        """One launch for flow_prep x2 + flo_rotate + warp_gcorr x2 (core/prior_raft.py:171-182), bit-identical to them.
        xa_split / xb_split: optional split twins -- or f16 maps, both alike (pf_motion_prep_f16) -- of the GRU input buffers
        (tails written at xa_off / xb_off)."""
        self._chk(c1a, c1b, g_w2c, g_c2w, f1a, f2a, flow4_a, flow2_b, conf, xa, xb)
        B, _, H, W = c1a.shape
        ma, mb = _opmap(xa_split), _opmap(xb_split)
        (sa, la), (sb, lb) = ma[:2], mb[:2]
        fn = "pf_motion_prep_f16" if _one_form(ma, mb) else "pf_motion_prep"
        self._rc(getattr(self._dll, fn)(
            _ptr(c1a), _ptr(c1b), _ptr(g_w2c), _ptr(g_c2w), _ptr(f1a), _ptr(f2a), _ptr(flow4_a), _ptr(flow2_b),
            _ptr(xa), 0 if xa is None else xa.shape[-1], xa_off, _ptr(xb), 0 if xb is None else xb.shape[-1], xb_off,
            sa, la, sb, lb, _ptr(conf), conf.shape[-1], B, H, W, f1a.shape[-1], self._stream(c1a)), fn)

    # ---- correlation -------------------------------------------------------------------------
    def corr_pyramid(self, f1, f2, levels, B, H8, W8):
        """f1,f2: channel-last [B*N, C]; levels: 4 tensors [B*N, (H8>>i)*(W8>>i)]."""
        self._chk(f1, f2, *levels)
        self._rc(self._dll.pf_corr_pyramid(_ptr(f1), _ptr(f2), *[_ptr(l) for l in levels],
                                           B, H8, W8, f1.shape[-1], self._stream(f1)), "pf_corr_pyramid")

    def split_bf16(self, x, out):
        """x fp32 [rows, C] -> out bfloat16 [rows, C/32, 2, 32] (hi | lo halves per 32-channel chunk)."""
        self._chk(x)
        if out.dtype != torch.bfloat16 or out.numel() != 2 * x.numel() or not out.is_contiguous():
            raise PfError("split_bf16: out must be contiguous bfloat16 with 2x the elements of x")
        self._rc(self._dll.pf_split_bf16(_ptr(x), C.c_void_p(out.data_ptr()), x.shape[0], x.shape[-1],
                                         self._stream(x)), "pf_split_bf16")
        return out

    def split_f16(self, x, out):
        """x fp32 rows [rows, C] (a column slice of wider rows is fine) -> f16 map out float16 [rows, lds * 64], fp16 round to
        nearest even; the map's columns >= C are left as they are (zero)."""
        self._chk_rows(x)
        p, lds, f16 = _opmap(out)
        if not f16 or out.shape[0] != x.shape[0]:
            raise PfError("split_f16: out must be an f16 map with the rows of x")
        self._rc(self._dll.pf_split_f16(_ptr(x), x.stride(0), p, lds, x.shape[0], x.shape[1], self._stream(x)), "pf_split_f16")
        return out

    def pack_conv_weights(self, w0, b0=None, w1=None, b1=None, mode=0, cin_rot=0, cout_pad_to=128):
        """[Cout,Cin,KH,KW] weights (optionally two tensors concatenated on Cout) -> (bf16 split operand of pf_conv2d
        [Cout_pad, KH*KW, Cin_pad/32, 2, 32], bias [Cout_pad]); mode 1: the data-gradient convolution's operand
        (packed Cout = Cin of the forward conv rotated by cin_rot; packed Cin = forward Cout rounded up to 4, then 32)."""
        self._chk(w0, w1, b0, b1)
        cout0, cin, kh, kw = w0.shape
        cout1 = 0 if w1 is None else w1.shape[0]
        oc, ic = (cout0 + cout1, cin) if mode == 0 else (cin, cout0 + cout1)
        op = (oc + cout_pad_to - 1) // cout_pad_to * cout_pad_to
        cp = (ic + 31) // 32 * 32
        dst_w = torch.empty(op, kh * kw, cp // 32, 2, 32, dtype=torch.bfloat16, device=w0.device)
        dst_b = torch.empty(op, dtype=torch.float32, device=w0.device)
        if self.pack_queue is not None:         # inside ``batched_packs()``: launched together when the block ends
            self.pack_queue.append((w0, w1, b0, b1, dst_w, dst_b, cout0, cout1, cin, kh, kw, mode, cin_rot, op, cp))
            return dst_w, dst_b
        self._rc(self._dll.pf_pack_conv_weights(_ptr(w0), cout0, _ptr(w1), cout1, _ptr(b0), _ptr(b1), cin, kh, kw, mode, cin_rot,
                                                C.c_void_p(dst_w.data_ptr()), _ptr(dst_b), op, cp, self._stream(w0)),
                 "pf_pack_conv_weights")
        return dst_w, dst_b

    def batched_packs(self):
        """Context: every ``pack_conv_weights`` inside returns its (still unwritten) destination tensors at once and the packs run
        as ceil(n / 16) launches of pf_pack_conv_weights_batch when the block ends -- before anything may read them."""
        lib = self

        class _Batch:
            def __enter__(self):
                self.outer = lib.pack_queue
                lib.pack_queue = []
                return self

            def __exit__(self, *exc):
                jobs, lib.pack_queue = lib.pack_queue, self.outer
                if exc[0] is None and jobs:
                    arr = (PackJob * len(jobs))()
                    for q, (w0, w1, b0, b1, dw, db, c0, c1, cin, kh, kw, mode, rot, op, cp) in zip(arr, jobs):
                        q.w0, q.w1, q.b0, q.b1 = _ptr(w0), _ptr(w1), _ptr(b0), _ptr(b1)
                        q.dst_w, q.dst_b = C.c_void_p(dw.data_ptr()), _ptr(db)
                        q.cout0, q.cout1, q.cin, q.kh, q.kw, q.mode, q.cin_rot, q.cout_pad, q.cin_pad = c0, c1, cin, kh, kw, mode, rot, op, cp
                    lib._rc(lib._dll.pf_pack_conv_weights_batch(arr, len(jobs), lib._stream(jobs[0][0])), "pf_pack_conv_weights_batch")
                return False
        return _Batch()

    def unpack_wgrads(self, jobs):
        """jobs: [(dw, db, gw, gb | None, cout, cin, taps, cin_pad, o_off, scale)]: gw += scale * unpacked(dw), gb += scale * db."""
        if not jobs:
            return
        arr = (UnpackJob * len(jobs))()
        for q, (dw, db, gw, gb, cout, cin, taps, cin_pad, o_off, scale) in zip(arr, jobs):
            self._chk(dw, db, gw, gb)
            if gw.numel() != cout * cin * taps or (gb is not None and gb.numel() != cout):
                raise PfError("pf_unpack_wgrads: gradient tensor does not match the convolution's shape")
            q.dw, q.db, q.gw, q.gb = _ptr(dw), _ptr(db), _ptr(gw), _ptr(gb)
            q.cout, q.cin, q.taps, q.cin_pad, q.o_off, q.scale = cout, cin, taps, cin_pad, o_off, scale
        self._rc(self._dll.pf_unpack_wgrads(arr, len(jobs), self._stream(jobs[0][0])), "pf_unpack_wgrads")

    def corr_pyramid_bf16x3(self, f1s, f2s, levels, B, H8, W8, Cch):
        self._chk(*levels)
        self._rc(self._dll.pf_corr_pyramid_bf16x3(C.c_void_p(f1s.data_ptr()), C.c_void_p(f2s.data_ptr()),
                                                  *[_ptr(l) for l in levels], B, H8, W8, Cch,
                                                  self._stream(levels[0])), "pf_corr_pyramid_bf16x3")

    def dccl_lookup(self, coords, pyr_own, pyr_other, g_w2c, own_out, raw_out, g_il=None):
        """g_il: optional interleaved copy [H8*W8, 2] of g_w2c (``interleave_grid``): fewer gather instructions."""
        self._chk(coords, g_w2c, own_out, raw_out, g_il, *pyr_own, *pyr_other)
        B, _, H, W = coords.shape
        if g_il is not None and g_il.numel() != g_w2c.numel():
            raise PfError("dccl_lookup: g_il must hold the same grid as g_w2c")
        self._rc(self._dll.pf_dccl_lookup_il(
            _ptr(coords), *[_ptr(p) for p in pyr_own], *[_ptr(p) for p in pyr_other],
            _ptr(g_w2c), _ptr(g_il), _ptr(own_out), _ptr(raw_out), B, H, W, own_out.shape[-1],
            self._stream(coords)), "pf_dccl_lookup_il")

    def feature_pyramid(self, f2, levels, B, H8, W8):
        """alternate_corr: f2 channel-last [B*N, C] -> levels 1-3 [B*N_i, C] (2x2 floor means, ``pf_feature_pyramid``)."""
        self._chk(f2, *levels)
        if len(levels) != 3:
            raise PfError("feature_pyramid: three pooled levels (1-3); level 0 is f2 itself")
        _feat_shapes([f2, *levels], B, H8, W8, f2.shape[-1], "feature_pyramid")
        self._rc(self._dll.pf_feature_pyramid(_ptr(f2), *[_ptr(l) for l in levels], B, H8, W8, f2.shape[-1],
                                              self._stream(f2)), "pf_feature_pyramid")

    def dccl_lookup_feat(self, coords, f1_own, f2_own, f1_oth, f2_oth, g_w2c, own_out, raw_out, path_counts=None):
        """alternate_corr form of ``dccl_lookup``: f2_own / f2_oth are the four feature levels [f2, l1, l2, l3]
        (``feature_pyramid``) instead of the four volume levels.  path_counts: optional int32 [2] the kernel adds its
        (tile, level, view) units on the LDS-tile path [0] and on the per-pixel path [1] to."""
        self._chk(coords, f1_own, f1_oth, g_w2c, own_out, raw_out, *f2_own, *f2_oth)
        if len(f2_own) != 4 or len(f2_oth) != 4:
            raise PfError("dccl_lookup_feat: four feature levels per view")
        B, _, H, W = coords.shape
        C = f1_own.shape[-1]
        for f in (f2_own, f2_oth):
            _feat_shapes(f, B, H, W, C, "dccl_lookup_feat")
        for t in (f1_own, f1_oth, own_out, raw_out):
            if t.dim() != 2 or t.shape[0] != B * H * W:
                raise PfError(f"dccl_lookup_feat: rows of {tuple(t.shape)} do not match B*H8*W8 = {B * H * W}")
        if f1_oth.shape[-1] != C or g_w2c.numel() != 2 * H * W:
            raise PfError("dccl_lookup_feat: f1_oth / g_w2c do not fit coords and f1_own")
        if path_counts is not None and (path_counts.dtype != torch.int32 or path_counts.numel() < 2
                                        or not path_counts.is_contiguous()):
            raise PfError("dccl_lookup_feat: path_counts is a contiguous int32 tensor of 2 elements")
        self._rc(self._dll.pf_dccl_lookup_feat(
            _ptr(coords), _ptr(f1_own), *[_ptr(p) for p in f2_own], _ptr(f1_oth), *[_ptr(p) for p in f2_oth],
            _ptr(g_w2c), _ptr(own_out), _ptr(raw_out), _ptr(path_counts), B, H, W, C, own_out.shape[-1],
            self._stream(coords)), "pf_dccl_lookup_feat")

    def dccl_combine(self, own, raw, g_back, out, B, H8, W8):
        self._chk(own, raw, g_back, out)
        self._rc(self._dll.pf_dccl_combine(_ptr(own), _ptr(raw), _ptr(g_back), _ptr(out), B, H8, W8,
                                           own.shape[-1], out.shape[-1], self._stream(own)),
                 "pf_dccl_combine")

    def dccl_combine_conv1x1(self, items, B, H8, W8):
        """items: 1 or 2 tuples (own, raw, g_back, conv, out, off_out[, out_split]) with `conv` a packed bf16x3 1x1 324->256
        engine.Conv: out[.., off_out:off_out+256] = relu(conv(own + rotate_back(raw))) without materialising the sum.
        out_split: optional split twin -- or f16 map, in every item alike (pf_dccl_combine_conv1x1_f16) -- of `out` (`out` may
        then be None)."""
        arr = (CombineConvDesc * len(items))()
        keep = []
        maps = [_opmap(item[6] if len(item) > 6 else None) for item in items]
        fn = "pf_dccl_combine_conv1x1_f16" if _one_form(*maps) else "pf_dccl_combine_conv1x1"
        for d, item, m in zip(arr, items, maps):
            own, raw, g_back, conv, out, off_out = item[:6]
            out_split = item[6] if len(item) > 6 else None
            d.out_split, d.lds_out = m[:2]
            self._chk(own, raw, g_back, conv.b, out)
            if conv.precision != PREC_BF16X3 or (conv.kh, conv.kw, conv.cin, conv.cout) != (1, 1, 324, 256):
                raise PfError("dccl_combine_conv1x1 needs the bf16x3 packing of a 1x1 324(352)->256 convolution")
            d.own, d.raw, d.ld, d.g_back = own.data_ptr(), raw.data_ptr(), own.shape[-1], g_back.data_ptr()
            d.weight, d.bias = conv.w.data_ptr(), conv.b.data_ptr()
            d.out = out.data_ptr() if out is not None else None
            d.ld_out, d.off_out, d.cout = (out.shape[-1] if out is not None else 0), off_out, conv.cout
            keep.append((own, raw, g_back, conv, out, out_split))
        self._rc(getattr(self._dll, fn)(arr, len(items), B, H8, W8, self._stream(items[0][0])), fn)

    def warp_gcorr(self, f1, f2, coords, add_grid, dst, dst_off):
        self._chk(f1, f2, coords, dst)
        B, _, H, W = coords.shape
        self._rc(self._dll.pf_warp_gcorr(_ptr(f1), _ptr(f2), _ptr(coords), int(add_grid), _ptr(dst),
                                         dst.shape[-1], dst_off, B, H, W, f1.shape[-1],
                                         self._stream(f1)), "pf_warp_gcorr")

    # ---- update blocks -----------------------------------------------------------------------
    def conv2d(self, descs: Sequence[ConvDesc], B, H8, W8, like: torch.Tensor):
        arr = (ConvDesc * len(descs))(*descs)
        self._rc(self._dll.pf_conv2d(arr, len(descs), B, H8, W8, self._stream(like)), "pf_conv2d")

    def conv2d_tile(self, descs: Sequence[ConvDesc], B, H8, W8) -> int:
        arr = (ConvDesc * len(descs))(*descs)
        rc = self._dll.pf_conv2d_tile(arr, len(descs), B, H8, W8)
        if rc < 0:
            self._rc(rc, "pf_conv2d_tile")
        return rc

    def conv2d_stats_blocks(self, descs: Sequence[ConvDesc], B, H8, W8) -> int:
        """fp64 partial blocks per image a launch with ``stats_out`` writes (0: the launch cannot fuse the statistics)."""
        arr = (ConvDesc * len(descs))(*descs)
        rc = self._dll.pf_conv2d_stats_blocks(arr, len(descs), B, H8, W8)
        if rc < 0:
            self._rc(rc, "pf_conv2d_stats_blocks")
        return rc

    def conv2d_roles(self, descs: Sequence[ConvDesc], B, H8, W8) -> int:
        arr = (ConvDesc * len(descs))(*descs)
        rc = self._dll.pf_conv2d_roles(arr, len(descs), B, H8, W8)
        if rc < 0:
            self._rc(rc, "pf_conv2d_roles")
        return rc

    def conv2d_direct(self, x, off_in, cin, weight, bias, out, off_out, cout, kh, kw, relu, B, H8, W8):
        self._chk(x, weight, bias, out)
        self._rc(self._dll.pf_conv2d_direct(_ptr(x), x.shape[-1], off_in, cin, _ptr(weight), _ptr(bias),
                                            _ptr(out), out.shape[-1], off_out, cout, kh, kw, int(relu),
                                            B, H8, W8, self._stream(x)), "pf_conv2d_direct")

    def conv2d_direct_group(self, problems, cin, cout, kh, kw, relu, B, H8, W8):
        """problems: 1..4 tuples (x, off_in, weight, bias, out, off_out[, out_split]) of one shape -> one launch.
        out_split: optional split twin -- or f16 map, in every problem alike (pf_conv2d_direct_group_f16) -- of `out` (7x7 2 -> C
        stems; `out` may then be None)."""
        arr = (DirectDesc * len(problems))()
        maps = [_opmap(item[6] if len(item) > 6 else None) for item in problems]
        fn = "pf_conv2d_direct_group_f16" if _one_form(*maps) else "pf_conv2d_direct_group"
        for d, item, m in zip(arr, problems, maps):
            x, off_in, weight, bias, out, off_out = item[:6]
            self._chk(x, weight, bias, out)
            d.in_, d.ld_in, d.off_in = _ptr(x), x.shape[-1], off_in
            d.weight, d.bias = _ptr(weight), _ptr(bias)
            d.out, d.ld_out, d.off_out = _ptr(out), (out.shape[-1] if out is not None else 0), off_out
            d.out_split, d.lds_out = m[:2]
        self._rc(getattr(self._dll, fn)(arr, len(problems), cin, cout, kh, kw, int(relu), B, H8, W8,
                                        self._stream(problems[0][0])), fn)

    def conv2d_small(self, x, nchw, off_in, cin, weight, bias, out, off_out, cout, kh, kw, stride, relu,
                     B, Hout, Wout):
        self._chk(x, weight, bias, out)
        self._rc(self._dll.pf_conv2d_small(_ptr(x), int(nchw), 0 if nchw else x.shape[-1], off_in, cin,
                                           _ptr(weight), _ptr(bias), _ptr(out), out.shape[-1], off_out, cout,
                                           kh, kw, stride, int(relu), B, Hout, Wout, self._stream(x)),
                 "pf_conv2d_small")

    def enc_stem(self, images, weight, bias, out=None, out_split=None, relu=False, stats=None):
        """The encoders' 7x7 / 2 stem from NCHW images [Bn,3,H,W] (pf_enc_stem); weight from engine.pack_stem7x7."""
        self._chk(images, bias, out)
        Bn, Cc, H, W = images.shape
        if Cc != 3 or weight.dtype != torch.bfloat16 or weight.numel() != 64 * 352 or not weight.is_contiguous():
            raise PfError("enc_stem: images must be [Bn,3,H,W] and weight the 64 x 704-byte pack of engine.pack_stem7x7")
        sp, _ = _twin(out_split)
        self._rc(self._dll.pf_enc_stem(_ptr(images), C.c_void_p(weight.data_ptr()), _ptr(bias), _ptr(out), sp, int(relu),
                                       None if stats is None else C.c_void_p(stats.data_ptr()), Bn, H, W, self._stream(images)),
                 "pf_enc_stem")

    def debug_dirty_lds(self, pattern: int = 0x7fc00000, like=None):
        """Test support: every CU's whole LDS is filled with `pattern` (default: a NaN) on the current stream (pf_debug_dirty_lds)."""
        stream = self._stream(like) if like is not None else C.c_void_p(torch.cuda.current_stream().cuda_stream)
        self._rc(self._dll.pf_debug_dirty_lds(C.c_uint(pattern & 0xffffffff), stream), "pf_debug_dirty_lds")

    def conv2d_wgrad_small(self, x, nchw, off_in, cin, dy, off_dy, cout, dw, db, kh, kw, stride, B, Hout, Wout, one_stage=False):
        """dw [Cout,Cin,KH,KW] (+= ), db [Cout] (+= or None) of a small-Cin convolution; x NCHW planes or channel-last.
        one_stage: the pf_conv2d_wgrad_small entry (one atomic per weight per workgroup, no workspace) instead of the
        two-stage pf_conv2d_wgrad_small_ws the product uses."""
        self._chk(x, dy, dw, db)
        if one_stage:
            self._rc(self._dll.pf_conv2d_wgrad_small(_ptr(x), int(nchw), 0 if nchw else x.shape[-1], off_in, cin,
                                                     _ptr(dy), dy.shape[-1], off_dy, cout, _ptr(dw), _ptr(db),
                                                     kh, kw, stride, B, Hout, Wout, self._stream(x)),
                     "pf_conv2d_wgrad_small")
            return
        n = int(self._dll.pf_conv2d_wgrad_small_ws_floats(cin, cout, kh, kw, B, Hout, Wout))
        ws = torch.empty(max(n, 1), dtype=torch.float32, device=x.device)      # per call: two streams may run stems side by side
        self._rc(self._dll.pf_conv2d_wgrad_small_ws(_ptr(x), int(nchw), 0 if nchw else x.shape[-1], off_in, cin,
                                                    _ptr(dy), dy.shape[-1], off_dy, cout, _ptr(dw), _ptr(db),
                                                    kh, kw, stride, B, Hout, Wout, _ptr(ws), n, self._stream(x)),
                 "pf_conv2d_wgrad_small_ws")

    def channel_stats(self, y, B, Np, Cch, scale, shift, partials, nblk, eps=1e-5):
        self._chk(y, scale, shift)
        if partials.dtype != torch.float64 or partials.numel() < B * nblk * Cch * 2:
            raise PfError("channel_stats: partials must be float64 with >= B*nblk*C*2 elements")
        self._rc(self._dll.pf_channel_stats(_ptr(y), B, Np, Cch, eps, _ptr(scale), _ptr(shift),
                                            C.c_void_p(partials.data_ptr()), nblk, self._stream(y)),
                 "pf_channel_stats")

    def channel_stats_final(self, partials, B, Np, Cch, nblk, scale, shift, eps=1e-5):
        """Second stage only: partials [B][nblk][C][2] float64 written by a conv launched with stats_out."""
        self._chk(scale, shift)
        if partials.dtype != torch.float64 or partials.numel() < B * nblk * Cch * 2:
            raise PfError("channel_stats_final: partials must be float64 with >= B*nblk*C*2 elements")
        self._rc(self._dll.pf_channel_stats_final(C.c_void_p(partials.data_ptr()), B, Np, Cch, nblk, eps,
                                                  _ptr(scale), _ptr(shift), self._stream(scale)),
                 "pf_channel_stats_final")

    def norm_act(self, y, s, t, out, B, Np, Cc, res=None, rs=None, rt=None, res_relu=False):
        self._chk(y, s, t, out, res, rs, rt)
        self._rc(self._dll.pf_norm_act(_ptr(y), _ptr(s), _ptr(t), _ptr(res), _ptr(rs), _ptr(rt), int(res_relu), _ptr(out),
                                       B, Np, Cc, self._stream(y)), "pf_norm_act")

    def flow_head_out(self, x, Cch, weight, bias, coords1, delta=None):
        self._chk(x, weight, bias, coords1, delta)
        B, _, H, W = coords1.shape
        self._rc(self._dll.pf_flow_head_out(_ptr(x), x.shape[-1], Cch, _ptr(weight), _ptr(bias), _ptr(coords1),
                                            _ptr(delta), 0 if delta is None else delta.shape[-1], B, H, W,
                                            self._stream(x)), "pf_flow_head_out")

    def coords_add(self, coords1, delta, src=None):
        """coords1 += delta, or (src given) coords1 = src + delta."""
        self._chk(coords1, delta, src)
        B, _, H, W = coords1.shape
        if src is None:
            self._rc(self._dll.pf_coords_add(_ptr(coords1), _ptr(delta), delta.shape[-1], B, H, W,
                                             self._stream(coords1)), "pf_coords_add")
        else:
            if src.shape != coords1.shape:
                raise PfError("pf_coords_add_to: src and dst differ in shape")
            self._rc(self._dll.pf_coords_add_to(_ptr(src), _ptr(delta), delta.shape[-1], _ptr(coords1), B, H, W,
                                                self._stream(coords1)), "pf_coords_add_to")

    def upsample_flow(self, coords1, mask, out):
        self._chk(coords1, mask, out)
        B, _, H, W = coords1.shape
        self._rc(self._dll.pf_upsample_flow(_ptr(coords1), _ptr(mask), mask.shape[-1], _ptr(out),
                                            B, H, W, self._stream(coords1)), "pf_upsample_flow")
        return out

    # ---- layout ------------------------------------------------------------------------------
    def to_channel_last(self, x, c_begin, c, out, off_out, act=ACT_NONE):
        """x: NCHW [B,Ct,H,W] -> out rows [B*H*W, ld] columns [off_out, off_out+c)."""
        self._chk(x, out)
        B, Ct = x.shape[:2]
        N = x.shape[2] * x.shape[3]
        self._rc(self._dll.pf_to_channel_last(_ptr(x), Ct, c_begin, c, _ptr(out), out.shape[-1], off_out,
                                              act, B, N, self._stream(x)), "pf_to_channel_last")
        return out

    def space_to_depth2(self, x, out):
        """x: NCHW [B,C,H,W] -> out rows [B*(H/2)*(W/2), ld], columns (py*2+px)*C + c."""
        self._chk(x, out)
        B, C, H, W = x.shape
        self._rc(self._dll.pf_space_to_depth2(_ptr(x), C, _ptr(out), out.shape[-1], B, H, W, self._stream(x)),
                 "pf_space_to_depth2")
        return out

    # ---- training-step pieces ---------------------------------------------------------------
    def warp_gcorr_bwd(self, f1, f2, coords, add_grid, d_flaw, off_d, d_f1, d_f2):
        """d_flaw: channel-last rows with the 4 group gradients at column off_d; d_f1 / d_f2 accumulated."""
        self._chk(f1, f2, coords, d_flaw, d_f1, d_f2)
        B, _, H, W = coords.shape
        self._rc(self._dll.pf_warp_gcorr_bwd(_ptr(f1), _ptr(f2), _ptr(coords), int(add_grid), _ptr(d_flaw),
                                             d_flaw.shape[-1], off_d, _ptr(d_f1), _ptr(d_f2), B, H, W, f1.shape[-1],
                                             self._stream(f1)), "pf_warp_gcorr_bwd")

    def upsample_flow_bwd(self, coords1, mask, g, d_mask, d_flow):
        """g [B,2,8H,8W] -> d_mask [B*N, >=576] (written), d_flow [B,2,H,W] (accumulated)."""
        self._chk(coords1, mask, g, d_mask, d_flow)
        B, _, H, W = coords1.shape
        self._rc(self._dll.pf_upsample_flow_bwd(_ptr(coords1), _ptr(mask), mask.shape[-1], _ptr(g), _ptr(d_mask),
                                                d_mask.shape[-1], _ptr(d_flow), B, H, W, self._stream(g)),
                 "pf_upsample_flow_bwd")

    def pyramid_bwd(self, g_levels, B, H8, W8):
        """g_levels: 4 level gradients [B*N, H_i*W_i]; level 0 becomes the dense volume gradient (in place)."""
        self._chk(*g_levels)
        self._rc(self._dll.pf_pyramid_bwd(*[_ptr(t) for t in g_levels], B, H8, W8, self._stream(g_levels[0])),
                 "pf_pyramid_bwd")
        return g_levels[0]

    def norm_bwd(self, dy, x, scale, shift, relu, instance, dx, B, Np, Cc, nblk=None):
        """Backward of act(x*scale+shift) (InstanceNorm when `instance`, else fixed statistics); rows [B*Np, C]."""
        self._chk(dy, x, scale, shift, dx)
        part = coef = None
        if instance:
            nblk = nblk or _norm_bwd_blocks(Np)
            part = torch.empty(B * nblk * Cc * 2, dtype=torch.float64, device=dy.device)
            coef = torch.empty(B * Cc * 2, dtype=torch.float32, device=dy.device)
        self._rc(self._dll.pf_norm_bwd(_ptr(dy), _ptr(x), _ptr(scale), _ptr(shift), int(relu), int(instance),
                                       _ptr(part), nblk or 0, _ptr(coef), _ptr(dx), B, Np, Cc, self._stream(dy)),
                 "pf_norm_bwd")

    def norm_bwd_sums(self, dy, x, scale, shift, B, Np, Cc, nblk=None):
        """Per-(image, channel) means of g and g * (x*scale+shift) over the Np pixels: [B, C, 2] (the reduction stage of
        pf_norm_bwd's InstanceNorm branch; its dx is written to a scratch buffer and discarded)."""
        self._chk(dy, x, scale, shift)
        nblk = nblk or _norm_bwd_blocks(Np)
        part = torch.empty(B * nblk * Cc * 2, dtype=torch.float64, device=dy.device)
        coef = torch.empty(B * Cc * 2, dtype=torch.float32, device=dy.device)
        scratch = torch.empty_like(x)
        self._rc(self._dll.pf_norm_bwd(_ptr(dy), _ptr(x), _ptr(scale), _ptr(shift), 0, 1, _ptr(part), nblk, _ptr(coef),
                                       _ptr(scratch), B, Np, Cc, self._stream(dy)), "pf_norm_bwd")
        return coef.view(B, Cc, 2)

    def add_relu(self, x, y, out):
        """out = relu(x + y), same-shape contiguous fp32 tensors."""
        self._chk(x, y, out)
        if x.numel() != y.numel() or x.numel() != out.numel():
            raise PfError("add_relu: shapes differ")
        self._rc(self._dll.pf_add_relu(_ptr(x), _ptr(y), _ptr(out), x.numel(), self._stream(x)), "pf_add_relu")
        return out

    def relu_mask(self, g, fwd_out, dx):
        """dx = fwd_out > 0 ? g : 0 (the backward of a ReLU from its output)."""
        self._chk(g, fwd_out, dx)
        if g.numel() != fwd_out.numel() or g.numel() != dx.numel():
            raise PfError("relu_mask: shapes differ")
        self._rc(self._dll.pf_relu_mask(_ptr(g), _ptr(fwd_out), _ptr(dx), g.numel(), self._stream(g)), "pf_relu_mask")
        return dx

    def bn_frozen_fwd(self, x, gamma, beta, mean, var, eps, relu, out):
        """out = [relu](frozen BatchNorm(x)) on channel-last rows [rows, C]."""
        self._chk(x, gamma, beta, mean, var, out)
        rows, Cc = x.shape
        self._rc(self._dll.pf_bn_frozen_fwd(_ptr(x), _ptr(gamma), _ptr(beta), _ptr(mean), _ptr(var), float(eps), int(bool(relu)),
                                            _ptr(out), rows, Cc, self._stream(x)), "pf_bn_frozen_fwd")
        return out

    def bn_frozen_bwd(self, dy, x, gamma, beta, mean, var, eps, relu, dx, dgamma, dbeta, accumulate):
        self._chk(dy, x, gamma, beta, mean, var, dx, dgamma, dbeta)
        rows, Cc = x.shape
        nblk = int(max(1, min(rows // 16, 2048)))        # >= 16 rows per partial sum; 2048 x C threads fill the chip at the encoder sizes
        part = torch.empty(nblk * Cc * 2, dtype=torch.float64, device=dy.device)
        self._rc(self._dll.pf_bn_frozen_bwd(_ptr(dy), _ptr(x), _ptr(gamma), _ptr(beta), _ptr(mean), _ptr(var), float(eps),
                                            int(bool(relu)), C.c_void_p(part.data_ptr()), nblk, _ptr(dx), _ptr(dgamma), _ptr(dbeta),
                                            int(bool(accumulate)), rows, Cc, self._stream(dy)), "pf_bn_frozen_bwd")
        return dx

    def gru_q_bwd(self, dh_new, z, q, h, dq_pre, dz, dh):
        """Stage Q of the GRU gate backward; every argument a channel-last [rows, >=C] view (C = dh_new.shape[-1])."""
        self._chk_rows(dh_new, z, q, h, dq_pre, dz, dh)
        rows, Cc = dh_new.shape
        args = []
        for t in (dh_new, z, q, h, dq_pre, dz, dh):
            args += [_ptr(t), t.stride(0)]
        self._rc(self._dll.pf_gru_q_bwd(*args, rows, Cc, self._stream(dh_new)), "pf_gru_q_bwd")

    def gru_zr_bwd(self, dz, d_rh, z, r, h, dzr_pre, dh):
        """Stage ZR; dzr_pre is [rows, >=2C] (z half | r half), dh is accumulated."""
        self._chk_rows(dz, d_rh, z, r, h, dzr_pre, dh)
        rows, Cc = dz.shape
        args = []
        for t in (dz, d_rh, z, r, h, dzr_pre, dh):
            args += [_ptr(t), t.stride(0)]
        self._rc(self._dll.pf_gru_zr_bwd(*args, rows, Cc, self._stream(dz)), "pf_gru_zr_bwd")

    def gru_dx_finish(self, f1, f2, x, d_inp, d_out, Cc, wout):
        """d_inp += (f1 + f2)[:, :C]; d_out[:, :wout] = (f1 + f2)[:, C:C+wout] masked by x[:, C:C+wout] > 0 (row views)."""
        self._chk_rows(f1, f2, x, d_inp, d_out)
        self._rc(self._dll.pf_gru_dx_finish(_ptr(f1), f1.stride(0), _ptr(f2), f2.stride(0), _ptr(x), x.stride(0),
                                            _ptr(d_inp), d_inp.stride(0), _ptr(d_out), d_out.stride(0), f1.shape[0], Cc, wout,
                                            self._stream(f1)), "pf_gru_dx_finish")

    def dccl_combine_bwd(self, d_corr, g_back, d_raw, B, H8, W8):
        self._chk(d_corr, g_back, d_raw)
        self._rc(self._dll.pf_dccl_combine_bwd(_ptr(d_corr), d_corr.shape[-1], _ptr(g_back), _ptr(d_raw), d_raw.shape[-1],
                                               B, H8, W8, self._stream(d_corr)), "pf_dccl_combine_bwd")

    def dccl_lookup_bwd(self, coords, g_w2c, d_own, d_raw, g_own, g_other, clear_raw=False):
        """g_own / g_other: lists of 4 level gradients [B*N, H_i*W_i], accumulated into.  clear_raw: d_raw is left all zero."""
        self._chk(coords, g_w2c, d_own, d_raw, *g_own, *g_other)
        B, _, H, W = coords.shape
        if d_raw.shape[-1] != d_own.shape[-1]:
            raise PfError("pf_dccl_lookup_bwd: d_own and d_raw must share their row length")
        self._rc(self._dll.pf_dccl_lookup_bwd(_ptr(coords), _ptr(g_w2c), _ptr(d_own), _ptr(d_raw), d_own.shape[-1],
                                              *[_ptr(t) for t in g_own], *[_ptr(t) for t in g_other], B, H, W, int(clear_raw),
                                              self._stream(coords)), "pf_dccl_lookup_bwd")

    def conv2d_wgrad(self, x0, off0, c0, dy, off_dy, cout, dw, db, kh, kw, B, H8, W8, x1=None, off1=0, c1=0):
        """dw [Cout_pad128, kh*kw, Cin_pad32] and db [Cout_pad128] (or None) are accumulated into."""
        self._chk(x0, x1, dy, dw, db)
        cin_pad = (c0 + c1 + 31) // 32 * 32
        if dw.shape[-1] != cin_pad or dw.shape[-2] != kh * kw or dw.shape[0] < cout:
            raise PfError(f"conv2d_wgrad: dw must be [>= {cout}, {kh * kw}, {cin_pad}], got {tuple(dw.shape)}")
        self._rc(self._dll.pf_conv2d_wgrad(_ptr(x0), x0.shape[-1], off0, c0, _ptr(x1), 0 if x1 is None else x1.shape[-1],
                                           off1, c1, _ptr(dy), dy.shape[-1], off_dy, cout, _ptr(dw), _ptr(db),
                                           kh, kw, B, H8, W8, self._stream(x0)), "pf_conv2d_wgrad")

    def seq_loss(self, pred, gt, valid, weight, i_weight, max_flow, grad, partials):
        """pred, gt [B,2,H,W]; valid [B,H,W]; weight [H*W]; grad [B,2,H,W] or None; partials float64 [B,nblk,6]."""
        self._chk(pred, gt, valid, weight, grad)
        B = pred.shape[0]
        N = pred.shape[2] * pred.shape[3]
        if partials.dtype != torch.float64 or partials.dim() != 3 or partials.shape[0] != B or partials.shape[2] != 6:
            raise PfError("seq_loss: partials must be float64 [B, nblk, 6]")
        if gt.shape != pred.shape or valid.numel() != B * N or weight.numel() != N:
            raise PfError("seq_loss: shape mismatch")
        self._rc(self._dll.pf_seq_loss(_ptr(pred), _ptr(gt), _ptr(valid), _ptr(weight), i_weight, max_flow, _ptr(grad),
                                       C.c_void_p(partials.data_ptr()), partials.shape[1], B, N, self._stream(pred)),
                 "pf_seq_loss")

    def seq_loss_batch(self, preds, gt, valid, weight, i_weights, max_flow, grads, partials):
        """The n <= 32 terms seq_loss(preds[i], ..., i_weights[i], grads[i], partials[i]) in one launch; grads: list of tensors or
        None; partials float64 [n, B, nblk, 6]."""
        n = len(preds)
        self._chk(gt, valid, weight, *preds, *(grads or ()))
        B = gt.shape[0]
        N = gt.shape[2] * gt.shape[3]
        if partials.dtype != torch.float64 or tuple(partials.shape[:2]) != (n, B) or partials.shape[3] != 6 or not partials.is_contiguous():
            raise PfError("seq_loss_batch: partials must be contiguous float64 [n, B, nblk, 6]")
        if any(p.shape != gt.shape or not p.is_contiguous() or p.dtype != torch.float32 for p in preds) or valid.numel() != B * N \
                or weight.numel() != N or (grads is not None and (len(grads) != n or any(g.shape != gt.shape for g in grads))):
            raise PfError("seq_loss_batch: shape mismatch")
        pa = (C.c_void_p * n)(*[p.data_ptr() for p in preds])
        ga = (C.c_void_p * n)(*[g.data_ptr() for g in grads]) if grads is not None else None
        wa = (C.c_float * n)(*[float(w) for w in i_weights])
        self._rc(self._dll.pf_seq_loss_batch(pa, _ptr(gt), _ptr(valid), _ptr(weight), wa, max_flow, ga,
                                             C.c_void_p(partials.data_ptr()), partials.shape[2], n, B, N, self._stream(gt)),
                 "pf_seq_loss_batch")

    def sum_squares(self, x, partials):
        self._chk(x)
        if partials.dtype != torch.float64 or not partials.is_contiguous():
            raise PfError("sum_squares: partials must be contiguous float64")
        self._rc(self._dll.pf_sum_squares(_ptr(x), x.numel(), C.c_void_p(partials.data_ptr()), partials.numel(),
                                          self._stream(x)), "pf_sum_squares")

    def adamw_step(self, p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0):
        self._chk(p, g, m, v)
        if not (p.numel() == g.numel() == m.numel() == v.numel()):
            raise PfError("adamw_step: buffers must have the same size")
        self._rc(self._dll.pf_adamw_step(_ptr(p), _ptr(g), _ptr(m), _ptr(v), p.numel(), lr, beta1, beta2, eps,
                                         weight_decay, step, grad_scale, self._stream(p)), "pf_adamw_step")

    def adamw_step_dev(self, p, g, m, v, beta1, beta2, eps, hyper):
        """pf_adamw_step with {decay, step_size, sqrt_bc2, grad_scale} read from the device tensor `hyper` (4 floats)."""
        self._chk(p, g, m, v, hyper)
        if not (p.numel() == g.numel() == m.numel() == v.numel()) or hyper.numel() < 4:
            raise PfError("adamw_step_dev: buffers must have the same size and hyper 4 floats")
        self._rc(self._dll.pf_adamw_step_dev(_ptr(p), _ptr(g), _ptr(m), _ptr(v), p.numel(), beta1, beta2, eps, _ptr(hyper),
                                             self._stream(p)), "pf_adamw_step_dev")

    def flow_metrics(self, pred, gt, epe=None, sd=None, cosine=False):
        """pred, gt: NCHW [B,2,H,W]; epe / sd: [B,H,W] outputs (either optional); cosine: the 'Cosine' form of the distance."""
        self._chk(pred, gt, epe, sd)
        B, _, H, W = pred.shape
        if gt.shape != pred.shape:
            raise PfError("flow_metrics: pred and gt must have the same shape")
        self._rc(self._dll.pf_flow_metrics(_ptr(pred), _ptr(gt), _ptr(epe), _ptr(sd), int(cosine), B, H, W, self._stream(pred)),
                 "pf_flow_metrics")

    FB_METRICS = {"plane": 0, "sphere": 1}          # PF_FB_PLANE / PF_FB_SPHERE

    def fb_check(self, flow_fw, flow_bw, occ_fw, occ_bw, res_fw, res_bw, metric="sphere", alpha=0.01, beta=0.5):
        """Forward-backward consistency of two opposite flows [B,2,H,W], both directions in one launch: occ_* uint8 [B,H,W]
        (1 = the round trip fails), res_* fp32 [B,2,H,W] (the round trip, pixels).  metric: "sphere" | "plane"."""
        self._chk(flow_fw, flow_bw, res_fw, res_bw)
        if metric not in self.FB_METRICS:
            raise PfError(f"fb_check: metric {metric!r}, expected 'sphere' or 'plane'")
        if flow_fw.dim() != 4 or flow_fw.shape[1] != 2 or any(t.shape != flow_fw.shape for t in (flow_bw, res_fw, res_bw)):
            raise PfError("fb_check: the flows and residuals must be four [B,2,H,W] tensors of one shape")
        B, _, H, W = flow_fw.shape
        for o in (occ_fw, occ_bw):
            if o.dtype != torch.uint8 or tuple(o.shape) != (B, H, W) or not o.is_contiguous() or (self.require_cuda and not o.is_cuda):
                raise PfError("fb_check: the masks must be contiguous uint8 [B,H,W] device tensors")
        self._rc(self._dll.pf_fb_check(_ptr(flow_fw), _ptr(flow_bw), _ptr(occ_fw), _ptr(occ_bw), _ptr(res_fw), _ptr(res_bw),
                                       B, H, W, self.FB_METRICS[metric], float(alpha), float(beta), self._stream(flow_fw)),
                 "pf_fb_check")

    # ---- chained flows and point tracks --------------------------------
    TRK_OCCLUDED, TRK_POLE, TRK_NONFINITE = 1, 2, 4     # PF_TRK_*
    COMPOSE_MAX = 4                                     # PF_COMPOSE_MAX

    def _chk_mask(self, t, shape, what):
        if t is not None and (t.dtype != torch.uint8 or tuple(t.shape) != tuple(shape) or not t.is_contiguous()
                              or (self.require_cuda and not t.is_cuda)):
            raise PfError(f"{what}: expected a contiguous uint8 {tuple(shape)} device tensor")

    def flow_compose(self, jobs):
        """pf_flow_compose: jobs = 1..4 tuples (f, state_f, g, occ_g, out, state_out) of one geometry, one launch.  f, g, out:
        fp32 [B,2,H,W]; state_f, occ_g, state_out: uint8 [B,H,W] or None.  out(x) = f(x) + g^(x + f(x)); out may be f."""
        jobs = list(jobs)
        if not 1 <= len(jobs) <= self.COMPOSE_MAX:
            raise PfError(f"flow_compose: {len(jobs)} jobs, expected 1..{self.COMPOSE_MAX}")
        f0 = jobs[0][0]
        if f0.dim() != 4 or f0.shape[1] != 2:
            raise PfError(f"flow_compose: f {tuple(f0.shape)}, expected [B,2,H,W]")
        B, _, H, W = f0.shape
        arr = (ComposeJob * len(jobs))()
        for q, (f, state_f, g, occ_g, out, state_out) in zip(arr, jobs):
            self._chk(f, g, out)
            if any(t.shape != f0.shape or t.device != f0.device for t in (f, g, out)):
                raise PfError("flow_compose: f, g and out of every job must be [B,2,H,W] tensors of one shape and device")
            for m in (state_f, occ_g, state_out):
                self._chk_mask(m, (B, H, W), "flow_compose: a state / mask")
            q.f, q.state_f, q.g, q.occ_g, q.out, q.state_out = (None if t is None else t.data_ptr()
                                                                for t in (f, state_f, g, occ_g, out, state_out))
        self._rc(self._dll.pf_flow_compose(arr, len(jobs), B, H, W, self._stream(f0)), "pf_flow_compose")

    def track_points(self, pos, state, flow, occ=None):
        """pf_track_points, in place: pos fp32 [B,N,2] (x unwrapped, y), state uint8 [B,N], flow [B,2,H,W], occ uint8 [B,H,W]."""
        self._chk(pos, flow)
        if pos.dim() != 3 or pos.shape[2] != 2 or flow.dim() != 4 or flow.shape[1] != 2 or flow.shape[0] != pos.shape[0]:
            raise PfError(f"track_points: pos {tuple(pos.shape)} / flow {tuple(flow.shape)}, expected [B,N,2] and [B,2,H,W]")
        B, N, _ = pos.shape
        H, W = flow.shape[2:]
        self._chk_mask(state, (B, N), "track_points: state")
        self._chk_mask(occ, (B, H, W), "track_points: occ")
        if state is None:
            raise PfError("track_points: state is required")
        self._rc(self._dll.pf_track_points(_ptr(pos), _ptr(state), _ptr(flow), _ptr(occ), B, N, H, W, self._stream(pos)),
                 "pf_track_points")
        return pos, state

    def track_grid(self, pos, H: int, W: int):
        """pf_track_grid: the pixel centres (x, y) of an H x W map into pos fp32 [B,H*W,2]."""
        self._chk(pos)
        if pos.dim() != 3 or tuple(pos.shape[1:]) != (H * W, 2):
            raise PfError(f"track_grid: pos {tuple(pos.shape)}, expected [B,{H * W},2]")
        self._rc(self._dll.pf_track_grid(_ptr(pos), pos.shape[0], H, W, self._stream(pos)), "pf_track_grid")
        return pos

    def region_sums(self, epe, sd, weight, bits, nregions, partials):
        """epe, sd: [B,H,W]; weight: [H*W] or None; bits: uint8 [H*W]; partials: float64 [B,nblk,nregions,3]."""
        self._chk(epe, sd, weight)
        if bits.dtype != torch.uint8 or partials.dtype != torch.float64 or not bits.is_contiguous() \
                or not partials.is_contiguous():
            raise PfError("region_sums: bits must be contiguous uint8, partials contiguous float64")
        B = epe.shape[0]
        N = epe[0].numel()
        if bits.numel() != N or partials.shape[0] != B or partials.shape[2] != nregions or partials.shape[3] != 3:
            raise PfError("region_sums: shape mismatch")
        self._rc(self._dll.pf_region_sums(_ptr(epe), _ptr(sd), _ptr(weight), C.c_void_p(bits.data_ptr()), nregions,
                                          C.c_void_p(partials.data_ptr()), partials.shape[1], B, N,
                                          self._stream(epe)), "pf_region_sums")

    # ---- flow rendering ------------------------------------------------
    RENDER_MODES = {"omni": 0, "plane": 1}          # PF_RENDER_OMNI / PF_RENDER_PLANE
    RENDER_LAYOUTS = {"hwc": 0, "chw": 1}           # PF_LAYOUT_HWC / PF_LAYOUT_CHW

    def _chk_bytes(self, t, what, dtype=None):
        """A contiguous device buffer handed over as raw memory (scratch, byte images, masks)."""
        if not t.is_contiguous() or (dtype is not None and t.dtype != dtype):
            raise PfError(f"{what}: expected a contiguous {dtype or 'device'} tensor, got {t.dtype} contiguous={t.is_contiguous()}")
        if self.require_cuda and not t.is_cuda:
            raise PfError(f"{what}: the HIP path needs tensors on a cuda (ROCm) device; there is no CPU fallback")

    def order_stat_scratch_bytes(self, B: int, n: int) -> int:
        r = self._dll.pf_order_stat_scratch_bytes(B, n)
        self._rc(min(r, 0), "pf_order_stat_scratch_bytes")
        return r

    def order_stat(self, x, k: int, out, scratch):
        """out[b] = sort(x[b])[k] of a non-negative fp32 [B, n] map, exact (pf_order_stat); scratch: order_stat_scratch_bytes."""
        self._chk(x, out)
        self._chk_bytes(scratch, "order_stat: scratch")
        if x.dim() != 2 or out.numel() != x.shape[0]:
            raise PfError(f"order_stat: x {tuple(x.shape)} / out {tuple(out.shape)}: expected [B, n] and [B]")
        self._rc(self._dll.pf_order_stat(_ptr(x), _ptr(out), _ptr(scratch), scratch.numel() * scratch.element_size(),
                                         x.shape[0], x.shape[1], int(k), self._stream(x)), "pf_order_stat")
        return out

    def flow_render_scratch_bytes(self, B: int, H: int, W: int) -> int:
        r = self._dll.pf_flow_render_scratch_bytes(B, H, W)
        self._rc(min(r, 0), "pf_flow_render_scratch_bytes")
        return r

    def flow_render(self, flow, out, scratch, mode="omni", percentile=0.95, layout="hwc", bgr=False):
        """Colour coding of flows [B,2,H,W] into a uint8 image [B,H,W,3] ("hwc") or [B,3,H,W] ("chw") (pf_flow_render)."""
        self._chk(flow)
        if mode not in self.RENDER_MODES or layout not in self.RENDER_LAYOUTS:
            raise PfError(f"flow_render: mode {mode!r} / layout {layout!r}, expected 'omni' | 'plane' and 'hwc' | 'chw'")
        if flow.dim() != 4 or flow.shape[1] != 2:
            raise PfError(f"flow_render: flow {tuple(flow.shape)}, expected [B,2,H,W]")
        B, _, H, W = flow.shape
        self._chk_bytes(out, "flow_render: out", torch.uint8)
        self._chk_bytes(scratch, "flow_render: scratch")
        if tuple(out.shape) != ((B, H, W, 3) if layout == "hwc" else (B, 3, H, W)):
            raise PfError(f"flow_render: out {tuple(out.shape)} does not fit flow {tuple(flow.shape)} in layout {layout!r}")
        self._rc(self._dll.pf_flow_render(_ptr(flow), _ptr(out), _ptr(scratch), scratch.numel() * scratch.element_size(), B, H, W,
                                          self.RENDER_MODES[mode], float(percentile), self.RENDER_LAYOUTS[layout], int(bool(bgr)),
                                          self._stream(flow)), "pf_flow_render")
        return out

    def cycle_warp(self, x, flo, out, ref=None, err=None):
        """my_cycle_warp: out = x [B,C,H,W] sampled at pixel + flo [B,2,H,W]; with ref and err [B,H,W]: err = mean_c |ref - out|."""
        self._chk(x, flo, out, ref, err)
        if x.dim() != 4 or flo.dim() != 4 or flo.shape[1] != 2 or flo.shape[0] != x.shape[0] or flo.shape[2:] != x.shape[2:] \
                or out.shape != x.shape or (ref is not None and ref.shape != x.shape):
            raise PfError(f"cycle_warp: x {tuple(x.shape)} / flo {tuple(flo.shape)} / out {tuple(out.shape)} do not fit")
        B, Cc, H, W = x.shape
        if (ref is None) != (err is None) or (err is not None and tuple(err.shape) != (B, H, W)):
            raise PfError("cycle_warp: ref [B,C,H,W] and err [B,H,W] go together")
        self._rc(self._dll.pf_cycle_warp(_ptr(x), _ptr(flo), _ptr(ref), _ptr(out), _ptr(err), B, Cc, H, W, self._stream(x)),
                 "pf_cycle_warp")
        return out

    # ---- training augmentation -----------------------------------------
    def _have(self, name: str):
        if name in self.missing:
            raise PfError(f"{self.path} does not export {name}")

    def augment_scratch_bytes(self, B: int) -> int:
        self._have("pf_augment_scratch_bytes")
        r = self._dll.pf_augment_scratch_bytes(B)
        self._rc(min(r, 0), "pf_augment_scratch_bytes")
        return r

    def augment_360(self, img1, img2, flow, params, image1, image2, flow_gt, valid, scratch):
        """FlowAugmentor_360 and the loader steps around it on B samples (pf_augment_360): img1, img2 uint8 [B,H,W,3], flow fp32
        [B,H,W,2], params int32 [B, AUG_ROW_WORDS] -> image1, image2 [B,3,H,W], flow_gt [B,2,H,W], valid [B,H,W], fp32."""
        self._have("pf_augment_360")
        if img1.dim() != 4 or img1.shape[3] != 3:
            raise PfError(f"augment_360: img1 {tuple(img1.shape)}, expected [B,H,W,3]")
        B, H, W, _ = img1.shape
        self._chk_bytes(img1, "augment_360: img1", torch.uint8)
        self._chk_bytes(img2, "augment_360: img2", torch.uint8)
        self._chk_bytes(params, "augment_360: params", torch.int32)
        self._chk_bytes(scratch, "augment_360: scratch")
        self._chk(flow, image1, image2, flow_gt, valid)
        want = ((img2, (B, H, W, 3)), (flow, (B, H, W, 2)), (params, (B, AUG_ROW_WORDS)), (image1, (B, 3, H, W)),
                (image2, (B, 3, H, W)), (flow_gt, (B, 2, H, W)), (valid, (B, H, W)))
        for t, shape in want:
            if tuple(t.shape) != shape:
                raise PfError(f"augment_360: a tensor of shape {tuple(t.shape)} where {shape} is expected (img1 {tuple(img1.shape)})")
        self._rc(self._dll.pf_augment_360(_ptr(img1), _ptr(img2), _ptr(flow), _ptr(params), _ptr(image1), _ptr(image2),
                                          _ptr(flow_gt), _ptr(valid), _ptr(scratch), scratch.numel() * scratch.element_size(),
                                          B, H, W, self._stream(img1)), "pf_augment_360")
        return image1, image2, flow_gt, valid

    def augment_convert(self, src, out, to_rgb: bool):
        """Pillow's 8-bit RGB -> HSV (to_rgb False) or HSV -> RGB on interleaved pixels [..., 3] (pf_augment_convert)."""
        self._have("pf_augment_convert")
        self._chk_bytes(src, "augment_convert: src", torch.uint8)
        self._chk_bytes(out, "augment_convert: out", torch.uint8)
        if src.dim() < 1 or src.shape[-1] != 3 or out.shape != src.shape:
            raise PfError(f"augment_convert: src {tuple(src.shape)} / out {tuple(out.shape)}, expected equal shapes [..., 3]")
        self._rc(self._dll.pf_augment_convert(_ptr(src), _ptr(out), src.numel() // 3, int(bool(to_rgb)), self._stream(src)),
                 "pf_augment_convert")
        return out

    # ---- perspective viewports and cube maps ---------------------------
    @staticmethod
    def view_table(rows):
        """The host table of pf_viewport_*: V rows {R row-major, f, h, w} as a ctypes float array (built once per view set)."""
        rows = [[float(v) for v in r] for r in rows]
        if not 1 <= len(rows) <= VIEW_MAX or any(len(r) != VIEW_WORDS for r in rows):
            raise PfError(f"a view table has 1..{VIEW_MAX} rows of {VIEW_WORDS} numbers")
        return (C.c_float * (len(rows) * VIEW_WORDS))(*[v for r in rows for v in r])

    def viewport_image(self, x, table, out):
        """ERP -> views (pf_viewport_image): x fp32 [B,C,H,W] -> out [B,V,C,h,w], or uint8 [B,H,W,C] -> out [B,V,h,w,C]."""
        self._have("pf_viewport_image")
        V = len(table) // VIEW_WORDS
        h, w = int(table[10]), int(table[11])
        if x.dim() != 4 or x.dtype not in (torch.float32, torch.uint8) or out.dtype != x.dtype:
            raise PfError(f"viewport_image: x {x.dtype} {tuple(x.shape)} / out {out.dtype}, expected fp32 [B,C,H,W] or uint8 [B,H,W,C]")
        self._chk_bytes(x, "viewport_image: x")
        self._chk_bytes(out, "viewport_image: out")
        if x.dtype == torch.float32:
            (B, Cc, H, W), form, want = x.shape, VIEW_F32, lambda: (B, V, Cc, h, w)
        else:
            (B, H, W, Cc), form, want = x.shape, VIEW_U8, lambda: (B, V, h, w, Cc)
        if tuple(out.shape) != want():
            raise PfError(f"viewport_image: out {tuple(out.shape)}, expected {want()} for x {tuple(x.shape)}")
        self._rc(self._dll.pf_viewport_image(_ptr(x), _ptr(out), table, V, B, Cc, H, W, form, self._stream(x)), "pf_viewport_image")
        return out

    def viewport_flow(self, flow, table, out, valid, min_forward: float):
        """ERP flow [B,2,H,W] -> pinhole flow out [B,V,2,h,w] and valid uint8 [B,V,h,w] (pf_viewport_flow)."""
        self._have("pf_viewport_flow")
        V = len(table) // VIEW_WORDS
        h, w = int(table[10]), int(table[11])
        self._chk(flow, out)
        self._chk_bytes(valid, "viewport_flow: valid", torch.uint8)
        if flow.dim() != 4 or flow.shape[1] != 2:
            raise PfError(f"viewport_flow: flow {tuple(flow.shape)}, expected [B,2,H,W]")
        B, _, H, W = flow.shape
        if tuple(out.shape) != (B, V, 2, h, w) or tuple(valid.shape) != (B, V, h, w):
            raise PfError(f"viewport_flow: out {tuple(out.shape)} / valid {tuple(valid.shape)}, expected {(B, V, 2, h, w)} and {(B, V, h, w)}")
        self._rc(self._dll.pf_viewport_flow(_ptr(flow), table, V, _ptr(out), _ptr(valid), B, H, W, float(min_forward),
                                            self._stream(flow)), "pf_viewport_flow")
        return out, valid

    def cubemap_to_erp(self, faces, out):
        """Cube faces [B,6,C,s,s] -> ERP out [B,C,H,W] (pf_cubemap_to_erp)."""
        self._have("pf_cubemap_to_erp")
        self._chk(faces, out)
        if faces.dim() != 5 or faces.shape[1] != 6 or faces.shape[3] != faces.shape[4] or out.dim() != 4 \
                or out.shape[0] != faces.shape[0] or out.shape[1] != faces.shape[2]:
            raise PfError(f"cubemap_to_erp: faces {tuple(faces.shape)} / out {tuple(out.shape)}, expected [B,6,C,s,s] and [B,C,H,W]")
        B, Cc, H, W = out.shape
        self._rc(self._dll.pf_cubemap_to_erp(_ptr(faces), _ptr(out), B, Cc, faces.shape[3], H, W, self._stream(faces)),
                 "pf_cubemap_to_erp")
        return out

    # ---- forward softmax splatting -------------------------------------
    def splat_scratch_bytes(self, B: int, C_: int, H: int, W: int) -> int:
        self._have("pf_splat_scratch_bytes")
        r = self._dll.pf_splat_scratch_bytes(B, C_, H, W)
        self._rc(min(r, 0), "pf_splat_scratch_bytes")
        return r

    def _chk_splat_acc(self, acc, B, Cc, H, W):
        self._chk_bytes(acc, "splat: acc", torch.int64)
        if tuple(acc.shape) != (B, Cc + 2, H, W):
            raise PfError(f"splat: acc {tuple(acc.shape)}, expected {(B, Cc + 2, H, W)}")

    def splat_accumulate(self, jobs, acc, alpha: float, zmax: float, vmax: float):
        """pf_splat_accumulate: jobs = 1..4 tuples (src, flow, metric, mask, tau, beta) of one geometry, one launch.  src fp32
        [B,C,H,W], flow [B,2,H,W], metric [B,1|2,H,W] or None, mask uint8 [B,H,W] or None; acc int64 [B,C+2,H,W] (all-zero)."""
        self._have("pf_splat_accumulate")
        jobs = list(jobs)
        if not 1 <= len(jobs) <= SPLAT_MAX:
            raise PfError(f"splat_accumulate: {len(jobs)} jobs, expected 1..{SPLAT_MAX}")
        s0 = jobs[0][0]
        if s0.dim() != 4:
            raise PfError(f"splat_accumulate: src {tuple(s0.shape)}, expected [B,C,H,W]")
        B, Cc, H, W = s0.shape
        self._chk_splat_acc(acc, B, Cc, H, W)
        arr = (SplatJob * len(jobs))()
        for q, (src, flow, metric, mask, tau, beta) in zip(arr, jobs):
            self._chk(src, flow, metric)
            if src.shape != s0.shape or tuple(flow.shape) != (B, 2, H, W) or any(
                    t is not None and t.device != acc.device for t in (src, flow, metric, mask)):
                raise PfError(f"splat_accumulate: src {tuple(src.shape)} / flow {tuple(flow.shape)} do not fit {tuple(s0.shape)} on {acc.device}")
            if metric is not None and (metric.dim() != 4 or metric.shape[1] not in (1, 2) or tuple(metric.shape[::2]) != (B, H)
                                       or metric.shape[3] != W):
                raise PfError(f"splat_accumulate: metric {tuple(metric.shape)}, expected [B,1,H,W] or [B,2,H,W]")
            self._chk_mask(mask, (B, H, W), "splat_accumulate: mask")
            q.src, q.flow, q.metric, q.mask = (None if t is None else t.data_ptr() for t in (src, flow, metric, mask))
            q.cm, q.tau, q.beta = (0 if metric is None else metric.shape[1]), float(tau), float(beta)
        self._rc(self._dll.pf_splat_accumulate(arr, len(jobs), _ptr(acc), B, Cc, H, W, float(alpha), float(zmax), float(vmax),
                                               self._stream(s0)), "pf_splat_accumulate")

    def splat_resolve(self, acc, out, hole, njobs: int, vmax: float, cmin: float, fill0=None, fill1=None, fill_t: float = 0.0):
        """pf_splat_resolve: out fp32 [B,C,H,W] and hole uint8 [B,H,W] from acc (zeroed again); njobs, vmax: the accumulate
        call's.  fill0, fill1 [B,C,H,W] (both or neither): a hole takes (1 - fill_t) fill0 + fill_t fill1, else 0."""
        self._have("pf_splat_resolve")
        self._chk(out, fill0, fill1)
        if out.dim() != 4:
            raise PfError(f"splat_resolve: out {tuple(out.shape)}, expected [B,C,H,W]")
        B, Cc, H, W = out.shape
        self._chk_splat_acc(acc, B, Cc, H, W)
        self._chk_mask(hole, (B, H, W), "splat_resolve: hole")
        if hole is None or (fill0 is None) != (fill1 is None) or any(f is not None and f.shape != out.shape for f in (fill0, fill1)):
            raise PfError("splat_resolve: hole is required; fill0 and fill1 go together and have out's shape")
        if any(t is not None and t.device != acc.device for t in (out, hole, fill0, fill1)):
            raise PfError("splat_resolve: every tensor must be on acc's device")
        self._rc(self._dll.pf_splat_resolve(_ptr(acc), _ptr(out), _ptr(hole), _ptr(fill0), _ptr(fill1), float(fill_t), float(cmin),
                                            int(njobs), B, Cc, H, W, float(vmax), self._stream(out)), "pf_splat_resolve")
        return out, hole

    # ---- camera rotation from 360-degree flow --------------------------
    def ego_scratch_bytes(self, B: int, H: int, W: int) -> int:
        self._have("pf_ego_scratch_bytes")
        r = self._dll.pf_ego_scratch_bytes(B, H, W)
        self._rc(min(r, 0), "pf_ego_scratch_bytes")
        return r

    def _chk_ego_mats(self, B, what, **mats):
        """Rotation matrices [B,3,3] fp32 (None allowed where the entry allows it), on one device."""
        self._chk(*mats.values())
        for name, t in mats.items():
            if t is not None and tuple(t.shape) != (B, 3, 3):
                raise PfError(f"{what}: {name} {tuple(t.shape)}, expected {(B, 3, 3)}")

    def ego_accumulate(self, flow, mask, R, sums, weighted: bool, scale_px: float, blocks: int = 0):
        """pf_ego_accumulate: one pass over flow fp32 [B,2,H,W] (mask uint8 [B,H,W] or None) under R [B,3,3] into sums int64
        [B,12]; blocks: workgroups per image (0: from the CU count)."""
        self._have("pf_ego_accumulate")
        self._chk(flow)
        if flow.dim() != 4 or flow.shape[1] != 2:
            raise PfError(f"ego_accumulate: flow {tuple(flow.shape)}, expected [B,2,H,W]")
        B, _, H, W = flow.shape
        self._chk_mask(mask, (B, H, W), "ego_accumulate: mask")
        self._chk_ego_mats(B, "ego_accumulate", R=R)
        self._chk_bytes(sums, "ego_accumulate: sums", torch.int64)
        if tuple(sums.shape) != (B, EGO_SUMS) or any(t is not None and t.device != flow.device for t in (mask, R, sums)):
            raise PfError(f"ego_accumulate: sums {tuple(sums.shape)}, expected {(B, EGO_SUMS)}, every tensor on {flow.device}")
        self._rc(self._dll.pf_ego_accumulate(_ptr(flow), _ptr(mask), _ptr(R), _ptr(sums), B, H, W, int(bool(weighted)),
                                             float(scale_px), int(blocks), self._stream(flow)), "pf_ego_accumulate")

    def ego_solve(self, sums, init, R, stats, H: int, W: int, gap_min: float):
        """pf_ego_solve: R [B,3,3] and stats [B,5] from sums int64 [B,12] (zeroed again); init [B,3,3] or None (identity)."""
        self._have("pf_ego_solve")
        self._chk(stats)
        self._chk_bytes(sums, "ego_solve: sums", torch.int64)
        if sums.dim() != 2 or sums.shape[1] != EGO_SUMS:
            raise PfError(f"ego_solve: sums {tuple(sums.shape)}, expected [B,{EGO_SUMS}]")
        B = sums.shape[0]
        self._chk_ego_mats(B, "ego_solve", init=init, R=R)
        if tuple(stats.shape) != (B, EGO_STATS) or any(t is not None and t.device != sums.device for t in (init, R, stats)):
            raise PfError(f"ego_solve: stats {tuple(stats.shape)}, expected {(B, EGO_STATS)}, every tensor on {sums.device}")
        self._rc(self._dll.pf_ego_solve(_ptr(sums), _ptr(init), _ptr(R), _ptr(stats), B, int(H), int(W), float(gap_min),
                                        self._stream(sums)), "pf_ego_solve")
        return R, stats

    def ego_track(self, R, state, orient, corr, smoothing: float):
        """pf_ego_track: state float64 [B,8] (two unit quaternions) advanced by R [B,3,3]; writes orient and corr [B,3,3]."""
        self._have("pf_ego_track")
        self._chk_bytes(state, "ego_track: state", torch.float64)
        if state.dim() != 2 or state.shape[1] != EGO_STATE:
            raise PfError(f"ego_track: state {tuple(state.shape)}, expected [B,{EGO_STATE}]")
        B = state.shape[0]
        self._chk_ego_mats(B, "ego_track", R=R, orient=orient, corr=corr)
        if any(t.device != state.device for t in (R, orient, corr)):
            raise PfError(f"ego_track: every tensor must be on {state.device}")
        self._rc(self._dll.pf_ego_track(_ptr(R), _ptr(state), _ptr(orient), _ptr(corr), B, float(smoothing), self._stream(state)),
                 "pf_ego_track")
        return orient, corr

    def erp_rotate(self, x, R, out):
        """pf_erp_rotate: x fp32 [B,C,H,W] or uint8 [B,H,W,C] (C = 1..4) resampled under R [B,3,3] into out (x's shape and dtype)."""
        self._have("pf_erp_rotate")
        if x.dim() != 4 or x.dtype not in (torch.float32, torch.uint8) or out.dtype != x.dtype or out.shape != x.shape:
            raise PfError(f"erp_rotate: x {x.dtype} {tuple(x.shape)} / out {out.dtype} {tuple(out.shape)}, expected fp32 [B,C,H,W] or "
                          "uint8 [B,H,W,C] and an out like x")
        self._chk_bytes(x, "erp_rotate: x")
        self._chk_bytes(out, "erp_rotate: out")
        if x.dtype == torch.float32:
            (B, Cc, H, W), form = x.shape, VIEW_F32
        else:
            (B, H, W, Cc), form = x.shape, VIEW_U8
        self._chk_ego_mats(B, "erp_rotate", R=R)
        if R.device != x.device or out.device != x.device:
            raise PfError(f"erp_rotate: every tensor must be on {x.device}")
        self._rc(self._dll.pf_erp_rotate(_ptr(x), _ptr(out), _ptr(R), B, Cc, H, W, form, self._stream(x)), "pf_erp_rotate")
        return out

    def ego_derotate(self, flow, mask, R, out, valid):
        """pf_ego_derotate: flow fp32 [B,2,H,W] with the rotation R [B,3,3] removed into out (may be flow); mask, valid: uint8
        [B,H,W] or None."""
        self._have("pf_ego_derotate")
        self._chk(flow, out)
        if flow.dim() != 4 or flow.shape[1] != 2 or out.shape != flow.shape:
            raise PfError(f"ego_derotate: flow {tuple(flow.shape)} / out {tuple(out.shape)}, expected [B,2,H,W] twice")
        B, _, H, W = flow.shape
        self._chk_mask(mask, (B, H, W), "ego_derotate: mask")
        self._chk_mask(valid, (B, H, W), "ego_derotate: valid")
        self._chk_ego_mats(B, "ego_derotate", R=R)
        if any(t is not None and t.device != flow.device for t in (mask, R, out, valid)):
            raise PfError(f"ego_derotate: every tensor must be on {flow.device}")
        self._rc(self._dll.pf_ego_derotate(_ptr(flow), _ptr(mask), _ptr(R), _ptr(out), _ptr(valid), B, H, W, self._stream(flow)),
                 "pf_ego_derotate")
        return out, valid

    # ---- camera translation from 360-degree flow -----------------------
    def epi_sums_bytes(self, B: int, H: int, W: int) -> int:
        self._have("pf_epi_sums_bytes")
        r = self._dll.pf_epi_sums_bytes(B, H, W)
        self._rc(min(r, 0), "pf_epi_sums_bytes")
        return r

    def _chk_epi_vecs(self, B, what, **vecs):
        """Translations [B,3] fp32 (None allowed where the entry allows it)."""
        self._chk(*vecs.values())
        for name, t in vecs.items():
            if t is not None and tuple(t.shape) != (B, 3):
                raise PfError(f"{what}: {name} {tuple(t.shape)}, expected {(B, 3)}")

    def epi_accumulate(self, flow, mask, R, t, sums, mode: int, scale_px: float, vote_px: float, blocks: int = 0):
        """pf_epi_accumulate: one pass of `mode` (EPI_T / EPI_R) over flow fp32 [B,2,H,W] (mask uint8 [B,H,W] or None) under R
        [B,3,3] and t [B,3] (None: zero, EPI_T only) into sums int64 [B,22]; blocks: workgroups per image (0: from the CU count)."""
        self._have("pf_epi_accumulate")
        self._chk(flow)
        if flow.dim() != 4 or flow.shape[1] != 2:
            raise PfError(f"epi_accumulate: flow {tuple(flow.shape)}, expected [B,2,H,W]")
        B, _, H, W = flow.shape
        self._chk_mask(mask, (B, H, W), "epi_accumulate: mask")
        self._chk_ego_mats(B, "epi_accumulate", R=R)
        self._chk_epi_vecs(B, "epi_accumulate", t=t)
        self._chk_bytes(sums, "epi_accumulate: sums", torch.int64)
        if tuple(sums.shape) != (B, EPI_SUMS) or any(x is not None and x.device != flow.device for x in (mask, R, t, sums)):
            raise PfError(f"epi_accumulate: sums {tuple(sums.shape)}, expected {(B, EPI_SUMS)}, every tensor on {flow.device}")
        self._rc(self._dll.pf_epi_accumulate(_ptr(flow), _ptr(mask), _ptr(R), _ptr(t), _ptr(sums), B, H, W, int(mode), float(scale_px),
                                             float(vote_px), int(blocks), self._stream(flow)), "pf_epi_accumulate")

    def epi_solve(self, sums, t_init, R, t, stats, H: int, W: int, mode: int, gap_min: float, min_parallax_px: float):
        """pf_epi_solve: EPI_T: t [B,3] and stats [B,6] from sums int64 [B,22]; t_init [B,3] or None (zero); R may be None.
        EPI_R: R [B,3,3] refined in place about t.  The sums read are zeroed again."""
        self._have("pf_epi_solve")
        self._chk(stats)
        self._chk_bytes(sums, "epi_solve: sums", torch.int64)
        if sums.dim() != 2 or sums.shape[1] != EPI_SUMS:
            raise PfError(f"epi_solve: sums {tuple(sums.shape)}, expected [B,{EPI_SUMS}]")
        B = sums.shape[0]
        self._chk_ego_mats(B, "epi_solve", R=R)
        self._chk_epi_vecs(B, "epi_solve", t_init=t_init, t=t)
        if t is None or tuple(stats.shape) != (B, EPI_STATS) or any(x is not None and x.device != sums.device for x in (t_init, R, t, stats)):
            raise PfError(f"epi_solve: t is required, stats {tuple(stats.shape)}, expected {(B, EPI_STATS)}, every tensor on {sums.device}")
        self._rc(self._dll.pf_epi_solve(_ptr(sums), _ptr(t_init), _ptr(R), _ptr(t), _ptr(stats), B, int(H), int(W), int(mode),
                                        float(gap_min), float(min_parallax_px), self._stream(sums)), "pf_epi_solve")
        return R, t, stats

    def epi_map(self, flow, mask, R, t, inv_depth, resid, conf, moving, thr_px: float, neg_px: float, conf_min: float):
        """pf_epi_map: flow fp32 [B,2,H,W] under R [B,3,3] and t [B,3] into inv_depth, resid, conf (fp32 [B,H,W]) and moving (uint8
        [B,H,W]); each output may be None."""
        self._have("pf_epi_map")
        self._chk(flow, inv_depth, resid, conf)
        if flow.dim() != 4 or flow.shape[1] != 2:
            raise PfError(f"epi_map: flow {tuple(flow.shape)}, expected [B,2,H,W]")
        B, _, H, W = flow.shape
        self._chk_mask(mask, (B, H, W), "epi_map: mask")
        self._chk_mask(moving, (B, H, W), "epi_map: moving")
        self._chk_ego_mats(B, "epi_map", R=R)
        self._chk_epi_vecs(B, "epi_map", t=t)
        for name, x in (("inv_depth", inv_depth), ("resid", resid), ("conf", conf)):
            if x is not None and tuple(x.shape) != (B, H, W):
                raise PfError(f"epi_map: {name} {tuple(x.shape)}, expected {(B, H, W)}")
        if R is None or t is None or any(x is not None and x.device != flow.device for x in (mask, R, t, inv_depth, resid, conf, moving)):
            raise PfError(f"epi_map: R and t are required, every tensor on {flow.device}")
        self._rc(self._dll.pf_epi_map(_ptr(flow), _ptr(mask), _ptr(R), _ptr(t), _ptr(inv_depth), _ptr(resid), _ptr(conf), _ptr(moving),
                                      B, H, W, float(thr_px), float(neg_px), float(conf_min), self._stream(flow)), "pf_epi_map")
        return inv_depth, resid, conf, moving

    # ---- camera trajectory ----------------------------------------------
    def odo_hist_bytes(self, B: int, H: int, W: int, bins: int) -> int:
        self._have("pf_odo_hist_bytes")
        r = self._dll.pf_odo_hist_bytes(B, H, W, int(bins))
        self._rc(min(r, 0), "pf_odo_hist_bytes")
        return r

    def _chk_odo_map(self, m, what):
        """A parallax map (inv_depth, conf fp32 [B,H,W], moving uint8 [B,H,W]) -> its shape."""
        if not isinstance(m, (tuple, list)) or len(m) != 3 or not all(isinstance(x, torch.Tensor) for x in m):
            raise PfError(f"{what}: a map is (inv_depth, conf, moving)")
        self._chk(m[0], m[1])
        if m[0].dim() != 3 or m[1].shape != m[0].shape or m[1].device != m[0].device or m[2].device != m[0].device:
            raise PfError(f"{what}: inv_depth {tuple(m[0].shape)}, conf {tuple(m[1].shape)}, expected two [B,H,W] on one device")
        self._chk_mask(m[2], m[0].shape, f"{what}: moving")
        return tuple(m[0].shape)

    def _chk_odo_vec(self, t, shape, what, dtype=torch.float32):
        self._chk_bytes(t, what, dtype)
        if tuple(t.shape) != tuple(shape):
            raise PfError(f"{what}: {tuple(t.shape)}, expected {tuple(shape)}")

    def odo_accumulate(self, map_a, map_b, hist, bins: int, log2_range: float, kappa_min: float, blocks: int = 0):
        """pf_odo_accumulate: the pixels of two maps (inv_depth, conf, moving) of one grid into hist int64 [B, 2 bins + 2]."""
        self._have("pf_odo_accumulate")
        B, H, W = self._chk_odo_map(map_a, "odo_accumulate: map_a")
        if self._chk_odo_map(map_b, "odo_accumulate: map_b") != (B, H, W) or map_b[0].device != map_a[0].device:
            raise PfError("odo_accumulate: the two maps differ in shape or device")
        self._chk_odo_vec(hist, (B, 2 * int(bins) + 2), "odo_accumulate: hist", torch.int64)
        if hist.device != map_a[0].device:
            raise PfError(f"odo_accumulate: every tensor must be on {map_a[0].device}")
        self._rc(self._dll.pf_odo_accumulate(_ptr(map_a[0]), _ptr(map_a[1]), _ptr(map_a[2]), _ptr(map_b[0]), _ptr(map_b[1]), _ptr(map_b[2]),
                                             _ptr(hist), B, H, W, int(bins), float(log2_range), float(kappa_min), int(blocks),
                                             self._stream(hist)), "pf_odo_accumulate")

    def odo_solve(self, hist, ratio, stats, H: int, W: int, bins: int, log2_range: float, trim_bins: int, min_used: float, max_iqr: float):
        """pf_odo_solve: ratio [B] and stats [B,6] from hist int64 [B, 2 bins + 2], which is zeroed again."""
        self._have("pf_odo_solve")
        self._chk_bytes(hist, "odo_solve: hist", torch.int64)
        if hist.dim() != 2 or hist.shape[1] != 2 * int(bins) + 2:
            raise PfError(f"odo_solve: hist {tuple(hist.shape)}, expected [B,{2 * int(bins) + 2}]")
        B = hist.shape[0]
        self._chk_odo_vec(ratio, (B,), "odo_solve: ratio")
        self._chk_odo_vec(stats, (B, ODO_STATS), "odo_solve: stats")
        if ratio.device != hist.device or stats.device != hist.device:
            raise PfError(f"odo_solve: every tensor must be on {hist.device}")
        self._rc(self._dll.pf_odo_solve(_ptr(hist), _ptr(ratio), _ptr(stats), B, int(H), int(W), int(bins), float(log2_range), int(trim_bins),
                                        float(min_used), float(max_iqr), self._stream(hist)), "pf_odo_solve")
        return ratio, stats

    def odo_reverse_pose(self, R, t, R_rev, t_rev):
        """pf_odo_reverse_pose: (R [B,3,3], t [B,3]) -> (R^T, -R^T t) into R_rev, t_rev."""
        self._have("pf_odo_reverse_pose")
        self._chk(R)
        if R.dim() != 3:
            raise PfError(f"odo_reverse_pose: R {tuple(R.shape)}, expected [B,3,3]")
        B = R.shape[0]
        self._chk_ego_mats(B, "odo_reverse_pose", R=R, R_rev=R_rev)
        self._chk_epi_vecs(B, "odo_reverse_pose", t=t, t_rev=t_rev)
        if any(x is None or x.device != R.device for x in (t, R_rev, t_rev)):
            raise PfError(f"odo_reverse_pose: every tensor is required, on {R.device}")
        self._rc(self._dll.pf_odo_reverse_pose(_ptr(R), _ptr(t), _ptr(R_rev), _ptr(t_rev), B, self._stream(R)), "pf_odo_reverse_pose")
        return R_rev, t_rev

    def odo_track(self, R, t, pose_stats, ratio, link_stats, state, orient, centre, baseline, flags):
        """pf_odo_track: state float64 [B,12] advanced by one pair; writes orient [B,3,3], centre [B,3], baseline [B], flags int32 [B,4]."""
        self._have("pf_odo_track")
        self._chk_bytes(state, "odo_track: state", torch.float64)
        if state.dim() != 2 or state.shape[1] != ODO_STATE:
            raise PfError(f"odo_track: state {tuple(state.shape)}, expected [B,{ODO_STATE}]")
        B = state.shape[0]
        self._chk_ego_mats(B, "odo_track", R=R, orient=orient)
        self._chk_epi_vecs(B, "odo_track", t=t, centre=centre)
        self._chk_odo_vec(pose_stats, (B, EPI_STATS), "odo_track: pose_stats")
        self._chk_odo_vec(link_stats, (B, ODO_STATS), "odo_track: link_stats")
        self._chk_odo_vec(ratio, (B,), "odo_track: ratio")
        self._chk_odo_vec(baseline, (B,), "odo_track: baseline")
        self._chk_odo_vec(flags, (B, ODO_FLAGS), "odo_track: flags", torch.int32)
        if any(x is None or x.device != state.device for x in (R, t, pose_stats, ratio, link_stats, orient, centre, baseline, flags)):
            raise PfError(f"odo_track: every tensor is required, on {state.device}")
        self._rc(self._dll.pf_odo_track(_ptr(R), _ptr(t), _ptr(pose_stats), _ptr(ratio), _ptr(link_stats), _ptr(state), _ptr(orient),
                                        _ptr(centre), _ptr(baseline), _ptr(flags), B, self._stream(state)), "pf_odo_track")
        return orient, centre

    def odo_fuse(self, map_a, map_b, S_a, S_b, link_valid, inv_depth, weight, disagree, conf_min: float, kappa_min: float, tol_log2: float):
        """pf_odo_fuse: two maps of one grid, brought to one unit by the device scalars S_a, S_b [B] (map a only where link_valid
        [B] != 0), into inv_depth, weight (fp32 [B,H,W]) and disagree (uint8 [B,H,W]); each output may be None."""
        self._have("pf_odo_fuse")
        B, H, W = self._chk_odo_map(map_a, "odo_fuse: map_a")
        if self._chk_odo_map(map_b, "odo_fuse: map_b") != (B, H, W):
            raise PfError("odo_fuse: the two maps differ in shape")
        dev = map_a[0].device
        for name, x in (("S_a", S_a), ("S_b", S_b), ("link_valid", link_valid)):
            self._chk_odo_vec(x, (B,), f"odo_fuse: {name}")
        self._chk(inv_depth, weight)
        for name, x in (("inv_depth", inv_depth), ("weight", weight)):
            if x is not None and tuple(x.shape) != (B, H, W):
                raise PfError(f"odo_fuse: {name} {tuple(x.shape)}, expected {(B, H, W)}")
        self._chk_mask(disagree, (B, H, W), "odo_fuse: disagree")
        if any(x is not None and x.device != dev for x in (map_b[0], S_a, S_b, link_valid, inv_depth, weight, disagree)):
            raise PfError(f"odo_fuse: every tensor must be on {dev}")
        self._rc(self._dll.pf_odo_fuse(_ptr(map_a[0]), _ptr(map_a[1]), _ptr(map_a[2]), _ptr(map_b[0]), _ptr(map_b[1]), _ptr(map_b[2]),
                                       _ptr(S_a), _ptr(S_b), _ptr(link_valid), _ptr(inv_depth), _ptr(weight), _ptr(disagree), B, H, W,
                                       float(conf_min), float(kappa_min), float(tol_log2), self._stream(map_a[0])), "pf_odo_fuse")
        return inv_depth, weight, disagree

    # ---- depth along the trajectory --------------------------------------
    def zsplat_bytes(self, B: int, C_: int, H: int, W: int) -> int:
        self._have("pf_zsplat_bytes")
        r = self._dll.pf_zsplat_bytes(B, C_, H, W)
        self._rc(min(r, 0), "pf_zsplat_bytes")
        return r

    def _chk_rp_maps(self, what, shape, dev, **maps):
        """fp32 maps of one shape on one device (None allowed where the entry allows it)."""
        self._chk(*maps.values())
        for name, t in maps.items():
            if t is not None and (tuple(t.shape) != tuple(shape) or t.device != dev):
                raise PfError(f"{what}: {name} {tuple(t.shape)} on {t.device}, expected {tuple(shape)} on {dev}")

    def _chk_rp_bytes(self, what, shape, dev, **maps):
        for name, t in maps.items():
            self._chk_mask(t, shape, f"{what}: {name}")
            if t is not None and t.device != dev:
                raise PfError(f"{what}: {name} must be on {dev}")

    def reproj_project(self, inv_depth, weight, mask, R, T, flow, d_new, valid, n_min: float):
        """pf_reproj_project: inv_depth, weight fp32 [B,H,W] (mask uint8 [B,H,W] or None) under R [B,3,3], T [B,3] into flow
        [B,2,H,W], d_new [B,H,W] and valid uint8 [B,H,W]."""
        self._have("pf_reproj_project")
        self._chk(inv_depth)
        if inv_depth.dim() != 3:
            raise PfError(f"reproj_project: inv_depth {tuple(inv_depth.shape)}, expected [B,H,W]")
        B, H, W = inv_depth.shape
        dev = inv_depth.device
        if weight is None or flow is None or d_new is None or valid is None or R is None or T is None:
            raise PfError("reproj_project: only mask may be None")
        self._chk_rp_maps("reproj_project", (B, H, W), dev, weight=weight, d_new=d_new)
        self._chk_rp_maps("reproj_project", (B, 2, H, W), dev, flow=flow)
        self._chk_rp_bytes("reproj_project", (B, H, W), dev, mask=mask, valid=valid)
        self._chk_ego_mats(B, "reproj_project", R=R)
        self._chk_epi_vecs(B, "reproj_project", T=T)
        if R.device != dev or T.device != dev:
            raise PfError(f"reproj_project: every tensor must be on {dev}")
        self._rc(self._dll.pf_reproj_project(_ptr(inv_depth), _ptr(weight), _ptr(mask), _ptr(R), _ptr(T), _ptr(flow), _ptr(d_new),
                                             _ptr(valid), B, H, W, float(n_min), self._stream(inv_depth)), "pf_reproj_project")
        return flow, d_new, valid

    def _chk_zsplat_in(self, what, src, flow, d, weight, valid, front):
        self._chk(d)
        if d.dim() != 3:
            raise PfError(f"{what}: d {tuple(d.shape)}, expected [B,H,W]")
        B, H, W = d.shape
        dev = d.device
        if flow is None or weight is None or valid is None or front is None:
            raise PfError(f"{what}: only src may be None")
        Cc = 0 if src is None else (src.shape[1] if src.dim() == 4 else -1)
        if not 0 <= Cc <= 4 or (src is not None and Cc == 0):
            raise PfError(f"{what}: src {tuple(src.shape)}, expected [B,C,H,W] with C = 1..4, or None")
        self._chk_rp_maps(what, (B, H, W), dev, weight=weight)
        self._chk_rp_maps(what, (B, 2, H, W), dev, flow=flow)
        self._chk_rp_maps(what, (B, Cc, H, W), dev, src=src)
        self._chk_rp_bytes(what, (B, H, W), dev, valid=valid)
        self._chk_bytes(front, f"{what}: front", torch.int32)
        if tuple(front.shape) != (B, H, W) or front.device != dev:
            raise PfError(f"{what}: front {tuple(front.shape)}, expected int32 {(B, H, W)} on {dev}")
        return B, Cc, H, W

    def zsplat_front(self, src, flow, d, weight, valid, front, b_min: float):
        """pf_zsplat_front: the nearest inverse depth that lands on each target, as bit patterns, into front int32 [B,H,W] (all-zero)."""
        self._have("pf_zsplat_front")
        B, Cc, H, W = self._chk_zsplat_in("zsplat_front", src, flow, d, weight, valid, front)
        self._rc(self._dll.pf_zsplat_front(_ptr(src), _ptr(flow), _ptr(d), _ptr(weight), _ptr(valid), _ptr(front), B, Cc, H, W,
                                           float(b_min), self._stream(d)), "pf_zsplat_front")

    def _chk_zsplat_acc(self, what, acc, B, Cc, H, W, dev):
        self._chk_bytes(acc, f"{what}: acc", torch.int64)
        if tuple(acc.shape) != (B, Cc + 3, H, W) or acc.device != dev:
            raise PfError(f"{what}: acc {tuple(acc.shape)}, expected int64 {(B, Cc + 3, H, W)} on {dev}")

    def zsplat_accumulate(self, src, flow, d, weight, valid, front, acc, b_min: float, tol_log2: float, w_max: float, dmax: float,
                          vmax: float):
        """pf_zsplat_accumulate: the taps that pass the depth test against front into acc int64 [B,C+3,H,W] (all-zero)."""
        self._have("pf_zsplat_accumulate")
        B, Cc, H, W = self._chk_zsplat_in("zsplat_accumulate", src, flow, d, weight, valid, front)
        self._chk_zsplat_acc("zsplat_accumulate", acc, B, Cc, H, W, d.device)
        self._rc(self._dll.pf_zsplat_accumulate(_ptr(src), _ptr(flow), _ptr(d), _ptr(weight), _ptr(valid), _ptr(front), _ptr(acc), B, Cc,
                                                H, W, float(b_min), float(tol_log2), float(w_max), float(dmax), float(vmax),
                                                self._stream(d)), "pf_zsplat_accumulate")

    def zsplat_resolve(self, acc, front, out, d_out, w_out, hole, cmin: float, w_max: float, dmax: float, vmax: float):
        """pf_zsplat_resolve: out fp32 [B,C,H,W] (None when C = 0), d_out, w_out fp32 [B,H,W] and hole uint8 [B,H,W] from acc and
        front, which are zeroed again; w_max, dmax, vmax: the accumulate call's."""
        self._have("pf_zsplat_resolve")
        self._chk(d_out)
        if d_out.dim() != 3:
            raise PfError(f"zsplat_resolve: d_out {tuple(d_out.shape)}, expected [B,H,W]")
        B, H, W = d_out.shape
        dev = d_out.device
        if w_out is None or hole is None or front is None:
            raise PfError("zsplat_resolve: only out may be None")
        Cc = 0 if out is None else (out.shape[1] if out.dim() == 4 else -1)
        if not 0 <= Cc <= 4 or (out is not None and Cc == 0):
            raise PfError(f"zsplat_resolve: out {tuple(out.shape)}, expected [B,C,H,W] with C = 1..4, or None")
        self._chk_rp_maps("zsplat_resolve", (B, H, W), dev, w_out=w_out)
        self._chk_rp_maps("zsplat_resolve", (B, Cc, H, W), dev, out=out)
        self._chk_rp_bytes("zsplat_resolve", (B, H, W), dev, hole=hole)
        self._chk_bytes(front, "zsplat_resolve: front", torch.int32)
        if tuple(front.shape) != (B, H, W) or front.device != dev:
            raise PfError(f"zsplat_resolve: front {tuple(front.shape)}, expected int32 {(B, H, W)} on {dev}")
        self._chk_zsplat_acc("zsplat_resolve", acc, B, Cc, H, W, dev)
        self._rc(self._dll.pf_zsplat_resolve(_ptr(acc), _ptr(front), _ptr(out), _ptr(d_out), _ptr(w_out), _ptr(hole), B, Cc, H, W,
                                             float(cmin), float(w_max), float(dmax), float(vmax), self._stream(d_out)),
                 "pf_zsplat_resolve")
        return out, d_out, w_out, hole

    def depth_update(self, d_s, w_s, d_m, w_m, disagree, flags, seg, tol_log2: float, decay: float, w_max: float):
        """pf_depth_update: the state (d_s, w_s) fp32 [B,H,W] in place from the measurement (d_m, w_m, disagree uint8 or None),
        flags int32 [B,4] and seg int32 [B], which is rewritten after the pixel pass."""
        self._have("pf_depth_update")
        self._chk(d_s)
        if d_s.dim() != 3:
            raise PfError(f"depth_update: d_s {tuple(d_s.shape)}, expected [B,H,W]")
        B, H, W = d_s.shape
        dev = d_s.device
        if w_s is None or d_m is None or w_m is None or flags is None or seg is None:
            raise PfError("depth_update: only disagree may be None")
        self._chk_rp_maps("depth_update", (B, H, W), dev, w_s=w_s, d_m=d_m, w_m=w_m)
        self._chk_rp_bytes("depth_update", (B, H, W), dev, disagree=disagree)
        self._chk_odo_vec(flags, (B, ODO_FLAGS), "depth_update: flags", torch.int32)
        self._chk_odo_vec(seg, (B,), "depth_update: seg", torch.int32)
        if flags.device != dev or seg.device != dev:
            raise PfError(f"depth_update: every tensor must be on {dev}")
        self._rc(self._dll.pf_depth_update(_ptr(d_s), _ptr(w_s), _ptr(d_m), _ptr(w_m), _ptr(disagree), _ptr(flags), _ptr(seg), B, H, W,
                                           float(tol_log2), float(decay), float(w_max), self._stream(d_s)), "pf_depth_update")
        return d_s, w_s

    # ---- moving objects -------------------------------------------------
    def seg_scratch_bytes(self, B: int, H: int, W: int) -> int:
        self._have("pf_seg_scratch_bytes")
        r = self._dll.pf_seg_scratch_bytes(B, H, W)
        self._rc(min(r, 0), "pf_seg_scratch_bytes")
        return r

    def seg_tables(self, rows, cols):
        """pf_seg_tables: rows fp32 [H,2] = (cos phi, sin phi), cols fp32 [W,2] = (cos theta, sin theta)."""
        self._have("pf_seg_tables")
        self._chk(rows, cols)
        if rows.dim() != 2 or cols.dim() != 2 or rows.shape[1] != 2 or cols.shape[1] != 2 or rows.device != cols.device:
            raise PfError(f"seg_tables: rows {tuple(rows.shape)}, cols {tuple(cols.shape)}, expected [H,2] and [W,2] on one device")
        self._rc(self._dll.pf_seg_tables(_ptr(rows), _ptr(cols), rows.shape[0], cols.shape[0], self._stream(rows)), "pf_seg_tables")
        return rows, cols

    def _chk_seg_scratch(self, what, scratch, dev):
        self._chk_bytes(scratch, f"{what}: scratch")
        if scratch.device != dev:
            raise PfError(f"{what}: scratch must be on {dev}")
        return scratch.numel() * scratch.element_size()

    def seg_label(self, mask, rows, labels, scratch, connectivity: int, poles: bool):
        """pf_seg_label: mask uint8 [B,H,W] into labels int32 [B,H,W] (1 + the smallest linear index of the component, 0 for
        background); rows: seg_tables' [H,2]; scratch: seg_scratch_bytes."""
        self._have("pf_seg_label")
        if mask.dim() != 3:
            raise PfError(f"seg_label: mask {tuple(mask.shape)}, expected [B,H,W]")
        B, H, W = mask.shape
        dev = mask.device
        self._chk_rp_bytes("seg_label", (B, H, W), dev, mask=mask)
        self._chk_rp_maps("seg_label", (H, 2), dev, rows=rows)
        self._chk_odo_vec(labels, (B, H, W), "seg_label: labels", torch.int32)
        if labels.device != dev or rows is None:
            raise PfError(f"seg_label: every tensor must be on {dev}")
        nbytes = self._chk_seg_scratch("seg_label", scratch, dev)
        self._rc(self._dll.pf_seg_label(_ptr(mask), _ptr(rows), _ptr(labels), _ptr(scratch), nbytes, B, H, W, int(connectivity),
                                        int(poles), self._stream(mask)), "pf_seg_label")
        return labels

    def seg_objects(self, labels, values, rows, cols, scratch, ids, keep, roots, count, table, sums, min_area: float):
        """pf_seg_objects: the components of labels int32 [B,H,W] (and scratch, as seg_label left them) into ids int32 [B,H,W],
        keep uint8 [B,H,W], roots int32 [B,M], count int32 [B], table fp32 [B,M,SEG_COLS + C] and sums int64 [B,M,SEG_SUMS];
        values fp32 [B,C,H,W] or None."""
        self._have("pf_seg_objects")
        if labels.dim() != 3 or roots.dim() != 2:
            raise PfError(f"seg_objects: labels {tuple(labels.shape)}, roots {tuple(roots.shape)}, expected [B,H,W] and [B,M]")
        B, H, W = labels.shape
        M = roots.shape[1]
        dev = labels.device
        Cc = 0 if values is None else (values.shape[1] if values.dim() == 4 else -1)
        if not 0 <= Cc <= 4 or (values is not None and Cc == 0):
            raise PfError(f"seg_objects: values {tuple(values.shape)}, expected [B,C,H,W] with C = 1..4, or None")
        self._chk_rp_maps("seg_objects", (B, Cc, H, W), dev, values=values)
        self._chk_rp_maps("seg_objects", (H, 2), dev, rows=rows)
        self._chk_rp_maps("seg_objects", (W, 2), dev, cols=cols)
        self._chk_rp_maps("seg_objects", (B, M, SEG_COLS + Cc), dev, table=table)
        self._chk_rp_bytes("seg_objects", (B, H, W), dev, keep=keep)
        for t, shape, what, dt in ((labels, (B, H, W), "labels", torch.int32), (ids, (B, H, W), "ids", torch.int32),
                                   (roots, (B, M), "roots", torch.int32), (count, (B,), "count", torch.int32),
                                   (sums, (B, M, SEG_SUMS), "sums", torch.int64)):
            self._chk_odo_vec(t, shape, f"seg_objects: {what}", dt)
            if t.device != dev:
                raise PfError(f"seg_objects: {what} must be on {dev}")
        if rows is None or cols is None or table is None or keep is None:
            raise PfError("seg_objects: only values may be None")
        nbytes = self._chk_seg_scratch("seg_objects", scratch, dev)
        self._rc(self._dll.pf_seg_objects(_ptr(labels), _ptr(values), _ptr(rows), _ptr(cols), _ptr(scratch), nbytes, _ptr(ids),
                                          _ptr(keep), _ptr(roots), _ptr(count), _ptr(table), _ptr(sums), B, Cc, H, W, M, float(min_area),
                                          self._stream(labels)), "pf_seg_objects")
        return ids, count, table

    # ---- object tracks ---------------------------------------------------
    def _chk_trk(self, what, dev, specs):
        """specs: (tensor, shape, name, dtype); every one a contiguous tensor of that dtype and shape on dev."""
        for t, shape, name, dt in specs:
            if t is None:
                raise PfError(f"{what}: {name} is required")
            self._chk_odo_vec(t, shape, f"{what}: {name}", dt)
            if t.device != dev:
                raise PfError(f"{what}: {name} must be on {dev}")

    def trk_begin(self, votes):
        """pf_trk_begin: clears votes int64 [B,M,M]."""
        self._have("pf_trk_begin")
        if votes.dim() != 3 or votes.shape[1] != votes.shape[2]:
            raise PfError(f"trk_begin: votes {tuple(votes.shape)}, expected [B,M,M]")
        self._chk_odo_vec(votes, tuple(votes.shape), "trk_begin: votes", torch.int64)
        self._rc(self._dll.pf_trk_begin(_ptr(votes), votes.shape[0], votes.shape[1], self._stream(votes)), "pf_trk_begin")
        return votes

    def trk_vote(self, prev_ids, ids, flow_prev, flow_cur, mask_prev, mask_cur, rows, votes):
        """pf_trk_vote: the pixels of prev_ids int32 [B,H,W] along flow_prev and those of ids along flow_cur (fp32 [B,2,H,W]; one may
        be None) into votes int64 [B,M,M]; mask_prev, mask_cur uint8 [B,H,W] or None; rows: seg_tables' [H,2]."""
        self._have("pf_trk_vote")
        if prev_ids.dim() != 3 or votes.dim() != 3 or votes.shape[1] != votes.shape[2]:
            raise PfError(f"trk_vote: prev_ids {tuple(prev_ids.shape)}, votes {tuple(votes.shape)}, expected [B,H,W] and [B,M,M]")
        B, H, W = prev_ids.shape
        M = votes.shape[1]
        dev = prev_ids.device
        if flow_prev is None and flow_cur is None:
            raise PfError("trk_vote: at least one flow is required")
        self._chk_trk("trk_vote", dev, ((prev_ids, (B, H, W), "prev_ids", torch.int32), (ids, (B, H, W), "ids", torch.int32),
                                        (votes, (B, M, M), "votes", torch.int64)))
        self._chk_rp_maps("trk_vote", (B, 2, H, W), dev, flow_prev=flow_prev, flow_cur=flow_cur)
        self._chk_rp_maps("trk_vote", (H, 2), dev, rows=rows)
        self._chk_rp_bytes("trk_vote", (B, H, W), dev, mask_prev=mask_prev, mask_cur=mask_cur)
        if rows is None:
            raise PfError("trk_vote: rows is required")
        self._rc(self._dll.pf_trk_vote(_ptr(prev_ids), _ptr(ids), _ptr(flow_prev), _ptr(flow_cur), _ptr(mask_prev), _ptr(mask_cur),
                                       _ptr(rows), _ptr(votes), B, H, W, M, self._stream(prev_ids)), "pf_trk_vote")
        return votes

    def trk_match(self, votes, count, sums, st_count, st_sums, st_track, st_age, st_path, next_id, track, age, origin, fate, step, path,
                  n_dir: int, min_overlap: float):
        """pf_trk_match: votes int64 [B,M,M] and the current count int32 [B], sums int64 [B,M,SEG_SUMS] against the state (st_count
        [B], st_sums [B,M,SEG_SUMS], st_track, st_age int32 [B,M], st_path fp32 [B,M], next_id int32 [B]; updated in place) into
        track, age, origin, fate int32 [B,M] and step, path fp32 [B,M]."""
        self._have("pf_trk_match")
        if votes.dim() != 3 or votes.shape[1] != votes.shape[2]:
            raise PfError(f"trk_match: votes {tuple(votes.shape)}, expected [B,M,M]")
        B, M = votes.shape[:2]
        dev = votes.device
        i32, i64, f32 = torch.int32, torch.int64, torch.float32
        self._chk_trk("trk_match", dev, (
            (votes, (B, M, M), "votes", i64), (count, (B,), "count", i32), (sums, (B, M, SEG_SUMS), "sums", i64),
            (st_count, (B,), "st_count", i32), (st_sums, (B, M, SEG_SUMS), "st_sums", i64), (st_track, (B, M), "st_track", i32),
            (st_age, (B, M), "st_age", i32), (st_path, (B, M), "st_path", f32), (next_id, (B,), "next_id", i32),
            (track, (B, M), "track", i32), (age, (B, M), "age", i32), (origin, (B, M), "origin", i32), (fate, (B, M), "fate", i32),
            (step, (B, M), "step", f32), (path, (B, M), "path", f32)))
        self._rc(self._dll.pf_trk_match(_ptr(votes), _ptr(count), _ptr(sums), _ptr(st_count), _ptr(st_sums), _ptr(st_track), _ptr(st_age),
                                        _ptr(st_path), _ptr(next_id), _ptr(track), _ptr(age), _ptr(origin), _ptr(fate), _ptr(step),
                                        _ptr(path), B, M, int(n_dir), float(min_overlap), self._stream(votes)), "pf_trk_match")
        return track, age

    def trk_paint(self, ids, track, track_map, st_ids):
        """pf_trk_paint: track_map int32 [B,H,W] = track int32 [B,M] of each pixel's id (0 where ids is 0); st_ids = ids."""
        self._have("pf_trk_paint")
        if ids.dim() != 3 or track.dim() != 2:
            raise PfError(f"trk_paint: ids {tuple(ids.shape)}, track {tuple(track.shape)}, expected [B,H,W] and [B,M]")
        B, H, W = ids.shape
        M = track.shape[1]
        i32 = torch.int32
        self._chk_trk("trk_paint", ids.device, ((ids, (B, H, W), "ids", i32), (track, (B, M), "track", i32),
                                                (track_map, (B, H, W), "track_map", i32), (st_ids, (B, H, W), "st_ids", i32)))
        self._rc(self._dll.pf_trk_paint(_ptr(ids), _ptr(track), _ptr(track_map), _ptr(st_ids), B, H, W, M, self._stream(ids)),
                 "pf_trk_paint")
        return track_map

    # ---- push-pull hole filling -----------------------------------------
    def fill_levels(self, H: int, W: int) -> int:
        self._have("pf_fill_levels")
        r = self._dll.pf_fill_levels(H, W)
        self._rc(min(r, 0), "pf_fill_levels")
        return r

    def fill_bytes(self, B: int, C_: int, H: int, W: int) -> int:
        self._have("pf_fill_bytes")
        r = self._dll.pf_fill_bytes(B, C_, H, W)
        self._rc(min(r, 0), "pf_fill_bytes")
        return r

    def _chk_fill_in(self, what, src, hole, weight):
        self._chk(src)
        if src.dim() != 4:
            raise PfError(f"{what}: src {tuple(src.shape)}, expected [B,C,H,W]")
        B, Cc, H, W = src.shape
        if hole is None:
            raise PfError(f"{what}: hole is required")
        self._chk_rp_bytes(what, (B, H, W), src.device, hole=hole)
        self._chk_rp_maps(what, (B, H, W), src.device, weight=weight)
        return B, Cc, H, W

    def fill_pushpull(self, src, hole, weight, out, empty, scratch, stage: Optional[int] = None):
        """pf_fill_pushpull: out fp32 [B,C,H,W] = src with the pixels of hole uint8 [B,H,W] (and those of weight fp32 [B,H,W] <= 0,
        when given) filled from the pyramid; empty uint8 [B] or None; scratch: fill_bytes(B, C, H, W) bytes.  out may be src.
        stage 0, 1 or 2: that stage alone (pf_fill_stage)."""
        self._have("pf_fill_pushpull" if stage is None else "pf_fill_stage")
        B, Cc, H, W = self._chk_fill_in("fill_pushpull", src, hole, weight)
        dev = src.device
        if out is None or scratch is None:
            raise PfError("fill_pushpull: out and scratch are required")
        self._chk_rp_maps("fill_pushpull", (B, Cc, H, W), dev, out=out)
        self._chk_rp_bytes("fill_pushpull", (B,), dev, empty=empty)
        self._chk_bytes(scratch, "fill_pushpull: scratch")
        need = self.fill_bytes(B, Cc, H, W)
        if scratch.device != dev or scratch.numel() * scratch.element_size() < need:
            raise PfError(f"fill_pushpull: scratch holds {scratch.numel() * scratch.element_size()} bytes on {scratch.device}, "
                          f"expected {need} on {dev}")
        if stage is None:
            self._rc(self._dll.pf_fill_pushpull(_ptr(src), _ptr(hole), _ptr(weight), _ptr(out), _ptr(empty), _ptr(scratch), B, Cc, H, W,
                                                self._stream(src)), "pf_fill_pushpull")
        else:
            self._rc(self._dll.pf_fill_stage(_ptr(src), _ptr(hole), _ptr(weight), _ptr(out), _ptr(empty), _ptr(scratch), B, Cc, H, W,
                                             int(stage), self._stream(src)), "pf_fill_stage")
        return out

    def fill_prepare(self, src, hole, weight, w0):
        """pf_fill_prepare: the level-0 weight w0 fp32 [B,H,W] of src, hole and the optional weight."""
        self._have("pf_fill_prepare")
        B, Cc, H, W = self._chk_fill_in("fill_prepare", src, hole, weight)
        if w0 is None:
            raise PfError("fill_prepare: w0 is required")
        self._chk_rp_maps("fill_prepare", (B, H, W), src.device, w0=w0)
        self._rc(self._dll.pf_fill_prepare(_ptr(src), _ptr(hole), _ptr(weight), _ptr(w0), B, Cc, H, W, self._stream(src)),
                 "pf_fill_prepare")
        return w0

    def fill_pull_level(self, fine_v, fine_w, coarse_v, coarse_w):
        """pf_fill_pull_level: (coarse_v [B,C,Hc,Wc], coarse_w [B,Hc,Wc]) from (fine_v [B,C,Hf,Wf], fine_w [B,Hf,Wf])."""
        self._have("pf_fill_pull_level")
        self._chk(fine_v)
        if fine_v.dim() != 4 or coarse_v is None or coarse_w is None or fine_w is None:
            raise PfError("fill_pull_level: fine_v is [B,C,Hf,Wf]; every map is required")
        B, Cc, Hf, Wf = fine_v.shape
        Hc, Wc = max(1, (Hf + 1) // 2), max(1, (Wf + 1) // 2)
        dev = fine_v.device
        self._chk_rp_maps("fill_pull_level", (B, Hf, Wf), dev, fine_w=fine_w)
        self._chk_rp_maps("fill_pull_level", (B, Cc, Hc, Wc), dev, coarse_v=coarse_v)
        self._chk_rp_maps("fill_pull_level", (B, Hc, Wc), dev, coarse_w=coarse_w)
        self._rc(self._dll.pf_fill_pull_level(_ptr(fine_v), _ptr(fine_w), _ptr(coarse_v), _ptr(coarse_w), B, Cc, Hf, Wf,
                                              self._stream(fine_v)), "pf_fill_pull_level")

    def fill_push_level(self, coarse_u, fine_v, fine_w, out, empty=None):
        """pf_fill_push_level: out [B,C,Hf,Wf] (may be fine_v) from the filled level above coarse_u [B,C,Hc,Wc] (None at the 1 x 1
        level: the apex step, which may write empty uint8 [B])."""
        self._have("pf_fill_push_level")
        self._chk(fine_v)
        if fine_v.dim() != 4 or fine_w is None or out is None:
            raise PfError("fill_push_level: fine_v is [B,C,Hf,Wf]; fine_w and out are required")
        B, Cc, Hf, Wf = fine_v.shape
        Hc, Wc = max(1, (Hf + 1) // 2), max(1, (Wf + 1) // 2)
        dev = fine_v.device
        self._chk_rp_maps("fill_push_level", (B, Hf, Wf), dev, fine_w=fine_w)
        self._chk_rp_maps("fill_push_level", (B, Cc, Hf, Wf), dev, out=out)
        self._chk_rp_maps("fill_push_level", (B, Cc, Hc, Wc), dev, coarse_u=coarse_u)
        self._chk_rp_bytes("fill_push_level", (B,), dev, empty=empty)
        self._rc(self._dll.pf_fill_push_level(_ptr(coarse_u), _ptr(fine_v), _ptr(fine_w), _ptr(out), _ptr(empty), B, Cc, Hf, Wf,
                                              self._stream(fine_v)), "pf_fill_push_level")
        return out

    # ---- self-supervised criterion --------------------------------------
    def selfsup_loss_batch(self, preds, image1, image2, weight, mask, i_weights, grads, partials, z: float, w_photo: float,
                           w_smooth: float, eps_photo: float, eps_smooth: float, edge_lambda: float, max_flow: float, blocks: int = 0):
        """pf_selfsup_loss_batch: the n <= 32 predictions preds[i] fp32 [B,2,H,W] against image1 / image2 fp32 [B,3,H,W], weight fp32
        [H*W], mask uint8 [B,H,W] or None; grads: None, or a list of n tensors like preds[i] (single entries may be None);
        partials float64 [n, B, nblk, 4]; z = B * sum weight; blocks: workgroups of the launch (0: one per chunk and image)."""
        self._have("pf_selfsup_loss_batch")
        n = len(preds)
        if not 1 <= n <= SS_MAX:
            raise PfError(f"selfsup_loss_batch: {n} predictions, expected 1..{SS_MAX}")
        self._chk(image1, image2, weight, *preds, *(g for g in (grads or ()) if g is not None))
        if image1.dim() != 4 or image1.shape[1] != 3 or image2.shape != image1.shape:
            raise PfError(f"selfsup_loss_batch: image1 {tuple(image1.shape)} / image2 {tuple(image2.shape)}, expected [B,3,H,W] twice")
        B, _, H, W = image1.shape
        want = (B, 2, H, W)
        if any(tuple(p.shape) != want for p in preds) or weight.numel() != H * W \
                or (grads is not None and (len(grads) != n or any(g is not None and tuple(g.shape) != want for g in grads))):
            raise PfError(f"selfsup_loss_batch: predictions and gradients must be {want}, weight must hold {H * W} values")
        self._chk_mask(mask, (B, H, W), "selfsup_loss_batch: mask")
        if partials.dtype != torch.float64 or partials.dim() != 4 or tuple(partials.shape[:2]) != (n, B) or partials.shape[3] != SS_SUMS \
                or not partials.is_contiguous():
            raise PfError(f"selfsup_loss_batch: partials must be contiguous float64 [n, B, nblk, {SS_SUMS}]")
        others = [image2, weight, mask, partials, *preds, *(g for g in (grads or ()) if g is not None)]
        if any(t is not None and t.device != image1.device for t in others):
            raise PfError(f"selfsup_loss_batch: every tensor must be on {image1.device}")
        pa = (C.c_void_p * n)(*[p.data_ptr() for p in preds])
        ga = (C.c_void_p * n)(*[None if g is None else g.data_ptr() for g in grads]) if grads is not None else None
        wa = (C.c_float * n)(*[float(w) for w in i_weights])
        self._rc(self._dll.pf_selfsup_loss_batch(pa, _ptr(image1), _ptr(image2), _ptr(weight), _ptr(mask), wa, ga,
                                                 C.c_void_p(partials.data_ptr()), partials.shape[2], n, B, H, W, float(w_photo),
                                                 float(w_smooth), float(eps_photo), float(eps_smooth), float(edge_lambda),
                                                 float(max_flow), float(z), int(blocks), self._stream(image1)), "pf_selfsup_loss_batch")

    def masked_mean(self, x, mask, out, scratch):
        """out[b] = mean of x[b] over mask[b] == 0 (mask None: everything); scratch: >= 1024 * B bytes."""
        self._chk(x, out)
        self._chk_bytes(scratch, "masked_mean: scratch")
        B = x.shape[0]
        N = x[0].numel()
        if mask is not None:
            self._chk_bytes(mask, "masked_mean: mask", torch.uint8)
            if mask.numel() != B * N:
                raise PfError("masked_mean: mask and x differ in size")
        if out.numel() != B:
            raise PfError("masked_mean: out must hold one value per image")
        self._rc(self._dll.pf_masked_mean(_ptr(x), _ptr(mask), _ptr(out), _ptr(scratch), scratch.numel() * scratch.element_size(),
                                          B, N, self._stream(x)), "pf_masked_mean")
        return out

    def to_nchw(self, x, off_in, c, out):
        self._chk(x, out)
        B = out.shape[0]
        N = out.shape[2] * out.shape[3]
        self._rc(self._dll.pf_to_nchw(_ptr(x), x.shape[-1], off_in, c, _ptr(out), B, N,
                                      self._stream(x)), "pf_to_nchw")
        return out


_cached: Optional[PfLib] = None


_WEIGHTS_EPOCH = [0]


def weights_epoch() -> int:
    """Counter of in-place parameter updates made through raw pointers (pf_adamw_step): torch's per-tensor
    version counters do not see those, so every cache of packed weights keys on this as well."""
    return _WEIGHTS_EPOCH[0]


def bump_weights_epoch() -> None:
    _WEIGHTS_EPOCH[0] += 1


def load() -> PfLib:
    """The product's library handle (built in-tree under prior-flow_amd/lib/)."""
    global _cached
    if _cached is None:
        _cached = PfLib(LIB_PATH, require_cuda=True)
    return _cached
