"""ctypes binding of csrc/libvitseg.so (C ABI: include/vitseg.h).

There is NO CPU fallback: if the HIP library is missing or fails to load, importing
this module's `lib()` raises -- the product path must never silently run elsewhere.
"""
from __future__ import annotations

import ctypes as C
import functools
import os

from .config import ViTSegConfig

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libvitseg.so")

OK, EINVAL, ESHAPE, EWORKSPACE, EHIP = 0, -1, -2, -3, -4
F32, BF16, F16, F32X3 = 0, 1, 2, 3
BUF_TOKENS, BUF_LOWRES = 0, 1

# enum vitseg_tensor
(T_CLS, T_POS, T_PATCH_W, T_PATCH_B, T_LN1_W, T_LN1_B, T_WQKV, T_BQKV, T_WO, T_BO, T_LN2_W, T_LN2_B,
 T_W1, T_B1, T_W2, T_B2, T_LNF_W, T_LNF_B, T_HEAD0_W, T_HEAD0_B, T_HEAD2_W, T_HEAD2_B, T_COUNT) = range(23)

SKELETON_AUTO, SKELETON_RESIDENT, SKELETON_GLOBAL = 0, 1, 2   # the `route` argument
AUGMENT_CONSTANT, AUGMENT_EDGE = 0, 1      # enum vitseg_augment_border
AUGMENT_U8_NHWC, AUGMENT_F32_NCHW = 0, 1   # enum vitseg_augment_format
TTA_LOGITS, TTA_PROBS = 0, 1   # the `mode` argument of vitseg_tta_blend
CLEAN_STATS = ("regions_removed", "pixels_removed", "holes_filled", "pixels_filled", "holes_mixed", "holes_over_area")
MATCH_STATS = ("n_gt", "n_pred", "tp", "gt_found", "pred_confirmed", "sum_q", "sum_i", "sum_u")
PROPS_FIELDS = 20   # include/vitseg.h VITSEG_PROPS_FIELDS
CONF_PROB, CONF_MARGIN = 0, 1   # enum vitseg_conf_kind
# enum vitseg_slices_path
SLICES_WHOLE_F32, SLICES_WHOLE_H16, SLICES_THIN_F32, SLICES_THIN_H16, SLICES_WGRAD_F32, SLICES_WGRAD_BF16_TT, SLICES_WGRAD_BF16_P8 = range(7)
VERSION = 110   # include/vitseg.h VITSEG_VERSION this binding was written against
KERNEL_KINDS = ["gemm_bias", "gemm_gelu", "gemm_resadd", "gemm_patch", "gemm_conv3", "attention", "layernorm",
                "head1x1", "upsample", "train_gemm_fwd", "train_dgrad", "train_wgrad", "train_attn_fwd", "train_attn_bwd"]


class CCEOptions(C.Structure):
    """struct vitseg_ce_options (include/vitseg.h)."""
    _fields_ = [("has_ignore_index", C.c_int32), ("reserved", C.c_int32), ("ignore_index", C.c_int64),
                ("class_weight", C.c_void_p), ("label_smoothing", C.c_float), ("scratch", C.c_void_p),
                ("scratch_bytes", C.c_size_t)]


class CDiceOptions(C.Structure):
    """struct vitseg_dice_options (include/vitseg.h)."""
    _fields_ = [("ce_weight", C.c_float), ("dice_weight", C.c_float), ("smooth", C.c_float),
                ("include_background", C.c_int32), ("scratch", C.c_void_p), ("scratch_bytes", C.c_size_t)]


class CAugmentMask(C.Structure):
    """struct vitseg_augment_mask (include/vitseg.h)."""
    _fields_ = [("src", C.c_void_p), ("matrix", C.c_void_p), ("out", C.c_void_p), ("src_is_i64", C.c_int32),
                ("out_is_i64", C.c_int32), ("h", C.c_int32), ("w", C.c_int32), ("oh", C.c_int32), ("ow", C.c_int32)]


class CTTAView(C.Structure):
    """struct vitseg_tta_view (include/vitseg.h)."""
    _fields_ = [("lowres", C.c_void_p), ("g", C.c_int32), ("op", C.c_int32), ("weight", C.c_float)]


class CConfig(C.Structure):
    _fields_ = [("num_classes", C.c_int32), ("patch_size", C.c_int32), ("hidden_size", C.c_int32),
                ("num_layers", C.c_int32), ("num_heads", C.c_int32), ("image_size", C.c_int32),
                ("intermediate_size", C.c_int32), ("num_channels", C.c_int32), ("layer_norm_eps", C.c_float)]

    @classmethod
    def from_config(cls, cfg: ViTSegConfig) -> "CConfig":
        return cls(cfg.num_classes, cfg.patch_size, cfg.hidden_size, cfg.num_hidden_layers,
                   cfg.num_attention_heads, cfg.image_size, cfg.intermediate_size, cfg.num_channels,
                   cfg.layer_norm_eps)


# short names, so that a row of SIGNATURES stays on one line
vp, sz, i32, f32, u32, u64, i64, ll, cstr = (C.c_void_p, C.c_size_t, C.c_int, C.c_float, C.c_uint32, C.c_uint64, C.c_int64,
                                             C.c_longlong, C.c_char_p)
psz, pint, pi32, pi64, pll, pf32, pdbl = (C.POINTER(t) for t in (sz, i32, C.c_int32, i64, ll, f32, C.c_double))
pcfg, popt, pdice, pmask, pview = (C.POINTER(t) for t in (CConfig, CCEOptions, CDiceOptions, CAugmentMask, CTTAView))

# Every entry point include/vitseg.h declares, stated once: group -> (required at load, the words after "built before" in
# `symbol`'s error, [(name, restype, argtypes)]).  `lib()` binds from it, every list of names below is read off it, and
# tests/test_binding_cpu.py compares it with the header.  A group that is not required is bound where the loaded library has
# it, so that a library built before a feature still serves everything else; that feature alone raises a "rebuild" error.
SIGNATURES = {
    "core": (True, None, [
        ("vitseg_version", i32, []),
        ("vitseg_last_error", cstr, []),
        ("vitseg_set_option", i32, [cstr, ll]),
        ("vitseg_get_option", i32, [cstr, pll]),
        ("vitseg_param_count", i32, [pcfg, psz]),
        ("vitseg_param_offset", i32, [pcfg, i32, i32, psz, psz]),
        ("vitseg_cast_params_bf16", i32, [vp, vp, sz, vp]),
        ("vitseg_query_workspace", i32, [pcfg, i32, i32, psz]),
        ("vitseg_workspace_offset", i32, [pcfg, i32, i32, i32, psz, psz]),
        ("vitseg_forward", i32, [pcfg, vp, vp, vp, i32, i32, vp, vp, vp, sz, vp]),
        ("vitseg_op_layernorm_f32", i32, [vp, vp, vp, vp, i32, i32, f32, vp]),
        ("vitseg_op_linear_f32", i32, [vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]),
        ("vitseg_op_attention_f32", i32, [vp, vp, i32, i32, i32, vp]),
        ("vitseg_op_upsample_argmax", i32, [vp, vp, vp, i32, i32, i32, i32, vp]),
        ("vitseg_op_upsample_bwd", i32, [vp, vp, i32, i32, i32, i32, vp]),
        ("vitseg_profile_enable", i32, [i32]),
        ("vitseg_profile_collect", i32, [i32, pdbl, pi64, pdbl]),
        ("vitseg_op_linear_bf16", i32, [vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]),
        ("vitseg_op_attention_bf16", i32, [vp, vp, i32, i32, i32, vp]),
        ("vitseg_ce_scratch_bytes", sz, [i32, i32]),
        ("vitseg_ce_loss", i32, [vp, vp, i32, vp, vp, vp, i32, i32, i32, i32, vp]),
        ("vitseg_train_workspace", i32, [pcfg, i32, i32, psz]),
        ("vitseg_forward_train", i32, [pcfg, vp, vp, vp, i32, i32, f32, u64, vp, vp, sz, vp]),
        ("vitseg_backward", i32, [pcfg, vp, vp, vp, i32, i32, f32, u64, vp, i32, vp, vp, vp, f32, vp, vp, sz, vp]),
        ("vitseg_adam_step", i32, [vp, vp, vp, vp, sz, f32, f32, f32, f32, i32, f32, vp]),
        ("vitseg_grad_bucket_count", i32, [pcfg]),
        ("vitseg_grad_bucket_range", i32, [pcfg, i32, psz, psz]),
        ("vitseg_cast_params_f16", i32, [vp, vp, sz, vp]),
        ("vitseg_op_linear_f16", i32, [vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]),
        ("vitseg_op_attention_f16", i32, [vp, vp, i32, i32, i32, vp]),
        ("vitseg_op_linear_f32x3", i32, [vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]),
        ("vitseg_op_attention_f32x3", i32, [vp, vp, i32, i32, i32, vp]),
        ("vitseg_cast_params_split", i32, [vp, vp, sz, vp]),
        ("vitseg_resize_taps", i32, [i32, i32]),
        ("vitseg_resize_coeffs", i32, [i32, i32, vp, vp]),
        ("vitseg_nearest_index", i32, [i32, i32, i32, vp]),
        ("vitseg_preprocess_u8", i32, [vp, i32, i32, i32, i32, vp, vp, i32, vp, vp, i32, i32, i32, vp, vp, vp]),
        ("vitseg_resize_nearest_u8", i32, [vp, i32, i32, i32, vp, vp, i32, i32, vp, i32, vp, vp]),
        ("vitseg_eval_counts", i32, [vp, vp, i32, i32, i32, i32, vp, vp, vp, vp]),
        ("vitseg_paed_scratch_bytes", sz, [i32, i32, i32, i32]),
        ("vitseg_paed_multiclass_loss", i32, [vp, vp, i32, i32, i32, i32, i32, f32, i32, vp, vp, vp, vp]),
        ("vitseg_op_gemm_f32", i32, [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp]),
        ("vitseg_op_attention_bwd_f32", i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, vp]),
        ("vitseg_op_layernorm_bwd_f32", i32, [vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, f32, vp]),
        ("vitseg_op_linear_h16_ex", i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, sz, f32, u32, u32, vp, vp, vp]),
        ("vitseg_op_wgrad_bf16", i32, [vp, vp, vp, vp, vp, i32, i32, i32, vp]),
        ("vitseg_op_wgrad_bf16_scratch_floats", sz, [i32, i32, i32]),
        ("vitseg_op_attention_bwd_bf16", i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, f32, u32, u32, vp, vp, vp]),
        ("vitseg_attention_dropmask_bytes", sz, [i32, i32, i32]),
        ("vitseg_attention_bwd_scratch_floats", sz, [i32, i32, i32]),
        ("vitseg_op_colsum_scratch_floats", sz, [i32, i32]),
        ("vitseg_paed_binary_scratch_bytes", sz, [i32, i32, i32]),
        ("vitseg_paed_binary_loss", i32, [vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp]),
        ("vitseg_op_linear_f32_ex", i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, f32, u32, u32, vp]),
        ("vitseg_resize_nearest_i64", i32, [vp, i32, i32, i32, vp, vp, i32, i32, i32, vp, vp]),
        ("vitseg_small_splits", i32, [i32, i32]),
        ("vitseg_op_linear_f32_small", i32, [vp, vp, vp, vp, i32, i32, i32, i32, vp]),
        ("vitseg_op_linear_resln_f32_small", i32, [vp, vp, vp, vp, vp, vp, vp, vp, sz, i32, i32, i32, f32, vp]),
        ("vitseg_op_attention_f32_small", i32, [vp, vp, i32, i32, i32, vp]),
        ("vitseg_op_attention_bwd_f32_small", i32, [vp, vp, vp, vp, vp, i32, i32, i32, f32, u32, u32, vp]),
        ("vitseg_op_linear_h16_small", i32, [vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, sz, vp]),
        ("vitseg_op_attention_h16_small", i32, [vp, vp, i32, i32, i32, i32, vp]),
        ("vitseg_forward_route", i32, [pcfg, i32, i32]),
        ("vitseg_op_layernorm_bwd_f32_small", i32, [vp, vp, vp, sz, i32, vp, vp, vp, vp, vp, i32, i32, f32, vp, vp, f32, u32, u32, vp]),
        ("vitseg_dbg_linear_f32_small", i32, [vp, vp, vp, vp, i32, i32, i32, i32, vp, i32, vp]),
        ("vitseg_adamw_step", i32, [vp, vp, vp, vp, sz, f32, f32, f32, f32, f32, i32, f32, vp]),
        ("vitseg_op_dgrad_f32_small", i32, [vp, vp, vp, vp, vp, sz, i32, i32, i32, i32, vp]),
        ("vitseg_op_wgrad_f32_small", i32, [vp, vp, vp, i32, i32, i32, vp]),
        ("vitseg_op_layernorm_bwd_scratch_floats", sz, [i32, i32]),
    ]),
    # other input sizes (interpolated position embeddings)
    "at": (False, "interpolated position embeddings", [
        ("vitseg_query_workspace_at", i32, [pcfg, i32, i32, i32, psz]),
        ("vitseg_workspace_offset_at", i32, [pcfg, i32, i32, i32, i32, psz, psz]),
        ("vitseg_forward_at", i32, [pcfg, i32, vp, vp, vp, i32, i32, vp, vp, vp, sz, vp]),
        ("vitseg_train_workspace_at", i32, [pcfg, i32, i32, i32, psz]),
        ("vitseg_forward_train_at", i32, [pcfg, i32, vp, vp, vp, i32, i32, f32, u64, vp, vp, sz, vp]),
        ("vitseg_backward_at", i32, [pcfg, i32, vp, vp, vp, i32, i32, f32, u64, vp, i32, vp, vp, vp, f32, vp, vp, sz, vp]),
        ("vitseg_pos_interp", i32, [vp, vp, i32, i32, i32, vp]),
        ("vitseg_pos_interp_bwd", i32, [vp, vp, vp, i32, i32, i32, vp]),
    ]),
    # connected regions of class masks and their boxes (regions.py)
    "region": (False, "connected regions", [
        ("vitseg_regions_scratch_bytes", sz, [i32, i32, i32]),
        ("vitseg_regions", i32, [vp, i32, i32, i32, i32, i32, vp, vp, i32, vp, vp, sz, vp]),
    ]),
    # exact distance transforms and the signed-distance targets of binary masks (sdf.py)
    "sdf": (False, "distance transforms", [
        ("vitseg_sdf_scratch_bytes", sz, [i32, i32, i32]),
        ("vitseg_sdf", i32, [vp, i32, i32, i32, i32, vp, vp, vp, sz, vp]),
    ]),
    # the K-sliced GEMM paths, one entry each, and the router's slice counts (tests/test_splitk_cpu.py, tests/test_gpu_splitk.py)
    "splitk": (False, "the split-K entry points", [
        ("vitseg_op_linear_f32_thin", i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, sz, f32, u32, u32, vp]),
        ("vitseg_op_wgrad_f32_scratch_floats", sz, [i32, i32, i32]),
        ("vitseg_op_wgrad_f32", i32, [vp, vp, vp, vp, i32, i32, i32, vp]),
        ("vitseg_dbg_gemm_slices", i32, [i32, i32, i32, i32]),
    ]),
    # the fused cross-entropy with ignore_index / class weights / label smoothing (model.ce_loss)
    "ce_opts": (False, "the cross-entropy options", [
        ("vitseg_ce_options_scratch_bytes", sz, [i32, i32]),
        ("vitseg_ce_loss_opts", i32, [vp, vp, i32, vp, vp, vp, i32, i32, i32, i32, popt, f32, vp]),
        ("vitseg_backward_opts", i32, [pcfg, i32, vp, vp, vp, i32, i32, f32, u64, vp, i32, vp, vp, vp, f32, vp, vp, sz, vp, popt]),
    ]),
    # the embedding, seg-head and training helper kernels, one entry per production launch (csrc/op_helpers.hip,
    # tests/test_gpu_helpers.py)
    "helper": (False, "the helper-kernel entry points", [
        ("vitseg_op_patch_embed_f32", i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp]),
        ("vitseg_op_conv3x3_f32", i32, [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp]),
        ("vitseg_op_conv3x3_h16", i32, [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp]),
        ("vitseg_op_head1x1", i32, [vp, vp, vp, vp, i32, i32, i32, vp]),
        ("vitseg_op_head1x1_bwd_scratch_floats", sz, [i32, i32, i32]),
        ("vitseg_op_head1x1_bwd", i32, [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp]),
        ("vitseg_op_colsum", i32, [vp, i32, vp, vp, i32, i32, i32, vp]),
        ("vitseg_op_embed_bwd", i32, [vp, vp, vp, i32, i32, i32, vp]),
        ("vitseg_op_im2col3x3", i32, [vp, i32, vp, i32, i32, i32, vp]),
        ("vitseg_op_im2col3x3_bf16", i32, [vp, vp, i32, i32, i32, vp]),
        ("vitseg_op_im2col_patch", i32, [vp, vp, i32, i32, i32, i32, vp]),
        ("vitseg_op_im2col_patch_bf16", i32, [vp, vp, i32, i32, i32, i32, vp]),
        ("vitseg_op_conv_dgrad_weight", i32, [vp, vp, i32, vp]),
        ("vitseg_op_transpose_bf16", i32, [vp, vp, i32, i32, i32, i32, vp]),
        ("vitseg_op_transpose_layers_bf16", i32, [vp, vp, psz, pint, pint, sz, i32, vp]),
        ("vitseg_op_dropout_rows", i32, [vp, vp, i32, i32, i32, f32, u32, u32, vp]),
        ("vitseg_op_layernorm_h16", i32, [vp, vp, vp, vp, i32, i32, f32, i32, vp]),
        ("vitseg_op_layernorm_bwd_bf16", i32, [vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, f32, vp, vp, f32, u32, u32, vp]),
    ]),
    # sliding-window inference (model.predict_mask_windowed): the window grid, the tile gather, the forward that stops at the
    # low-res head output and the overlapping-tile blend
    "window": (False, "sliding-window inference", [
        ("vitseg_window_count", i32, [i32, i32, i32]),
        ("vitseg_window_origins", i32, [i32, i32, i32, vp]),
        ("vitseg_window_gather", i32, [vp, i32, i32, i32, i32, i32, vp, i32, vp, i32, i32, i32, vp, vp]),
        ("vitseg_forward_lowres", i32, [pcfg, i32, vp, vp, vp, i32, i32, vp, vp, sz, vp]),
        ("vitseg_window_blend", i32, [vp, vp, i32, vp, i32, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp]),
    ]),
    # CE + soft Dice in one fused loss (model.ce_dice_loss)
    "dice": (False, "the CE + Dice loss", [
        ("vitseg_dice_options_scratch_bytes", sz, [i32, i32, i32]),
        ("vitseg_ce_dice_loss", i32, [vp, vp, i32, vp, vp, vp, i32, i32, i32, i32, popt, pdice, f32, vp]),
        ("vitseg_backward_dice", i32, [pcfg, i32, vp, vp, vp, i32, i32, f32, u64, vp, i32, vp, vp, vp, f32, vp, vp, sz, vp, popt,
                                       pdice, vp]),
    ]),
    # boundary-distance statistics of class maps: PAED, Hausdorff, HD95, ASSD (metrics.Evaluator.distance_metrics)
    "distance": (False, "the boundary-distance metrics", [
        ("vitseg_distance_scratch_bytes", sz, [i32, i32, i32]),
        ("vitseg_distance_stats", i32, [vp, vp, i32, i32, i32, pi32, i32, i32, i32, i32, vp, vp, vp, sz, vp]),
    ]),
    # skeletons by Zhang-Suen thinning and the crack statistics on them: clDice, length, width (skeleton.py,
    # metrics.Evaluator.crack_metrics)
    "skeleton": (False, "the skeletons", [
        ("vitseg_skeleton_scratch_bytes", sz, [i32, i32, i32, i32]),
        ("vitseg_skeleton", i32, [vp, i32, i32, i32, i32, vp, vp, vp, sz, vp]),
        ("vitseg_skeleton_stats_scratch_bytes", sz, [i32, i32, i32, i32]),
        ("vitseg_skeleton_stats", i32, [vp, vp, i32, i32, i32, pi32, i32, i32, vp, vp, vp, sz, vp]),
    ]),
    # training augmentation: the paired affine warp + colour jitter launch and its host-side matrix composer (augment.py)
    "augment": (False, "the training augmentation", [
        ("vitseg_augment_matrix", i32, [vp, i32, i32, i32, i32, vp]),   # (double[6] in, int64[6] out)
        ("vitseg_augment", i32, [vp, i32, i32, i32, i32, i32, i32, vp, vp, vp, pmask, i32, i32, pf32, i64, vp]),
    ]),
    # test-time augmentation (model.predict_mask_tta): the exact affine of a flip / quarter-turn view and the launch that
    # merges the views' low-res maps
    "tta": (False, "test-time augmentation", [
        ("vitseg_tta_affine", i32, [i32, vp]),   # (double[6] out)
        ("vitseg_tta_blend", i32, [pview, i32, i32, i32, i32, i32, vp, vp, vp]),
    ]),
    # mask clean-up: regions below a minimum area out, enclosed holes filled (clean.py)
    "clean": (False, "the mask clean-up", [
        ("vitseg_clean_scratch_bytes", sz, [i32, i32, i32]),
        ("vitseg_clean_mask", i32, [vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp, sz, vp]),
    ]),
    # region-level detection statistics: predicted regions matched against the true ones, PQ (metrics.Evaluator.region_metrics)
    "match": (False, "the region matching", [
        ("vitseg_region_match_scratch_bytes", sz, [i32, i32, i32]),
        ("vitseg_region_match", i32, [vp, vp, i32, i32, i32, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, sz, vp]),
    ]),
    # per-region measurements: moments, perimeter, frame contact, per-region skeleton length and widths (regions.region_props)
    "props": (False, "the per-region measurements", [
        ("vitseg_region_props_scratch_bytes", sz, [i32, i32, i32, i32, i32]),
        ("vitseg_region_props", i32, [vp, i32, i32, i32, i32, i32, pi32, i32, i32, vp, vp, i32, vp, vp, sz, vp]),
    ]),
    # confidence of a stated mask: per-pixel scores, per-region score rows, calibration histogram (confidence.py)
    "confidence": (False, "the confidence scores", [
        ("vitseg_confidence", i32, [vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, i32, i32, vp, i32, vp, i32, vp]),
    ]),
}
_WHAT = {name: what for _, what, rows in SIGNATURES.values() for name, _, _ in rows}

_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -m visiontransformer_amd.build` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback for this path.")
        l = C.CDLL(LIB_PATH)
        for required, _, rows in SIGNATURES.values():
            for name, restype, argtypes in rows:
                fn = getattr(l, name) if required else getattr(l, name, None)   # AttributeError: the build is stale
                if fn is not None:
                    fn.restype = restype
                    fn.argtypes = argtypes
        if l.vitseg_version() != VERSION:   # argument lists changed between versions: a stale .so would misread them
            raise RuntimeError(f"{LIB_PATH} is version {l.vitseg_version()}, this binding expects {VERSION}: rebuild it "
                               "(python -m visiontransformer_amd.build)")
        _lib = l
    return _lib


def symbol(name: str, what: str = None):
    """The bound entry point `name`, or a RuntimeError naming the rebuild when the loaded library predates it.  `what`: the
    feature to name for a `name` that SIGNATURES does not know."""
    fn = getattr(lib(), name, None)
    if fn is None:
        what = _WHAT.get(name) or what or "this entry point"
        raise RuntimeError(f"{LIB_PATH} has no {name} (built before {what}): rebuild it (python -m visiontransformer_amd.build)")
    return fn


def _public(group: str):
    """What callers outside the package know a group by: the list of its names and `symbol` carrying the group's words."""
    _, what, rows = SIGNATURES[group]
    return [name for name, _, _ in rows], functools.partial(symbol, what=what)


AT_EXPORTS, at_symbol = _public("at")
REGION_EXPORTS, region_symbol = _public("region")
SDF_EXPORTS, sdf_symbol = _public("sdf")
SPLITK_EXPORTS, splitk_symbol = _public("splitk")
CE_OPTS_EXPORTS, ce_opts_symbol = _public("ce_opts")
HELPER_EXPORTS, helper_symbol = _public("helper")
WINDOW_EXPORTS, window_symbol = _public("window")
DICE_EXPORTS, dice_symbol = _public("dice")
DISTANCE_EXPORTS, distance_symbol = _public("distance")
SKELETON_EXPORTS, skeleton_symbol = _public("skeleton")
AUGMENT_EXPORTS, augment_symbol = _public("augment")
TTA_EXPORTS, tta_symbol = _public("tta")
CLEAN_EXPORTS, clean_symbol = _public("clean")
MATCH_EXPORTS, match_symbol = _public("match")
PROPS_EXPORTS, props_symbol = _public("props")
CONFIDENCE_EXPORTS, confidence_symbol = _public("confidence")
_LATE_EXPORTS = [name for required, _, rows in SIGNATURES.values() if not required for name, _, _ in rows]
EXPORTS = list(_WHAT)   # every symbol include/vitseg.h declares


def augment_matrix(affine, src_hw, dst_hw) -> list:
    """The Q16 int64 matrix (six entries) of one normalised 2x3 affine for one (source, output) size pair
    (vitseg_augment_matrix); ValueError for an extent outside 1..16384 or an entry past the kernel's clamp bounds."""
    a = (C.c_double * 6)(*[float(v) for v in affine])
    out = (C.c_int64 * 6)()
    check(symbol("vitseg_augment_matrix")(a, int(src_hw[0]), int(src_hw[1]), int(dst_hw[0]), int(dst_hw[1]), out))
    return list(out)


def tta_affine(op: int) -> list:
    """The normalised 2x3 affine (six doubles) of view(., op) for `augment_matrix` (vitseg_tta_affine); ValueError for an
    op outside 0..7."""
    out = (C.c_double * 6)()
    if symbol("vitseg_tta_affine")(int(op), out):
        raise ValueError(lib().vitseg_last_error().decode(errors="replace"))
    return list(out)


def window_origins(extent: int, S: int, stride: int) -> list:
    """Origins of the windows along one axis (vitseg_window_origins): i * stride, the last one shifted back to end at the edge.
    ValueError for an extent shorter than the window, a stride outside 1..S or an extent above 16384."""
    n = int(symbol("vitseg_window_count")(int(extent), int(S), int(stride)))
    if n < 0:
        check(n)
    out = (C.c_int32 * n)()
    check(symbol("vitseg_window_origins")(int(extent), int(S), int(stride), out))
    return list(out)


def gemm_slices(path: int, M: int, N: int, K: int) -> int:
    """K slices of a GEMM with a dense [M, N] output on one of the router's sliced paths (SLICES_*); 0: the path does not apply."""
    return int(symbol("vitseg_dbg_gemm_slices")(path, M, N, K))


def _native(cfg: ViTSegConfig, image_size) -> bool:
    return image_size is None or int(image_size) == cfg.image_size


def check(rc: int) -> None:
    """Maps C status codes to the exception types the reference raises
    (ValueError for shapes the reference rejects, modeling_vit.py:63-68,152-156)."""
    if rc == OK:
        return
    msg = lib().vitseg_last_error().decode(errors="replace")
    if rc == ESHAPE:
        raise ValueError(msg)
    raise RuntimeError(f"libvitseg error {rc}: {msg}")


def set_option(name: str, value: int) -> None:
    """Dispatcher switch (include/vitseg.h vitseg_set_option): e.g. set_option("no_f32p", 1)."""
    check(lib().vitseg_set_option(name.encode(), int(value)))


def get_option(name: str) -> int:
    v = C.c_longlong()
    check(lib().vitseg_get_option(name.encode(), C.byref(v)))
    return int(v.value)


class option:
    """`with _lib.option("no_p8", 1): ...` -- the switch is restored on exit."""

    def __init__(self, name: str, value: int):
        self.name, self.value = name, value

    def __enter__(self):
        self.old = get_option(self.name)
        set_option(self.name, self.value)
        return self

    def __exit__(self, *exc):
        set_option(self.name, self.old)
        return False


def param_count(cfg: ViTSegConfig) -> int:
    n = C.c_size_t()
    check(lib().vitseg_param_count(C.byref(CConfig.from_config(cfg)), C.byref(n)))
    return n.value


def param_offset(cfg: ViTSegConfig, tensor: int, layer: int = 0):
    off, n = C.c_size_t(), C.c_size_t()
    check(lib().vitseg_param_offset(C.byref(CConfig.from_config(cfg)), tensor, layer, C.byref(off), C.byref(n)))
    return off.value, n.value


def query_workspace(cfg: ViTSegConfig, batch: int, precision: int, image_size=None) -> int:
    """Bytes of the forward workspace; `image_size`: the input's side when it differs from cfg's (vitseg_query_workspace_at)."""
    n = C.c_size_t()
    if _native(cfg, image_size):
        check(lib().vitseg_query_workspace(C.byref(CConfig.from_config(cfg)), batch, precision, C.byref(n)))
    else:
        check(symbol("vitseg_query_workspace_at")(C.byref(CConfig.from_config(cfg)), int(image_size), batch, precision,
                                                  C.byref(n)))
    return n.value


def forward_route(cfg: ViTSegConfig, batch: int, precision: int, image_size=None) -> str:
    """"small" (the small-batch route of csrc/small.hpp) or "large": which kernels vitseg_forward takes for this call.  The
    route depends on the activations only, so an input of another size asks with cfg at that size."""
    c = CConfig.from_config(cfg)
    if not _native(cfg, image_size):
        c.image_size = int(image_size)
    rc = lib().vitseg_forward_route(C.byref(c), batch, precision)
    if rc < 0:
        check(rc)
    return "small" if rc == 1 else "large"


def workspace_offset(cfg: ViTSegConfig, batch: int, precision: int, buffer: int, image_size=None):
    off, n = C.c_size_t(), C.c_size_t()
    if _native(cfg, image_size):
        check(lib().vitseg_workspace_offset(C.byref(CConfig.from_config(cfg)), batch, precision, buffer,
                                            C.byref(off), C.byref(n)))
    else:
        check(symbol("vitseg_workspace_offset_at")(C.byref(CConfig.from_config(cfg)), int(image_size), batch, precision,
                                                   buffer, C.byref(off), C.byref(n)))
    return off.value, n.value


def train_workspace(cfg: ViTSegConfig, batch: int, precision: int, image_size=None) -> int:
    n = C.c_size_t()
    if _native(cfg, image_size):
        check(lib().vitseg_train_workspace(C.byref(CConfig.from_config(cfg)), batch, precision, C.byref(n)))
    else:
        check(symbol("vitseg_train_workspace_at")(C.byref(CConfig.from_config(cfg)), int(image_size), batch, precision,
                                                  C.byref(n)))
    return n.value


def grad_buckets(cfg: ViTSegConfig) -> list:
    """[(offset_floats, n_floats)] of the gradient arena in the order vitseg_backward finishes them
    (0 = final norm + seg_head, 1 .. L = layers L-1 .. 0, L + 1 = embeddings)."""
    c = CConfig.from_config(cfg)
    n = lib().vitseg_grad_bucket_count(C.byref(c))
    if n < 0:
        check(n)
    out = []
    for i in range(n):
        off, cnt = C.c_size_t(), C.c_size_t()
        check(lib().vitseg_grad_bucket_range(C.byref(c), i, C.byref(off), C.byref(cnt)))
        out.append((off.value, cnt.value))
    return out


def profile_enable(on: bool) -> None:
    check(lib().vitseg_profile_enable(1 if on else 0))


def profile_collect() -> dict:
    """kind -> dict(ms, launches, work) for every kernel kind recorded since profile_enable(True)."""
    out = {}
    for i, name in enumerate(KERNEL_KINDS):
        ms, n, w = C.c_double(), C.c_int64(), C.c_double()
        check(lib().vitseg_profile_collect(i, C.byref(ms), C.byref(n), C.byref(w)))
        out[name] = dict(ms=ms.value, launches=n.value, work=w.value)
    return out
