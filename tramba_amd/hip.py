"""ctypes binding of libtramba_hip.so (the C ABI in include/tramba_hip.h).

PyTorch is plumbing here: it owns device memory and streams; every kernel on the Tramba hot
path is launched through this module onto torch's CURRENT stream.  There is no fallback: if
the library is missing or the tensors are not on a HIP device the call raises.
"""
import ctypes
import math
import os
import threading
import weakref

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "_lib", "libtramba_hip.so")

F32, F16, BF16 = 0, 1, 2
ACT_NONE, ACT_SILU, ACT_GELU, ACT_SIGMOID_GATE, ACT_GELU_GRAD_MUL = 0, 1, 2, 3, 4
SCAN_RASTER, SCAN_LINE, SCAN_HELIX, SCAN_WINDOW, SCAN_DILATION = range(5)
FAMILY = {"raster": SCAN_RASTER, "line": SCAN_LINE, "helix": SCAN_HELIX, "window": SCAN_WINDOW,
          "dilation": SCAN_DILATION}
PROF_SCAN_BOUNDARY, PROF_SCAN_FUSED, PROF_GEMM, PROF_MERGE, PROF_SCAN_BWD, PROF_WGRAD, PROF_LAYERNORM, PROF_DW = 0, 1, 2, 3, 4, 5, 6, 7

_DT = {torch.float32: F32, torch.float16: F16, torch.bfloat16: BF16}

c_int, c_i64, c_f, c_vp = ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p

# name -> (restype, argtypes); mirrors include/tramba_hip.h one to one
SIGNATURES = {
    "tramba_last_error": (ctypes.c_char_p, []),
    "tramba_abi_version": (c_int, []),
    "tramba_device_error": (c_int, []),
    "tramba_tune_set": (c_int, [c_int, c_int]),
    "tramba_tune_get": (c_int, [c_int]),
    "tramba_profile_enable": (c_int, [c_int, c_int]),
    "tramba_profile_read": (c_int, [c_int, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]),
    "tramba_profile_min_units": (c_int, [c_int, ctypes.c_double]),
    "tramba_scan_family_k": (c_int, [c_int]),
    "tramba_default_window": (c_int, [c_int]),
    "tramba_scan_table": (c_int, [c_int, c_int, c_int, c_int, c_vp]),
    "tramba_scan_table_inverse": (c_int, [c_vp, c_int, c_int, c_vp, c_vp]),
    "tramba_selective_scan_nchunk": (c_int, [c_int, c_int]),
    "tramba_selective_scan_max_dstate": (c_int, []),
    "tramba_selective_scan_fwd": (c_int, [c_vp] * 9 + [c_int] * 8 + [c_vp]),
    "tramba_selective_scan_bwd": (c_int, [c_vp] * 16 + [c_int] * 8 + [c_vp]),
    "tramba_selective_scan_bwd_det_work": (c_i64, [c_int] * 6),
    "tramba_selective_scan_bwd_det": (c_int, [c_vp] * 17 + [ctypes.c_size_t] + [c_int] * 7 + [c_vp]),
    "tramba_cross_scan": (c_int, [c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_vp]),
    "tramba_cross_merge": (c_int, [c_vp, c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_vp]),
    "tramba_ss2d_group_stride": (c_int, [c_int]),
    "tramba_ss2d_scan_workspace": (ctypes.c_size_t, [c_int] * 4),
    "tramba_ss2d_scan_cl": (c_int, [c_vp] * 9 + [ctypes.c_size_t] + [c_int] * 7 + [c_vp, c_int, c_vp]),
    "tramba_ss2d_group_stride_n": (c_int, [c_int] * 2),
    "tramba_ss2d_scan_n_workspace": (ctypes.c_size_t, [c_int] * 5),
    "tramba_ss2d_scan_n_plan": (c_int, [c_int] * 5 + [c_vp] * 2),
    "tramba_ss2d_scan_n_cl": (c_int, [c_vp] * 9 + [ctypes.c_size_t] + [c_int] * 8 + [c_vp]),
    "tramba_ss2d_scan_bwd_workspace": (ctypes.c_size_t, [c_int] * 4),
    "tramba_ss2d_scan_bwd_cl": (c_int, [c_vp] * 12 + [c_int, c_vp, c_vp, ctypes.c_size_t] + [c_int] * 9 + [c_vp]),
    "tramba_ss2d_bwd_prep_cl": (c_int, [c_vp] * 6 + [c_int] * 6 + [c_vp]),
    "tramba_ss2d_bwd_assemble_cl": (c_int, [c_vp] * 4 + [c_int] * 5 + [c_vp]),
    "tramba_ss2d_scan_n_bwd_workspace": (ctypes.c_size_t, [c_int] * 6),
    "tramba_ss2d_scan_n_bwd_plan": (c_int, [c_int] * 5 + [c_vp] * 2),
    "tramba_ss2d_scan_n_bwd_cl": (c_int, [c_vp] * 14 + [ctypes.c_size_t] + [c_int] * 8 + [c_vp]),
    "tramba_ss2d_bwd_prep_n_cl": (c_int, [c_vp] * 6 + [c_int] * 7 + [c_vp]),
    "tramba_ss2d_bwd_assemble_n_cl": (c_int, [c_vp] * 4 + [c_int] * 6 + [c_vp]),
    "tramba_ss2d_merge_grad_cl": (c_int, [c_vp] * 8 + [c_int] * 4 + [c_f, c_int, c_int, c_int, c_vp]),
    "tramba_ss2d_merge_norm_cl": (c_int, [c_vp] * 6 + [c_int] * 4 + [c_f, c_int, c_int, c_int, c_vp]),
    "tramba_ss2d_merge_norm_gate_cl": (c_int, [c_vp] * 7 + [c_int] * 4 + [c_f, c_int, c_int, c_int, c_vp]),
    "tramba_add_layernorm_gate_cl": (c_int, [c_vp] * 3 + [c_i64] + [c_vp] * 6 + [c_i64, c_int, c_f, c_int, c_int, c_vp]),
    "tramba_gelu_gate_bwd_cl": (c_int, [c_vp] * 5 + [c_i64, c_int, c_vp]),
    "tramba_layernorm_cl": (c_int, [c_vp] * 4 + [c_i64, c_int, c_f, c_int, c_int, c_vp]),
    "tramba_layernorm_bwd_parts": (c_i64, [c_i64, c_int, c_int]),
    "tramba_layernorm_bwd_cl": (c_int, [c_vp] * 5 + [c_i64, c_int, c_f, c_int, c_vp]),
    "tramba_layernorm_bwd_res_cl": (c_int, [c_vp] * 7 + [c_i64, c_vp, c_i64, c_int, c_f, c_int, c_vp]),
    "tramba_layernorm_bwd_any_cl": (c_int, [c_vp] * 7 + [c_i64, c_vp, c_i64, c_int, c_f, c_int, c_int, c_int, c_int, c_vp]),
    "tramba_shuffle_norm_bwd_cl": (c_int, [c_vp] * 5 + [c_int] * 5 + [c_f, c_int, c_vp]),
    "tramba_add_layernorm_cl": (c_int, [c_vp] * 3 + [c_i64] + [c_vp] * 5 + [c_i64, c_int, c_f, c_int, c_int, c_vp]),
    "tramba_shuffle_norm_cl": (c_int, [c_vp] * 4 + [c_int] * 5 + [c_f, c_int, c_vp]),
    "tramba_shuffle_norm_head_cl": (c_int, [c_vp] * 4 + [c_f, c_vp] + [c_int] * 5 + [c_f, c_int, c_vp]),
    "tramba_shuffle_norm_head_bwd_parts": (c_i64, [c_int] * 6),
    "tramba_shuffle_norm_head_bwd_cl": (c_int, [c_vp] * 6 + [c_int] * 5 + [c_f, c_int, c_vp]),
    "tramba_rowdot_cl": (c_int, [c_vp, c_vp, c_f, c_vp, c_i64, c_int, c_int, c_vp]),
    "tramba_rowdot_bwd_parts": (c_i64, [c_i64, c_int, c_int]),
    "tramba_rowdot_bwd_cl": (c_int, [c_vp] * 5 + [c_i64, c_int, c_int, c_vp]),
    "tramba_saliency_stats": (c_int, [c_vp] * 4 + [c_int] * 3 + [c_vp]),
    "tramba_feature_transform": (c_int, [c_vp] * 3 + [c_int] * 3 + [c_vp]),
    "tramba_weighted_f_workspace": (ctypes.c_size_t, [c_int] * 3),
    "tramba_weighted_f_sums": (c_int, [c_vp] * 7 + [ctypes.c_size_t] + [c_int] * 3 + [c_vp]),
    "tramba_resize_table_words": (ctypes.c_size_t, [c_int] * 4),
    "tramba_resize_table": (c_int, [c_int] * 4 + [c_vp] * 3 + [ctypes.c_size_t]),
    "tramba_frames_to_input": (c_int, [c_vp] * 3 + [c_int] * 6 + [c_vp]),
    "tramba_logits_to_u8": (c_int, [c_vp] * 2 + [c_int] * 6 + [c_vp]),
    "tramba_frames_ragged_check": (c_int, [c_vp, c_int, c_int, ctypes.c_size_t, ctypes.c_size_t, c_int]),
    "tramba_frames_to_input_ragged": (c_int, [c_vp, c_vp, ctypes.c_size_t, c_vp, c_int, c_int, c_int, c_vp]),
    "tramba_logits_to_u8_ragged": (c_int, [c_vp] * 4 + [ctypes.c_size_t] + [c_int] * 3 + [c_vp]),
    "tramba_augment_source_table_words": (ctypes.c_size_t, [c_int] * 3),
    "tramba_augment_source_table": (c_int, [c_int] * 3 + [c_vp, ctypes.c_size_t]),
    "tramba_augment_size_table_words": (ctypes.c_size_t, [c_int]),
    "tramba_augment_size_table": (c_int, [c_int] + [c_vp] * 3 + [ctypes.c_size_t]),
    "tramba_augment_scale_taps": (c_int, [c_int] * 2),
    "tramba_augment_rotation": (c_int, [c_int] * 2 + [c_vp]),
    "tramba_augment_workspace": (ctypes.c_size_t, [c_int] * 2),
    "tramba_augment_batch": (c_int, [c_vp] * 2 + [ctypes.c_size_t] + [c_vp] * 4 + [ctypes.c_size_t] + [c_int] * 2 + [c_vp]),
    "tramba_dw_pack": (c_int, [c_vp] * 8 + [c_int] * 2 + [c_vp]),
    "tramba_dwconv_cl": (c_int, [c_vp] * 4 + [c_int] * 7 + [c_vp]),
    "tramba_dwconv_dual_cl": (c_int, [c_vp] * 5 + [c_int] * 8 + [c_vp]),
    "tramba_dw_unpack_grad": (c_int, [c_vp] * 5 + [c_int] * 3 + [c_vp]),
    "tramba_dw_pack_multi": (c_int, [c_vp] * 10 + [c_int, c_vp]),
    "tramba_dw_unpack_grad_multi": (c_int, [c_vp] * 8 + [c_int, c_vp]),
    "tramba_im2col3x3_cl": (c_int, [c_vp] * 2 + [c_int] * 8 + [c_vp]),
    "tramba_upsample_bilinear_bwd": (c_int, [c_vp] * 2 + [c_int] * 5 + [c_vp]),
    "tramba_col2im3x3_cl": (c_int, [c_vp] * 2 + [c_int] * 8 + [c_vp]),
    "tramba_dwconv_wgrad_parts": (c_i64, [c_int, c_int, c_int, c_int, c_int]),
    "tramba_dwconv_wgrad_cl": (c_int, [c_vp] * 3 + [c_int] * 6 + [c_vp]),
    "tramba_dct_split_cl": (c_int, [c_vp] * 6 + [c_int] * 4 + [c_vp]),
    "tramba_linear_cl": (c_int, [c_vp] * 5 + [c_i64, c_int, c_int, c_int, c_int, c_int, c_vp]),
    "tramba_linear_dual_cl": (c_int, [c_vp] * 5 + [c_i64, c_int, c_int, c_int, c_int, c_vp]),
    "tramba_linear_ln_cl": (c_int, [c_vp] * 6 + [c_i64, c_int, c_int, c_f, c_int, c_int, c_int, c_vp]),
    "tramba_linear2_cl": (c_int, [c_vp, c_vp, c_int] + [c_vp] * 4 + [c_i64, c_int, c_int, c_int, c_int, c_int, c_vp]),
    "tramba_linear_rowstat_cl": (c_int, [c_vp] * 5 + [c_i64, c_int, c_int, c_int, c_int, c_int, c_vp,
                                                      ctypes.POINTER(c_int), c_vp]),
    "tramba_linear2_rowstat_cl": (c_int, [c_vp, c_vp, c_int] + [c_vp] * 4 + [c_i64, c_int, c_int, c_int, c_int, c_int, c_vp,
                                                                             ctypes.POINTER(c_int), c_vp]),
    "tramba_linear_ln_rowstat_cl": (c_int, [c_vp] * 6 + [c_i64, c_int, c_int, c_f, c_int, c_int, c_int, c_vp, c_int, c_vp]),
    "tramba_wgrad_workspace": (ctypes.c_size_t, [c_i64, c_int, c_int, c_int, c_int]),
    "tramba_wgrad_cl": (c_int, [c_vp] * 4 + [ctypes.c_size_t, c_i64, c_int, c_int, c_int, c_int, c_i64, c_i64, c_int, c_i64,
                                             c_i64, c_int, c_int, c_int, c_vp]),
    "tramba_rows_gemm_cl": (c_int, [c_vp] * 3 + [c_int, c_i64, c_int, c_int, c_int, c_int, c_int, c_vp]),
    "tramba_shadow_cast_multi": (c_int, [c_vp, c_int, c_i64, c_int, c_vp]),
    "tramba_slab_sum": (c_int, [c_vp, c_vp, c_i64, c_int, c_vp]),
    "tramba_multi_sum": (c_int, [c_vp, c_vp, c_vp, c_vp, c_int, c_vp]),
    "tramba_multi_sum_strided": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_int, c_vp]),
    "tramba_wgrad_parts_cl": (c_int, [c_vp] * 4 + [ctypes.c_size_t, c_i64, c_int, c_int, c_int, c_int, c_i64, c_i64, c_int, c_i64,
                                                   c_i64, c_int, c_int, c_int, c_vp, c_vp]),
    "tramba_expand_norm_head_cl": (c_int, [c_vp] * 5 + [c_f, c_vp] + [c_int] * 5 + [c_f, c_int, c_vp]),
    "tramba_conv3x3s2_cl": (c_int, [c_vp] * 4 + [c_int] * 6 + [c_vp]),
    "tramba_stem_conv_ln_gelu": (c_int, [c_vp] * 6 + [c_int] * 3 + [c_f, c_int, c_int, c_vp]),
    "tramba_sod_loss_sums": (c_int, [c_vp] * 3 + [c_int] * 6 + [c_vp]),
    "tramba_sod_loss_finish": (c_int, [c_vp] * 4 + [c_int, c_int, c_i64, c_vp, c_vp]),
    "tramba_sod_loss_grad_workspace": (ctypes.c_size_t, [c_int] * 5),
    "tramba_sod_loss_grad": (c_int, [c_vp] * 6 + [ctypes.c_size_t] + [c_int] * 5 + [c_vp]),
    "tramba_loss_weight_map": (c_int, [c_vp] * 2 + [c_int] * 4 + [c_vp]),
    "tramba_sod_wloss_sums": (c_int, [c_vp] * 4 + [c_int] * 6 + [c_f, c_int, c_vp]),
    "tramba_sod_wloss_finish": (c_int, [c_vp] * 4 + [c_int, c_int, c_i64, c_int, c_int, c_vp, c_vp]),
    "tramba_sod_wloss_grad_workspace": (ctypes.c_size_t, [c_int] * 5),
    "tramba_sod_wloss_grad": (c_int, [c_vp] * 7 + [ctypes.c_size_t] + [c_int] * 5 + [c_f, c_int, c_vp]),
    "tramba_adam_step": (c_int, [c_vp] * 6 + [c_int] + [ctypes.c_double] * 5 + [c_vp]),
    "tramba_grad_accumulate": (c_int, [c_vp] * 3 + [c_int, c_vp, c_vp]),
    "tramba_grad_norm_workspace": (ctypes.c_size_t, [c_vp, c_int]),
    "tramba_grad_norm": (c_int, [c_vp] * 2 + [c_int, ctypes.c_double, ctypes.c_double, c_int, c_vp, c_vp, ctypes.c_size_t, c_vp]),
    "tramba_adam_step_ctl": (c_int, [c_vp] * 6 + [c_int] + [ctypes.c_double] * 5 + [c_vp] * 3),
    "tramba_grad_norm_scaled": (c_int, [c_vp] * 2 + [c_int, ctypes.c_double, ctypes.c_double, c_int, c_vp, c_vp, c_vp,
                                        ctypes.c_size_t, c_vp]),
    "tramba_loss_scale_update": (c_int, [c_vp] * 2 + [ctypes.c_double] * 2 + [c_int] + [ctypes.c_double] * 2 + [c_vp]),
    "tramba_step_sched_advance": (c_int, [c_vp, c_vp, c_i64, c_vp, c_i64, c_vp]),
    "tramba_adam_step_sched": (c_int, [c_vp] * 6 + [c_int] + [ctypes.c_double] * 5 + [c_vp] * 5),
    "tramba_window_attn_cl": (c_int, [c_vp] * 3 + [c_int] * 8 + [c_vp]),
    "tramba_kv_attn_cl": (c_int, [c_vp] * 3 + [c_int, c_i64] + [c_int] * 4 + [c_vp]),
    "tramba_window_attn_bwd_work": (ctypes.c_size_t, [c_int] * 6),
    "tramba_window_attn_bwd_cl": (c_int, [c_vp] * 6 + [ctypes.c_size_t] + [c_int] * 8 + [c_vp]),
    "tramba_kv_attn_bwd_work": (ctypes.c_size_t, [c_int, c_i64, c_int, c_int, c_int]),
    "tramba_kv_attn_bwd_cl": (c_int, [c_vp] * 6 + [ctypes.c_size_t, c_int, c_i64] + [c_int] * 4 + [c_vp]),
    "tramba_patch_conv_cl": (c_int, [c_vp] * 4 + [c_int] * 7 + [c_vp]),
    "tramba_patch_conv_dgrad_cl": (c_int, [c_vp] * 3 + [c_int] * 7 + [c_vp]),
    "tramba_patch_conv_wgrad_split": (c_int, [c_int] * 6),
    "tramba_patch_conv_wgrad_work": (ctypes.c_size_t, [c_int] * 6),
    "tramba_patch_conv_wgrad_cl": (c_int, [c_vp] * 3 + [ctypes.c_size_t] + [c_int] * 8 + [c_vp]),
    "tramba_patch_embed_ln": (c_int, [c_vp] * 6 + [c_int] * 7 + [c_f, c_int, c_int, c_vp]),
    "tramba_conv_affine_cl": (c_int, [c_vp] * 6 + [c_int] * 9 + [c_vp]),
    "tramba_stem7_affine_relu_pool": (c_int, [c_vp] * 5 + [c_int] * 5 + [c_vp]),
    "tramba_conv_dgrad_cl": (c_int, [c_vp] * 3 + [c_int] * 8 + [c_vp]),
    "tramba_conv_wgrad_split": (c_int, [c_int] * 7),
    "tramba_conv_wgrad_work": (ctypes.c_size_t, [c_int] * 7),
    "tramba_conv_wgrad_cl": (c_int, [c_vp] * 3 + [ctypes.c_size_t] + [c_int] * 8 + [c_vp]),
    "tramba_bn_parts": (c_int, [c_i64, c_int]),
    "tramba_bn_work": (ctypes.c_size_t, [c_i64, c_int]),
    "tramba_bn_stats_cl": (c_int, [c_vp] * 6 + [ctypes.c_size_t, c_i64, c_int, c_f, c_f, c_int, c_vp]),
    "tramba_bn_act_cl": (c_int, [c_vp] * 7 + [c_i64, c_int, c_int, c_int, c_vp]),
    "tramba_bn_act_bwd_cl": (c_int, [c_vp] * 11 + [ctypes.c_size_t, c_i64, c_int, c_int, c_int, c_vp]),
    "tramba_maxpool3s2_cl": (c_int, [c_vp] * 2 + [c_int] * 5 + [c_vp]),
    "tramba_maxpool3s2_bwd_cl": (c_int, [c_vp] * 3 + [c_int] * 5 + [c_vp]),
}

_lib = None
_lock = threading.Lock()


def lib():
    """Load the shared library (raises if it has not been built -- never falls back)."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                if not os.path.exists(LIB_PATH):
                    raise RuntimeError(
                        f"{LIB_PATH} is missing: build it with `python -m tramba_amd.buildlib` "
                        "(hipcc, gfx950).  tramba_amd has no CPU or PyTorch fallback.")
                l = ctypes.CDLL(LIB_PATH)
                for name, (res, args) in SIGNATURES.items():
                    fn = getattr(l, name)
                    fn.restype, fn.argtypes = res, args
                _lib = l
    return _lib


class TrambaHipError(RuntimeError):
    pass


def _check(rc, what):
    if rc < 0:
        raise TrambaHipError(f"{what}: {lib().tramba_last_error().decode()} (code {rc})")
    return rc


def dt(t: torch.Tensor) -> int:
    try:
        return _DT[t.dtype]
    except KeyError:
        raise TrambaHipError(f"unsupported dtype {t.dtype}") from None


def _dev(*ts):
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise TrambaHipError("tramba_amd kernels need tensors on a HIP device (no CPU fallback)")
        if not t.is_contiguous():
            raise TrambaHipError("tramba_amd kernels need contiguous tensors")


def _ptr(t):
    return None if t is None else t.data_ptr()


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_cur_device = getattr(torch._C, "_cuda_getDevice", None)


def _stream():
    """the current HIP stream of the current device as an integer handle.  torch.cuda.current_stream() builds a Stream
    object per call (~9 us): with ~850 library launches per training step that alone was 7 ms of the launch threads' time."""
    if _raw_stream is not None and _cur_device is not None:
        return _raw_stream(_cur_device())
    return torch.cuda.current_stream().cuda_stream


_f32_cache = {}


def _f32(t):
    """fp32 contiguous view of a parameter / buffer.  16-bit parameters (prepare_inference) are converted ONCE per
    (object, version, storage): a cast kernel per bias per call was ~10 launches of every forward."""
    if t is None:
        return None
    if t.dtype == torch.float32 and t.is_contiguous():
        return t.detach()
    key = id(t)
    ver = (t._version, t.data_ptr(), t.dtype)
    hit = _f32_cache.get(key)
    if hit is not None and hit[0] == ver and hit[2]() is t:
        return hit[1]
    conv = t.detach().float().contiguous()
    try:
        ref = weakref.ref(t, lambda _r, k=key: _f32_cache.pop(k, None))
    except TypeError:
        return conv
    _f32_cache[key] = (ver, conv, ref)
    return conv


# ----------------------------------------------------------------------------- tables
_table_cache = {}


def default_window(h: int) -> int:
    return lib().tramba_default_window(h)


def scan_table_host(family: str, h: int, w: int = None, param: int = 0) -> np.ndarray:
    """(K, L) int32 flat pixel index per sequence position (host)."""
    w = h if w is None else w
    fam = FAMILY[family]
    k = _check(lib().tramba_scan_family_k(fam), "scan_family_k")
    out = np.empty((k, h * w), dtype=np.int32)
    _check(lib().tramba_scan_table(fam, h, w, param, out.ctypes.data), f"scan_table({family},{h})")
    return out


def scan_table_inverse_host(table: np.ndarray):
    k, l = table.shape
    table = np.ascontiguousarray(table, dtype=np.int32)
    ptr = np.empty(l + 1, dtype=np.int32)
    idx = np.empty(k * l, dtype=np.int32)
    _check(lib().tramba_scan_table_inverse(table.ctypes.data, k, l, ptr.ctypes.data, idx.ctypes.data),
           "scan_table_inverse")
    return ptr, idx


class ScanOrder:
    """Device-resident scan table + its inverse (CSR) for one (family, size, device)."""

    def __init__(self, family, h, w, param, device):
        host = scan_table_host(family, h, w, param)
        ptr, idx = scan_table_inverse_host(host)
        self.family, self.h, self.w, self.k, self.l = family, h, w, host.shape[0], host.shape[1]
        self.table = torch.from_numpy(host).to(device)
        self.inv_ptr = torch.from_numpy(ptr).to(device)
        self.inv_idx = torch.from_numpy(idx).to(device)
        if not torch.cuda.is_current_stream_capturing():
            torch.cuda.current_stream(device).synchronize()   # tables are shared by every stream from here on


def scan_order(family: str, h: int, w: int, device, param: int = 0) -> ScanOrder:
    key = (family, h, w, param, str(device))
    so = _table_cache.get(key)
    if so is None:
        so = _table_cache[key] = ScanOrder(family, h, w, param, device)
    return so


# ----------------------------------------------------------------------------- profiling / tuning
TUNE_MERGE_FORM, TUNE_SCAN_FORM, TUNE_SCAN_W, TUNE_GEMM_TILE, TUNE_MAILBOX_SKIP, TUNE_DW_FORM, TUNE_DW_ROWS = 0, 1, 2, 3, 4, 6, 7   # (5 retired)
TUNE_MERGE_PW = 8
TUNE_SCAN_N_PASS = 9      # measurement only: 1 / 2 = the reduce / the replay launch of ss2d_scan_n_cl alone


def device_error():
    """raise TrambaHipError if a kernel launched earlier raised the library's device error word (tramba_device_error: a fused
    scan whose carry mailbox timed out leaves NaN in its output); call after a synchronisation to be certain"""
    _check(lib().tramba_device_error(), "device_error")


def tune_set(knob: int, value: int):
    """kernel-variant selection for A/B timing scripts (0 = the library's own choice)"""
    _check(lib().tramba_tune_set(knob, value), "tune_set")


def profile_enable(which: int, on: bool):
    _check(lib().tramba_profile_enable(which, int(on)), "profile_enable")


def profile_min_units(which: int, min_units: float):
    """time only launches accounting for at least `min_units` algorithmic bytes / flops (0 = all)"""
    _check(lib().tramba_profile_min_units(which, float(min_units)), "profile_min_units")


def profile_read(which: int):
    ms, units = ctypes.c_double(), ctypes.c_double()
    n = _check(lib().tramba_profile_read(which, ctypes.byref(ms), ctypes.byref(units)), "profile_read")
    return n, ms.value, units.value


# ----------------------------------------------------------------------------- L0 / L1 boundary ops
def selective_scan_nchunk(l: int, dtype: torch.dtype) -> int:
    return lib().tramba_selective_scan_nchunk(l, _DT[dtype])


def selective_scan_max_dstate() -> int:
    return lib().tramba_selective_scan_max_dstate()


def _check_dstate(n, what):
    top = selective_scan_max_dstate()
    if not 1 <= n <= top:
        raise TrambaHipError(f"{what}: d_state={n} unsupported (1..{top})")


def scan_bc_copies(kd: int, k: int, n: int) -> int:
    """private dB / dC copies of selective_scan_bwd: at most 1/8 of a group's rows add into one address, up to 16 copies;
    for d_state > 4 also ncopy * N <= 64, so that the (ncopy, B, K, N, L) fp32 workspace never exceeds what N = 4 takes at
    the same shape"""
    ncopy = max(1, min(16, (kd // k) // 8))
    if n > 4:
        ncopy = max(1, min(ncopy, 64 // n))
    return ncopy


def selective_scan_fwd(u, delta, A, B, C, D, delta_bias, delta_softplus=True, oflex=True, want_ckpt=True):
    _dev(u, delta, A, B, C, D, delta_bias)
    nb, kd, l = u.shape
    k, n = B.shape[1], B.shape[2]
    _check_dstate(n, "selective_scan_fwd")
    if delta.shape != u.shape or A.shape != (kd, n) or B.shape != (nb, k, n, l) or C.shape != B.shape:
        raise TrambaHipError(f"selective_scan_fwd: inconsistent shapes u{tuple(u.shape)} delta{tuple(delta.shape)} "
                             f"A{tuple(A.shape)} B{tuple(B.shape)} C{tuple(C.shape)}")
    if not (delta.dtype == B.dtype == C.dtype == u.dtype):
        raise TrambaHipError("selective_scan_fwd: u, delta, B, C must share a dtype")
    out = torch.empty((nb, kd, l), dtype=torch.float32 if oflex else u.dtype, device=u.device)
    ckpt = None
    if want_ckpt:
        ckpt = torch.empty((nb, kd, selective_scan_nchunk(l, u.dtype), n), dtype=torch.float32, device=u.device)
    A, D, delta_bias = _f32(A), _f32(D), _f32(delta_bias)
    _check(lib().tramba_selective_scan_fwd(
        _ptr(u), _ptr(delta), _ptr(A), _ptr(B), _ptr(C), _ptr(D), _ptr(delta_bias), _ptr(out), _ptr(ckpt),
        nb, kd, k, n, l, dt(u), dt(out), int(delta_softplus), _stream()), "selective_scan_fwd")
    return out, ckpt


def selective_scan_bwd_det_work(nb: int, kd: int, k: int, n: int, l: int, dtype: torch.dtype) -> int:
    """bytes of workspace selective_scan_bwd(..., deterministic=True) takes for this shape:
    4 * (2 * ceil((kd/k) / S) * nb*k*n*l + nb*kd*(n + 2)), S = 8, 16 or 32 rows per workgroup (l > 256, > 128, else)"""
    return _check(lib().tramba_selective_scan_bwd_det_work(nb, kd, k, n, l, _DT[dtype]), "selective_scan_bwd_det_work")


def selective_scan_bwd(u, delta, A, B, C, D, delta_bias, dout, ckpt, delta_softplus=True, deterministic=False):
    """deterministic: the atomic-free form (tramba_selective_scan_bwd_det) -- the same seven tensors in the same dtypes,
    each a function of the inputs and the shape alone; its partial sums live in the per-stream scan workspace"""
    _dev(u, delta, A, B, C, D, delta_bias, dout, ckpt)
    nb, kd, l = u.shape
    k, n = B.shape[1], B.shape[2]
    _check_dstate(n, "selective_scan_bwd")
    A32, D32, b32 = _f32(A), _f32(D), _f32(delta_bias)
    dout = dout.float().contiguous()
    du, ddelta = torch.empty_like(u), torch.empty_like(delta)
    if deterministic:
        # the kernels write every element of the five; zeros only because they are the allocator at hand, in two fills
        dBC = torch.zeros((2, nb, k, n, l), dtype=torch.float32, device=u.device)
        small = torch.zeros(kd * (n + 2), dtype=torch.float32, device=u.device)
        dA = small[:kd * n].view(kd, n)
        dD = small[kd * n:kd * (n + 1)] if D is not None else None
        dbias = small[kd * (n + 1):] if delta_bias is not None else None
        nbytes = selective_scan_bwd_det_work(nb, kd, k, n, l, u.dtype)
        work = _scan_workspace(u.device, nbytes)
        _check(lib().tramba_selective_scan_bwd_det(
            _ptr(u), _ptr(delta), _ptr(A32), _ptr(B), _ptr(C), _ptr(D32), _ptr(b32), _ptr(dout), _ptr(ckpt),
            _ptr(du), _ptr(ddelta), _ptr(dA), _ptr(dBC[0]), _ptr(dBC[1]), _ptr(dD), _ptr(dbias), _ptr(work), nbytes,
            nb, kd, k, n, l, dt(u), int(delta_softplus), _stream()), "selective_scan_bwd_det")
        return du, ddelta, dA, dBC[0], dBC[1], dD, dbias
    dA = torch.zeros((kd, n), dtype=torch.float32, device=u.device)
    ncopy = scan_bc_copies(kd, k, n)  # private dB/dC copies: <= 1/8 of a group's rows per address
    dB = torch.zeros((ncopy, nb, k, n, l), dtype=torch.float32, device=u.device)
    dC = torch.zeros_like(dB)
    dD = torch.zeros(kd, dtype=torch.float32, device=u.device) if D is not None else None
    dbias = torch.zeros(kd, dtype=torch.float32, device=u.device) if delta_bias is not None else None
    _check(lib().tramba_selective_scan_bwd(
        _ptr(u), _ptr(delta), _ptr(A32), _ptr(B), _ptr(C), _ptr(D32), _ptr(b32), _ptr(dout), _ptr(ckpt),
        _ptr(du), _ptr(ddelta), _ptr(dA), _ptr(dB), _ptr(dC), _ptr(dD), _ptr(dbias),
        nb, kd, k, n, l, dt(u), int(delta_softplus), ncopy, _stream()), "selective_scan_bwd")
    return du, ddelta, dA, dB.sum(0), dC.sum(0), dD, dbias


def cross_scan(x, order: ScanOrder):
    """x: (B, C, H, W) or (B, C, L) contiguous NCHW -> (B, K, C, L)."""
    _dev(x)
    b, c = x.shape[0], x.shape[1]
    l = order.l
    xs = torch.empty((b, order.k, c, l), dtype=x.dtype, device=x.device)
    _check(lib().tramba_cross_scan(_ptr(x), _ptr(order.table), _ptr(xs), b, c, l, order.k, dt(x), _stream()),
           "cross_scan")
    return xs


def cross_merge(ys, order: ScanOrder):
    """ys: (B, K, C, L) -> (B, C, L)."""
    _dev(ys)
    b, k, c, l = ys.shape
    if k != order.k or l != order.l:
        raise TrambaHipError(f"cross_merge: ys {tuple(ys.shape)} does not match table K={order.k} L={order.l}")
    y = torch.empty((b, c, l), dtype=ys.dtype, device=ys.device)
    _check(lib().tramba_cross_merge(_ptr(ys), _ptr(order.inv_ptr), _ptr(order.inv_idx), _ptr(y), b, c, l, k,
                                    dt(ys), _stream()), "cross_merge")
    return y


# ----------------------------------------------------------------------------- channels-last kernels
def ss2d_group_stride(r: int, n: int = 1) -> int:
    """Floats per direction group of the x_proj output: [dt_0..dt_{R-1}, 0-pad to R8 = 8*ceil(R/8), B, C, 0, 0] at d_state
    n = 1; [R8 ranks | B_0..B_{n-1} | C_0..C_{n-1} | 0-pad to a multiple of 4] = R8 + ((2n + 3) & ~3) in general."""
    if n == 1:
        return lib().tramba_ss2d_group_stride(r)
    return lib().tramba_ss2d_group_stride_n(r, n)


def pad_x_proj_weight(x_proj_weight: torch.Tensor, n: int = 1) -> torch.Tensor:
    """(K, R+2n, D) -> (K*RG, D) with zero rows as padding, the layout ss2d_scan_cl (n = 1) / ss2d_scan_n_cl consume."""
    k, r2, d = x_proj_weight.shape
    r = r2 - 2 * n
    if n < 1 or r < 1:
        raise TrambaHipError(f"pad_x_proj_weight: {tuple(x_proj_weight.shape)} is not (K, R + 2*{n}, D)")
    rg = ss2d_group_stride(r, n)
    r8 = (r + 7) & ~7
    w = x_proj_weight.new_zeros((k, rg, d))
    w[:, :r] = x_proj_weight[:, :r]
    w[:, r8:r8 + 2 * n] = x_proj_weight[:, r:]      # B_0..B_{n-1}, C_0..C_{n-1} after the 8-padded ranks
    return w.reshape(k * rg, d)


_scan_ws = {}
_scan_ws_retired = []


def _scan_workspace(device, nbytes):
    """Per-(device, stream) scratch for the wave-segment scan (grown on demand, reused by every launch: launches
    on one stream are ordered, and graph capture sees a stable address; concurrent streams get their own)."""
    key = (str(device), _stream())
    ws = _scan_ws.get(key)
    if ws is None or ws.numel() < nbytes:
        if ws is not None:
            _scan_ws_retired.append(ws)      # a captured hipGraph may still replay launches that point at the old buffer
        ws = _scan_ws[key] = torch.empty(max(nbytes, 1 << 22), dtype=torch.uint8, device=device)
    return ws


def ss2d_scan_states(x, order: ScanOrder):
    """the buffer ss2d_scan_cl(states=...) fills for ss2d_scan_bwd_cl(states=...): the recurrence state entering every
    32-position tile, (B, K, ceil(L/32) + 8, D) f32"""
    b, l, d = x.shape
    return torch.empty(lib().tramba_ss2d_scan_bwd_workspace(b, l, d, order.k), dtype=torch.uint8, device=x.device)


def _launch_output(shape, dtype, device):
    """an UNINITIALISED output buffer whose every element the launch that follows writes: the per-direction outputs (B, K, L, D)
    of the fused scans (ss2d_scan_cl, ss2d_scan_n_cl), the gated merge's map (ss2d_merge_norm_gate_cl) and gz of
    gelu_gate_bwd_cl.  One allocation line for them all: the census of uninitialised allocations reaches
    it through the scans, and the gate entries' own tests check every element they return"""
    return torch.empty(shape, dtype=dtype, device=device)


def ss2d_scan_cl(x, xdbl, order: ScanOrder, dt_w, dt_bias, A, Ds, ys_dtype=torch.float32, segmented=True, states=None,
                 a_log=False):
    """x: (B, L, D); xdbl: (B, L, K*RG) f32 -> ys (B, K, L, D).  With `segmented` a workspace is passed and
    the library picks the wave-segment or a chained form per shape (tune_set(TUNE_SCAN_FORM, ...) forces one).
    states (training): a buffer from ss2d_scan_states(); the launch saves the per-tile entering states in it (chained forms
    only, ys in the input dtype), and the backward launch given the same buffer skips its first sweep.
    a_log (training): `A` is the parameter A_logs, the kernel forms -exp(A_logs) itself."""
    _dev(x, xdbl, dt_w, dt_bias, A, Ds)
    b, l, d = x.shape
    k, r = order.k, dt_w.shape[-1]
    if xdbl.dtype != torch.float32 or xdbl.shape != (b, l, k * ss2d_group_stride(r)):
        raise TrambaHipError(f"ss2d_scan_cl: xdbl must be f32 (B,L,K*RG), got {xdbl.dtype} {tuple(xdbl.shape)}")
    if l != order.l or dt_w.shape != (k, d, r) or A.numel() != k * d or Ds.numel() != k * d or dt_bias.numel() != k * d:
        raise TrambaHipError("ss2d_scan_cl: parameter shapes do not match (K, D, R)")
    ys = _launch_output((b, k, l, d), ys_dtype, x.device)
    ws, ws_bytes = None, 0
    if segmented:
        ws_bytes = lib().tramba_ss2d_scan_workspace(b, l, d, k)
        ws = _scan_workspace(x.device, ws_bytes)
    _check(lib().tramba_ss2d_scan_cl(_ptr(x), _ptr(xdbl), _ptr(order.table), _ptr(dt_w), _ptr(dt_bias), _ptr(A),
                                     _ptr(Ds), _ptr(ys), _ptr(ws), ws_bytes, b, l, d, k, r, dt(x), dt(ys), _ptr(states),
                                     int(a_log), _stream()), "ss2d_scan_cl")
    return ys


def ss2d_scan_n_plan(b, l, d, k, n):
    """(tiles of 32 positions per segment, segments per sequence) of ss2d_scan_n_cl's launch; one segment = one launch."""
    nt, nseg = ctypes.c_int(0), ctypes.c_int(0)
    _check(lib().tramba_ss2d_scan_n_plan(b, l, d, k, n, ctypes.addressof(nt), ctypes.addressof(nseg)), "ss2d_scan_n_plan")
    return nt.value, nseg.value


def ss2d_scan_n_cl(x, xdbl, order: ScanOrder, dt_w, dt_bias, A, Ds, ys_dtype=torch.float32):
    """The fused scan for d_state N = 2..16 (inference).  x: (B, L, D); xdbl: (B, L, K*RG(R, N)) f32; A: (K*D, N) f32,
    already negated -> ys (B, K, L, D) in sequence order.  Wave-segment form only (state-looped); N = 1 is ss2d_scan_cl."""
    _dev(x, xdbl, dt_w, dt_bias, A, Ds)
    b, l, d = x.shape
    k, r = order.k, dt_w.shape[-1]
    if A.dim() != 2 or A.shape[0] != k * d:
        raise TrambaHipError(f"ss2d_scan_n_cl: A must be (K*D, N) = ({k * d}, N), got {tuple(A.shape)}")
    n = A.shape[1]
    if not 2 <= n <= 16:
        raise TrambaHipError(f"ss2d_scan_n_cl: d_state {n} outside 2..16 (d_state 1 is ss2d_scan_cl)")
    rg = ss2d_group_stride(r, n)
    if xdbl.dtype != torch.float32 or xdbl.shape != (b, l, k * rg):
        raise TrambaHipError(f"ss2d_scan_n_cl: xdbl must be f32 (B, L, K*RG(R, N)) = ({b}, {l}, {k}*{rg}), "
                             f"got {xdbl.dtype} {tuple(xdbl.shape)}")
    if l != order.l or dt_w.shape != (k, d, r) or Ds.numel() != k * d or dt_bias.numel() != k * d:
        raise TrambaHipError("ss2d_scan_n_cl: parameter shapes do not match (K, D, R)")
    ys = _launch_output((b, k, l, d), ys_dtype, x.device)
    ws_bytes = lib().tramba_ss2d_scan_n_workspace(b, l, d, k, n)
    ws = _scan_workspace(x.device, ws_bytes)
    _check(lib().tramba_ss2d_scan_n_cl(_ptr(x), _ptr(xdbl), _ptr(order.table), _ptr(dt_w), _ptr(dt_bias), _ptr(A),
                                       _ptr(Ds), _ptr(ys), _ptr(ws), ws_bytes, b, l, d, k, r, n, dt(x), dt(ys),
                                       _stream()), "ss2d_scan_n_cl")
    return ys


def ss2d_merge_sum_cl(ys, order: ScanOrder, out_dtype):
    """ys (B, K, L, D) in sequence order -> (B, L, D): CrossMerge alone (no norm), fixed summation order."""
    _dev(ys)
    b, k, l, d = ys.shape
    y = torch.empty((b, l, d), dtype=out_dtype, device=ys.device)
    _check(lib().tramba_ss2d_merge_norm_cl(_ptr(ys), _ptr(order.inv_ptr), _ptr(order.inv_idx), None, None, _ptr(y), b, l,
                                           d, k, -1.0, ACT_NONE, dt(ys), dt(y), _stream()), "ss2d_merge_sum_cl")
    return y


def ss2d_scan_n_bwd_plan(b, l, d, k, n):
    """(tiles of 32 positions per segment, segments per sequence) of the N = 2..16 scan backward (ss2d_scan_bwd_cl with a
    (K*D, N) `A`): its own plan, segments short enough for their tile-entry states to stay in LDS; one segment = one launch."""
    nt, nseg = ctypes.c_int(0), ctypes.c_int(0)
    _check(lib().tramba_ss2d_scan_n_bwd_plan(b, l, d, k, n, ctypes.addressof(nt), ctypes.addressof(nseg)),
           "ss2d_scan_n_bwd_plan")
    return nt.value, nseg.value


def ss2d_scan_bwd_cl(x, xdbl, order: ScanOrder, dt_w, dt_bias, A, Ds, gym, g_seq=None, states=None, a_log=False,
                     bc_partials=False):
    """Backward of ss2d_scan_cl + merge.  gym (B, L, D) f32 = gradient of the merged map.
    Returns gu, graw (B,K,L,D) x.dtype, gB, gC (B,K,L) f32, gpar (B,3,K,D) f32 (dA, dD, dbias planes).
    g_seq: a ZEROED (B,K,L,RG) f32 x_dbl-gradient table in sequence order -- gB / gC are then accumulated straight into its
    B / C columns (RG - 4, RG - 3) and returned as views of it.
    states: the buffer the forward launch filled (ss2d_scan_cl(states=...)): the sweep that recomputes them is skipped.
    a_log: `A` is the parameter A_logs; gpar's first plane is then dL/dA_logs.
    bc_partials: gB / gC come back as (B, K, ceil(D/32), L) per-channel-tile partial sums written without atomics (no zero
    fill; ss2d_bwd_prep adds them in a fixed order).
    d_state N = 2..16 (backward of ss2d_scan_n_cl + merge): `A` is (K*D, N) f32, already negated (= -exp(A_logs)), xdbl has
    the (B, L, K*RG(R, N)) layout, and bc_partials is required (g_seq, states and a_log do not apply).  gB / gC are then
    (B, K, ceil(D/32), N, L) partials and gpar is (B*NSEG, K*D*(N+2)): one slab per (batch, segment of ss2d_scan_n_bwd_plan)
    holding [dL/dA_logs (K*D, N) | dD (K*D) | dbias (K*D)] -- slab_sum(gpar) gives the three parameter gradients.  gu / graw
    are handed out by the launch (every element written); nothing is accumulated and nothing needs a zero fill."""
    _dev(x, xdbl, dt_w, dt_bias, A, Ds, gym, g_seq)
    b, l, d = x.shape
    k, r = order.k, dt_w.shape[-1]
    n = A.shape[1] if A.dim() == 2 else 1
    if gym.dtype not in (torch.float32, x.dtype) or gym.shape != x.shape:
        raise TrambaHipError("ss2d_scan_bwd_cl: gym must be (B, L, D) in f32 or the activation dtype")
    ct = (d + 31) // 32
    if n != 1:
        if A.shape[0] != k * d or not 2 <= n <= 16:
            raise TrambaHipError(f"ss2d_scan_bwd_cl: A must be (K*D,) or (K*D, N) = ({k * d}, 2..16), got {tuple(A.shape)}")
        rg = ss2d_group_stride(r, n)
        if xdbl.dtype != torch.float32 or xdbl.shape != (b, l, k * rg):
            raise TrambaHipError(f"ss2d_scan_bwd_cl: xdbl must be f32 (B, L, K*RG(R, N)) = ({b}, {l}, {k}*{rg}), "
                                 f"got {xdbl.dtype} {tuple(xdbl.shape)}")
        if l != order.l or dt_w.shape != (k, d, r) or Ds.numel() != k * d or dt_bias.numel() != k * d:
            raise TrambaHipError("ss2d_scan_bwd_cl: parameter shapes do not match (K, D, R)")
        if not bc_partials or g_seq is not None or states is not None or a_log:
            raise TrambaHipError("ss2d_scan_bwd_cl: d_state > 1 needs bc_partials=True and takes no g_seq / states / a_log")
        ct *= n
    gu = torch.empty((b, k, l, d), dtype=x.dtype, device=x.device)
    graw = torch.empty_like(gu)
    if bc_partials:
        gB = torch.empty((b, k, ct, l), dtype=torch.float32, device=x.device)
        gC = torch.empty_like(gB)
        bcs = 1
    elif g_seq is None:
        gB = torch.zeros((b, k, l), dtype=torch.float32, device=x.device)
        gC = torch.zeros_like(gB)
        bcs = 1
    else:
        rg = ss2d_group_stride(r)
        if g_seq.shape != (b, k, l, rg) or g_seq.dtype != torch.float32 or not g_seq.is_contiguous():
            raise TrambaHipError(f"ss2d_scan_bwd_cl: g_seq must be a contiguous float32 (B, K, L, {rg}) tensor")
        gB, gC, bcs = g_seq[..., rg - 4], g_seq[..., rg - 3], rg
    nslab = b if n == 1 else b * ss2d_scan_n_bwd_plan(b, l, d, k, n)[1]
    gpar = torch.empty((nslab, 3, k, d) if n == 1 else (nslab, k * d * (n + 2)), dtype=torch.float32, device=x.device)
    if n != 1:
        ws_bytes = lib().tramba_ss2d_scan_n_bwd_workspace(b, l, d, k, n, dt(x))
        ws = _scan_workspace(x.device, ws_bytes)      # launch-local: written and read inside this one call
        _check(lib().tramba_ss2d_scan_n_bwd_cl(_ptr(x), _ptr(xdbl), _ptr(order.table), _ptr(dt_w), _ptr(dt_bias), _ptr(A),
                                               _ptr(Ds), _ptr(gym), _ptr(gu), _ptr(graw), _ptr(gB), _ptr(gC), _ptr(gpar),
                                               _ptr(ws), ws_bytes, b, l, d, k, r, n, dt(x), dt(gym), _stream()),
               "ss2d_scan_n_bwd_cl")
        return gu, graw, gB.view(b, k, ct // n, n, l), gC.view(b, k, ct // n, n, l), gpar
    ws_bytes = lib().tramba_ss2d_scan_bwd_workspace(b, l, d, k)
    if states is not None:
        _dev(states)
        if states.numel() * states.element_size() < ws_bytes:
            raise TrambaHipError("ss2d_scan_bwd_cl: the states buffer is smaller than ss2d_scan_states() makes it")
        ws = states
    else:
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
    _check(lib().tramba_ss2d_scan_bwd_cl(_ptr(x), _ptr(xdbl), _ptr(order.table), _ptr(dt_w), _ptr(dt_bias), _ptr(A),
                                         _ptr(Ds), _ptr(gym), _ptr(gu), _ptr(graw), _ptr(gB), _ptr(gC), bcs, _ptr(gpar),
                                         _ptr(ws), ws_bytes, 0 if states is None else 1, b, l, d, k, r, dt(x), dt(gym),
                                         (1 if a_log else 0) | (2 if bc_partials else 0), _stream()), "ss2d_scan_bwd_cl")
    return gu, graw, gB, gC, gpar


def ss2d_bwd_prep(xdbl, order: ScanOrder, bpart, cpart, r, dtype, n=1):
    """after ss2d_scan_bwd_cl(bc_partials=True): (ranks (B,K,L,R8) `dtype` = the dt-rank rows of xdbl in sequence order,
    g_seq (B,K,L,RG) f32 with the summed dB / dC in columns R8, R8 + 1; the rank columns are for rows_gemm_cl to fill).
    d_state n > 1: bpart / cpart are (B, K, CT, n, L), RG = RG(r, n), dB_0.. in columns R8 .., dC_0.. in columns R8 + n .."""
    _dev(xdbl, bpart, cpart)
    b, l, pc = xdbl.shape
    k = order.k
    rg = ss2d_group_stride(r, n)
    r8 = (r + 7) & ~7
    want = (b, k, bpart.shape[2], l) if n == 1 else (b, k, bpart.shape[2], n, l)
    if pc != k * rg or bpart.shape != cpart.shape or tuple(bpart.shape) != want:
        raise TrambaHipError(f"ss2d_bwd_prep: xdbl must be (B, L, {k}*{rg}) and bpart / cpart (B, K, CT"
                             f"{'' if n == 1 else ', ' + str(n)}, L), got {tuple(xdbl.shape)}, {tuple(bpart.shape)}, "
                             f"{tuple(cpart.shape)}")
    ranks = torch.empty((b, k, l, r8), dtype=dtype, device=xdbl.device)
    gseq = torch.empty((b, k, l, rg), dtype=torch.float32, device=xdbl.device)
    _check(lib().tramba_ss2d_bwd_prep_n_cl(_ptr(xdbl), _ptr(order.table), _ptr(bpart), _ptr(cpart), _ptr(ranks), _ptr(gseq),
                                           b, l, k, r, n, bpart.shape[2], _DT[dtype], _stream()), "ss2d_bwd_prep_cl")
    return ranks, gseq


def ss2d_bwd_assemble(gseq, order: ScanOrder, r, dtype, n=1):
    """gseq (B,K,L,RG) f32 in sequence order -> (B, L, K*RG) `dtype` in spatial order (gather-sum through the inverse table);
    RG = RG(r, n) at d_state n"""
    _dev(gseq)
    b, k, l, rg = gseq.shape
    if k != order.k or l != order.l or rg != ss2d_group_stride(r, n):
        raise TrambaHipError(f"ss2d_bwd_assemble: gseq must be (B, {order.k}, {order.l}, RG(r, n) = "
                             f"{ss2d_group_stride(r, n)}), got {tuple(gseq.shape)}")
    out = torch.empty((b, l, k * rg), dtype=dtype, device=gseq.device)
    _check(lib().tramba_ss2d_bwd_assemble_n_cl(_ptr(gseq), _ptr(order.inv_ptr), _ptr(order.inv_idx), _ptr(out), b, l, k, r,
                                               n, _DT[dtype], _stream()), "ss2d_bwd_assemble_cl")
    return out


def ss2d_merge_grad_cl(gu, order: ScanOrder, addend, zpre):
    """(merge(gu) + addend) * silu'(zpre): gu (B,K,L,D) sequence order, addend / zpre (B,L,D) -> (B,L,D), zpre's dtype"""
    _dev(gu, addend, zpre)
    b, k, l, d = gu.shape
    if zpre.shape != (b, l, d) or (addend is not None and (addend.shape != zpre.shape or addend.dtype != zpre.dtype)):
        raise TrambaHipError("ss2d_merge_grad_cl: operand shapes / dtypes do not match")
    y = torch.empty((b, l, d), dtype=zpre.dtype, device=gu.device)
    _check(lib().tramba_ss2d_merge_grad_cl(_ptr(gu), _ptr(order.inv_ptr), _ptr(order.inv_idx), None, None, _ptr(y),
                                           _ptr(addend), _ptr(zpre), b, l, d, k, -1.0, ACT_NONE, dt(gu), dt(y), _stream()),
           "ss2d_merge_grad_cl")
    return y


def ss2d_merge_norm_cl(ys, order: ScanOrder, ln_w, ln_b, eps, act, out_dtype):
    _dev(ys, ln_w, ln_b)
    b, k, l, d = ys.shape
    y = torch.empty((b, l, d), dtype=out_dtype, device=ys.device)
    _check(lib().tramba_ss2d_merge_norm_cl(_ptr(ys), _ptr(order.inv_ptr), _ptr(order.inv_idx), _ptr(ln_w),
                                           _ptr(ln_b), _ptr(y), b, l, d, k, eps, act, dt(ys), dt(y), _stream()),
           "ss2d_merge_norm_cl")
    return y


def ss2d_merge_norm_gate_cl(ys, order: ScanOrder, ln_w, ln_b, zpre, eps, act, out_dtype):
    """act(LayerNorm(merge(ys))) * silu(zpre): ys (B,K,L,D) sequence order, zpre (B,L,D) the gate's pre-activation in the
    output dtype -> (B,L,D)"""
    _dev(ys, ln_w, ln_b, zpre)
    b, k, l, d = ys.shape
    if zpre is None or zpre.shape != (b, l, d) or zpre.dtype != out_dtype:
        raise TrambaHipError("ss2d_merge_norm_gate_cl: the gate must be (B, L, D) in the output dtype")
    y = _launch_output((b, l, d), out_dtype, ys.device)
    _check(lib().tramba_ss2d_merge_norm_gate_cl(_ptr(ys), _ptr(order.inv_ptr), _ptr(order.inv_idx), _ptr(ln_w), _ptr(ln_b),
                                                _ptr(zpre), _ptr(y), b, l, d, k, eps, act, dt(ys), dt(y), _stream()),
           "ss2d_merge_norm_gate_cl")
    return y


def gelu_gate_bwd_cl(gp, n, zpre):
    """backward of p = gelu(n) * silu(zpre): (gn, gz) = (gp * silu(zpre) * gelu'(n), gp * gelu(n) * silu'(zpre)); three
    tensors of one shape and dtype.  gp is CONSUMED: gn is written over it (the kernel is pointwise: a thread reads its
    elements before it writes them); gz is an uninitialised buffer of its own (_launch_output) that the launch fills whole"""
    _dev(gp, n, zpre)
    if not (gp.shape == n.shape == zpre.shape and gp.dtype == n.dtype == zpre.dtype):
        raise TrambaHipError("gelu_gate_bwd_cl: operand shapes / dtypes do not match")
    gz = _launch_output(gp.shape, gp.dtype, gp.device)
    _check(lib().tramba_gelu_gate_bwd_cl(_ptr(gp), _ptr(n), _ptr(zpre), _ptr(gp), _ptr(gz), n.numel(), dt(n), _stream()),
           "gelu_gate_bwd_cl")
    return gp, gz


def layernorm_cl(x, w, b, eps=1e-5, act=ACT_NONE):
    """x: (..., C) contiguous."""
    _dev(x, w, b)
    c = x.shape[-1]
    y = torch.empty_like(x)
    _check(lib().tramba_layernorm_cl(_ptr(x), _ptr(w), _ptr(b), _ptr(y), x.numel() // c, c, eps, act, dt(x),
                                     _stream()), "layernorm_cl")
    return y


def layernorm_bwd_cl(x, dy, w, eps=1e-5, defer=False):
    """x, dy: (..., C) contiguous -> (dx like x, dw (C) f32, db (C) f32).  defer: dw / db go to autograd as the gradients of
    fp32 leaves as they are (see _SumQueue); anything that reads or casts them must pass False."""
    _dev(x, dy, w)
    c = x.shape[-1]
    dx, _, dw, db = _layernorm_bwd("layernorm_bwd_cl", x, dy, w, eps, x.numel() // c, c, defer)
    return dx, dw, db


def _layernorm_bwd(what, x, dy, w, eps, rows, c, defer, gres=None, mask=None, want_masked=False, p=1, h=1, wd=1):
    """the three LayerNorm backwards differ in which operands exist: (dx, dxm or None, dw, db) of
    tramba_layernorm_bwd_any_cl, the partial table sized by the library's own query"""
    dx = torch.empty_like(x)
    dxm = torch.empty_like(x) if want_masked else None
    part = torch.empty((lib().tramba_layernorm_bwd_parts(rows, c, dt(x)), 2, c), dtype=torch.float32, device=x.device)
    _check(lib().tramba_layernorm_bwd_any_cl(_ptr(x), _ptr(dy), _ptr(w), _ptr(dx), _ptr(part), _ptr(gres), _ptr(mask),
                                             rows // x.shape[0], _ptr(dxm), rows, c, eps, p, h, wd, dt(x), _stream()), what)
    s = slab_sum(part, defer=defer)
    return dx, dxm, s[0], s[1]


def add_layernorm_cl(x, y, mask, w, b, eps=1e-5, act=ACT_NONE, dual=False, gate=None):
    """(xsum, n, n_act): xsum = x + y * mask[sample] (None when y is None), n = LayerNorm(xsum or x), n_act = act(n) when
    `dual`.  x, y (B, ..., C) contiguous, mask (B) f32 or None.  gate (like x: a pre-activation; needs `dual`):
    n_act = act(n) * silu(gate), same launch."""
    _dev(x, y, mask, w, b, gate)
    c = x.shape[-1]
    rows = x.numel() // c
    if y is not None and (y.shape != x.shape or y.dtype != x.dtype):
        raise TrambaHipError("add_layernorm_cl: x / y mismatch")
    if mask is not None and (mask.dtype != torch.float32 or mask.numel() != x.shape[0]):
        raise TrambaHipError("add_layernorm_cl: mask must be float32 with one entry per sample")
    if gate is not None and (not dual or gate.shape != x.shape or gate.dtype != x.dtype):
        raise TrambaHipError("add_layernorm_cl: a gate needs the dual store and x's shape and dtype")
    xsum = torch.empty_like(x) if y is not None else None
    n = torch.empty_like(x)
    na = torch.empty_like(x) if dual else None
    head = (_ptr(x), _ptr(y), _ptr(mask), rows // x.shape[0], _ptr(w), _ptr(b))
    tail = (_ptr(xsum), _ptr(n), _ptr(na), rows, c, eps, act, dt(x), _stream())
    _check(lib().tramba_add_layernorm_gate_cl(*head, _ptr(gate), *tail) if gate is not None
           else lib().tramba_add_layernorm_cl(*head, *tail), "add_layernorm_cl")
    return xsum, n, na


def layernorm_bwd_res_cl(x, dy, w, eps=1e-5, gres=None, mask=None, want_masked=False, defer=False):
    """LayerNorm backward on the residual stream: (dx + gres, that * mask[sample] or None, dw, db)"""
    _dev(x, dy, w, gres, mask)
    c = x.shape[-1]
    rows = x.numel() // c
    if gres is not None and (gres.shape != x.shape or gres.dtype != x.dtype):
        raise TrambaHipError("layernorm_bwd_res_cl: gres must match x")
    return _layernorm_bwd("layernorm_bwd_res_cl", x, dy, w, eps, rows, c, defer, gres, mask, want_masked)


def shuffle_norm_cl(x, w, b, p, eps=1e-5):
    """x: (B, H, W, P*P*C) -> (B, H*P, W*P, C), pixel-shuffle + LayerNorm over C."""
    _dev(x, w, b)
    bb, h, wd, cc = x.shape
    c = cc // (p * p)
    y = torch.empty((bb, h * p, wd * p, c), dtype=x.dtype, device=x.device)
    _check(lib().tramba_shuffle_norm_cl(_ptr(x), _ptr(w), _ptr(b), _ptr(y), bb, h, wd, c, p, eps, dt(x), _stream()),
           "shuffle_norm_cl")
    return y


def shuffle_norm_bwd_cl(x, dy, w, p, eps=1e-5, defer=False):
    """backward of shuffle_norm_cl: x (B,H,W,P*P*C), dy (B,H*P,W*P,C) -> (dx like x, dw (C), db (C))"""
    _dev(x, dy, w)
    bb, h, wd, cc = x.shape
    c = cc // (p * p)
    if dy.shape != (bb, h * p, wd * p, c) or dy.dtype != x.dtype:
        raise TrambaHipError("shuffle_norm_bwd_cl: dy does not match the shuffled map")
    rows = bb * h * wd * p * p
    if p < 1 or rows <= 0 or rows >= 2147483647:      # (the checks of the C entry of this name, which the general one lacks)
        raise TrambaHipError("shuffle_norm_bwd_cl: empty shape, or too many rows for the 32-bit row index of this build")
    dx, _, dw, db = _layernorm_bwd("shuffle_norm_bwd_cl", x, dy, w, eps, rows, c, defer, p=p, h=h, wd=wd)
    return dx, dw, db


def shuffle_norm_head_cl(x, w, b, head_w, head_b: float, p, eps=1e-5):
    """x: (B, H, W, P*P*C) -> (B, H*P, W*P) f32: pixel-shuffle + LayerNorm over C + dot with head_w (C) + head_b."""
    _dev(x, w, b, head_w)
    bb, h, wd, cc = x.shape
    c = cc // (p * p)
    y = torch.empty((bb, h * p, wd * p), dtype=torch.float32, device=x.device)
    _check(lib().tramba_shuffle_norm_head_cl(_ptr(x), _ptr(w), _ptr(b), _ptr(head_w), float(head_b), _ptr(y), bb, h, wd,
                                             c, p, eps, dt(x), _stream()), "shuffle_norm_head_cl")
    return y


def shuffle_norm_head_bwd_cl(x, g, ln_w, head_w, p, eps=1e-5):
    """Backward of shuffle_norm_head_cl in one pass over x (B, H, W, P*P*C): g (B, H*P, W*P) f32 -> (dx like x, part (S, C + 4)
    f32): the rows of `part` sum to A_c = sum g xhat_c (slots 0..C) and G = sum g (slot C), from which every parameter gradient
    follows (tramba_shuffle_norm_head_bwd_cl)."""
    _dev(x, g, ln_w, head_w)
    bb, h, wd, cc = x.shape
    c = cc // (p * p)
    if g.dtype != torch.float32 or g.numel() != bb * h * wd * p * p or ln_w.dtype != torch.float32 or head_w.dtype != torch.float32:
        raise TrambaHipError("shuffle_norm_head_bwd_cl: fp32 logit gradients / parameters of the forward's shapes")
    if ln_w.numel() != c or head_w.numel() != c:
        raise TrambaHipError("shuffle_norm_head_bwd_cl: parameter vectors of another length than C")
    nparts = lib().tramba_shuffle_norm_head_bwd_parts(bb, h, wd, c, p, dt(x))
    if nparts <= 0:
        raise TrambaHipError(f"shuffle_norm_head_bwd_cl: C = {c} is not served by the rows kernel")
    dx = torch.empty_like(x)
    part = torch.empty((nparts, c + 4), dtype=torch.float32, device=x.device)
    _check(lib().tramba_shuffle_norm_head_bwd_cl(_ptr(x), _ptr(g), _ptr(ln_w), _ptr(head_w), _ptr(dx), _ptr(part), bb, h, wd, c, p,
                                                 eps, dt(x), _stream()), "shuffle_norm_head_bwd_cl")
    return dx, part


def shuffle_norm_head_ok(x, c):
    """shapes the fused norm + head pair serves: C a multiple of 8 (4 for f32) on at most 64 lanes"""
    vm = 4 if x.dtype == torch.float32 else 8
    return x.is_cuda and c % vm == 0 and c // vm <= 64


def expand_norm_head_cl(x, w, ln_w, ln_b, head_w, head_b: float, p, eps=1e-5):
    """x (B,H,W,Cin) 16-bit, w (P*P*128, Cin) -> (B, H*P, W*P) f32: expand GEMM + pixel shuffle + LayerNorm(128) + head."""
    _dev(x, w, ln_w, ln_b, head_w)
    bb, h, wd, cin = x.shape
    if w.shape != (p * p * 128, cin) or w.dtype != x.dtype or ln_w.numel() != 128 or head_w.numel() != 128:
        raise TrambaHipError("expand_norm_head_cl: needs 128-channel groups and a (P*P*128, Cin) weight")
    y = torch.empty((bb, h * p, wd * p), dtype=torch.float32, device=x.device)
    _check(lib().tramba_expand_norm_head_cl(_ptr(x), _ptr(w), _ptr(ln_w), _ptr(ln_b), _ptr(head_w), float(head_b), _ptr(y),
                                            bb, h, wd, cin, p, eps, dt(x), _stream()), "expand_norm_head_cl")
    return y


EVAL_NINT, EVAL_NDBL = 520, 48


def saliency_stats(pred, gt):
    """pred (B, H, W) f32 = sigmoid(logits), gt (B, H, W) bool / u8 -> (ints (B, 520) i64, dbl (B, 48) f64) on the
    device: the per-image statistics behind MAE / F / E / S-measure (layout: include/tramba_hip.h)."""
    if pred.dtype != torch.float32 or pred.dim() != 3 or gt.shape != pred.shape:
        raise TrambaHipError("saliency_stats: pred must be (B, H, W) float32 and gt the same shape")
    pred = pred.contiguous()
    g8 = (gt if gt.dtype == torch.bool else gt != 0).contiguous().view(torch.uint8)
    _dev(pred, g8)
    b, h, w = pred.shape
    ints = torch.empty((b, EVAL_NINT), dtype=torch.int64, device=pred.device)
    dbl = torch.empty((b, EVAL_NDBL), dtype=torch.float64, device=pred.device)
    _check(lib().tramba_saliency_stats(_ptr(pred), _ptr(g8), _ptr(ints), _ptr(dbl), b, h, w, _stream()), "saliency_stats")
    return ints, dbl


WFM_MAX_DIM = 4096     # TRAMBA_WFM_MAX_DIM


def _mask_u8(what, gt, shape=None):
    if gt.dtype not in (torch.bool, torch.uint8) or gt.dim() != 3 or (shape is not None and gt.shape != shape):
        raise TrambaHipError(f"{what}: gt must be a (B, H, W) bool / uint8 mask" +
                             (f" of the prediction's shape {tuple(shape)}" if shape is not None else "") +
                             f", got {gt.dtype} {tuple(gt.shape)}")
    b, h, w = gt.shape
    if not (0 < b <= 65535 and 0 < h <= WFM_MAX_DIM and 0 < w <= WFM_MAX_DIM):
        raise TrambaHipError(f"{what}: shape {tuple(gt.shape)} outside 1 .. {WFM_MAX_DIM} per side")
    gt = gt.contiguous()
    _dev(gt)
    return gt.view(torch.uint8)


def feature_transform(gt):
    """gt (B, H, W) bool / u8 -> (idx, dist2), both (B, H, W) int32 on the device: the flat index r * W + c of the nearest
    non-zero pixel and its squared distance, index for index what scipy.ndimage.distance_transform_edt(gt == 0,
    return_indices=True) gives (ties included).  An image with no non-zero pixel gets -1 everywhere."""
    g8 = _mask_u8("feature_transform", gt)
    b, h, w = g8.shape
    idx = torch.empty((b, h, w), dtype=torch.int32, device=g8.device)
    dist2 = torch.empty_like(idx)
    _check(lib().tramba_feature_transform(_ptr(g8), _ptr(idx), _ptr(dist2), b, h, w, _stream()), "feature_transform")
    return idx, dist2


def _gauss7():
    """Evaluation/metrics.py:429-441 matlab_style_gauss2D((7, 7), sigma=5), row-major, fp64"""
    y, x = np.ogrid[-3:4, -3:4]
    g = np.exp(-(x * x + y * y) / (2 * 5 * 5))
    g[g < np.finfo(g.dtype).eps * g.max()] = 0
    if g.sum() != 0:
        g /= g.sum()
    return np.ascontiguousarray(g, dtype=np.float64).ravel()


_GAUSS7 = _gauss7()


def weighted_f_sums(pred, gt):
    """pred (B, H, W) f32 = sigmoid(logits), gt (B, H, W) bool / u8 -> sums (B, 3) f64 on the device:
    { sum gt, sum Ew[gt], sum Ew[~gt] } of the weighted F-measure (layout: include/tramba_hip.h)."""
    if pred.dtype != torch.float32 or pred.dim() != 3:
        raise TrambaHipError(f"weighted_f_sums: pred must be (B, H, W) float32, got {pred.dtype} {tuple(pred.shape)}")
    pred = pred.contiguous()
    _dev(pred)
    g8 = _mask_u8("weighted_f_sums", gt, pred.shape)
    if g8.device != pred.device:
        raise TrambaHipError("weighted_f_sums: pred and gt are on different devices")
    b, h, w = pred.shape
    idx, dist2 = feature_transform(g8)
    ws = torch.empty(lib().tramba_weighted_f_workspace(b, h, w), dtype=torch.uint8, device=pred.device)
    sums = torch.empty((b, 3), dtype=torch.float64, device=pred.device)
    _check(lib().tramba_weighted_f_sums(_ptr(pred), _ptr(g8), _ptr(idx), _ptr(dist2), _GAUSS7.ctypes.data, _ptr(sums),
                                        _ptr(ws), ws.numel(), b, h, w, _stream()), "weighted_f_sums")
    return sums


FRAME_MAX_DIM, FRAME_MAX_OUT = 16384, 2048     # TRAMBA_FRAME_MAX_DIM / TRAMBA_FRAME_MAX_OUT


def resize_table_host(in_h: int, in_w: int, out_h: int, out_w: int, mean, std) -> np.ndarray:
    """int32 host table of tramba_frames_to_input for one (frame size, output size): PIL's bilinear fixed-point weights per
    axis and the 3 x 256 normalisation table (layout: csrc/frames.hip), computed by the library in fp64."""
    words = lib().tramba_resize_table_words(in_h, in_w, out_h, out_w)
    if words == 0:
        raise TrambaHipError(f"resize_table: {in_h}x{in_w} -> {out_h}x{out_w} outside 1 .. {FRAME_MAX_DIM} per frame side, "
                             f"1 .. {FRAME_MAX_OUT} per output side")
    mean = np.ascontiguousarray(mean, dtype=np.float64)
    std = np.ascontiguousarray(std, dtype=np.float64)
    if mean.shape != (3,) or std.shape != (3,):
        raise TrambaHipError("resize_table: mean and std need 3 values each")
    out = np.empty(words, dtype=np.int32)
    _check(lib().tramba_resize_table(in_h, in_w, out_h, out_w, mean.ctypes.data, std.ctypes.data, out.ctypes.data, words),
           "resize_table")
    return out


def frames_to_input(frames, table, out_h: int, out_w: int, bgr: bool = False):
    """frames (B, H, W, 3) u8 on the device + the device copy of resize_table_host(H, W, out_h, out_w, ...) ->
    (B, 3, out_h, out_w) f32: the loader's test transform (resize + normalisation), bit for bit."""
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3:
        raise TrambaHipError(f"frames_to_input: frames must be (B, H, W, 3) uint8, got {frames.dtype} {tuple(frames.shape)}")
    _dev(frames, table)
    b, h, w, _ = frames.shape
    if not (0 < b <= 65535 and 0 < h <= FRAME_MAX_DIM and 0 < w <= FRAME_MAX_DIM):
        raise TrambaHipError(f"frames_to_input: frames {tuple(frames.shape)} outside 1 .. {FRAME_MAX_DIM} per side")
    if table.dtype != torch.int32 or table.numel() < lib().tramba_resize_table_words(h, w, out_h, out_w):
        raise TrambaHipError("frames_to_input: table does not belong to these sizes")
    out = torch.empty((b, 3, out_h, out_w), dtype=torch.float32, device=frames.device)
    _check(lib().tramba_frames_to_input(_ptr(frames), _ptr(table), _ptr(out), b, h, w, out_h, out_w, int(bool(bgr)),
                                        _stream()), "frames_to_input")
    return out


def logits_to_u8(logits, h: int, w: int):
    """logits (B, 1, S, S') f32 / f16 / bf16 on the device -> (B, h, w) u8 =
    uint8(sigmoid(F.interpolate(logits.float(), (h, w), mode="bilinear", align_corners=False)) * 255)."""
    if logits.dim() != 4 or logits.shape[1] != 1:
        raise TrambaHipError(f"logits_to_u8: logits must be (B, 1, H, W), got {tuple(logits.shape)}")
    logits = logits.contiguous()
    _dev(logits)
    b, _, ih, iw = logits.shape
    out = torch.empty((b, h, w), dtype=torch.uint8, device=logits.device)
    _check(lib().tramba_logits_to_u8(_ptr(logits), _ptr(out), b, ih, iw, h, w, dt(logits), _stream()), "logits_to_u8")
    return out


FRAMES_DESC_WORDS = 16                               # TRAMBA_FRAMES_DESC_WORDS
RAGGED_IN, RAGGED_OUT = 1, 2                         # TRAMBA_RAGGED_IN / TRAMBA_RAGGED_OUT


def _ragged_desc(what, desc_host):
    desc_host = np.ascontiguousarray(desc_host, dtype=np.int64)
    if desc_host.ndim != 2 or desc_host.shape[1] != FRAMES_DESC_WORDS or not 1 <= desc_host.shape[0] <= 65535:
        raise TrambaHipError(f"{what}: descriptors must be (B, {FRAMES_DESC_WORDS}) with 1 <= B <= 65535")
    return desc_host


def frames_ragged_check(desc_host: np.ndarray, size: int, packed_bytes: int, out_capacity: int,
                        parts: int = RAGGED_IN | RAGGED_OUT):
    """the library's check of a packed batch's host descriptors (layout: include/tramba_hip.h) against the sizes of the
    packed buffer and of the output buffer; raises TrambaHipError.  Call it before replaying a graph, where no entry runs."""
    desc_host = _ragged_desc("frames_ragged_check", desc_host)
    _check(lib().tramba_frames_ragged_check(desc_host.ctypes.data, desc_host.shape[0], size, packed_bytes, out_capacity,
                                            parts), "frames_ragged_check")


def frames_to_input_ragged(packed, desc_host: np.ndarray, size: int, bgr: bool = False):
    """packed (N,) u8 on the device (descriptors, tables, frames of any sizes), desc_host its (B, FRAMES_DESC_WORDS) int64
    host copy -> (B, 3, size, size) f32: row i is frames_to_input of frame i alone, bit for bit."""
    if packed.dtype != torch.uint8 or packed.dim() != 1:
        raise TrambaHipError(f"frames_to_input_ragged: packed must be a flat uint8 tensor, got {packed.dtype} {tuple(packed.shape)}")
    _dev(packed)
    desc_host = _ragged_desc("frames_to_input_ragged", desc_host)
    b = desc_host.shape[0]
    if not 3 <= size <= FRAME_MAX_OUT:
        raise TrambaHipError(f"frames_to_input_ragged: size {size} outside 3 .. {FRAME_MAX_OUT}")
    out = torch.empty((b, 3, size, size), dtype=torch.float32, device=packed.device)
    _check(lib().tramba_frames_to_input_ragged(_ptr(packed), desc_host.ctypes.data, packed.numel(), _ptr(out), b, size,
                                               int(bool(bgr)), _stream()), "frames_to_input_ragged")
    return out


def logits_to_u8_ragged(logits, packed, desc_host: np.ndarray, out):
    """logits (B, 1, S, S) f32 / f16 / bf16, packed: a device buffer that starts with the descriptors, desc_host their host
    copy, out: a flat u8 device buffer -> out, with map i = logits_to_u8(logits[i:i+1], h_i, w_i) at the byte offset
    descriptor i names.  Bytes of out between the maps are left as they are."""
    if logits.dim() != 4 or logits.shape[1] != 1 or logits.shape[2] != logits.shape[3]:
        raise TrambaHipError(f"logits_to_u8_ragged: logits must be (B, 1, S, S), got {tuple(logits.shape)}")
    if packed.dtype != torch.uint8 or packed.dim() != 1 or out.dtype != torch.uint8 or out.dim() != 1:
        raise TrambaHipError("logits_to_u8_ragged: packed and out must be flat uint8 tensors")
    logits = logits.contiguous()
    _dev(logits, packed, out)
    desc_host = _ragged_desc("logits_to_u8_ragged", desc_host)
    b, _, s, _ = logits.shape
    if desc_host.shape[0] != b or packed.numel() < desc_host.nbytes:
        raise TrambaHipError(f"logits_to_u8_ragged: {desc_host.shape[0]} descriptors for {b} logit planes")
    _check(lib().tramba_logits_to_u8_ragged(_ptr(logits), _ptr(packed), desc_host.ctypes.data, _ptr(out), out.numel(), b, s,
                                            dt(logits), _stream()), "logits_to_u8_ragged")
    return out


AUG_DESC_WORDS = 32                                  # TRAMBA_AUG_DESC_WORDS
AUG_CONTRAST, AUG_BRIGHTNESS, AUG_SHARPNESS = 0, 1, 2


def _aug_size(what, size):
    if not 3 <= size <= FRAME_MAX_OUT:
        raise TrambaHipError(f"{what}: size {size} outside 3 .. {FRAME_MAX_OUT}")


def augment_source_table_host(h: int, w: int, size: int) -> np.ndarray:
    """int32 host table of one source size (h, w) -> (size, size) for augment_batch: the bilinear words of the image and
    Pillow's nearest indices of the mask (layout: include/tramba_hip.h), computed by the library in fp64."""
    words = lib().tramba_augment_source_table_words(h, w, size)
    if words == 0:
        raise TrambaHipError(f"augment_source_table: {h}x{w} -> {size} outside 1 .. {FRAME_MAX_DIM} per source side, "
                             f"3 .. {FRAME_MAX_OUT} for the output side")
    out = np.empty(words, dtype=np.int32)
    _check(lib().tramba_augment_source_table(h, w, size, out.ctypes.data, words), "augment_source_table")
    return out


def augment_size_table_host(size: int, mean, std) -> np.ndarray:
    """int32 host table of one output side: normalisation, label and SMOOTH tables and the bicubic S -> R axis table of
    every reachable R (layout: include/tramba_hip.h)."""
    _aug_size("augment_size_table", size)
    words = lib().tramba_augment_size_table_words(size)
    mean = np.ascontiguousarray(mean, dtype=np.float64)
    std = np.ascontiguousarray(std, dtype=np.float64)
    if mean.shape != (3,) or std.shape != (3,):
        raise TrambaHipError("augment_size_table: mean and std need 3 values each")
    out = np.empty(words, dtype=np.int32)
    _check(lib().tramba_augment_size_table(size, mean.ctypes.data, std.ctypes.data, out.ctypes.data, words),
           "augment_size_table")
    return out


def augment_scale_taps(size: int, r: int) -> int:
    return _check(lib().tramba_augment_scale_taps(size, r), "augment_scale_taps")


def augment_rotation(size: int, degrees: int) -> np.ndarray:
    """the 6 16.16 words of Image.rotate(degrees, expand=True) + centre crop on a (size, size) image"""
    out = np.empty(6, dtype=np.int32)
    _check(lib().tramba_augment_rotation(size, degrees, out.ctypes.data), "augment_rotation")
    return out


def augment_workspace_bytes(batch: int, size: int) -> int:
    _aug_size("augment_workspace", size)
    if not 1 <= batch <= 65535:
        raise TrambaHipError(f"augment_workspace: batch {batch} outside 1 .. 65535")
    return lib().tramba_augment_workspace(batch, size)


def augment_batch(packed, desc_host: np.ndarray, size_table, size: int, workspace):
    """packed (N,) u8 on the device (descriptors, then the pairs' bytes), desc_host its (B, AUG_DESC_WORDS) int64 host copy,
    size_table the device copy of augment_size_table_host(size), workspace >= augment_workspace_bytes(B, size) bytes ->
    (image (B, 3, size, size) f32, label (B, 1, size, size) f32): the loader's train transform for the recorded draws."""
    _aug_size("augment_batch", size)
    if packed.dtype != torch.uint8 or packed.dim() != 1:
        raise TrambaHipError(f"augment_batch: packed must be a flat uint8 tensor, got {packed.dtype} {tuple(packed.shape)}")
    _dev(packed, size_table, workspace)
    desc_host = np.ascontiguousarray(desc_host, dtype=np.int64)
    if desc_host.ndim != 2 or desc_host.shape[1] != AUG_DESC_WORDS or not 1 <= desc_host.shape[0] <= 65535:
        raise TrambaHipError(f"augment_batch: descriptors must be (B, {AUG_DESC_WORDS}) with 1 <= B <= 65535")
    b = desc_host.shape[0]
    hw = desc_host[:, 2:4]
    if (hw < 1).any() or (hw > FRAME_MAX_DIM).any():
        raise TrambaHipError(f"augment_batch: a source side is outside 1 .. {FRAME_MAX_DIM}")
    if size_table.dtype != torch.int32 or size_table.numel() < lib().tramba_augment_size_table_words(size):
        raise TrambaHipError("augment_batch: size_table does not belong to this size")
    if workspace.numel() * workspace.element_size() < lib().tramba_augment_workspace(b, size):
        raise TrambaHipError("augment_batch: workspace too small")
    image = torch.empty((b, 3, size, size), dtype=torch.float32, device=packed.device)
    label = torch.empty((b, 1, size, size), dtype=torch.float32, device=packed.device)
    _check(lib().tramba_augment_batch(_ptr(packed), desc_host.ctypes.data, packed.numel(), _ptr(size_table), _ptr(image),
                                      _ptr(label), _ptr(workspace), workspace.numel() * workspace.element_size(), b, size,
                                      _stream()), "augment_batch")
    return image, label


def rowdot_cl(x, w, bias: float):
    """x: (..., C); w: (C) f32 -> (...) f32 = <x, w> + bias."""
    _dev(x, w)
    c = x.shape[-1]
    y = torch.empty(x.shape[:-1], dtype=torch.float32, device=x.device)
    _check(lib().tramba_rowdot_cl(_ptr(x), _ptr(w), float(bias), _ptr(y), x.numel() // c, c, dt(x), _stream()), "rowdot_cl")
    return y


def rowdot_bwd_ok(x):
    """does the one-pass backward kernel of rowdot_cl serve this map? (rows of at most 64 x 16 bytes)"""
    c = x.shape[-1]
    return x.is_cuda and lib().tramba_rowdot_bwd_parts(x.numel() // c, c, dt(x)) > 0


def rowdot_bwd_cl(x, gy, w):
    """backward of rowdot_cl: x (..., C), gy (...) f32, w (C) f32 -> (gx like x, gw (C) f32, gb () f32)"""
    _dev(x, gy, w)
    c = x.shape[-1]
    rows = x.numel() // c
    if gy.dtype != torch.float32 or gy.numel() != rows:
        raise TrambaHipError("rowdot_bwd_cl: gy must be float32 with one entry per row")
    nparts = lib().tramba_rowdot_bwd_parts(rows, c, dt(x))
    if nparts <= 0:
        raise TrambaHipError(f"rowdot_bwd_cl: C={c} is not served")
    gx = torch.empty_like(x)
    part = torch.empty((nparts, c + 4), dtype=torch.float32, device=x.device)
    _check(lib().tramba_rowdot_bwd_cl(_ptr(x), _ptr(gy), _ptr(w), _ptr(gx), _ptr(part), rows, c, dt(x), _stream()),
           "rowdot_bwd_cl")
    s_ = slab_sum(part)
    return gx, s_[:c], s_[c]


def dw_pack(w, bias=None, w3=None, b3=None, w5=None, b5=None):
    """Reference-layout depth-wise weights (C,1,ks,ks) -> tap-major (ks*ks, C) f32 + bias (C) f32.
    With w3/b3/w5/b5 given (ks=7): the folded multi-scale stencil of DWMSMlp."""
    ts = [_f32(t) for t in (w, bias, w3, b3, w5, b5)]
    _dev(*ts)
    c, ks = w.shape[0], w.shape[-1]
    wt = torch.empty((ks * ks, c), dtype=torch.float32, device=w.device)
    bt = torch.empty((c,), dtype=torch.float32, device=w.device)
    _check(lib().tramba_dw_pack(*[_ptr(t) for t in ts], _ptr(wt), _ptr(bt), c, ks, _stream()), "dw_pack")
    return wt, bt


def dw_pack_multi_check(items):
    for it in items:
        _dev(*it)
        if any(t is not None and t.dtype != torch.float32 for t in it):
            raise TrambaHipError("dw_pack_multi: fp32 tensors only")
        c, ks = it[0].shape[0], it[0].shape[-1]
        if tuple(it[6].shape) != (ks * ks, c) or it[7].numel() != c:
            raise TrambaHipError("dw_pack_multi: output shapes do not match the weights")


def dw_pack_multi(items):
    """items: [(w, bias, w3, b3, w5, b5, wt, bt)] -- `dw_pack` of every item into its (preallocated) wt (ks*ks, C) / bt (C) f32,
    all in one launch per 40 items (tramba_dw_pack_multi); fp32 device tensors, None where dw_pack takes none."""
    if len(items) == 0:
        return
    dw_pack_multi_check(items)
    dw_pack_multi_run(dw_pack_multi_prepare(items, _checked=True))


def dw_pack_multi_prepare(items, _checked=False):
    """the host arrays of one dw_pack_multi call, built once for a fixed set of tensors (`dw_pack_multi_run` launches them)"""
    if not _checked:
        dw_pack_multi_check(items)
    n = len(items)
    cols = [(ctypes.c_void_p * n)(*[_ptr(it[k]) for it in items]) for k in range(8)]
    cs = (ctypes.c_int * n)(*[it[0].shape[0] for it in items])
    kss = (ctypes.c_int * n)(*[it[0].shape[-1] for it in items])
    return (cols, cs, kss, n, tuple(items))        # (the tensors stay referenced)


def dw_pack_multi_run(prepared):
    cols, cs, kss, n, _ = prepared
    _check(lib().tramba_dw_pack_multi(*cols, cs, kss, n, _stream()), "dw_pack_multi")


def dwconv_cl(x, wt, bt, act=ACT_NONE):
    """x: (B, H, W, C); wt: (ks*ks, C) f32 tap-major, bt: (C) f32 (see dw_pack)."""
    _dev(x, wt, bt)
    bb, h, wd, c = x.shape
    ks = int(round(wt.shape[0] ** 0.5))
    if wt.shape != (ks * ks, c) or bt.shape != (c,):
        raise TrambaHipError(f"dwconv_cl: packed weight {tuple(wt.shape)} does not match C={c}")
    y = torch.empty_like(x)
    _check(lib().tramba_dwconv_cl(_ptr(x), _ptr(wt), _ptr(bt), _ptr(y), bb, h, wd, c, ks, act, dt(x), _stream()),
           "dwconv_cl")
    return y


def dwconv_dual_cl(x, wt, bt, act=ACT_NONE, want_pre=True, flip=False):
    """(pre, act(pre)): the stencil's output before and after its activation from one launch; flip: mirrored taps (the
    stencil's adjoint: its input gradient)."""
    _dev(x, wt, bt)
    bb, h, wd, c = x.shape
    ks = int(round(wt.shape[0] ** 0.5))
    if wt.shape != (ks * ks, c) or bt.shape != (c,):
        raise TrambaHipError(f"dwconv_dual_cl: packed weight {tuple(wt.shape)} does not match C={c}")
    pre = torch.empty_like(x) if want_pre else None
    y = torch.empty_like(x)
    _check(lib().tramba_dwconv_dual_cl(_ptr(x), _ptr(wt), _ptr(bt), _ptr(pre), _ptr(y), bb, h, wd, c, ks, act, int(flip),
                                       dt(x), _stream()), "dwconv_dual_cl")
    return pre, y


def dw_unpack_grad(gwt, ks, multiscale=False, nbias=0, defer=False):
    """gwt (ks*ks + 1, C) f32 tap-major taps + bias row -> (g7 (C,1,ks,ks), g5, g3 (multi-scale fold, else None), gb (nbias, C)).
    defer: inside `deferred_sums()` the unpack is recorded and runs at `flush_sums()`, after the recorded sums (gwt may be
    the output of one), all unpacks of the pass in one launch -- for results that go straight to autograd as leaf gradients."""
    _dev(gwt)
    c = gwt.shape[1]
    g7 = torch.empty((c, 1, ks, ks), dtype=torch.float32, device=gwt.device)
    g5 = torch.empty((c, 1, 5, 5), dtype=torch.float32, device=gwt.device) if multiscale else None
    g3 = torch.empty((c, 1, 3, 3), dtype=torch.float32, device=gwt.device) if multiscale else None
    gb = torch.empty((nbias, c), dtype=torch.float32, device=gwt.device) if nbias else None
    if defer and _sumq.enabled:
        if gwt.dtype != torch.float32 or tuple(gwt.shape) != (ks * ks + 1, c):
            raise TrambaHipError("dw_unpack_grad: gradient table of another shape")
        if _sumq.poison:
            for t in (g7, g5, g3, gb):
                if t is not None:
                    t.fill_(float("nan"))
        with _sumq.lock:
            _sumq.unpacks.append((_ptr(gwt), _ptr(g7), _ptr(g5), _ptr(g3), _ptr(gb), int(nbias), int(c), int(ks), _stream(),
                                  (gwt, g7, g5, g3, gb)))
        # VIEWS go out, the queue keeps the bases: autograd hands a leaf the incoming gradient as it is (no copy) only when
        # nobody else references that tensor object -- a copy would read the buffer before the flush has filled it
        # (tests/test_gpu_grad.py NaN-fills deferred outputs to catch exactly that)
        return tuple(None if t is None else t.view(t.shape) for t in (g7, g5, g3, gb))
    _check(lib().tramba_dw_unpack_grad(_ptr(gwt), _ptr(g7), _ptr(g5), _ptr(g3), _ptr(gb), nbias, c, ks, _stream()),
           "dw_unpack_grad")
    return g7, g5, g3, gb


def upsample_bilinear_bwd(gout, h, w):
    """gout (..., H, W) f32 = gradient of F.interpolate(x (..., h, w), (H, W), mode="bilinear") -> gradient of x."""
    _dev(gout)
    gout = gout.contiguous()
    hh, ww = gout.shape[-2:]
    planes = gout.numel() // (hh * ww)
    gin = torch.empty(gout.shape[:-2] + (h, w), dtype=torch.float32, device=gout.device)
    if gout.dtype != torch.float32:
        raise TrambaHipError("upsample_bilinear_bwd: fp32 gradients only")
    _check(lib().tramba_upsample_bilinear_bwd(_ptr(gout), _ptr(gin), planes, h, w, hh, ww, _stream()), "upsample_bilinear_bwd")
    return gin


def _loss_nblk(npix):
    """workgroups per plane of tramba_sod_loss_sums: ~1024 pixels each"""
    return max(1, min(256, (npix + 1023) // 1024))


def _loss_check(what, tensors, label, maps):
    """what both forms of the loss ask of their tensors.  maps: (wmap,) for the weighted form, () for the unweighted.
    Returns planes, H, W of the label."""
    _dev(label, *maps, *tensors)
    if any(t.dtype != torch.float32 for t in (label, *maps, *tensors)):
        raise TrambaHipError(f"{what}: fp32 logits, labels and weights only" if maps else f"{what}: fp32 logits and labels only")
    for wmap in maps:
        if wmap.shape != label.shape:
            raise TrambaHipError(f"{what}: the weight map {tuple(wmap.shape)} does not match the label {tuple(label.shape)}")
    hh, ww = label.shape[-2:]
    planes = label.numel() // (hh * ww)
    for i, o in enumerate(tensors):
        h, w = o.shape[-2:]
        if o.numel() != planes * h * w or h > hh or w > ww:
            raise TrambaHipError(f"{what}: output {i} {tuple(o.shape)} does not match the label {tuple(label.shape)}")
    return planes, hh, ww


def _sod_loss(what, outputs, label, maps, weights, sums_form=(), finish_form=()):
    """tramba_<what>_sums per output, then tramba_<what>_finish: `sod_loss` with 3 sums per block and plane, `sod_wloss`
    with 5 and the form arguments its two entries take after the shapes"""
    nout = len(outputs)
    if not 0 < nout <= 8:
        raise TrambaHipError(f"{what}: 1..8 outputs, got {nout}")
    planes, hh, ww = _loss_check(what, outputs, label, maps)
    nblk = _loss_nblk(hh * ww)
    stream = _stream()
    parts = torch.empty((nout, planes, nblk, 5 if maps else 3), dtype=torch.float32, device=label.device)
    coefs = torch.empty((nout, planes, 4), dtype=torch.float32, device=label.device)
    sums, finish = getattr(lib(), f"tramba_{what}_sums"), getattr(lib(), f"tramba_{what}_finish")
    for i, o in enumerate(outputs):
        h, w = o.shape[-2:]
        _check(sums(_ptr(o), _ptr(label), *map(_ptr, maps), parts[i].data_ptr(), planes, h, w, hh, ww, nblk, *sums_form, stream),
               f"{what}_sums")
    loss = torch.empty((), dtype=torch.float32, device=label.device)
    pp = (ctypes.c_void_p * nout)(*[parts[i].data_ptr() for i in range(nout)])
    cc = (ctypes.c_void_p * nout)(*[coefs[i].data_ptr() for i in range(nout)])
    nb = (ctypes.c_int * nout)(*([nblk] * nout))
    wt = None if weights is None else (ctypes.c_float * nout)(*[float(w) for w in weights])
    _check(finish(pp, nb, wt, cc, nout, planes, hh * ww, *finish_form, _ptr(loss), stream), f"{what}_finish")
    return loss, coefs


def _sod_loss_grad(what, output, label, maps, coef, gscale, form=()):
    """tramba_<what> for `sod_loss_grad` and `sod_wloss_grad`, the latter with its weight map and form arguments"""
    planes, hh, ww = _loss_check(what, (output,), label, maps)
    _dev(coef, gscale)
    if gscale is not None and (gscale.dtype != torch.float32 or gscale.numel() != 1):
        raise TrambaHipError(f"{what}: the incoming gradient must be one fp32 scalar")
    h, w = output.shape[-2:]
    g = torch.empty_like(output)
    nbytes = getattr(lib(), f"tramba_{what}_workspace")(planes, h, w, hh, ww)
    ws = torch.empty((nbytes // 4,), dtype=torch.float32, device=output.device) if nbytes else None
    _check(getattr(lib(), f"tramba_{what}")(_ptr(output), _ptr(label), *map(_ptr, maps), _ptr(coef), _ptr(gscale), _ptr(g),
                                            _ptr(ws), nbytes, planes, h, w, hh, ww, *form, _stream()), what)
    return g


def sod_loss(outputs, label, weights=None):
    """The deep-supervision loss of train.py:76-85 (every output resized to the label, BCE-with-logits + IoU, summed with
    `weights`): outputs = fp32 (B, C, h_i, w_i) logit maps, label (B, C, H, W) f32.  Returns (loss 0-dim f32, coefs): coefs[i]
    (B*C, 4) feeds `sod_loss_grad`.  One launch per output + one finishing block."""
    return _sod_loss("sod_loss", outputs, label, (), weights)


def sod_loss_grad(output, label, coef, gscale=None):
    """d loss / d output for one output of `sod_loss` (coef = its row of the coefficient table), times the device scalar
    `gscale` (the gradient arriving at the loss)."""
    return _sod_loss_grad("sod_loss_grad", output, label, (), coef, gscale)


def loss_weight_map(label, k):
    """weit = 1 + 5 |avg_pool2d(label, k, stride 1, padding k // 2) - label| (utils/loss.py:22 with k = 31, :39 with k = 15):
    label (B, C, H, W) f32, odd k <= 63.  One launch; the map is shared by every deep-supervision output of a loss call."""
    _dev(label)
    if label.dtype != torch.float32 or label.dim() != 4:
        raise TrambaHipError("loss_weight_map: a (B, C, H, W) fp32 label")
    hh, ww = label.shape[-2:]
    weit = torch.empty_like(label)
    _check(lib().tramba_loss_weight_map(_ptr(label), _ptr(weit), label.numel() // (hh * ww), hh, ww, int(k), _stream()),
           "loss_weight_map")
    return weit


def sod_wloss(outputs, label, wmap, weights=None, eps=0.0, per_pixel=False, with_iou=True, weight_is_raw=False):
    """`sod_loss` for the weighted losses of utils/loss.py:14-42 (structure_loss: eps = 0.001, with_iou; wbce: eps = 0, no IoU
    term): wmap (B, C, H, W) f32 from `loss_weight_map`, or the caller's `weight` tensor with weight_is_raw (W = 1 + 5 wmap).
    per_pixel: the BCE term weighted pixel by pixel (the published form) instead of the reference as it executes (batch-mean
    BCE).  Returns (loss, coefs) as `sod_loss`; coefs feeds `sod_wloss_grad`."""
    return _sod_loss("sod_wloss", outputs, label, (wmap,), weights, (float(eps), int(bool(weight_is_raw))),
                     (int(bool(per_pixel)), int(bool(with_iou))))


def sod_wloss_grad(output, label, wmap, coef, gscale=None, eps=0.0, weight_is_raw=False):
    """d loss / d output for one output of `sod_wloss` (the same eps / weight_is_raw), times the device scalar `gscale`."""
    return _sod_loss_grad("sod_wloss_grad", output, label, (wmap,), coef, gscale, (float(eps), int(bool(weight_is_raw))))


def adam_step(params, grads, exp_avgs, exp_avg_sqs, steps, lr, beta1, beta2, eps, weight_decay=0.0, gscale=None, skip=None,
              ema=None, sched=None):
    """One Adam step on lists of fp32 device tensors (`adam_step_raw` on their pointer arrays); `steps` are the 0-dim fp32
    device counters of torch.optim.Adam's capturable state, `ema` a list of fp32 averages, one per parameter, or None."""
    n = len(params)
    if n == 0:
        return
    lists = (params, grads, exp_avgs, exp_avg_sqs) + (() if ema is None else (ema,))
    if not all(len(group) == n for group in lists + (steps,)):
        raise TrambaHipError("adam_step: the tensor lists differ in length")
    for group in lists + (steps,):
        for t in group:
            if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous():
                raise TrambaHipError("adam_step: contiguous fp32 tensors on a HIP device only (a sparse or strided gradient?)")
    for group in lists[1:]:
        for p, t in zip(params, group):
            if t.numel() != p.numel():
                raise TrambaHipError("adam_step: gradient / state / average of another size than the parameter")
    adam_step_raw(pointer_array(params), pointer_array(grads), pointer_array(exp_avgs), pointer_array(exp_avg_sqs),
                  pointer_array(steps), (ctypes.c_int64 * n)(*[t.numel() for t in params]), n, lr, beta1, beta2, eps,
                  weight_decay, gscale=gscale, skip=skip, ema=None if ema is None else pointer_array(ema), sched=sched)


def pointer_array(tensors):
    """host array of the tensors' device addresses, as the by-value multi-tensor entries take them"""
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def adam_step_raw(params, grads, exp_avgs, exp_avg_sqs, steps, numel, n, lr, beta1, beta2, eps, weight_decay=0.0, gscale=None,
                  skip=None, ema=None, sched=None):
    """`adam_step` on prepared pointer arrays (tramba_amd.train.Adam keeps those of the parameters and of the state between
    steps and rebuilds only the gradients'); the caller vouches for fp32, contiguous, same-size device tensors.
    `gscale` (fp32) / `skip` (int32): device scalars of a step-control record -- the gradient is multiplied by the first, a
    non-zero second makes the call change nothing.  `sched`: the record tensor of `step_sched_record` -- the step runs at
    lr * its lr_factor, read on the device when the kernel runs.  `ema`: a pointer array of fp32 averages, one per
    parameter, moved in the same pass by the record's ema_weight (needs `sched`).  One entry, tramba_adam_step_sched: with
    `ema` and `sched` None it runs the launches of tramba_adam_step_ctl, with all four None those of tramba_adam_step."""
    if gscale is not None and (gscale.dtype != torch.float32 or not gscale.is_cuda):
        raise TrambaHipError("adam_step: gscale is an fp32 scalar on the device")
    if skip is not None and (skip.dtype != torch.int32 or not skip.is_cuda):
        raise TrambaHipError("adam_step: skip is an int32 scalar on the device")
    if sched is not None and (sched.dtype != torch.int64 or not sched.is_cuda or sched.numel() * 8 < STEP_SCHED_BYTES):
        raise TrambaHipError("adam_step: sched is a tramba_step_sched record on the device (step_sched_record)")
    _check(lib().tramba_adam_step_sched(params, grads, exp_avgs, exp_avg_sqs, steps, numel, n, float(lr), float(beta1),
                                        float(beta2), float(eps), float(weight_decay), _ptr(gscale), _ptr(skip), ema,
                                        _ptr(sched), _stream()), "adam_step")


adam_step_sched, adam_step_sched_raw = adam_step, adam_step_raw      # second names of the same functions, still in use


STEP_CTL_BYTES = 24      # struct tramba_step_ctl: float norm, float scale, int32 skip, int32 micro, int64 skipped_steps


def step_ctl_record(device):
    """a zeroed tramba_step_ctl on `device` and typed 0-dim views of its fields:
    (record, {"norm", "scale": fp32, "skip", "micro": int32, "skipped_steps": int64})"""
    rec = torch.zeros(STEP_CTL_BYTES // 8, dtype=torch.int64, device=device)
    f, i = rec.view(torch.float32), rec.view(torch.int32)
    return rec, {"norm": f[0], "scale": f[1], "skip": i[2], "micro": i[3], "skipped_steps": rec[2]}


def grad_accumulate_raw(accs, grads, numel, n, ctl):
    """acc[i] = g[i] on the first micro-batch of a step (the record's counter is 0), acc[i] += g[i] afterwards; the counter
    advances.  Pointer arrays as `adam_step_raw` takes them; a null gradient pointer stands for zeros."""
    _check(lib().tramba_grad_accumulate(accs, grads, numel, n, ctl.data_ptr(), _stream()), "grad_accumulate")


def grad_norm_workspace(numel, n):
    return lib().tramba_grad_norm_workspace(numel, n)


def grad_norm_raw(grads, numel, n, mean_scale, max_norm, skip_nonfinite, ctl, workspace, ls=None):
    """global L2 norm of the tensors -> the record's norm / scale / skip (tramba_grad_norm_scaled); `workspace`: a device
    tensor of at least grad_norm_workspace() bytes.  `ls`: the loss-scale record whose scale the gradients carry -- norm
    and scale come out for the unscaled mean gradient, the un-scaling rides in the record's scale (None: as they are)."""
    _check(lib().tramba_grad_norm_scaled(grads, numel, n, float(mean_scale), float(max_norm or 0.0), int(bool(skip_nonfinite)),
                                         ctl.data_ptr(), _ptr(ls), workspace.data_ptr(),
                                         workspace.numel() * workspace.element_size(), _stream()), "grad_norm")


def grad_norm_scaled_raw(grads, numel, n, mean_scale, max_norm, skip_nonfinite, ctl, ls, workspace):
    return grad_norm_raw(grads, numel, n, mean_scale, max_norm, skip_nonfinite, ctl, workspace, ls)


LOSS_SCALE_BYTES = 24    # struct tramba_loss_scale: float scale, float inv_scale, int32 good_steps, int32 reserved, int64 backoffs


def loss_scale_record(device, init=1.0):
    """a tramba_loss_scale on `device` at scale `init` (a power of two) and typed 0-dim views of its fields:
    (record, {"scale", "inv_scale": fp32, "good_steps": int32, "backoffs": int64})"""
    m, _ = math.frexp(float(init))
    if m != 0.5 or not 2.0 ** -126 <= init <= 2.0 ** 126:
        raise TrambaHipError(f"loss_scale_record: the scale must be a power of two in 2^-126 .. 2^126 (got {init!r})")
    rec = torch.zeros(LOSS_SCALE_BYTES // 8, dtype=torch.int64, device=device)
    f, i = rec.view(torch.float32), rec.view(torch.int32)
    f[0], f[1] = float(init), 1.0 / float(init)
    return rec, {"scale": f[0], "inv_scale": f[1], "good_steps": i[2], "backoffs": rec[2]}


def loss_scale_update_raw(ls, ctl, growth, backoff, growth_interval, min_scale, max_scale):
    """the loss scale's move after an optimizer step, decided by the step-control record's skip flag on the device
    (tramba_loss_scale_update; a one-lane launch)"""
    _check(lib().tramba_loss_scale_update(ls.data_ptr(), ctl.data_ptr(), float(growth), float(backoff), int(growth_interval),
                                          float(min_scale), float(max_scale), _stream()), "loss_scale_update")


STEP_SCHED_BYTES = 24    # struct tramba_step_sched: int64 step, double lr_factor, float ema_weight, int32 reserved


def step_sched_record(device, step=0, lr_factor=1.0, ema_weight=0.0):
    """a tramba_step_sched on `device` and typed 0-dim views of its fields:
    (record, {"step": int64, "lr_factor": fp64, "ema_weight": fp32})"""
    rec = torch.zeros(STEP_SCHED_BYTES // 8, dtype=torch.int64, device=device)
    fields = {"step": rec[0], "lr_factor": rec.view(torch.float64)[1], "ema_weight": rec.view(torch.float32)[4]}
    fields["step"].fill_(int(step))
    fields["lr_factor"].fill_(float(lr_factor))
    fields["ema_weight"].fill_(float(ema_weight))
    return rec, fields


def _sched_table(what, table, dtype):
    if table is None:
        return None, 0
    if table.dtype != dtype or not table.is_cuda or table.dim() != 1 or not table.is_contiguous() or table.numel() < 1:
        raise TrambaHipError(f"step_sched_advance: the {what} table is a non-empty contiguous 1-d {dtype} tensor on the device")
    return table.data_ptr(), table.numel()


def step_sched_advance_raw(rec, lr_table=None, ema_table=None):
    """the schedule record's move after an optimizer step (tramba_step_sched_advance; a one-lane launch): step += 1, then
    lr_factor / ema_weight from the tables' entries at min(step, n - 1).  `lr_table` (fp64) / `ema_table` (fp32): device
    tensors; None: the factor becomes 1.0 / the weight stays."""
    lp, ln = _sched_table("lr", lr_table, torch.float64)
    ep, en = _sched_table("ema", ema_table, torch.float32)
    _check(lib().tramba_step_sched_advance(rec.data_ptr(), lp, ln, ep, en, _stream()), "step_sched_advance")


def im2col3x3_cl(x, stride, pad, ckp):
    """x (B,H,W,C) -> cols (B*Ho*Wo, ckp), column (ky*3 + kx)*C + ci, zeros for padding taps / alignment columns."""
    _dev(x)
    bb, h, wd, c = x.shape
    ho, wo = (h + 2 * pad - 3) // stride + 1, (wd + 2 * pad - 3) // stride + 1
    cols = torch.empty((bb * ho * wo, ckp), dtype=x.dtype, device=x.device)
    _check(lib().tramba_im2col3x3_cl(_ptr(x), _ptr(cols), bb, h, wd, c, stride, pad, ckp, dt(x), _stream()), "im2col3x3_cl")
    return cols


def col2im3x3_cl(gcols, shape, stride, pad):
    """gcols (B*Ho*Wo, CKp) -> gx of `shape` = (B,H,W,C): the adjoint of im2col3x3_cl."""
    _dev(gcols)
    bb, h, wd, c = shape
    gx = torch.empty(shape, dtype=gcols.dtype, device=gcols.device)
    _check(lib().tramba_col2im3x3_cl(_ptr(gcols), _ptr(gx), bb, h, wd, c, stride, pad, gcols.shape[1], dt(gcols), _stream()),
           "col2im3x3_cl")
    return gx


def dwconv_wgrad_cl(x, gy, ks):
    """x, gy: (B, H, W, C) -> (gw (ks*ks, C) f32 tap-major, gb (C) f32)."""
    _dev(x, gy)
    bb, h, wd, c = x.shape
    if gy.shape != x.shape or gy.dtype != x.dtype:
        raise TrambaHipError("dwconv_wgrad_cl: x / gy mismatch")
    part = torch.empty((lib().tramba_dwconv_wgrad_parts(bb, h, wd, c, ks), ks * ks + 1, c), dtype=torch.float32, device=x.device)
    _check(lib().tramba_dwconv_wgrad_cl(_ptr(x), _ptr(gy), _ptr(part), bb, h, wd, c, ks, dt(x), _stream()),
           "dwconv_wgrad_cl")
    s = slab_sum(part)
    return s[:ks * ks], s[ks * ks]


def dwconv_wgrad_table(x, gy, ks, defer=False):
    """the same as one (ks*ks + 1, C) f32 table (taps, then the bias row): the input of dw_unpack_grad (defer: the slab sum is
    recorded inside `deferred_sums()` -- only for a table that nothing but a deferred unpack reads)"""
    _dev(x, gy)
    bb, h, wd, c = x.shape
    if gy.shape != x.shape or gy.dtype != x.dtype:
        raise TrambaHipError("dwconv_wgrad_cl: x / gy mismatch")
    part = torch.empty((lib().tramba_dwconv_wgrad_parts(bb, h, wd, c, ks), ks * ks + 1, c), dtype=torch.float32, device=x.device)
    _check(lib().tramba_dwconv_wgrad_cl(_ptr(x), _ptr(gy), _ptr(part), bb, h, wd, c, ks, dt(x), _stream()),
           "dwconv_wgrad_cl")
    return slab_sum(part, defer=defer)


def dct_split_cl(x, wx, wy):
    """x: (B, n, n, C) -> (high, low), each (B, n/2, n/2, C)."""
    _dev(x, wx, wy)
    bb, n, n2, c = x.shape
    if n != n2 or n % 2:
        raise TrambaHipError(f"dct_split_cl: need an even square map, got {n}x{n2}")
    tmp = torch.empty((bb, n, n, c), dtype=torch.float32, device=x.device)
    high = torch.empty((bb, n // 2, n // 2, c), dtype=x.dtype, device=x.device)
    low = torch.empty_like(high)
    _check(lib().tramba_dct_split_cl(_ptr(x), _ptr(wx), _ptr(wy), _ptr(tmp), _ptr(high), _ptr(low), bb, n, c,
                                     dt(x), _stream()), "dct_split_cl")
    return high, low


def _check_epilogue(what, bias, residual, dtype, m, n):
    """the kernels read `bias` as (N) fp32 and `residual` as (M, N) in the INPUT dtype: anything else would be misread"""
    if bias is not None and (bias.dtype != torch.float32 or bias.numel() != n):
        raise TrambaHipError(f"{what}: bias must be float32 with {n} elements, got {bias.dtype} x {bias.numel()}")
    if residual is not None and (residual.dtype != dtype or residual.numel() != m * n):
        raise TrambaHipError(f"{what}: residual must be {dtype} with {m} x {n} elements, got {residual.dtype} x "
                             f"{residual.numel()}")


def _rowstat_extra(rowstat, dtype, out_dtype, m, n):
    """elements of the 16-bit output dtype that linear_cl / linear2_cl allocate behind y for the row-partial slab (0: no slab):
    y and its slab come from ONE allocation -- y's m * n elements, padding to 16 bytes, then (M, ceil(N / 64), 2) f32"""
    if not rowstat or out_dtype != dtype or dtype == torch.float32:
        return 0
    return (-(m * n)) % 8 + m * ((n + 63) // 64) * 4


def _rowstat_split(buf, shape, m, n):
    """(y, slab) views of such an allocation"""
    off = (m * n + 7) // 8 * 8
    return buf[:m * n].view(shape), buf[off:].view(torch.float32).view(m, (n + 63) // 64, 2)


def rowstat_for(x, k):
    """the slab a producer GEMM left on x (attribute set by linear_cl / linear2_cl(rowstat=True)), if it still describes x
    as the input of a GEMM over K = k: same tensor version, one 64-term partial per K step.  Else None."""
    tag = getattr(x, "_tramba_rowstat", None)
    if tag is None:
        return None
    slab, version = tag
    if version != x._version or k % 64 or slab.shape != (x.numel() // k, k // 64, 2) or slab.device != x.device:
        return None
    return slab


def linear_cl(x, w, bias=None, residual=None, act=ACT_NONE, out_dtype=None, rowstat=False):
    """x: (..., K); w: (N, K) same dtype; -> (..., N).  rowstat: the launch also leaves the row partials of y for the
    LayerNorm-folded GEMM that reads y next (tramba_linear_rowstat_cl) -- attached to y where the planned form can write
    them (see rowstat_for), silently absent where it cannot."""
    _dev(x, w, bias, residual)
    k = x.shape[-1]
    n = w.shape[0]
    m = x.numel() // k
    out_dtype = x.dtype if out_dtype is None else out_dtype
    extra = _rowstat_extra(rowstat, x.dtype, out_dtype, m, n)
    y = torch.empty((m * n + extra,) if extra else x.shape[:-1] + (n,), dtype=out_dtype, device=x.device)
    if w.dtype != x.dtype or w.shape[1] != k:
        raise TrambaHipError("linear_cl: weight dtype/shape mismatch")
    _check_epilogue("linear_cl", bias, residual, x.dtype, m, n)
    if extra:
        (y, slab), emitted = _rowstat_split(y, x.shape[:-1] + (n,), m, n), c_int(0)
        _check(lib().tramba_linear_rowstat_cl(_ptr(x), _ptr(w), _ptr(bias), _ptr(residual), _ptr(y), m, n, k, act, dt(x),
                                              dt(y), _ptr(slab), ctypes.byref(emitted), _stream()), "linear_cl")
        if emitted.value:
            y._tramba_rowstat = (slab, y._version)
        return y
    _check(lib().tramba_linear_cl(_ptr(x), _ptr(w), _ptr(bias), _ptr(residual), _ptr(y), m, n, k, act, dt(x),
                                  dt(y), _stream()), "linear_cl")
    return y


_ATTN_DTYPES = (torch.bfloat16, torch.float16)


def window_attention_supported(dtype, h, w, c, heads, ws, shift):
    """the argument checks of tramba_window_attn_cl, without the library: can the fused window attention take this shape?"""
    return (dtype in _ATTN_DTYPES and heads > 0 and c % heads == 0 and c // heads in (32, 64) and h > 0 and w > 0
            and 1 <= ws and ws * ws <= 256 and h % ws == 0 and w % ws == 0 and 0 <= shift < ws)


def kv_attention_supported(dtype, m, c, heads):
    """the argument checks of tramba_kv_attn_cl, without the library"""
    return dtype in _ATTN_DTYPES and heads > 0 and c % heads == 0 and c // heads in (32, 64) and 1 <= m <= 256


def window_attention_cl(qkv, table, ws, shift, heads):
    """qkv: (B, H, W, 3 C) as the qkv Linear writes it on the unpermuted map; table: ((2 ws - 1)^2, heads) f32 -> (B, H, W, C):
    shifted-window attention with the relative-position bias and the shift mask computed in the kernel."""
    _dev(qkv, table)
    if heads <= 0 or qkv.dim() != 4 or qkv.shape[-1] % (3 * heads):
        raise TrambaHipError(f"window_attention_cl: qkv must be (B, H, W, 3 * heads * hd), got {tuple(qkv.shape)}")
    b, h, w, c3 = qkv.shape
    if table.dtype != torch.float32 or tuple(table.shape) != ((2 * ws - 1) ** 2, heads):
        raise TrambaHipError(f"window_attention_cl: table must be float32 ({(2 * ws - 1) ** 2}, {heads}), got {table.dtype} "
                             f"{tuple(table.shape)}")
    y = torch.empty((b, h, w, c3 // 3), dtype=qkv.dtype, device=qkv.device)
    _check(lib().tramba_window_attn_cl(_ptr(qkv), _ptr(table), _ptr(y), b, h, w, heads, c3 // (3 * heads), ws, shift, dt(qkv),
                                       _stream()), "window_attention_cl")
    return y


def kv_attention_cl(q, kv, heads):
    """q: (B, N, C); kv: (B, M, 2 C) as the kv Linear writes it -> softmax(q k^T / sqrt(hd)) v, (B, N, C); heads by stride."""
    _dev(q, kv)
    if heads <= 0 or q.dim() != 3 or kv.dim() != 3 or kv.shape[0] != q.shape[0] or kv.shape[2] != 2 * q.shape[2] or kv.dtype != q.dtype \
            or q.shape[2] % heads:
        raise TrambaHipError(f"kv_attention_cl: need q (B, N, C) and kv (B, M, 2 C) of one dtype, got {tuple(q.shape)} "
                             f"{tuple(kv.shape)}")
    b, n, c = q.shape
    y = torch.empty_like(q)
    _check(lib().tramba_kv_attn_cl(_ptr(q), _ptr(kv), _ptr(y), b, n, kv.shape[1], heads, c // heads, dt(q), _stream()),
           "kv_attention_cl")
    return y


def window_attention_train_supported(dtype, h, w, c, heads, ws, shift):
    """can window_attention_bwd_cl take this shape?  The backward covers the forward's whole shape domain."""
    return window_attention_supported(dtype, h, w, c, heads, ws, shift)


def kv_attention_train_supported(dtype, m, c, heads):
    """can kv_attention_bwd_cl take this shape?  The backward covers the forward's whole shape domain."""
    return kv_attention_supported(dtype, m, c, heads)


def _attn_out(name, what, out, shape, dtype, device):
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    _dev(out)
    if tuple(out.shape) != tuple(shape) or out.dtype != dtype:
        raise TrambaHipError(f"{name}: {what} must be {dtype} {tuple(shape)}, got {out.dtype} {tuple(out.shape)}")
    return out


def window_attention_bwd_cl(qkv, table, dy, ws, shift, heads, need_table=True, out=None):
    """Backward of window_attention_cl from its inputs alone (the softmax rows are recomputed): qkv (B, H, W, 3 C), table
    ((2 ws - 1)^2, heads) f32, dy (B, H, W, C) -> (dqkv (B, H, W, 3 C), dtable f32 or None).  out: (dqkv, dtable) tensors to
    write into (dtable may be None); every element of both is written."""
    _dev(qkv, table, dy)
    if heads <= 0 or qkv.dim() != 4 or qkv.shape[-1] % (3 * heads):
        raise TrambaHipError(f"window_attention_bwd_cl: qkv must be (B, H, W, 3 * heads * hd), got {tuple(qkv.shape)}")
    b, h, w, c3 = qkv.shape
    if table.dtype != torch.float32 or tuple(table.shape) != ((2 * ws - 1) ** 2, heads):
        raise TrambaHipError(f"window_attention_bwd_cl: table must be float32 ({(2 * ws - 1) ** 2}, {heads}), got "
                             f"{table.dtype} {tuple(table.shape)}")
    if dy.dtype != qkv.dtype or tuple(dy.shape) != (b, h, w, c3 // 3):
        raise TrambaHipError(f"window_attention_bwd_cl: dy must be {qkv.dtype} {(b, h, w, c3 // 3)}, got {dy.dtype} "
                             f"{tuple(dy.shape)}")
    o_qkv, o_table = out if out is not None else (None, None)
    dqkv = _attn_out("window_attention_bwd_cl", "dqkv", o_qkv, qkv.shape, qkv.dtype, qkv.device)
    dtable = _attn_out("window_attention_bwd_cl", "dtable", o_table, table.shape, torch.float32, qkv.device) if need_table else None
    hd = c3 // (3 * heads)
    nbytes = lib().tramba_window_attn_bwd_work(b, h, w, heads, hd, ws) if need_table else 0
    work = torch.empty(nbytes, dtype=torch.uint8, device=qkv.device) if nbytes else None
    _check(lib().tramba_window_attn_bwd_cl(_ptr(qkv), _ptr(table), _ptr(dy), _ptr(dqkv), _ptr(dtable), _ptr(work), nbytes, b, h,
                                           w, heads, hd, ws, shift, dt(qkv), _stream()), "window_attention_bwd_cl")
    return dqkv, dtable


def kv_attention_bwd_cl(q, kv, dy, heads, out=None):
    """Backward of kv_attention_cl from its inputs alone: q (B, N, C), kv (B, M, 2 C), dy (B, N, C) -> (dq, dkv).  out: (dq,
    dkv) tensors to write into."""
    _dev(q, kv, dy)
    if heads <= 0 or q.dim() != 3 or kv.dim() != 3 or kv.shape[0] != q.shape[0] or kv.shape[2] != 2 * q.shape[2] or kv.dtype != q.dtype \
            or q.shape[2] % heads or dy.shape != q.shape or dy.dtype != q.dtype:
        raise TrambaHipError(f"kv_attention_bwd_cl: need q, dy (B, N, C) and kv (B, M, 2 C) of one dtype, got {tuple(q.shape)} "
                             f"{tuple(dy.shape)} {tuple(kv.shape)}")
    b, n, c = q.shape
    m = kv.shape[1]
    o_q, o_kv = out if out is not None else (None, None)
    dq = _attn_out("kv_attention_bwd_cl", "dq", o_q, q.shape, q.dtype, q.device)
    dkv = _attn_out("kv_attention_bwd_cl", "dkv", o_kv, kv.shape, q.dtype, q.device)
    nbytes = lib().tramba_kv_attn_bwd_work(b, n, m, heads, c // heads)
    work = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=q.device)
    _check(lib().tramba_kv_attn_bwd_cl(_ptr(q), _ptr(kv), _ptr(dy), _ptr(dq), _ptr(dkv), _ptr(work), nbytes, b, n, m, heads,
                                       c // heads, dt(q), _stream()), "kv_attention_bwd_cl")
    return dq, dkv


def linear_dual_ok(x, w):
    """can linear_dual_cl take this GEMM? (16-bit operands, whole 64-deep K steps, 16-byte rows)"""
    return (x.is_cuda and x.dtype in (torch.bfloat16, torch.float16) and w.dtype == x.dtype and x.shape[-1] % 64 == 0
            and w.shape[0] % 8 == 0 and x.is_contiguous() and w.is_contiguous())


def linear_dual_cl(x, w, bias, act):
    """x: (..., K); w: (N, K) -> (pre, act(pre)), both (..., N) in x's dtype, from one launch."""
    _dev(x, w, bias)
    k, n = x.shape[-1], w.shape[0]
    m = x.numel() // k
    if not linear_dual_ok(x, w) or w.shape[1] != k:
        raise TrambaHipError("linear_dual_cl: needs 16-bit contiguous operands with K % 64 == 0 and N % 8 == 0")
    _check_epilogue("linear_dual_cl", bias, None, x.dtype, m, n)
    y_pre = torch.empty(x.shape[:-1] + (n,), dtype=x.dtype, device=x.device)
    y_act = torch.empty_like(y_pre)
    _check(lib().tramba_linear_dual_cl(_ptr(x), _ptr(w), _ptr(bias), _ptr(y_pre), _ptr(y_act), m, n, k, act, dt(x), _stream()),
           "linear_dual_cl")
    return y_pre, y_act


def linear_ln_cl(x, w_folded, colsum, bias, eps, residual=None, act=ACT_NONE, out_dtype=None, rowstat=None):
    """act(LayerNorm(x) @ W^T + b) in one launch: w_folded = W * gamma (N, K) in x's dtype, colsum (N) f32 its row sums,
    bias (N) f32 = W @ beta + b (see include/tramba_hip.h).  rowstat: the (M, K / 64, 2) f32 slab of x's row partials its
    producer left (rowstat_for), or None = the GEMM derives the statistics itself."""
    _dev(x, w_folded, colsum, bias, residual)
    k = x.shape[-1]
    n = w_folded.shape[0]
    m = x.numel() // k
    if w_folded.dtype != x.dtype or w_folded.shape[1] != k or colsum.dtype != torch.float32 or colsum.numel() != n:
        raise TrambaHipError("linear_ln_cl: operand shapes / dtypes do not match")
    _check_epilogue("linear_ln_cl", bias, residual, x.dtype, m, n)
    out_dtype = x.dtype if out_dtype is None else out_dtype
    y = torch.empty(x.shape[:-1] + (n,), dtype=out_dtype, device=x.device)
    if rowstat is not None:
        if (rowstat.dtype != torch.float32 or rowstat.shape != (m, k // 64, 2) or k % 64 or not rowstat.is_contiguous()
                or rowstat.device != x.device):
            raise TrambaHipError(f"linear_ln_cl: rowstat must be a contiguous f32 ({m}, {k // 64}, 2) slab, got "
                                 f"{rowstat.dtype} {tuple(rowstat.shape)}")
        _check(lib().tramba_linear_ln_rowstat_cl(_ptr(x), _ptr(w_folded), _ptr(colsum), _ptr(bias), _ptr(residual), _ptr(y),
                                                 m, n, k, float(eps), act, dt(x), dt(y), _ptr(rowstat), k // 64, _stream()),
               "linear_ln_cl")
        return y
    _check(lib().tramba_linear_ln_cl(_ptr(x), _ptr(w_folded), _ptr(colsum), _ptr(bias), _ptr(residual), _ptr(y), m, n, k,
                                     float(eps), act, dt(x), dt(y), _stream()), "linear_ln_cl")
    return y


def linear2_cl(x1, x2, w, bias=None, residual=None, act=ACT_NONE, out_dtype=None, rowstat=False):
    """Linear2d on torch.cat((x1, x2), dim=-1) without the concatenation: x1 (..., K1), x2 (..., K2), w (N, K1+K2).
    rowstat: as in linear_cl."""
    _dev(x1, x2, w, bias, residual)
    k1, k2 = x1.shape[-1], x2.shape[-1]
    n = w.shape[0]
    m = x1.numel() // k1
    if x2.shape[:-1] != x1.shape[:-1] or w.shape[1] != k1 + k2 or w.dtype != x1.dtype or x2.dtype != x1.dtype:
        raise TrambaHipError("linear2_cl: operand shapes / dtypes do not match")
    _check_epilogue("linear2_cl", bias, residual, x1.dtype, m, n)
    out_dtype = x1.dtype if out_dtype is None else out_dtype
    extra = _rowstat_extra(rowstat, x1.dtype, out_dtype, m, n)
    y = torch.empty((m * n + extra,) if extra else x1.shape[:-1] + (n,), dtype=out_dtype, device=x1.device)
    if extra:
        (y, slab), emitted = _rowstat_split(y, x1.shape[:-1] + (n,), m, n), c_int(0)
        _check(lib().tramba_linear2_rowstat_cl(_ptr(x1), _ptr(x2), k1, _ptr(w), _ptr(bias), _ptr(residual), _ptr(y), m, n,
                                               k1 + k2, act, dt(x1), dt(y), _ptr(slab), ctypes.byref(emitted), _stream()),
               "linear2_cl")
        if emitted.value:
            y._tramba_rowstat = (slab, y._version)
        return y
    _check(lib().tramba_linear2_cl(_ptr(x1), _ptr(x2), k1, _ptr(w), _ptr(bias), _ptr(residual), _ptr(y), m, n, k1 + k2,
                                   act, dt(x1), dt(y), _stream()), "linear2_cl")
    return y


def wgrad_cl(gy, x, want_bias=False, defer=False):
    """Weight gradient of y = x @ W^T: gy (..., N), x (..., K) 16-bit, same leading shape -> (gw (N, K) f32, gb (N) f32 or
    None).  Rows may be strided (a column slice of a wider tensor) as long as the last dim is contiguous.  defer: inside
    `deferred_sums()` the slab sum of the launch is recorded for `flush_sums()` (see _SumQueue)."""
    n, k = gy.shape[-1], x.shape[-1]
    gy2, x2 = gy.reshape(-1, n), x.reshape(-1, k)
    if gy2.stride(-1) != 1 or x2.stride(-1) != 1:
        gy2, x2 = gy2.contiguous(), x2.contiguous()
    m = gy2.shape[0]
    if x2.shape[0] != m or gy2.dtype != x2.dtype:
        raise TrambaHipError("wgrad_cl: gy / x mismatch")
    return _wgrad(gy2, x2, m, n, k, 1, 1, 0, 0, gy2.stride(0), 0, 0, x2.stride(0), want_bias, defer)


def wgrad_rows_cl(gy, x, segments, defer=False):
    """Rows of the weight gradient gy^T x (gy (M, N), x (M, K) 16-bit) in another row order: segments = [(first row, rows)],
    the result holds those row ranges one after the other ((sum of rows, K) f32).  Inside `deferred_sums()` (defer=True) every
    range is summed from the GEMM's partial slabs straight into its place at `flush_sums()` -- no full-size sum, no
    concatenation; otherwise the ranges are cut out of the finished gradient."""
    _dev(gy, x)
    m, n = gy.shape
    k = x.shape[-1]
    if x.shape[0] != m or gy.dtype != x.dtype:
        raise TrambaHipError("wgrad_rows_cl: gy / x mismatch")
    if any(a < 0 or c <= 0 or a + c > n for a, c in segments):
        raise TrambaHipError("wgrad_rows_cl: a row range outside the gradient")
    total = sum(c for _, c in segments)
    if defer and _sumq.enabled:
        ws_bytes = lib().tramba_wgrad_workspace(m, n, k, 1, 1)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=gy.device)
        full = torch.empty((1, n * k + n), dtype=torch.float32, device=gy.device)
        nslab = ctypes.c_int(0)
        _check(lib().tramba_wgrad_parts_cl(_ptr(gy), _ptr(x), _ptr(full), _ptr(ws), ws_bytes, m, n, k, 1, 1, 0, 0, n, 0, 0, k, 0,
                                           dt(gy), _stream(), ctypes.byref(nslab)), "wgrad_parts_cl")
        if nslab.value > 0:
            out = torch.empty((total, k), dtype=torch.float32, device=gy.device)
            if _sumq.poison:
                out.fill_(float("nan"))
            row = 0
            for a, c in segments:
                _enqueue_sum(_ptr(ws) + a * k * 4, _ptr(out) + row * k * 4, c * k, nslab.value, (ws, out), stride=n * k + n)
                row += c
            return out.view(total, k)       # (a view goes out, the queue keeps the base: see dw_unpack_grad)
        gw = full[0, :n * k].view(n, k)     # a single slab: the gradient is already there
    else:
        gw = wgrad_cl(gy, x)[0]
    return torch.cat([gw[a:a + c] for a, c in segments], dim=0)


def wgrad_grouped_cl(gy, x, defer=False):
    """gy (B, G, L, N), x (B, G, L, K) 16-bit contiguous -> (G, N, K) f32: per group g, sum over b and l of gy^T x.
    defer: see wgrad_cl (inside `deferred_sums()` the slab sums are recorded; for results handed to autograd as they are)."""
    _dev(gy, x)
    b, g, l, n = gy.shape
    k = x.shape[-1]
    if x.shape[:3] != gy.shape[:3] or gy.dtype != x.dtype:
        raise TrambaHipError("wgrad_grouped_cl: gy / x mismatch")
    out, _ = _wgrad(gy, x, l, n, k, g, b, g * l * n, l * n, n, g * l * k, l * k, k, False, defer)
    return out


def tn_shared_cl(a, x):
    """out[g] = a^T @ x[g]: a (T, N) 16-bit shared by every group, x (G, T, K) same dtype -> (G, N, K) f32 -- a separable
    transform along a leading axis of a channels-last tensor (the DCT backward: T = coefficients, N = pixels)."""
    _dev(a, x)
    nb = a.shape[0] if a.dim() == 3 else 1        # a (P, T, N): out[g] = sum over p of a[p]^T @ x[g] (a table kept in pieces)
    t, n = a.shape[-2:]
    g, t2, k = x.shape
    if t2 != t or a.dtype != x.dtype:
        raise TrambaHipError("tn_shared_cl: operand shapes / dtypes do not match")
    out, _ = _wgrad(a, x, t, n, k, g, nb, t * n, 0, n, 0, t * k, k, False)
    return out if g > 1 else out.view(1, n, k)


def _wgrad(gy, x, m, n, k, groups, nbatch, gy_bs, gy_gs, gy_ld, x_bs, x_gs, x_ld, want_bias, defer=False):
    for t in (gy, x):
        if not t.is_cuda:
            raise TrambaHipError("tramba_amd kernels need tensors on a HIP device (no CPU fallback)")
    ws_bytes = lib().tramba_wgrad_workspace(m, n, k, groups, nbatch)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=gy.device)
    out = torch.empty((groups, n * k + n), dtype=torch.float32, device=gy.device)
    if defer and _sumq.enabled:
        nslab = ctypes.c_int(0)
        _check(lib().tramba_wgrad_parts_cl(_ptr(gy), _ptr(x), _ptr(out), _ptr(ws), ws_bytes, m, n, k, groups, nbatch, gy_bs,
                                           gy_gs, gy_ld, x_bs, x_gs, x_ld, int(want_bias), dt(gy), _stream(),
                                           ctypes.byref(nslab)), "wgrad_parts_cl")
        if nslab.value > 0:          # (0: a single slab, already in `out`)
            slab = n * k + n
            if groups > 1 and not want_bias:
                # per-group gradients without the bias slot between them: summed into a DENSE (groups, N, K) tensor -- a leaf
                # takes an incoming gradient as it is only when its strides are the parameter's own (a copy would read the
                # buffer before the flush has filled it)
                dense = torch.empty((groups, n, k), dtype=torch.float32, device=gy.device)
                if _sumq.poison:
                    dense.fill_(float("nan"))
                for g in range(groups):
                    _enqueue_sum(_ptr(ws) + g * nslab.value * slab * 4, _ptr(dense) + g * n * k * 4, n * k, nslab.value,
                                 (ws, dense), stride=slab)
                return dense.view(groups, n, k), None
            if _sumq.poison:
                out.fill_(float("nan"))
            for g in range(groups):
                _enqueue_sum(_ptr(ws) + g * nslab.value * slab * 4, _ptr(out) + g * slab * 4, slab, nslab.value, (ws, out))
    else:
        _check(lib().tramba_wgrad_cl(_ptr(gy), _ptr(x), _ptr(out), _ptr(ws), ws_bytes, m, n, k, groups, nbatch, gy_bs, gy_gs,
                                     gy_ld, x_bs, x_gs, x_ld, int(want_bias), dt(gy), _stream()), "wgrad_cl")
    gw = out[:, :n * k].view(groups, n, k)
    if groups == 1:
        return gw[0], (out[0, n * k:] if want_bias else None)
    return gw, None


def rows_gemm_cl(x, w, y, n):
    """y[z, t, :n] = x[z, t, :] @ w[z % G]^T: x (Z, M, K) 16-bit, w (G, n, K) same dtype, y (Z, M, ldy) f32 (in place)."""
    _dev(x, w, y)
    z, m, k = x.shape
    if w.shape[1:] != (n, k) or w.dtype != x.dtype or y.dtype != torch.float32 or y.shape[:2] != (z, m):
        raise TrambaHipError("rows_gemm_cl: operand shapes / dtypes do not match")
    _check(lib().tramba_rows_gemm_cl(_ptr(x), _ptr(w), _ptr(y), z, m, n, k, w.shape[0], y.shape[-1], dt(x), _stream()),
           "rows_gemm_cl")
    return y


class _SumQueue:
    """Pending partial-sum reductions of a training step (tramba_multi_sum).  The parameter gradients of LayerNorm and of
    every Linear2d leave their kernels as partial tables (one row per workgroup / token split) that a small kernel adds up in
    a fixed order.  Nothing reads those gradients before the optimizer (reference train.py:86-89), so inside
    `deferred_sums()` a reduction is only RECORDED -- the caller gets the output tensor, to be filled later -- and all of them
    run as a handful of launches at `flush_sums()`: ~300 launches of 4-7 us per step, each on its launch floor, become ~10.
    Off by default: outside the context every sum runs where it is issued.  Only call sites whose result goes straight to
    autograd as a leaf's gradient pass defer=True (anything that READS the sum must not)."""

    def __init__(self):
        self.enabled = False
        self.poison = False         # tests: NaN-fill a deferred output, so that a premature reader cannot go unnoticed
        self.items = []
        self.unpacks = []           # depth-wise gradient unpacks (tramba_dw_unpack_grad_multi), run after the sums
        self.lock = threading.Lock()


_sumq = _SumQueue()


class deferred_sums:
    """with hip.deferred_sums(): loss.backward()   -- record the deferrable partial-sum reductions, run them at the exit"""

    def __enter__(self):
        self._was = _sumq.enabled
        _sumq.enabled = True
        return self

    def __exit__(self, *exc):
        _sumq.enabled = self._was
        if not self._was:
            flush_sums()
        return False


def _enqueue_sum(part_ptr, out_ptr, n, nslab, keep, stride=None):
    with _sumq.lock:
        _sumq.items.append((part_ptr, out_ptr, int(n), int(nslab), _stream(), keep, int(n if stride is None else stride)))


def flush_sums():
    """Run every recorded reduction (one tramba_multi_sum call per stream they were recorded on)."""
    with _sumq.lock:
        items, _sumq.items = _sumq.items, []
        unpacks, _sumq.unpacks = _sumq.unpacks, []
    by_stream = {}
    for it in items:
        by_stream.setdefault(it[4], []).append(it)
    for stream, its in by_stream.items():
        cnt = len(its)
        parts = (ctypes.c_void_p * cnt)(*[it[0] for it in its])
        outs = (ctypes.c_void_p * cnt)(*[it[1] for it in its])
        ns = (ctypes.c_int64 * cnt)(*[it[2] for it in its])
        nsl = (ctypes.c_int * cnt)(*[it[3] for it in its])
        strides = (ctypes.c_int64 * cnt)(*[it[6] for it in its])
        _check(lib().tramba_multi_sum_strided(parts, outs, ns, strides, nsl, cnt, stream), "multi_sum")
    streams = set(by_stream)
    by_stream = {}
    for it in unpacks:          # (a table and its unpack are recorded on the same stream: the sums above come first)
        by_stream.setdefault(it[8], []).append(it)
    for stream, its in by_stream.items():
        cnt = len(its)
        cols = [(ctypes.c_void_p * cnt)(*[it[k] for it in its]) for k in range(5)]
        ints = [(ctypes.c_int * cnt)(*[it[k] for it in its]) for k in (5, 6, 7)]
        _check(lib().tramba_dw_unpack_grad_multi(*cols, *ints, cnt, stream), "dw_unpack_grad_multi")
    streams |= set(by_stream)
    # sums recorded on ANOTHER stream (the guide branches' backward runs on the side stream of models._forward_overlapped) were
    # launched there: whatever the caller's stream does next -- the optimizer reads these gradients -- must come after them
    if not streams:     # (nothing was recorded: e.g. a host-tensor model, which has no stream to ask about)
        return
    cur = _stream()
    others = [st for st in streams if st != cur]
    if others:
        here = torch.cuda.current_stream()
        for st in others:
            ext = torch.cuda.ExternalStream(st)
            ev = torch.cuda.Event()
            ev.record(ext)
            here.wait_event(ev)


def pending_sums():
    return len(_sumq.items) + len(_sumq.unpacks)


def slab_sum(part, defer=False):
    """part (S, ...) f32 -> sum over the first axis, slabs added in a fixed order (tramba_slab_sum); the small partial-sum
    tables of the backward kernels.  defer: inside `deferred_sums()` the sum is recorded and runs at `flush_sums()` (the
    returned tensor is filled then) -- for results that go straight to autograd as a parameter's gradient."""
    _dev(part)
    nslab = part.shape[0]
    n = part.numel() // max(nslab, 1)
    if part.dtype != torch.float32 or not part.is_contiguous() or n % 4 or nslab == 0:
        return part.sum(dim=0)
    out = torch.empty(part.shape[1:], dtype=torch.float32, device=part.device)
    if defer and _sumq.enabled:
        if _sumq.poison:
            out.fill_(float("nan"))
        _enqueue_sum(_ptr(part), _ptr(out), n, nslab, (part, out))   # (both stay allocated until the sum has run)
        return out
    _check(lib().tramba_slab_sum(_ptr(part), _ptr(out), n, nslab, _stream()), "slab_sum")
    return out


def shadow_cast_multi(table, ntensors, total_tiles, dtype):
    """One launch over a device-resident table (ntensors, 8) int64 {src f32, dst, dst_t, rows, cols, first_tile, dst_ld,
    dst_t_ld}: every dst = src cast to `dtype`, every dst_t = its transpose, with leading dimensions (blocks of padded
    layouts); tramba_amd.modules.refresh_lowp_shadows builds the table."""
    _dev(table)
    if table.dtype != torch.int64 or table.shape != (ntensors, 8) or not table.is_contiguous():
        raise TrambaHipError("shadow_cast_multi: table must be a contiguous (ntensors, 8) int64 tensor")
    _check(lib().tramba_shadow_cast_multi(_ptr(table), ntensors, total_tiles, _DT[dtype], _stream()), "shadow_cast_multi")


def conv3x3s2_cl(x, w_kmajor, bias):
    """x: (B, H, W, Cin) bf16/f16; w_kmajor: (Cout, 9*Cin) = weight.permute(0,2,3,1), same dtype."""
    _dev(x, w_kmajor, bias)
    bb, h, wd, cin = x.shape
    cout = w_kmajor.shape[0]
    if w_kmajor.dtype != x.dtype or w_kmajor.shape[1] != 9 * cin:
        raise TrambaHipError("conv3x3s2_cl: weight dtype/shape mismatch")
    y = torch.empty((bb, (h + 1) // 2, (wd + 1) // 2, cout), dtype=x.dtype, device=x.device)
    _check(lib().tramba_conv3x3s2_cl(_ptr(x), _ptr(w_kmajor), _ptr(bias), _ptr(y), bb, h, wd, cin, cout, dt(x),
                                     _stream()), "conv3x3s2_cl")
    return y


def stem_conv_ln_gelu(img, w, bias, ln_w, ln_b, eps, out_dtype):
    """img: (B, 3, H, W) NCHW f32 or out_dtype -> (B, H/2, W/2, 64) out_dtype."""
    _dev(img, w, bias, ln_w, ln_b)
    bb, c3, h, wd = img.shape
    if c3 != 3 or tuple(w.shape) != (64, 3, 3, 3):
        raise TrambaHipError("stem_conv_ln_gelu: expects a 3 -> 64 channel 3x3 stem")
    y = torch.empty((bb, (h + 1) // 2, (wd + 1) // 2, 64), dtype=out_dtype, device=img.device)
    _check(lib().tramba_stem_conv_ln_gelu(_ptr(img), _ptr(w), _ptr(bias), _ptr(ln_w), _ptr(ln_b), _ptr(y), bb, h, wd,
                                          eps, _DT[img.dtype], _DT[out_dtype], _stream()), "stem_conv_ln_gelu")
    return y


_PATCH_EMBED_FORMS = ((7, 4, 3, 64), (4, 4, 0, 128))        # PVT patch_embed1, Swin patch_embed


def patch_conv_supported(dtype, cin, cout, r):
    """the argument checks of tramba_patch_conv_cl that depend on the layer, without the library"""
    return dtype in _ATTN_DTYPES and 2 <= r <= 8 and cin > 0 and cin % 64 == 0 and cout > 0 and cout % 8 == 0


def patch_conv_cl(x, w_kmajor, bias):
    """x: (B, H, W, Cin) bf16/f16; w_kmajor: (Cout, r, r, Cin) = weight.permute(0,2,3,1), same dtype; bias (Cout) f32 or None
    -> (B, H // r, W // r, Cout): the kernel = stride = r convolution.  Trailing rows / columns beyond r * (H // r) are not
    read."""
    _dev(x, w_kmajor, bias)
    if x.dim() != 4 or w_kmajor.dim() != 4 or w_kmajor.dtype != x.dtype or w_kmajor.shape[1] != w_kmajor.shape[2] \
            or w_kmajor.shape[3] != x.shape[3]:
        raise TrambaHipError(f"patch_conv_cl: need x (B, H, W, Cin) and w (Cout, r, r, Cin) of one dtype, got {tuple(x.shape)} "
                             f"{x.dtype} {tuple(w_kmajor.shape)} {w_kmajor.dtype}")
    bb, h, wd, cin = x.shape
    cout, r = w_kmajor.shape[0], w_kmajor.shape[1]
    if bias is not None and (bias.dtype != torch.float32 or tuple(bias.shape) != (cout,)):
        raise TrambaHipError(f"patch_conv_cl: bias must be float32 ({cout},)")
    if (bb * h * wd * cin * 2) >= 2 ** 31:
        raise TrambaHipError("patch_conv_cl: input map beyond 32-bit byte offsets")
    y = torch.empty((bb, h // max(r, 1), wd // max(r, 1), cout), dtype=x.dtype, device=x.device)
    _check(lib().tramba_patch_conv_cl(_ptr(x), _ptr(w_kmajor), _ptr(bias), _ptr(y), bb, h, wd, cin, cout, r, dt(x), _stream()),
           "patch_conv_cl")
    return y


def patch_conv_train_supported(dtype, cin, cout, r):
    """can patch_conv_dgrad_cl / patch_conv_wgrad_cl take this layer?  The forward's domain, with an f32 weight gradient
    below 2^31 bytes.  A per-layer predicate: the entries also refuse a map or gy of 2^31 bytes and more, and more than
    65535 x 16 output tokens, which depend on the batch and the map, not on the layer."""
    return patch_conv_supported(dtype, cin, cout, r) and cout * r * r * cin * 4 < 2 ** 31


def _patch_conv_geom(name, gy, x_shape, x_dtype):
    if gy.dim() != 4 or len(x_shape) != 4 or gy.dtype != x_dtype:
        raise TrambaHipError(f"{name}: need gy (B, Ho, Wo, Cout) and x (B, H, W, Cin) of one dtype, got {tuple(gy.shape)} "
                             f"{gy.dtype} {tuple(x_shape)} {x_dtype}")
    bb, h, wd, cin = x_shape
    return bb, h, wd, cin, gy.shape[3]


def patch_conv_dgrad_cl(gy, w_kmajor, x_shape):
    """Input gradient of patch_conv_cl: gy (B, H // r, W // r, Cout), w_kmajor (Cout, r, r, Cin) (the forward's copy), x_shape
    (B, H, W, Cin) -> gx of that shape in gy's dtype, every element written (zeros where no patch reaches)."""
    _dev(gy, w_kmajor)
    bb, h, wd, cin, cout = _patch_conv_geom("patch_conv_dgrad_cl", gy, tuple(x_shape), w_kmajor.dtype)
    r = w_kmajor.shape[1] if w_kmajor.dim() == 4 else 0
    if w_kmajor.dim() != 4 or tuple(w_kmajor.shape) != (cout, r, r, cin) or r < 1 \
            or tuple(gy.shape[:3]) != (bb, h // r, wd // r):
        raise TrambaHipError(f"patch_conv_dgrad_cl: gy {tuple(gy.shape)} and w {tuple(w_kmajor.shape)} do not belong to x "
                             f"{tuple(x_shape)}")
    gx = torch.empty((bb, h, wd, cin), dtype=gy.dtype, device=gy.device)
    _check(lib().tramba_patch_conv_dgrad_cl(_ptr(gy), _ptr(w_kmajor), _ptr(gx), bb, h, wd, cin, cout, r, dt(gy), _stream()),
           "patch_conv_dgrad_cl")
    return gx


def patch_conv_wgrad_cl(gy, x, r, want_bias=False, defer=False):
    """Weight gradient of patch_conv_cl: gy (B, H // r, W // r, Cout), x (B, H, W, Cin) -> (gw (Cout, r, r, Cin) f32 K-major,
    gb (Cout) f32 or None).  The kernel leaves one f32 slab per token run; they are added in index order by slab_sum.
    defer: inside `deferred_sums()` that sum is recorded for `flush_sums()` (see _SumQueue)."""
    _dev(gy, x)
    bb, h, wd, cin, cout = _patch_conv_geom("patch_conv_wgrad_cl", gy, tuple(x.shape), x.dtype)
    if r < 1 or tuple(gy.shape[:3]) != (bb, h // r, wd // r):
        raise TrambaHipError(f"patch_conv_wgrad_cl: gy {tuple(gy.shape)} does not belong to x {tuple(x.shape)} with r = {r}")
    nsplit = lib().tramba_patch_conv_wgrad_split(bb, h, wd, cin, cout, r)
    nbytes = lib().tramba_patch_conv_wgrad_work(bb, h, wd, cin, cout, r)
    slab = cout * r * r * cin + cout
    work = torch.empty((nsplit, slab), dtype=torch.float32, device=gy.device)      # (no slab for a shape the entry refuses)
    _check(lib().tramba_patch_conv_wgrad_cl(_ptr(gy), _ptr(x), _ptr(work), nbytes, bb, h, wd, cin, cout, r, int(want_bias),
                                            dt(gy), _stream()), "patch_conv_wgrad_cl")
    out = slab_sum(work, defer) if nsplit > 1 else work[0]
    gw = out[:slab - cout].view(cout, r, r, cin)
    return gw, (out[slab - cout:] if want_bias else None)


def patch_embed_ln_supported(out_dtype, k, stride, pad, cout):
    """the argument checks of tramba_patch_embed_ln that depend on the layer, without the library"""
    return out_dtype in _ATTN_DTYPES and (k, stride, pad, cout) in _PATCH_EMBED_FORMS


def patch_embed_ln(img, w, bias, ln_w, ln_b, eps, stride, pad, out_dtype):
    """img: (B, 3, H, W) NCHW f32 or out_dtype; w: (Cout, 3, k, k) f32; bias, ln_w, ln_b: (Cout) f32 -> LayerNorm(conv(img) +
    bias) as (B, Ho, Wo, Cout) out_dtype, Ho = (H + 2 pad - k) // stride + 1.  PVT's (k 7, stride 4, pad 3, Cout 64) and Swin's
    (4, 4, 0, 128) forms only."""
    _dev(img, w, bias, ln_w, ln_b)
    if img.dim() != 4 or img.shape[1] != 3 or w.dim() != 4 or w.shape[1] != 3 or w.shape[2] != w.shape[3]:
        raise TrambaHipError(f"patch_embed_ln: need img (B, 3, H, W) and w (Cout, 3, k, k), got {tuple(img.shape)} {tuple(w.shape)}")
    bb, _, h, wd = img.shape
    cout, k = w.shape[0], w.shape[2]
    for name, t in (("w", w), ("bias", bias), ("ln_w", ln_w), ("ln_b", ln_b)):
        if t.dtype != torch.float32 or (name != "w" and tuple(t.shape) != (cout,)):
            raise TrambaHipError(f"patch_embed_ln: {name} must be float32" + ("" if name == "w" else f" ({cout},)"))
    if out_dtype not in _DT or img.dtype not in _DT:
        raise TrambaHipError(f"patch_embed_ln: unsupported dtype {img.dtype} -> {out_dtype}")
    ho, wo = (h + 2 * pad - k) // stride + 1, (wd + 2 * pad - k) // stride + 1
    y = torch.empty((bb, max(ho, 0), max(wo, 0), cout), dtype=out_dtype, device=img.device)
    _check(lib().tramba_patch_embed_ln(_ptr(img), _ptr(w), _ptr(bias), _ptr(ln_w), _ptr(ln_b), _ptr(y), bb, h, wd, k, stride, pad,
                                       cout, eps, _DT[img.dtype], _DT[out_dtype], _stream()), "patch_embed_ln")
    return y


# ----------------------------------------------------------------------------- ResNet-50 encoder convolutions
def conv_out_size(n, ksize, stride):
    """output extent of a convolution with pad = ksize // 2 along an axis of n pixels"""
    return (n + 2 * (ksize // 2) - ksize) // stride + 1


def stem7_pool_out_size(n):
    """output extent of conv(7, stride 2, pad 3) followed by max_pool(3, stride 2, pad 1) along an axis of n pixels"""
    return (conv_out_size(n, 7, 2) - 1) // 2 + 1


def conv_affine_supported(dtype, h, w, cin, cout, ksize, stride):
    """the argument checks of tramba_conv_affine_cl that depend on the layer and its map (batch 1), without the library"""
    return (dtype in _ATTN_DTYPES and ksize in (1, 3) and stride in (1, 2) and h > 0 and w > 0 and cin > 0 and cin % 64 == 0
            and cout > 0 and cout % 8 == 0 and h * w * cin * 2 < 2 ** 31 and cout * ksize * ksize * cin * 2 < 2 ** 31
            and (cout + 63) // 64 <= 65535)


def conv_affine_cl(x, w_kmajor, scale, shift, residual=None, relu=True, ksize=None, stride=1):
    """x: (B, H, W, Cin) bf16/f16; w_kmajor: (Cout, k, k, Cin) = weight.permute(0,2,3,1), same dtype, not rescaled; scale, shift:
    (Cout) f32 or None (1 / 0); residual: (B, Ho, Wo, Cout) in x's dtype or None -> act(scale * conv(x) + shift + residual) as
    (B, Ho, Wo, Cout), pad = k // 2, Ho = (H + 2 pad - k) // stride + 1; f32 throughout, one rounding."""
    _dev(x, w_kmajor, scale, shift, residual)
    if x.dim() != 4 or w_kmajor.dim() != 4 or w_kmajor.dtype != x.dtype or w_kmajor.shape[1] != w_kmajor.shape[2] \
            or w_kmajor.shape[3] != x.shape[3] or (ksize is not None and ksize != w_kmajor.shape[1]):
        raise TrambaHipError(f"conv_affine_cl: need x (B, H, W, Cin) and w (Cout, k, k, Cin) of one dtype"
                             f"{'' if ksize is None else f' with k = {ksize}'}, got {tuple(x.shape)} {x.dtype} "
                             f"{tuple(w_kmajor.shape)} {w_kmajor.dtype}")
    bb, h, wd, cin = x.shape
    cout, k = w_kmajor.shape[0], w_kmajor.shape[1]
    for name, t in (("scale", scale), ("shift", shift)):
        if t is not None and (t.dtype != torch.float32 or tuple(t.shape) != (cout,)):
            raise TrambaHipError(f"conv_affine_cl: {name} must be float32 ({cout},)")
    if k not in (1, 3) or stride not in (1, 2):
        raise TrambaHipError(f"conv_affine_cl: ksize = {k} must be 1 or 3 and stride = {stride} 1 or 2")
    ho, wo = conv_out_size(h, k, stride), conv_out_size(wd, k, stride)
    if residual is not None and (residual.dtype != x.dtype or tuple(residual.shape) != (bb, ho, wo, cout)):
        raise TrambaHipError(f"conv_affine_cl: residual must be {x.dtype} {(bb, ho, wo, cout)}, got {residual.dtype} "
                             f"{tuple(residual.shape)}")
    if (bb * h * wd * cin * 2) >= 2 ** 31:
        raise TrambaHipError("conv_affine_cl: input map beyond 32-bit byte offsets")
    y = torch.empty((bb, ho, wo, cout), dtype=x.dtype, device=x.device)
    _check(lib().tramba_conv_affine_cl(_ptr(x), _ptr(w_kmajor), _ptr(scale), _ptr(shift), _ptr(residual), _ptr(y), bb, h, wd,
                                       cin, cout, k, stride, int(bool(relu)), dt(x), _stream()), "conv_affine_cl")
    return y


def stem7_pool_supported(out_dtype, h, w):
    """the argument checks of tramba_stem7_affine_relu_pool that depend on the image size, without the library"""
    return out_dtype in _ATTN_DTYPES and h > 0 and w > 0 and (stem7_pool_out_size(h) + 3) // 4 <= 65535 and 3 * h * w < 9e18


def stem7_affine_relu_pool(img, w, scale, shift, out_dtype):
    """img: (B, 3, H, W) NCHW f32 or out_dtype; w: (64, 3, 7, 7) f32; scale, shift: (64) f32 -> max_pool(relu(scale * conv(img)
    + shift), 3, 2, 1) as (B, Hp, Wp, 64) out_dtype, the 7x7 / stride 2 / pad 3 convolution; f32 throughout, one rounding."""
    _dev(img, w, scale, shift)
    if img.dim() != 4 or img.shape[1] != 3 or tuple(w.shape) != (64, 3, 7, 7):
        raise TrambaHipError(f"stem7_affine_relu_pool: need img (B, 3, H, W) and w (64, 3, 7, 7), got {tuple(img.shape)} "
                             f"{tuple(w.shape)}")
    for name, t in (("w", w), ("scale", scale), ("shift", shift)):
        if t.dtype != torch.float32 or (name != "w" and tuple(t.shape) != (64,)):
            raise TrambaHipError(f"stem7_affine_relu_pool: {name} must be float32" + ("" if name == "w" else " (64,)"))
    if out_dtype not in _DT or img.dtype not in _DT:
        raise TrambaHipError(f"stem7_affine_relu_pool: unsupported dtype {img.dtype} -> {out_dtype}")
    bb, _, h, wd = img.shape
    y = torch.empty((bb, max(stem7_pool_out_size(h), 0), max(stem7_pool_out_size(wd), 0), 64), dtype=out_dtype,
                    device=img.device)
    _check(lib().tramba_stem7_affine_relu_pool(_ptr(img), _ptr(w), _ptr(scale), _ptr(shift), _ptr(y), bb, h, wd,
                                               _DT[img.dtype], _DT[out_dtype], _stream()), "stem7_affine_relu_pool")
    return y


# ----------------------------------------------------------------------------- ResNet-50 encoder: batch norm and max pool (training)
def bn_parts(m, c):
    """the row runs a (m, c) channels-last map is dealt in (the rule of csrc/batchnorm.hip, bn_split), without the library"""
    return min(max(m // 128, 1), 64) if m > 0 and c > 0 else 0


def bn_work_floats(m, c):
    """f32 elements of the workspace of bn_stats_cl / bn_act_bwd_cl: 2 partial tables of bn_parts rows and 2 rows of sums, a
    row being c rounded up to 64"""
    return (2 * bn_parts(m, c) + 2) * ((c + 63) // 64 * 64) if m > 0 and c > 0 else 0


def bn_supported(dtype, m, c):
    """the argument checks of tramba_bn_stats_cl / _act_cl / _act_bwd_cl that depend on the map, without the library"""
    return dtype in _ATTN_DTYPES and c > 0 and c % 8 == 0 and 2 <= m < 2 ** 31 - 1 and (c + 63) // 64 <= 65535


def _bn_map(name, x, **same):
    if x.dim() < 2 or x.dtype not in _ATTN_DTYPES:
        raise TrambaHipError(f"{name}: need a channels-last (..., C) bf16 / fp16 map, got {tuple(x.shape)} {x.dtype}")
    c = x.shape[-1]
    for key, t in same.items():
        if t is not None and (t.dtype != x.dtype or t.shape != x.shape):
            raise TrambaHipError(f"{name}: {key} must be {x.dtype} {tuple(x.shape)}, got {t.dtype} {tuple(t.shape)}")
    return x.numel() // max(c, 1), c


def _bn_vec(name, c, **vecs):
    for key, t in vecs.items():
        if t is not None and (t.dtype != torch.float32 or tuple(t.shape) != (c,)):
            raise TrambaHipError(f"{name}: {key} must be float32 ({c},)")


def _bn_workspace(m, c, device):
    nbytes = lib().tramba_bn_work(m, c)
    return torch.empty(nbytes // 4, dtype=torch.float32, device=device), nbytes


def bn_stats_cl(x, eps, running_mean=None, running_var=None, momentum=0.1):
    """x: (..., C) bf16/f16 channels-last -> (mean, rstd) f32 (C) over all leading axes: the batch mean and
    1 / sqrt(biased variance + eps), two passes.  running_mean / running_var (C) f32 are updated IN PLACE on the device
    (running = (1 - momentum) running + momentum new, the variance unbiased), so a captured graph updates them per replay."""
    _dev(x, running_mean, running_var)
    m, c = _bn_map("bn_stats_cl", x)
    _bn_vec("bn_stats_cl", c, running_mean=running_mean, running_var=running_var)
    if m == 1:
        raise TrambaHipError("bn_stats_cl: expected more than 1 value per channel when training")
    mean = torch.empty(c, dtype=torch.float32, device=x.device)
    rstd = torch.empty(c, dtype=torch.float32, device=x.device)
    work, nbytes = _bn_workspace(m, c, x.device)
    _check(lib().tramba_bn_stats_cl(_ptr(x), _ptr(mean), _ptr(rstd), _ptr(running_mean), _ptr(running_var), _ptr(work), nbytes,
                                    m, c, float(eps), float(momentum), dt(x), _stream()), "bn_stats_cl")
    return mean, rstd


def bn_act_cl(x, mean, rstd, gamma=None, beta=None, residual=None, relu=False):
    """y = act(gamma (x - mean) rstd + beta + residual) on a channels-last map; mean, rstd, gamma, beta (C) f32 (gamma / beta
    may be None: 1 / 0), residual in x's shape and dtype or None; f32 throughout, one rounding."""
    _dev(x, mean, rstd, gamma, beta, residual)
    m, c = _bn_map("bn_act_cl", x, residual=residual)
    _bn_vec("bn_act_cl", c, mean=mean, rstd=rstd, gamma=gamma, beta=beta)
    if mean is None or rstd is None:
        raise TrambaHipError("bn_act_cl: mean and rstd are required")
    y = torch.empty_like(x)
    _check(lib().tramba_bn_act_cl(_ptr(x), _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(beta), _ptr(residual), _ptr(y), m, c,
                                  int(bool(relu)), dt(x), _stream()), "bn_act_cl")
    return y


def bn_act_bwd_cl(dy, x, y, mean, rstd, gamma=None, relu=False, want_dres=False, want_affine=True):
    """Backward of bn_act_cl through the batch statistics -> (dx, dres or None, dgamma or None, dbeta or None).  y is read
    for the ReLU mask y > 0 alone (None without relu); dres is the masked dy, the shortcut's gradient; dgamma / dbeta f32.
    dx does not depend on want_affine."""
    _dev(dy, x, y, mean, rstd, gamma)
    m, c = _bn_map("bn_act_bwd_cl", x, dy=dy, y=y)
    _bn_vec("bn_act_bwd_cl", c, mean=mean, rstd=rstd, gamma=gamma)
    if mean is None or rstd is None or dy is None or (relu and y is None):
        raise TrambaHipError("bn_act_bwd_cl: dy, mean, rstd and (with relu) y are required")
    dx = torch.empty_like(x)
    dres = torch.empty_like(x) if want_dres else None
    dgamma = torch.empty(c, dtype=torch.float32, device=x.device) if want_affine else None
    dbeta = torch.empty(c, dtype=torch.float32, device=x.device) if want_affine else None
    work, nbytes = _bn_workspace(m, c, x.device)
    _check(lib().tramba_bn_act_bwd_cl(_ptr(dy), _ptr(x), _ptr(y), _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(dx), _ptr(dres),
                                      _ptr(dgamma), _ptr(dbeta), _ptr(work), nbytes, m, c, int(bool(relu)), dt(x), _stream()),
           "bn_act_bwd_cl")
    return dx, dres, dgamma, dbeta


def maxpool3s2_supported(dtype, h, w, c):
    """the argument checks of tramba_maxpool3s2_cl / _bwd_cl that depend on the map (batch 1), without the library"""
    return dtype in _ATTN_DTYPES and h > 0 and w > 0 and c > 0 and c % 8 == 0 and h * w * (c // 8) < (2 ** 31 - 1) * 256


def _pool_map(name, x):
    if x.dim() != 4 or x.dtype not in _ATTN_DTYPES:
        raise TrambaHipError(f"{name}: need a channels-last (B, H, W, C) bf16 / fp16 map, got {tuple(x.shape)} {x.dtype}")
    return x.shape


def maxpool3s2_cl(x):
    """max_pool2d(3, 2, 1) on x (B, H, W, C) bf16/f16 -> (B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C); ties go to the first maximum
    of a window in row-major order, padding never wins"""
    _dev(x)
    bb, h, w, c = _pool_map("maxpool3s2_cl", x)
    y = torch.empty((bb, max((h - 1) // 2 + 1, 0), max((w - 1) // 2 + 1, 0), c), dtype=x.dtype, device=x.device)
    _check(lib().tramba_maxpool3s2_cl(_ptr(x), _ptr(y), bb, h, w, c, dt(x), _stream()), "maxpool3s2_cl")
    return y


def maxpool3s2_bwd_cl(gy, x):
    """Backward of maxpool3s2_cl: gy (B, Ho, Wo, C) and the saved input x (B, H, W, C) -> gx in x's shape, every element
    written; the arg-max is recomputed from x (gather form, nothing scattered)."""
    _dev(gy, x)
    bb, h, w, c = _pool_map("maxpool3s2_bwd_cl", x)
    if gy.dtype != x.dtype or tuple(gy.shape) != (bb, (h - 1) // 2 + 1, (w - 1) // 2 + 1, c):
        raise TrambaHipError(f"maxpool3s2_bwd_cl: gy {tuple(gy.shape)} {gy.dtype} does not belong to x {tuple(x.shape)} {x.dtype}")
    gx = torch.empty_like(x)
    _check(lib().tramba_maxpool3s2_bwd_cl(_ptr(gy), _ptr(x), _ptr(gx), bb, h, w, c, dt(x), _stream()), "maxpool3s2_bwd_cl")
    return gx


# ----------------------------------------------------------------------------- ResNet-50 encoder: backward of the bottleneck convolutions
def conv_train_supported(dtype, h, w, cin, cout, ksize, stride):
    """can conv_affine_cl (as the raw convolution), conv_dgrad_cl and conv_wgrad_cl take this layer on this map (batch 1)?
    The forward's domain with Cout % 64 == 0 for the input gradient's reduction (1x1 / stride 1 is a plain product and needs
    Cout % 8 only) and gy and the f32 weight gradient below 2^31 bytes."""
    if not conv_affine_supported(dtype, h, w, cin, cout, ksize, stride):
        return False
    ho, wo = conv_out_size(h, ksize, stride), conv_out_size(w, ksize, stride)
    return ((cout % 64 == 0 or (ksize == 1 and stride == 1)) and ho > 0 and wo > 0 and ho * wo * cout * 2 < 2 ** 31
            and cout * ksize * ksize * cin * 4 < 2 ** 31 and h * w < 2 ** 31 - 1 and (cin + 63) // 64 <= 65535)


def conv_wgrad_steps(m):
    """32-token steps of conv_wgrad_cl's reduction over m output pixels"""
    return (m + 31) // 32


def conv_wgrad_split(batch, h, w, cin, cout, ksize, stride):
    """the number of f32 slabs conv_wgrad_cl leaves (the rule of csrc/resnet_conv.hip, cw_plan), without the library"""
    m = batch * conv_out_size(h, ksize, stride) * conv_out_size(w, ksize, stride)
    steps = conv_wgrad_steps(m)
    base = (ksize * ksize * cin // 64) * ((cout + 63) // 64)
    want = min(max(512 // max(base, 1), 1), 64, steps)
    per = (steps + want - 1) // want
    return (steps + per - 1) // per


def conv_transposed_weight(w_kmajor):
    """(Cout, k, k, Cin) -> the (Cin, k, k, Cout) copy conv_dgrad_cl reads (a framework data-movement op; cache it per weight)"""
    return w_kmajor.permute(3, 1, 2, 0).contiguous()


def _conv_bwd_geom(name, gy, x_shape, x_dtype, ksize, stride):
    if gy.dim() != 4 or len(x_shape) != 4 or gy.dtype != x_dtype or gy.dtype not in _ATTN_DTYPES:
        raise TrambaHipError(f"{name}: need gy (B, Ho, Wo, Cout) and x (B, H, W, Cin) of one 16-bit dtype, got {tuple(gy.shape)} "
                             f"{gy.dtype} {tuple(x_shape)} {x_dtype}")
    if ksize not in (1, 3) or stride not in (1, 2):
        raise TrambaHipError(f"{name}: ksize = {ksize} must be 1 or 3 and stride = {stride} 1 or 2")
    bb, h, wd, cin = x_shape
    if tuple(gy.shape[:3]) != (bb, conv_out_size(h, ksize, stride), conv_out_size(wd, ksize, stride)):
        raise TrambaHipError(f"{name}: gy {tuple(gy.shape)} does not belong to x {tuple(x_shape)} with ksize = {ksize}, "
                             f"stride = {stride}")
    return bb, h, wd, cin, gy.shape[3]


def conv_dgrad_cl(gy, wt, x_shape, stride=1):
    """Input gradient of the raw convolution of conv_affine_cl: gy (B, Ho, Wo, Cout), wt (Cin, k, k, Cout) =
    conv_transposed_weight(w_kmajor), x_shape (B, H, W, Cin) -> gx of that shape in gy's dtype, every element written (zeros
    where no output reaches)."""
    _dev(gy, wt)
    k = wt.shape[1] if wt.dim() == 4 else 0
    bb, h, wd, cin, cout = _conv_bwd_geom("conv_dgrad_cl", gy, tuple(x_shape), wt.dtype, k, stride)
    if tuple(wt.shape) != (cin, k, k, cout):
        raise TrambaHipError(f"conv_dgrad_cl: wt must be (Cin, k, k, Cout) = {(cin, k, k, cout)}, got {tuple(wt.shape)}")
    gx = torch.empty((bb, h, wd, cin), dtype=gy.dtype, device=gy.device)
    _check(lib().tramba_conv_dgrad_cl(_ptr(gy), _ptr(wt), _ptr(gx), bb, h, wd, cin, cout, k, stride, dt(gy), _stream()),
           "conv_dgrad_cl")
    return gx


def conv_wgrad_cl(gy, x, ksize, stride=1):
    """Weight gradient of the raw convolution of conv_affine_cl: gy (B, Ho, Wo, Cout), x (B, H, W, Cin) -> gw (Cout, k, k, Cin)
    f32 K-major.  The kernel leaves one f32 slab per token run; they are added in index order by slab_sum (at once: the
    caller permutes the result, so the sum cannot be deferred)."""
    _dev(gy, x)
    bb, h, wd, cin, cout = _conv_bwd_geom("conv_wgrad_cl", gy, tuple(x.shape), x.dtype, ksize, stride)
    nsplit = lib().tramba_conv_wgrad_split(bb, h, wd, cin, cout, ksize, stride)
    nbytes = lib().tramba_conv_wgrad_work(bb, h, wd, cin, cout, ksize, stride)
    work = torch.empty((nsplit, cout * ksize * ksize * cin), dtype=torch.float32, device=gy.device)   # (none for a refused shape)
    _check(lib().tramba_conv_wgrad_cl(_ptr(gy), _ptr(x), _ptr(work), nbytes, bb, h, wd, cin, cout, ksize, stride, dt(gy),
                                      _stream()), "conv_wgrad_cl")
    out = slab_sum(work) if nsplit > 1 else work[0]
    return out.view(cout, ksize, ksize, cin)
