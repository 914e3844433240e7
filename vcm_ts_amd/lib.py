"""ctypes bindings of the two C-ABI libraries (include/dcvc_hip*.h, include/dcvc_rans.h).

There is no fallback: if a library is missing the import of the product path fails loudly
(`LibraryMissing`) -- build with ``python -c "import __graft_entry__ as g; g.build()"`` or
``make -C vcm_ts_amd/csrc``.
"""
from __future__ import annotations

import ctypes as C
import functools
import os

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")


class LibraryMissing(RuntimeError):
    pass


class KernelError(RuntimeError):
    pass


def _load(name):
    # DCVC_HIP_LIB: developer override used by the kernel probes (tools/conv_probe.py) only
    path = os.environ.get("DCVC_HIP_LIB") if name == "libdcvc_hip.so" and os.environ.get("DCVC_HIP_LIB") else \
        os.path.join(CSRC, name)
    if not os.path.exists(path):
        raise LibraryMissing(f"{path} not built; run `make -C {CSRC}` (no CPU fallback exists)")
    return C.CDLL(path)


# ----------------------------------------------------------------------------- rans (host)
@functools.lru_cache(maxsize=None)
def rans():
    L = _load("libdcvc_rans.so")
    L.dcvc_rans_encoder_create.restype = C.c_void_p
    L.dcvc_rans_encoder_destroy.argtypes = [C.c_void_p]
    L.dcvc_rans_encoder_reset.argtypes = [C.c_void_p]
    L.dcvc_rans_encoder_encode_with_indexes.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                                        C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    L.dcvc_rans_encoder_flush_bound.argtypes = [C.c_void_p]
    L.dcvc_rans_encoder_flush_bound.restype = C.c_int64
    L.dcvc_rans_encoder_flush.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    L.dcvc_rans_encoder_flush.restype = C.c_int64
    L.dcvc_rans_decoder_create.restype = C.c_void_p
    L.dcvc_rans_decoder_destroy.argtypes = [C.c_void_p]
    L.dcvc_rans_decoder_set_stream.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
    L.dcvc_rans_decoder_decode_stream.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32,
                                                  C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.dcvc_pmf_to_quantized_cdf.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    return L


# ----------------------------------------------------------------------------- hip kernels
class Seg(C.Structure):
    _fields_ = [("ptr", C.c_void_p), ("C", C.c_int32), ("cs", C.c_int32)]


class ConvArgs(C.Structure):
    _fields_ = [
        ("seg", Seg * 3), ("nseg", C.c_int32), ("N", C.c_int32), ("Hin", C.c_int32), ("Win", C.c_int32),
        ("in_act", C.c_int32), ("in_slope", C.c_float), ("wpack", C.c_void_p), ("bpack", C.c_void_p),
        ("ks", C.c_int32), ("stride", C.c_int32), ("Cout", C.c_int32), ("Cout_pad", C.c_int32),
        ("out", C.c_void_p), ("out_cs", C.c_int32), ("out_act", C.c_int32), ("out_slope", C.c_float),
        ("pixel_shuffle", C.c_int32), ("res", C.c_void_p), ("res_cs", C.c_int32), ("res_gate", C.c_void_p),
        ("res2", C.c_void_p), ("res2_cs", C.c_int32), ("precision", C.c_int32), ("status", C.c_void_p),
        ("chan_partial", C.c_void_p), ("tile_row0", C.c_int32), ("tile_rows", C.c_int32), ("pair_taps", C.c_int32),
    ]


class DualPriorArgs(C.Structure):
    _fields_ = [
        ("y", C.c_void_p), ("y_cs", C.c_int32), ("fusion", C.c_void_p), ("fusion_cs", C.c_int32),
        ("spatial", C.c_void_p), ("spatial_cs", C.c_int32), ("params", C.c_void_p), ("params_cs", C.c_int32),
        ("y_hat", C.c_void_p), ("y_q", C.c_void_p), ("y_res", C.c_void_p), ("scales_hat", C.c_void_p),
        ("sym", C.c_void_p), ("idx", C.c_void_p), ("out", C.c_void_p), ("out_cs", C.c_int32),
        ("q_basic", C.c_void_p), ("q_scale", C.c_void_p), ("N", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
        ("C", C.c_int32), ("step", C.c_int32), ("idx_edges", C.c_void_p), ("forced_q", C.c_void_p),
        ("q_map", C.c_void_p),
    ]


class ConvBwdArgs(C.Structure):
    _fields_ = [
        ("dout", C.c_void_p), ("dout_cs", C.c_int32), ("out", C.c_void_p), ("out_cs", C.c_int32),
        ("res", C.c_void_p), ("res_cs", C.c_int32), ("gate", C.c_void_p), ("res2", C.c_void_p), ("res2_cs", C.c_int32),
        ("dres", C.c_void_p), ("dres_cs", C.c_int32), ("dres2", C.c_void_p), ("dres2_cs", C.c_int32),
        ("dpre", C.c_void_p), ("dpre_cs", C.c_int32), ("zs", C.c_int32), ("Hd", C.c_int32), ("Wd", C.c_int32),
        ("N", C.c_int32), ("Ho", C.c_int32), ("Wo", C.c_int32), ("Cout", C.c_int32), ("pixel_shuffle", C.c_int32),
        ("act", C.c_int32), ("slope", C.c_float),
    ]


class WgradArgs(C.Structure):
    _fields_ = [
        ("x", C.c_void_p), ("x_cs", C.c_int32), ("C", C.c_int32), ("in_act", C.c_int32), ("in_slope", C.c_float),
        ("dpre", C.c_void_p), ("dpre_cs", C.c_int32), ("zs", C.c_int32), ("Hd", C.c_int32), ("Wd", C.c_int32),
        ("N", C.c_int32), ("Hin", C.c_int32), ("Win", C.c_int32), ("Ho", C.c_int32), ("Wo", C.c_int32),
        ("Cout", C.c_int32), ("ks", C.c_int32), ("stride", C.c_int32), ("dw", C.c_void_p), ("Cin_total", C.c_int32),
        ("cin_offset", C.c_int32), ("scratch", C.c_void_p), ("scratch_floats", C.c_int64), ("overwrite", C.c_int32),
        ("db", C.c_void_p), ("precision", C.c_int32),
    ]


class PackJob(C.Structure):  # dcvc_pack_job (include/dcvc_hip_grad.h)
    _fields_ = [
        ("w", C.c_void_p), ("b", C.c_void_p), ("Cout", C.c_int32), ("Cin_total", C.c_int32), ("ks", C.c_int32),
        ("nseg", C.c_int32), ("seg_C", C.c_int32 * 3), ("cin_offset", C.c_int32), ("pixel_shuffle", C.c_int32),
        ("precision", C.c_int32), ("transposed", C.c_int32), ("wpack", C.c_void_p), ("bpack", C.c_void_p),
    ]


class DualPriorBwdArgs(C.Structure):
    _fields_ = [
        ("y", C.c_void_p), ("y_cs", C.c_int32), ("fusion", C.c_void_p), ("fusion_cs", C.c_int32),
        ("y_hat", C.c_void_p), ("dout", C.c_void_p), ("dout_cs", C.c_int32), ("dy_res", C.c_void_p),
        ("dscales_hat", C.c_void_p), ("dparams", C.c_void_p), ("dparams_cs", C.c_int32),
        ("dspatial", C.c_void_p), ("dspatial_cs", C.c_int32), ("dy", C.c_void_p), ("dy_cs", C.c_int32),
        ("dfusion", C.c_void_p), ("dfusion_cs", C.c_int32), ("dq_plane", C.c_void_p),
        ("q_basic", C.c_void_p), ("q_scale", C.c_void_p), ("N", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
        ("C", C.c_int32), ("step", C.c_int32),
    ]


class ColorCoeffs(C.Structure):  # dcvc_color_coeffs_t (include/dcvc_hip_color.h)
    _fields_ = [(n, C.c_float) for n in ("y_off", "c_off", "y_scale", "c_scale", "crr", "cgb", "cgr", "cbb", "kr", "kg", "kb",
                                         "icb", "icr", "y_range", "c_range")] + \
               [(n, C.c_int32) for n in ("max_code", "bit_depth", "siting", "matrix", "range")]


class RoiBox(C.Structure):  # dcvc_roi_box_t (include/dcvc_hip_roi.h)
    _fields_ = [(n, C.c_int32) for n in ("x1", "y1", "x2", "y2", "cls")]


class RoiClassRec(C.Structure):  # dcvc_roi_class_t
    _fields_ = [("border", C.c_int32), ("shrink", C.c_int32), ("feather", C.c_float * 64)]


PRECISIONS = {"fp32": 0, "fp16x3": 1}

i32, i64, f32, vp = C.c_int32, C.c_int64, C.c_float, C.c_void_p

# One table per header of include/, in the headers' order.  A function that answers the int status is bound as the list of
# its argtypes; the size queries and the void destructor as a tuple (restype, argtype, ...).  Everything below is derived
# from this table, and tests/test_bindings_host.py holds it against the headers' own declarations.
HEADERS = {
    "dcvc_hip.h": {
        "dcvc_conv_tile_rows": (i32, i32, i32),
        "dcvc_conv_chan_partial_parts": (i32, i32, i32, i32, i32),
        "dcvc_channel_mean_finish": [vp, i32, i32, vp, i32, i32, i32, vp],
        "dcvc_conv_pack_size": (i64, i32, i32, i32, vp, C.POINTER(i32)),
        "dcvc_conv_pack_weights": [vp, vp, i32, i32, i32, vp, i32, i32, vp, vp],
        "dcvc_conv_pack_size_paired": (i64, i32, i32, C.POINTER(i32)),
        "dcvc_conv_pack_weights_paired": [vp, vp, i32, i32, vp, vp],
        "dcvc_conv2d": [C.POINTER(ConvArgs), vp],
        "dcvc_conv_set_lookahead": [i32],
        "dcvc_conv_small_pack_bytes": (i64, i32, i32, i32, vp),
        "dcvc_conv_small_pack_weights": [vp, vp, i32, i32, i32, vp, vp, vp],
        "dcvc_conv2d_small": [C.POINTER(ConvArgs), vp],
        "dcvc_conv_k32_pack_bytes": (i64, i32, i32, i32, vp, C.POINTER(i32)),
        "dcvc_conv_k32_pack_weights": [vp, vp, i32, i32, i32, vp, i32, vp, vp],
        "dcvc_conv2d_k32": [C.POINTER(ConvArgs), vp],
        "dcvc_conv_k32_set_waves": [i32],
        "dcvc_warp": [vp, i32, vp, i32, vp, i32, i32, i32, i32, i32, vp],
        "dcvc_up2": [vp, i32, vp, i32, vp, i32, i32, i32, i32, i32, f32, vp],
        "dcvc_down2": [vp, i32, vp, i32, i32, i32, i32, i32, f32, i32, vp],
        "dcvc_maxpool2": [vp, i32, vp, i32, i32, i32, i32, i32, vp],
        "dcvc_copy_channels": [vp, i32, vp, i32, i64, i32, vp],
        "dcvc_nchw_to_nhwc": [vp, vp, i32, i32, i32, i32, i32, vp],
        "dcvc_nhwc_to_nchw": [vp, i32, vp, i32, i32, i32, i32, i32, vp],
        "dcvc_channel_mean": [vp, i32, vp, vp, i32, i32, i32, vp],
        "dcvc_se_gate": [vp, vp, vp, vp, i32, i32, i32, vp],
        "dcvc_scale_channels": [vp, i32, vp, i32, vp, vp, i32, i32, i32, i32, vp],
        "dcvc_scale_channels_map": [vp, i32, vp, i32, vp, vp, i32, i32, i32, i32, vp, i32, i32, vp],
        "dcvc_round_symbols": [vp, i32, vp, i32, vp, i32, i32, i32, i32, vp],
        "dcvc_symbols_to_nhwc": [vp, vp, i32, i32, i32, i32, i32, vp],
        "dcvc_scale_indexes": [vp, vp, i64, vp, vp],
        "dcvc_dual_prior_enc": [C.POINTER(DualPriorArgs), vp],
        "dcvc_dual_prior_dec_index": [C.POINTER(DualPriorArgs), vp],
        "dcvc_dual_prior_dec_apply": [C.POINTER(DualPriorArgs), vp],
        "dcvc_scale_bits": [vp, vp, vp, vp, i32, i32, i64, vp],
        "dcvc_factorized_bits": [vp, i32, vp, vp, vp, i32, i32, i32, vp],
        "dcvc_sq_err": [vp, i32, vp, i32, vp, vp, i32, i32, i32, vp],
        "dcvc_cdf_table_cols": (i32,),
        "dcvc_build_scale_cdfs": [vp, i32, i32, vp, vp, vp, vp],
        "dcvc_build_factorized_cdfs": [vp, i32, vp, vp, vp, vp],
        "dcvc_hip_version": (C.c_char_p,),
    },
    "dcvc_hip_grad.h": {
        "dcvc_conv_pack_weights_dev": [vp, vp, i32, i32, i32, i32, vp, i32, i32, i32, i32, vp, vp, vp],
        "dcvc_pack_plan_create": [C.POINTER(PackJob), i32, C.POINTER(C.c_void_p)],
        "dcvc_pack_plan_run": [vp, vp],
        "dcvc_pack_plan_destroy": (None, vp),
        "dcvc_conv_bwd_prologue": [C.POINTER(ConvBwdArgs), vp],
        "dcvc_conv_wgrad_scratch_min": (i64, i32, i32, i32),
        "dcvc_conv_wgrad": [C.POINTER(WgradArgs), vp],
        "dcvc_channel_dot": [vp, i32, vp, i32, vp, vp, i32, i32, i32, i32, i32, vp],
        "dcvc_mask_accumulate": [vp, i32, vp, i32, f32, vp, i32, i64, i32, vp],
        "dcvc_add_planes": [vp, i32, vp, i32, vp, i32, i64, i32, vp],
        "dcvc_warp_bwd": [vp, i32, vp, i32, vp, i32, vp, i32, vp, i32, i32, i32, i32, i32, vp, vp],
        "dcvc_up2_bwd": [vp, i32, vp, i32, i32, i32, i32, i32, f32, vp],
        "dcvc_down2_bwd": [vp, i32, vp, i32, i32, i32, i32, i32, f32, vp],
        "dcvc_maxpool2_bwd": [vp, i32, vp, i32, vp, i32, i32, i32, i32, i32, vp],
        "dcvc_se_bwd": [vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp],
        "dcvc_add_channel_vec": [vp, i32, vp, f32, i32, i32, i32, vp],
        "dcvc_scale_channels_bwd": [vp, i32, vp, i32, vp, vp, i32, i32, i32, i32, vp],
        "dcvc_q_finish": [vp, vp, vp, vp, vp, vp, i32, i32, vp],
        "dcvc_dual_prior_bwd": [C.POINTER(DualPriorBwdArgs), vp],
        "dcvc_scale_bits_bwd": [vp, vp, vp, vp, vp, i32, i32, i64, vp],
        "dcvc_factorized_bits_bwd": [vp, i32, vp, vp, vp, i32, vp, i32, i32, i32, vp],
        "dcvc_sq_err_bwd": [vp, i32, vp, i32, vp, vp, i32, i32, i32, i32, vp],
    },
    "dcvc_hip_rans.h": {
        "dcvc_drans_default_lanes": (i32, i64),
        "dcvc_drans_scratch_words": (i64, i64, i32),
        "dcvc_drans_build_lut": [vp, i32, i32, vp, vp],
        "dcvc_drans_encode": [vp, vp, i32, i32, i64, vp, i32, i32, vp, vp, i32, vp, i64, vp, i64, vp, vp, vp, vp],
        "dcvc_drans_decode": [vp, i64, vp, vp, vp, i32, i32, i64, vp, i32, i32, vp, vp, vp, i32, vp, vp, vp],
    },
    "dcvc_hip_metrics.h": {
        "dcvc_ms_ssim": [vp, vp, i32, i32, i32, i32, i32, i64, i32, i64, f32, i32, vp, vp, vp, vp, vp],
        "dcvc_ms_ssim_grad": [vp, vp, i32, i32, i32, i32, i32, i64, i32, i64, f32, i32, vp, vp, vp, vp],
        "dcvc_ms_ssim_workspace_bytes": (i64, i32, i32, i32, i32, i32),
    },
    "dcvc_hip_color.h": {
        "dcvc_color_coeffs": [i32, i32, i32, i32, vp],
        "dcvc_yuv420_to_rgb": [vp, vp, vp, i32, i32, i32, i32, vp, vp, i32, i32, i32, i64, i32, vp],
        "dcvc_rgb_to_yuv420": [vp, i32, i32, i32, i64, vp, vp, vp, vp, i32, i32, vp, vp, vp, i32, i32, vp, vp],
    },
    "dcvc_hip_roi.h": {
        "dcvc_roi_residual": [vp, i32, i64, vp, i32, i64, i32, i32, vp, vp, i32, vp, i64, i64, i32, i32, i32, i32, vp],
        "dcvc_roi_fuse": [vp, i32, i64, vp, i64, i64, i32, i32, i32, i32, i32, i32, vp, vp, i32, vp, i32, vp, i32, i64, vp],
        "dcvc_roi_sse": [vp, i32, i64, vp, i32, i64, i32, i32, vp, vp, i32, vp, i32, vp, vp],
        "dcvc_roi_qmap": [i32, i32, vp, vp, i32, i32, vp, i32, vp, vp],
    },
    "dcvc_hip_roil.h": {
        "dcvc_roil_cells": [i32, i32, vp, i32, vp, vp, i32],
        "dcvc_roil_check": [vp, i64, vp, i32],
        "dcvc_roil_encode": [vp, i32, i64, vp, i32, i64, i32, i32, vp, vp, i32, i32, vp, i32, vp, vp, i64, vp, vp],
        "dcvc_roil_decode": [vp, vp, i64, i32, i32, vp, vp, i32, vp, vp, i64, i64, i32, i32, i32, i32, vp, vp],
    },
    "dcvc_hip_scene.h": {"dcvc_scene_hist": [vp, i32, i64, i32, i32, vp, vp]},
    "dcvc_hip_bits.h": {
        "dcvc_bits_map_scale": [vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, i32, i32, i32, i32, vp, vp],
        "dcvc_bits_map_factorized": [vp, vp, i32, i32, vp, vp, vp, i32, i32, i32, i32, vp, vp],
        "dcvc_bits_regions": [vp, vp, i32, vp, i32, i32, i32, vp, vp],
        "dcvc_bits_sweep_scale": [vp, vp, vp, vp, i32, vp, i32, i32, vp, vp, vp, i32, i32, i32, i32, vp, vp],
    },
    "dcvc_hip_hash.h": {
        "dcvc_hash_pixels": [vp, i32, i64, i32, i32, vp, vp, vp],
        "dcvc_hash_f32": [vp, i32, i64, i32, i32, i32, vp, vp, vp],
    },
    "dcvc_hip_scale.h": {"dcvc_scale_planes": [vp, i32, i64, vp, i32, i64, i32, i32, i32, i32, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp, i32, vp]},
    "dcvc_hip_aq.h": {
        "dcvc_aq_activity": [vp, i32, i64, i32, i32, vp, vp, vp],
        "dcvc_aq_map": [vp, vp, i32, i32, vp, vp, vp, vp, vp],
    },
    "dcvc_hip_motion.h": {"dcvc_motion_step": [vp, i32, i64, i32, i32, vp, i32, i32, i32, i32, vp, vp]},
    "dcvc_hip_tnr.h": {"dcvc_tnr_step": [vp, i32, i64, vp, i32, i64, vp, i32, i64, i32, i32, vp, i32, vp, vp, vp]},
    "dcvc_hip_redact.h": {"dcvc_redact": [vp, i32, i64, vp, i32, i64, i32, i32, vp, vp, i32, i32, i32, i32, i32, vp, vp]},
    "dcvc_hip_me.h": {
        "dcvc_me_search": [vp, i32, i64, vp, i32, i64, i32, i32, i32, i32, vp, vp, vp, vp],
        "dcvc_me_compensate": [vp, i32, i64, vp, i32, i64, i32, i32, vp, vp],
    },
    "dcvc_hip_png.h": {
        "dcvc_png_bound": (i64, i32, i32, i32),
        "dcvc_png_tables_check": [vp, i32],
        "dcvc_png_encode": [vp, i32, i64, i32, i32, i32, vp, vp, i32, vp, vp, i64, vp, vp],
    },
    "dcvc_hip_grain.h": {
        "dcvc_grain_measure": [vp, i32, i64, vp, i32, i64, i32, i32, vp, vp, vp],
        "dcvc_grain_apply": [vp, i32, i64, vp, i32, i64, i32, i32, i32, i32, i32, vp, vp],
    },
    "dcvc_hip_tnr_fuse.h": {
        "dcvc_tnr_fuse": [vp, i32, i64, vp, vp, vp, vp, i32, i64, i32, vp, i32, i64, i32, i32, vp, vp, i32, vp, vp, vp],
    },
    "dcvc_hip_mesub.h": {
        "dcvc_me_refine": [vp, i32, i64, vp, i32, i64, i32, i32, i32, vp, vp, vp, vp],
        "dcvc_me_compensate_sub": [vp, i32, i64, vp, i32, i64, i32, i32, vp, vp],
    },
    "dcvc_hip_mesplit.h": {
        "dcvc_me_split": [vp, i32, i64, vp, i32, i64, i32, i32, i32, i32, vp, vp, vp, vp],
        "dcvc_me_compensate_split": [vp, i32, i64, vp, i32, i64, i32, i32, vp, vp],
    },
    "dcvc_hip_mepyr.h": {
        "dcvc_me_pyramid": [vp, i32, i64, i32, i32, i32, vp, i32, vp, i32, vp, i32, vp],
        "dcvc_me_coarse": [vp, i32, vp, i32, i32, i32, i32, i32, i32, vp, vp],
        "dcvc_me_descend": [vp, i32, vp, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp],
    },
    "dcvc_hip_deint.h": {
        "dcvc_deinterlace420": [vp, vp, vp, i32, i32, vp, vp, vp, i32, i32, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp, i32, i32,
                                vp, i32, vp],
    },
    "dcvc_hip_noise.h": {
        "dcvc_noise_cells": [vp, i32, i64, i32, i32, vp, vp, i32, vp, vp],
        "dcvc_noise_hist": [vp, i64, vp, vp],
    },
    "dcvc_hip_shake.h": {
        "dcvc_shake_plane": [vp, i32, i64, i32, i32, vp, i32, vp],
        "dcvc_shake_tiles": [vp, i32, i64, i32, i32, vp, i32, i32, vp, vp],
        "dcvc_shake_vote": [vp, i32, i32, i32, i32, i32, vp, vp, vp],
    },
}


def _signature(entry):  # (restype, argtypes) of a table entry
    return (entry[0], list(entry[1:])) if isinstance(entry, tuple) else (C.c_int, entry)


# every function of libdcvc_hip.so, and the argtypes of those that answer a status (or nothing: the void destructor)
ALL_HIP_SYMBOLS = [name for funcs in HEADERS.values() for name in funcs]
_SIGS = {name: _signature(e)[1] for funcs in HEADERS.values() for name, e in funcs.items() if isinstance(e, list) or e[0] is None}
# the three kernel headers share HIP_SYMBOLS; every feature header has a list of its own, in the table's order
_CORE = ("dcvc_hip.h", "dcvc_hip_grad.h", "dcvc_hip_rans.h")
HIP_SYMBOLS = sorted(name for h in _CORE for name in HEADERS[h])
(METRICS_SYMBOLS, COLOR_SYMBOLS, ROI_SYMBOLS, ROIL_SYMBOLS, SCENE_SYMBOLS, BITS_SYMBOLS, HASH_SYMBOLS, SCALE_SYMBOLS, AQ_SYMBOLS,
 MOTION_SYMBOLS, TNR_SYMBOLS, REDACT_SYMBOLS, ME_SYMBOLS, PNG_SYMBOLS, GRAIN_SYMBOLS, TNR_FUSE_SYMBOLS, MESUB_SYMBOLS, MESPLIT_SYMBOLS,
 MEPYR_SYMBOLS, DEINT_SYMBOLS, NOISE_SYMBOLS, SHAKE_SYMBOLS) = (list(funcs) for h, funcs in HEADERS.items() if h not in _CORE)
HASH_CONSTANTS = ["dcvc_hash_chunk_bytes", "dcvc_hash_block_bytes", "dcvc_hash_scratch_bytes"]  # (int32 data symbols)
RANS_SYMBOLS = [  # include/dcvc_rans.h (libdcvc_rans.so, bound in rans() above)
    "dcvc_rans_encoder_create", "dcvc_rans_encoder_destroy", "dcvc_rans_encoder_reset",
    "dcvc_rans_encoder_encode_with_indexes", "dcvc_rans_encoder_flush_bound", "dcvc_rans_encoder_flush",
    "dcvc_rans_decoder_create", "dcvc_rans_decoder_destroy", "dcvc_rans_decoder_set_stream",
    "dcvc_rans_decoder_decode_stream", "dcvc_pmf_to_quantized_cdf",
]


@functools.lru_cache(maxsize=None)
def hip():
    L = _load("libdcvc_hip.so")
    for funcs in HEADERS.values():
        for name, entry in funcs.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = _signature(entry)
    return L


def hash_constant(name):
    """One of HASH_CONSTANTS: the library's own value, not a copy of the header's."""
    return int(i32.in_dll(hip(), name).value)


def check(code, what):
    if code != 0:
        raise KernelError(f"{what} failed with status {code}")
