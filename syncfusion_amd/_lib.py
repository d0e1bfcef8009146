"""ctypes binding of ``libsyncfusion_amd.so`` (the C ABI declared in include/syncfusion_amd.h).

The product path has no CPU fallback: if the shared library is missing, or a CPU tensor reaches a
forward/sample call, this module raises.  ``torch`` is used for device memory and streams only;
no torch type crosses the ABI (raw ``data_ptr()`` integers and the HIP stream handle do).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import torch

SF_MAX_DEPTH = 12
SF_F32, SF_BF16, SF_F16, SF_F32X = 0, 1, 2, 3
UPSAMPLE_MODES = {"nearest": 0, "transpose": 1}
DTYPES = {"fp32": SF_F32, "float32": SF_F32, "f32": SF_F32, "bf16": SF_BF16, "bfloat16": SF_BF16, "fp16": SF_F16, "float16": SF_F16, "f16": SF_F16, "half": SF_F16,
          "fp32x": SF_F32X}

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SF_LIB_PATH") or os.path.join(_HERE, "lib", "libsyncfusion_amd.so")   # SF_LIB_PATH: A/B builds of the HIP library (tuning aid)


class SfTensor(C.Structure):
    _fields_ = [("name", C.c_char_p), ("data", C.c_void_p), ("numel", C.c_int64)]


class UnetConfig(C.Structure):
    _fields_ = [
        ("n_layers", C.c_int32), ("in_channels", C.c_int32),
        ("channels", C.c_int32 * SF_MAX_DEPTH), ("factors", C.c_int32 * SF_MAX_DEPTH),
        ("items", C.c_int32 * SF_MAX_DEPTH), ("attentions", C.c_int32 * SF_MAX_DEPTH),
        ("cross_attentions", C.c_int32 * SF_MAX_DEPTH), ("context_channels", C.c_int32 * SF_MAX_DEPTH),
        ("attention_heads", C.c_int32), ("attention_features", C.c_int32),
        ("embedding_features", C.c_int32), ("embedding_max_length", C.c_int32),
        ("modulation_features", C.c_int32), ("resnet_groups", C.c_int32), ("dtype", C.c_int32),
        ("upsample_mode", C.c_int32),
        ("time_fourier_features", C.c_int32), ("time_no_first_act", C.c_int32), ("attention_out_bias", C.c_int32),
    ]


class EncoderConfig(C.Structure):
    _fields_ = [
        ("n_layers", C.c_int32), ("in_channels", C.c_int32), ("channels", C.c_int32),
        ("multipliers", C.c_int32 * (SF_MAX_DEPTH + 1)), ("factors", C.c_int32 * SF_MAX_DEPTH),
        ("num_blocks", C.c_int32 * SF_MAX_DEPTH), ("resnet_groups", C.c_int32), ("patch_size", C.c_int32),
    ]


class VConvDesc(C.Structure):
    """sf_vconv_desc: one video-geometry convolution of the onset net's training path."""
    _fields_ = [(n, C.c_int32) for n in ("N", "T", "Hi", "Wi", "cin", "cin_ld", "cout", "cout_ld", "kt", "kh", "kw", "sh", "sw", "pt", "ph", "pw")]


class Conv1dEpiDesc(C.Structure):
    """sf_conv1d_epi_desc: one implicit-GEMM launch with its whole epilogue (sf_op_conv1d_epi / sf_op_conv1d_ln)."""
    _fields_ = [(n, C.c_int32) for n in ("dtype", "B", "L", "C", "C2", "N", "taps", "stride", "pad", "upsample", "act", "out_f32", "mt_ln", "res_ln",
                                         "ln_operand", "solo")] + \
               [("ln_eps", C.c_float), ("src_x3", C.c_int32)] + \
               [(n, C.c_void_p) for n in ("x", "x2", "w", "bias", "bscale", "badd", "residual", "out", "rowpart", "gnpart", "ln_part", "ln_ss")]


SF_CLAP_MAX_STAGES = 8


class ClapAudioEngineConfig(C.Structure):
    """sf_clap_audio_config: the Swin network behind the log-mel image (syncfusion_amd/clap.py)."""
    _fields_ = [("spec_size", C.c_int32), ("embed_dim", C.c_int32), ("n_stages", C.c_int32),
                ("depths", C.c_int32 * SF_CLAP_MAX_STAGES), ("heads", C.c_int32 * SF_CLAP_MAX_STAGES),
                ("window", C.c_int32), ("mlp_ratio", C.c_int32), ("joint_dim", C.c_int32),
                ("ln_eps", C.c_float), ("mask_value", C.c_float), ("projection_relu", C.c_int32), ("normalize", C.c_int32)]


class ClapTextEngineConfig(C.Structure):
    """sf_clap_text_config: RoBERTa and the projection behind the token ids (syncfusion_amd/clap_text.py)."""
    _fields_ = [(n, C.c_int32) for n in ("vocab_size", "hidden", "layers", "heads", "intermediate", "max_positions", "pad_id", "max_length", "joint_dim")] + \
               [("ln_eps", C.c_float), ("pooling", C.c_int32), ("projection_relu", C.c_int32), ("normalize", C.c_int32)]


class JpegDesc(C.Structure):
    """sf_jpeg_desc: what the parser says about one JPEG file (syncfusion_amd/jpeg.py)."""
    _fields_ = [("status", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("ncomp", C.c_int32),
                ("h", C.c_int32 * 3), ("v", C.c_int32 * 3), ("tq", C.c_int32 * 3), ("td", C.c_int32 * 3), ("ta", C.c_int32 * 3),
                ("restart_interval", C.c_int32), ("mcus_x", C.c_int32), ("mcus_y", C.c_int32), ("quant_precision", C.c_int32 * 4),
                ("huff_present", C.c_int32), ("seg_count", C.c_int32), ("seg_begin", C.c_int64), ("data_begin", C.c_int64),
                ("data_end", C.c_int64), ("coef_offset", C.c_int64), ("plane_offset", C.c_int64), ("reserved", C.c_int64),
                ("quant", (C.c_uint16 * 64) * 4), ("huff_counts", (C.c_uint8 * 16) * 4), ("huff_values", (C.c_uint8 * 256) * 4),
                ("reason", C.c_char * 64)]


class JpegSegment(C.Structure):
    """sf_jpeg_segment: one independently decodable stretch of entropy-coded bytes."""
    _fields_ = [("image", C.c_int32), ("first_mcu", C.c_int32), ("mcu_count", C.c_int32), ("reserved", C.c_int32),
                ("byte_begin", C.c_int64), ("byte_end", C.c_int64)]


# every symbol include/syncfusion_amd.h declares: (restype, argtypes)
_P, _I, _L, _F = C.c_void_p, C.c_int, C.c_int64, C.c_float
SYMBOLS = {
    "sf_version": (C.c_char_p, []),
    "sf_last_error": (C.c_char_p, []),
    "sf_device_ok": (_I, []),
    "sf_clock_probe_start": (_I, [C.c_double, _P]),
    "sf_clock_probe_read": (_I, [C.POINTER(C.c_double)]),
    "sf_unet_create": (_I, [C.POINTER(UnetConfig), C.POINTER(SfTensor), _I, _P, C.POINTER(_P)]),
    "sf_unet_destroy": (None, [_P]),
    "sf_unet_param_count": (_I, [C.POINTER(UnetConfig)]),
    "sf_unet_param_name": (_I, [C.POINTER(UnetConfig), _I, C.c_char_p, _I, C.POINTER(_L)]),
    "sf_unet_workspace_bytes": (_L, [_P, _I, _I, _I]),
    "sf_vsample_workspace_bytes": (_L, [_P, _I, _I, _I, _I]),
    "sf_unet_forward": (_I, [_P, _P, _P, C.POINTER(_P), _P, _I, _I, _F, _P, _P, _L, _P]),
    "sf_vsample": (_I, [_P, _P, C.POINTER(_P), _P, _I, _I, _I, _F, _I, _P, _L, _P]),
    "sf_vinpaint_workspace_bytes": (_L, [_P, _I, _I, _I, _I, _I]),
    "sf_vinpaint": (_I, [_P, _P, _P, _P, C.POINTER(_P), _P, _I, _I, _I, _I, C.c_uint64, _F, _I, _P, _L, _P]),
    "sf_vsample_ms_workspace_bytes": (_L, [_P, _I, _I, _I, _I]),
    # (h, x_inout, ctx, emb, B, L0, num_steps, embedding_scale, sigmas_host, table_host, use_graph, ws, ws_bytes, stream)
    "sf_vsample_ms": (_I, [_P, _P, C.POINTER(_P), _P, _I, _I, _I, _F, _P, _P, _I, _P, _L, _P]),
    # (x, v, v_uncond, scale, hist, table, step_idx, e0, e1, stream)
    "sf_op_vsampler_update_ms": (_I, [_P, _P, _P, _F, _P, _P, _P, _L, _L, _P]),
    "sf_vsample_gx_workspace_bytes": (_L, [_P, _I, _I, _I, _I]),
    # (h, x_inout, ctx, emb, B, L0, num_steps, sigmas_host, table_host, scales_host, rescale, hist_io, use_graph, ws, ws_bytes, stream)
    "sf_vsample_gx": (_I, [_P, _P, C.POINTER(_P), _P, _I, _I, _I, _P, _P, _P, _F, _P, _I, _P, _L, _P]),
    "sf_op_guidance_stats_bytes": (_L, [_I, _L]),
    # (v, v_uncond, gtab, step_idx, B, clip_len, part, part_bytes, stream)
    "sf_op_guidance_stats": (_I, [_P, _P, _P, _P, _I, _L, _P, _L, _P]),
    # (x, v, v_uncond, hist, table, gtab, step_idx, part, rescale, B, clip_len, factor_out, e0, e1, stream)
    "sf_op_vsampler_update_g": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _F, _I, _L, _P, _L, _L, _P]),
    "sf_op_philox_normal": (_I, [C.c_uint64, C.c_uint32, _L, _L, _P, _P]),
    "sf_op_vinpaint_update": (_I, [_P, _P, _P, _F, _P, _P, _P, _P, _P, _L, _L, _P]),
    "sf_unet_debug_enable": (_I, [_P, _P, _L]),
    "sf_unet_debug_count": (_I, [_P]),
    "sf_unet_debug_info": (_I, [_P, _I, C.c_char_p, _I, C.POINTER(_L), C.POINTER(_L), C.POINTER(C.c_int32)]),
    "sf_unet_launch_count": (_I, [_P]),
    "sf_unet_graph_captures": (_I, [_P]),
    "sf_unet_set_branches": (_I, [_P, _I]),
    "sf_unet_profile_enable": (_I, [_P, _I]),
    "sf_unet_profile_count": (_I, [_P]),
    "sf_unet_profile_get": (_I, [_P, _I, C.c_char_p, _I, C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "sf_unet_profile_depth": (_I, [_P, _I]),
    "sf_encoder1d_create": (_I, [C.POINTER(EncoderConfig), C.POINTER(SfTensor), _I, _P, C.POINTER(_P)]),
    "sf_encoder1d_destroy": (None, [_P]),
    "sf_encoder1d_workspace_bytes": (_L, [_P, _I, _I]),
    "sf_encoder1d_forward": (_I, [_P, _P, _I, _I, C.POINTER(_P), _P, _L, _P]),
    "sf_onsetnet_create": (_I, [C.POINTER(SfTensor), _I, _I, _P, C.POINTER(_P)]),
    "sf_onsetnet_destroy": (None, [_P]),
    "sf_onsetnet_workspace_bytes": (_L, [_P, _I, _I, _I, _I]),
    "sf_onsetnet_forward": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _L, _P]),
    "sf_onsetnet_debug_enable": (_I, [_P, _P, _L]),
    "sf_onsetnet_debug_count": (_I, [_P]),
    "sf_onsetnet_debug_detail": (_I, [_P, _I, C.POINTER(C.c_int32), _I]),
    "sf_onsetnet_debug_path": (_I, [_P, _I]),
    "sf_onsetnet_debug_info": (_I, [_P, _I, C.c_char_p, _I, C.POINTER(_L), C.POINTER(_L), C.POINTER(C.c_int32)]),
    "sf_onsets_to_track": (_I, [_P, _I, _I, _P, _F, _F, _F, _P, _I, _P]),
    "sf_frames_preprocess": (_I, [_P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P]),
    "sf_frames_augment_workspace_bytes": (_L, [_I, _I, _I, _I]),
    # (frames, N, T, H, W, resize_h, resize_w, out_h, out_w, table_host, table_dev, mean3, std3, out, ws, ws_bytes, stream)
    "sf_frames_augment": (_I, [_P, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _L, _P]),
    "sf_times_to_track": (_I, [_P, _P, _I, C.c_double, _I, _I, _P, _P]),
    "sf_cut_prefix_crop": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _P]),
    "sf_resampler_create": (_I, [_I, _I, _I, _F, C.POINTER(_P)]),
    "sf_resampler_destroy": (None, [_P]),
    "sf_resampler_out_length": (_I, [_P, _I]),
    "sf_resampler_forward": (_I, [_P, _P, _I, _I, _P, _P]),
    "sf_op_conv1d_cl": (_I, [_I, _P, _P, _P, _P, _P, _I, _F, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _L, _P]),
    "sf_op_conv1d_bwd_workspace_bytes": (_L, [_I, _I, _I, _I, _I, _I]),
    "sf_op_conv1d_bwd_cl": (_I, [_P, _P, _P, _P, _I, _F, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _L, _P]),
    "sf_op_conv1d_bwd_cl_act": (_I, [_P, _P, _P, _P, _P, _P, _I, _F, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _L, _P]),
    "sf_op_conv1d_bwd_cl_x": (_I, [_I, _P, _P, _P, _P, _P, _P, _I, _F, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _L, _P]),
    "sf_op_conv1d_dgrad_pack_bytes": (_L, [_I, _I, _I]),
    # (dtype, x, w, bias, gamma, beta, groups, eps, residual, B, L, C, N, taps, pad, out, dgrad_pack, dgrad_pack_bytes, ws, ws_bytes, stream)
    "sf_op_conv1d_train_fwd": (_I, [_I, _P, _P, _P, _P, _P, _I, _F, _P, _I, _I, _I, _I, _I, _I, _P, _P, _L, _P, _L, _P]),
    # (dtype, x, act, stats, w, dgrad_pack, gamma, beta, groups, eps, dy, dx_add, B, L, C, N, taps, pad, dx, dw, db, dgb, ws, ws_bytes, stream)
    "sf_op_conv1d_bwd_cl_p": (_I, [_I, _P, _P, _P, _P, _P, _P, _P, _I, _F, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _L, _P]),
    "sf_op_conv1d_train_images": (_I, [_I, _P, _I, _I, _I, _I, _I, _I, _I]),
    # (dtype, B, L, C, N, taps, stride, pad, upsample, groups, label, label_bytes)
    "sf_op_conv1d_variant": (_I, [_I, _I, _I, _I, _I, _I, _I, _I, _I, _I, C.c_char_p, _I]),
    "sf_op_conv1d_bwd_variant": (_I, [_I, _I, _I, _I, _I, _I, _I, C.c_char_p, _I]),
    "sf_train_pack_many": (_I, [_P, _I, _I, _P]),
    # (dtype, x, w, fw, fwx, bias, gamma, beta, groups, eps, residual, B, L, C, N, taps, pad, out, ws, ws_bytes, stream)
    "sf_op_conv1d_train_fwd_pk": (_I, [_I, _P, _P, _P, _P, _P, _P, _P, _I, _F, _P, _I, _I, _I, _I, _I, _I, _P, _P, _L, _P]),
    "sf_op_ln_modulate_bwd_add": (_I, [_P, _P, _P, _P, _F, _I, _I, _I, _P, _P, _P, _L, _P]),
    "sf_op_gn_silu_train_stats_floats": (_L, [_I, _I, _I, _I]),
    "sf_op_gn_silu_train": (_I, [_P, _P, _P, _I, _F, _I, _I, _I, _P, _P, _P]),
    "sf_op_ln_modulate_bwd_workspace_bytes": (_L, [_I, _I, _I]),
    "sf_op_ln_modulate_bwd": (_I, [_P, _P, _P, _F, _I, _I, _I, _P, _P, _P, _L, _P]),
    "sf_op_attention_bwd": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _L, _P]),
    "sf_op_attention_fwd_lse": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _P]),
    "sf_op_attention_fwd_lse_x": (_I, [_I, _P, _P, _I, _I, _I, _I, _P, _P, _P]),
    "sf_op_attention_bwd_lse": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _L, _P]),
    "sf_op_attention_bwd_lse_x": (_I, [_I, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _L, _P]),
    "sf_op_length_sums_workspace_bytes": (_L, [_I, _I, _I]),
    "sf_op_length_sums": (_I, [_P, _P, _I, _I, _I, _P, _P, _L, _P]),
    "sf_bench_conv1d": (_I, [_I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, C.POINTER(C.c_float)]),
    "sf_op_gn_silu": (_I, [_I, _P, _P, _P, _I, _F, _I, _I, _I, _P, _P, _L, _P]),
    "sf_op_inject_prenorm_proj_workspace_bytes": (_L, [_I, _I, _I, _I, _I]),
    "sf_op_inject_prenorm_proj": (_I, [_I, _P, _P, _P, _P, _P, _P, _F, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _L, _P]),
    # one launch with the whole epilogue: (desc, rowpart_done, gnpart_done, ws, ws_bytes, stream); the queries (desc, label, label_bytes, flags...)
    "sf_op_conv1d_epi_workspace_bytes": (_L, [C.POINTER(Conv1dEpiDesc)]),
    "sf_op_conv1d_epi": (_I, [C.POINTER(Conv1dEpiDesc), C.POINTER(C.c_int), C.POINTER(C.c_int), _P, _L, _P]),
    "sf_op_conv1d_epi_variant": (_I, [C.POINTER(Conv1dEpiDesc), C.c_char_p, _I, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "sf_op_conv1d_ln": (_I, [C.POINTER(Conv1dEpiDesc), C.POINTER(C.c_int), _P, _L, _P]),
    "sf_op_conv1d_ln_variant": (_I, [C.POINTER(Conv1dEpiDesc), C.c_char_p, _I, C.POINTER(C.c_int)]),
    # (dtype, x, w, bias, gn_g, gn_b, groups, eps, tile_stats, B, L, C, h_out, stats_out, nch_out, chunk_rows_out, ws, ws_bytes, stream)
    "sf_op_conv_cb_tiles_workspace_bytes": (_L, [_I, _I, _I, _I]),
    "sf_op_conv_cb_tiles": (_I, [_I, _P, _P, _P, _P, _P, _I, _F, _P, _I, _I, _I, _P, _P, C.POINTER(C.c_int), C.POINTER(C.c_int), _P, _L, _P]),
    "sf_op_resnet_mod_cb_workspace_bytes": (_L, [_I, _I, _I]),
    "sf_op_resnet_mod_cb": (_I, [_I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _F, _P, _F, _I, _I, _I, _I, _P, _P, _P, _L, _P]),
    "sf_op_resnet_mod_cbd_workspace_bytes": (_L, [_I, _I, _I, _I]),
    "sf_op_resnet_mod_cbd": (_I, [_I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _F, _P, _F, _I, _I, _I, _P, _P, _P, _I, _I, _P, _P, _P, _P, _P, _P,
                                  _L, _P]),
    "sf_op_thin_tail_workspace_bytes": (_L, [_I, _I, _I]),
    # (dtype, h, x, ctx, ctx_ld, c2_real, C2, stats_in, nch_in, chunk_in, w2, b2, gn_g, gn_b, groups, eps_gn, scale_shift, eps_ln, w_inj, b_inj,
    #  badd, B, L, C, rw, z_out, stats_out, rw_out, ws, ws_bytes, stream)
    "sf_op_thin_tail": (_I, [_I, _P, _P, _P, _I, _I, _I, _P, _I, _I, _P, _P, _P, _P, _I, _F, _P, _F, _P, _P, _P, _I, _I, _I, _I, _P, _P,
                             C.POINTER(C.c_int), _P, _L, _P]),
    "sf_bench_conv_cb": (_I, [_I, _I, _I, _I, _I, _I, _I, _I, C.POINTER(C.c_float)]),
    "sf_op_ln_modulate": (_I, [_I, _P, _P, _F, _I, _I, _I, _P, _P]),
    "sf_op_attention": (_I, [_I, _P, _P, _I, _I, _I, _I, _P, _P]),
    # the same launchers with the output stride and the pre-split row format (xfmt) exposed
    # (dtype, x, gamma, beta, groups, eps, B, L, C, out, out_ld, xfmt, stream)
    "sf_op_gn_silu_rows": (_I, [_I, _P, _P, _P, _I, _F, _I, _I, _I, _P, _I, _I, _P]),
    # (dtype, x, scale_shift, eps, B, L, C, out, out_ld, xfmt, stream)
    "sf_op_ln_modulate_rows": (_I, [_I, _P, _P, _F, _I, _I, _I, _P, _I, _I, _P]),
    # (dtype, q, ldq, kv, ldkv, B, L, heads, head_dim, out, ldo, xfmt, stream)
    "sf_op_attention_rows": (_I, [_I, _P, _I, _P, _I, _I, _I, _I, _I, _P, _I, _I, _P]),
    # VideoOnsetNet training (fp32, channels-last video rows)
    "sf_op_vconv_workspace_bytes": (_L, [C.POINTER(VConvDesc)]),
    "sf_op_vconv_fwd": (_I, [C.POINTER(VConvDesc), _P, _P, _P, _P, _L, _P]),
    "sf_op_vconv_bwd": (_I, [C.POINTER(VConvDesc), _P, _P, _P, _P, _P, _P, _L, _P]),
    "sf_op_bn_train_workspace_bytes": (_L, [_L, _I]),
    # (x, res, rows, C, ld, gamma, beta, eps, momentum, running_mean, running_var, num_batches_tracked, relu, y, save_mean, save_invstd, ws, ws_bytes, stream)
    "sf_op_bn_train_fwd": (_I, [_P, _P, _L, _I, _I, _P, _P, _F, _F, _P, _P, _P, _I, _P, _P, _P, _P, _L, _P]),
    # (x, y, dy, rows, C, ld, gamma, save_mean, save_invstd, dx, dres, dgamma, dbeta, ws, ws_bytes, stream)
    "sf_op_bn_train_bwd": (_I, [_P, _P, _P, _L, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _L, _P]),
    # the same BatchNorm with cross-rank statistics, in split phases around the caller's all-gather
    "sf_op_bn_sync_workspace_bytes": (_L, [_L, _I]),
    # (x, rows, C, ld, local_stats, ws, ws_bytes, stream)
    "sf_op_bn_sync_stats": (_I, [_P, _L, _I, _I, _P, _P, _L, _P]),
    # (x, res, rows, C, ld, gathered_stats, row_counts, world, gamma, beta, eps, momentum, running_mean, running_var, num_batches_tracked, relu, y,
    #  save_mean, save_invstd, ws, ws_bytes, stream)
    "sf_op_bn_sync_fwd_apply": (_I, [_P, _P, _L, _I, _I, _P, _P, _I, _P, _P, _F, _F, _P, _P, _P, _I, _P, _P, _P, _P, _L, _P]),
    # (x, y, dy, rows, C, ld, save_mean, save_invstd, local_sums, dgamma, dbeta, ws, ws_bytes, stream)
    "sf_op_bn_sync_bwd_sums": (_I, [_P, _P, _P, _L, _I, _I, _P, _P, _P, _P, _P, _P, _L, _P]),
    # (x, y, dy, rows, C, ld, gathered_sums, row_counts, world, gamma, save_mean, save_invstd, dx, dres, ws, ws_bytes, stream)
    "sf_op_bn_sync_bwd_apply": (_I, [_P, _P, _P, _L, _I, _I, _P, _P, _I, _P, _P, _P, _P, _P, _P, _L, _P]),
    "sf_op_video_to_cl": (_I, [_P, _I, _I, _I, _I, _I, _I, _P, _P]),
    "sf_op_video_pool": (_I, [_P, _L, _I, _I, _I, _P, _P]),
    "sf_op_video_pool_bwd": (_I, [_P, _L, _I, _I, _I, _P, _P]),
    # the end of the onset training step: class-balanced BCE, its gradient and the step metrics (syncfusion_amd/onset_loss.py)
    "sf_op_onset_loss_workspace_bytes": (_L, [_L]),
    # (z, t, n, loss, stats, ws, ws_bytes, stream)
    "sf_op_onset_bce_fwd": (_I, [_P, _P, _L, _P, _P, _P, _L, _P]),
    # (z, t, stats, g, n, dz, stream)
    "sf_op_onset_bce_bwd": (_I, [_P, _P, _P, _P, _L, _P, _P]),
    # (z, t, N, T, threshold, out, ws, ws_bytes, stream)
    "sf_op_onset_metrics": (_I, [_P, _P, _I, _I, _F, _P, _P, _L, _P]),
    # the device step of the onset test stage (syncfusion_amd/onset_test.py)
    "sf_op_onset_test_workspace_bytes": (_L, [_I, _I]),
    # (logits, labels, N, T, logit_threshold, metric_threshold, clip0, capacity, pred_count, pred_frames, target_count, target_frames, sums,
    #  ws, ws_bytes, stream)
    "sf_op_onset_test_step": (_I, [_P, _P, _I, _I, _F, _F, _L, _L, _P, _P, _P, _P, _P, _P, _L, _P]),
    # the optimizer stage: clip-by-global-norm + AdamW over one device descriptor table (syncfusion_amd/optim.py)
    "sf_optim_workspace_bytes": (_L, [_I]),
    # (desc_dev, n_tensors, total_chunks, hyper_dev, n_groups, clip, result_dev, ws, ws_bytes, stream)
    "sf_optim_adamw_step": (_I, [_P, _I, _I, _P, _I, _I, _P, _P, _L, _P]),
    # the audio front end of the onset-sync evaluation (syncfusion_amd/audio_features.py)
    # (n_fft, hop, n_mels, pad_mode, first_bin_host, bin_count_host, weights_host, n_weights, out)
    "sf_audio_features_create": (_I, [_I, _I, _I, _I, _P, _P, _P, _L, C.POINTER(_P)]),
    "sf_audio_features_destroy": (None, [_P]),
    "sf_audio_features_workspace_bytes": (_L, [_P, _I, _I]),
    # (h, wav, B, L, amin, top_db, mel_power, db, ws, ws_bytes, stream)
    "sf_logmel_forward": (_I, [_P, _P, _I, _I, _F, _F, _P, _P, _P, _L, _P]),
    # (h, wav, B, L, amin, top_db, lag, pre_max, post_max, pre_avg, post_avg, wait, delta, conf_interval, capacity, envelope, count, positions,
    #  confidence, strength, ws, ws_bytes, stream)
    "sf_onset_detect": (_I, [_P, _P, _I, _I, _F, _F, _I, _I, _I, _I, _I, _I, _F, _I, _I, _P, _P, _P, _P, _P, _P, _L, _P]),
    # the STFT pair and the spectral-gating denoiser (syncfusion_amd/denoise.py)
    # (n_fft, win_length, hop, center, pad_mode, scale_spectrum, freq_taps_host, n_freq_taps, time_taps_host, n_time_taps, out)
    "sf_spectral_gate_create": (_I, [_I, _I, _I, _I, _I, _I, _P, _I, _P, _I, C.POINTER(_P)]),
    "sf_spectral_gate_destroy": (None, [_P]),
    "sf_spectral_gate_frames": (_I, [_P, _I]),
    "sf_spectral_gate_workspace_bytes": (_L, [_P, _I, _I]),
    # (h, wav, B, L, spec, stream)
    "sf_stft_forward": (_I, [_P, _P, _I, _I, _P, _P]),
    # (h, spec, B, T, out, out_len, ws, ws_bytes, stream)
    "sf_istft_forward": (_I, [_P, _P, _I, _I, _P, _I, _P, _L, _P]),
    # (h, noise, B, L, n_std, thresh, ws, ws_bytes, stream)
    "sf_spectral_gate_noise_threshold": (_I, [_P, _P, _I, _I, _F, _P, _P, _L, _P]),
    # (h, wav, B, L, stationary, smooth_b, thresh_mult, slope, prop_decrease, prop_before_smoothing, thresh, spec, mask_raw, mask_smooth, out, ws, ws_bytes, stream)
    "sf_spectral_gate": (_I, [_P, _P, _I, _I, _I, _F, _F, _F, _F, _I, _P, _P, _P, _P, _P, _P, _L, _P]),
    # the FAD evaluation (syncfusion_amd/fad.py)
    # (n_fft, win_length, hop, n_mels, first_bin_host, bin_count_host, weights_host, n_weights, out)
    "sf_audio_features_create_framed": (_I, [_I, _I, _I, _I, _P, _P, _P, _L, C.POINTER(_P)]),
    "sf_logmel_examples_count": (_I, [_P, _I, _I]),
    # (h, wav, B, L, frames_per_example, log_offset, examples, mel, stream)
    "sf_logmel_examples_forward": (_I, [_P, _P, _I, _I, _I, _F, _P, _P, _P]),
    # (n_stages, stages_host, n_fc, fc_widths_host, H, W, final_relu, conv_w, conv_b, fc_w, fc_b, stream, out)
    "sf_vggish_create": (_I, [_I, _P, _I, _P, _I, _I, _I, _P, _P, _P, _P, _P, C.POINTER(_P)]),
    "sf_vggish_destroy": (None, [_P]),
    "sf_vggish_max_examples": (_I, [_P]),
    "sf_vggish_workspace_bytes": (_L, [_P, _I]),
    # (h, examples, n, embeddings, pool_taps, ws, ws_bytes, stream)
    "sf_vggish_forward": (_I, [_P, _P, _I, _P, _P, _P, _L, _P]),
    "sf_op_maxpool2x2_cl": (_I, [_P, _L, _I, _I, _I, _P, _P]),
    "sf_op_moments": (_I, [_P, _L, _I, _P, _P, _P]),
    # the CLAP audio embedder (syncfusion_amd/clap.py)
    # (mel_power, B, n_mels, T, ratio, scale, shift, amin, image, stream)
    "sf_op_logmel_image": (_I, [_P, _I, _I, _I, _I, _P, _P, _F, _P, _P]),
    # (qkv, B, H, W, C, heads, shift, bias_table, mask_value, out, stream)
    "sf_op_window_attention": (_I, [_P, _I, _I, _I, _I, _I, _I, _P, _F, _P, _P]),
    # (cfg, weights, n_weights, stream, out)
    "sf_clap_audio_create": (_I, [C.POINTER(ClapAudioEngineConfig), C.POINTER(SfTensor), _I, _P, C.POINTER(_P)]),
    "sf_clap_audio_destroy": (None, [_P]),
    "sf_clap_audio_max_batch": (_I, [_P]),
    "sf_clap_audio_workspace_bytes": (_L, [_P, _I]),
    # (h, image, B, embedding, taps, ws, ws_bytes, stream)
    "sf_clap_audio_forward": (_I, [_P, _P, _I, _P, _P, _P, _L, _P]),
    # (cfg, B, text_host, capacity)
    "sf_clap_audio_describe": (_I, [C.POINTER(ClapAudioEngineConfig), _I, C.c_char_p, _L]),
    # the CLAP text embedder (syncfusion_amd/clap_text.py)
    # (ids, B, S, C, vocab, n_pos, pad_id, word, pos, type, gamma, beta, eps, out, stream)
    "sf_op_text_embed": (_I, [_P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _F, _P, _P]),
    # (x, rows, C, gamma, beta, eps, y, stream)
    "sf_op_layernorm_affine": (_I, [_P, _L, _I, _P, _P, _F, _P, _P]),
    # (qkv, mask, B, S, heads, out, stream)
    "sf_op_masked_attention": (_I, [_P, _P, _I, _I, _I, _P, _P]),
    # (cfg, weights, n_weights, stream, out)
    "sf_clap_text_create": (_I, [C.POINTER(ClapTextEngineConfig), C.POINTER(SfTensor), _I, _P, C.POINTER(_P)]),
    "sf_clap_text_destroy": (None, [_P]),
    "sf_clap_text_workspace_bytes": (_L, [_P, _I, _I]),
    # (h, ids, mask, B, S, embedding, taps, ws, ws_bytes, stream)
    "sf_clap_text_forward": (_I, [_P, _P, _P, _I, _I, _P, _P, _P, _L, _P]),
    # (cfg, B, S, text_host, capacity)
    "sf_clap_text_describe": (_I, [C.POINTER(ClapTextEngineConfig), _I, _I, C.c_char_p, _L]),
    # JPEG frames on the device (syncfusion_amd/jpeg.py)
    # (bytes_host, offsets_host, N, desc_out, segs_out, seg_capacity, n_segs_out)
    "sf_jpeg_parse": (_I, [_P, _P, _I, _P, _P, _L, C.POINTER(_L)]),
    "sf_jpeg_decode_workspace_bytes": (_L, [_P, _I]),
    # (bytes_dev, n_bytes, desc_host, desc_dev, segs_dev, n_segs, N, H, W, out, status_dev, ws, ws_bytes, stream)
    "sf_jpeg_decode": (_I, [_P, _L, _P, _P, _P, _L, _I, _I, _I, _P, _P, _P, _L, _P]),
}

_lib: Optional[C.CDLL] = None


class SyncFusionAmdError(RuntimeError):
    pass


def load() -> C.CDLL:
    """Load the shared library (once) and declare every prototype.  Raises if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SyncFusionAmdError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C syncfusion_amd/csrc`).  There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError if the header and the library drift apart
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().sf_last_error()
        raise SyncFusionAmdError(f"{what} failed (code {rc}): {msg.decode() if msg else '?'}")


def require_gpu_tensor(t: torch.Tensor, where: str) -> None:
    if not t.is_cuda:
        raise SyncFusionAmdError(f"{where}: expected a tensor on an MI355X (cuda/hip) device, got {t.device}; "
                                 "this build has no CPU execution path")


def stream_ptr(device: torch.device) -> int:
    return int(torch.cuda.current_stream(device).cuda_stream)


def f32c(t: torch.Tensor) -> torch.Tensor:
    return t.detach().to(torch.float32).contiguous()


class TensorTable:
    """Keeps the (name, fp32 contiguous device tensor) pairs alive while the C side reads them."""

    def __init__(self, named: Iterable[Tuple[str, torch.Tensor]], device: torch.device):
        self.keep: List[torch.Tensor] = []
        self.names: List[bytes] = []
        items = list(named)
        self.array = (SfTensor * max(1, len(items)))()
        self.n = len(items)
        for i, (name, t) in enumerate(items):
            tt = f32c(t).to(device)
            self.keep.append(tt)
            self.names.append(name.encode())
            self.array[i].name = self.names[-1]
            self.array[i].data = tt.data_ptr()
            self.array[i].numel = tt.numel()


def ptr_array(tensors: Sequence[torch.Tensor]):
    arr = (C.c_void_p * len(tensors))()
    for i, t in enumerate(tensors):
        arr[i] = t.data_ptr()
    return arr
