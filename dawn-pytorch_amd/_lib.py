"""ctypes binding of libdawn_hip.so (C ABI declared in include/dawn_hip.h).

The library is mandatory: there is NO CPU / eager fallback on the product path.  Import of this module
never fails (so that host-side logic stays testable without a GPU), but :func:`lib` raises loudly when
the shared object is missing or cannot be loaded."""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

_HERE = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ.get("DAWN_HIP_LIB", str(_HERE / "libdawn_hip.so")))

c_f = C.c_void_p          # device pointers travel as void*
_i, _l, _f, _d = C.c_int, C.c_long, C.c_float, C.c_double


class ConvDesc(C.Structure):
    """Mirror of ``dawn_conv_desc`` (include/dawn_hip.h)."""
    _fields_ = [
        ("in0", c_f), ("in1", c_f),
        ("C0", _i), ("C1", _i), ("ld0", _i), ("ld1", _i),
        ("F", _i), ("Hi", _i), ("Wi", _i), ("Ho", _i), ("Wo", _i),
        ("KH", _i), ("KW", _i), ("stride", _i), ("pad", _i),
        ("mode", _i),
        ("w", c_f), ("bias", c_f),
        ("N", _i),
        ("row_mean", c_f), ("row_rstd", c_f),
        ("ch_a", c_f), ("ch_b", c_f),
        ("pro_act", _i),
        ("pro_add", c_f), ("ld_add", _i),
        ("res", c_f), ("ld_res", _i),
        ("tr", c_f), ("ld_tr", _i),
        ("tr_a", c_f), ("tr_b", c_f),
        ("out", c_f), ("ld_out", _i),
        ("gn_part", c_f),
        ("w_bf3", c_f),
        ("gn_rows", C.POINTER(C.c_int)),
        ("policy", _i),
        ("ln_eps", _f),
        ("sk_ws", c_f), ("sk_ws_bytes", C.c_size_t),
        ("w_wino", c_f),
        ("gn_gamma", c_f), ("gn_beta", c_f), ("gn_fs", c_f), ("gn_fsh", c_f),
        ("gn_count", C.c_double), ("gn_eps", _f),
        ("gn_a", c_f), ("gn_b", c_f),
        ("gn_ticket", c_f),
        ("w_wino4", c_f),
        ("border", _i),
    ]


# name -> argtypes (every function returns int; `stream` is the trailing void*)
SIGNATURES = {
    "dawn_conv_gemm": [C.POINTER(ConvDesc), c_f],
    "dawn_conv3x3_form": [C.POINTER(ConvDesc)],
    "dawn_conv3x3_direct_form": [C.POINTER(ConvDesc)],
    "dawn_gemm1x1_form": [C.POINTER(ConvDesc)],
    "dawn_conv_gemm_nblocks": [_l, _i],
    "dawn_conv3x3_wino_ok": [_i, _i, _i, _i, _i, _i],
    "dawn_conv3x3_wino4_ok": [_i, _i, _i, _i, _i, _i],
    "dawn_gn_partial": [c_f, _l, _i, _i, c_f, _i, c_f],
    "dawn_gn_reduce": [c_f, _i, c_f, c_f],
    "dawn_gn_finalize": [c_f, _d, c_f, c_f, c_f, c_f, _i, _f, c_f, c_f, c_f],
    "dawn_gn_reduce_finalize": [c_f, _i, _d, c_f, c_f, c_f, c_f, _i, _f, c_f, c_f, c_f],
    "dawn_gn_ticket_reset": [c_f, c_f],
    "dawn_gn_apply_res": [c_f, c_f, c_f, c_f, c_f, _l, _i, c_f],
    "dawn_ln_rowstats": [c_f, _i, _i, c_f, _i, _i, _l, _f, c_f, c_f, c_f],
    "dawn_ln_rows": [c_f, _i, _i, c_f, _i, _i, _l, _f, c_f, c_f],
    "dawn_xattn_prep": [c_f, _i, c_f, c_f, c_f, _i, c_f, c_f],
    "dawn_xattn_core": [c_f, c_f, _l, _i, c_f, c_f, c_f, c_f],
    "dawn_xattn_ln_sum": [c_f, c_f, c_f, _l, _i, _f, c_f],
    "dawn_xattn_tables": [c_f, c_f, c_f, c_f, c_f, c_f, _i, _i, c_f, c_f],
    "dawn_xattn_sigma_out": [c_f, _l, _i, c_f, c_f, _i, _f, c_f, c_f],
    "dawn_xattn_sigma_out_h1": [c_f, _l, _i, c_f, c_f, _i, _f, c_f, c_f, c_f, c_f, c_f],
    "dawn_xattn_layer_c64": [c_f, _i, _i, c_f, _i, _i, _l, _i, c_f, c_f, c_f, c_f, _f, c_f, c_f],
    "dawn_xattn_layer_c64_h1": [c_f, _i, _i, c_f, _i, _i, _l, _i, c_f, c_f, c_f, c_f, _f, c_f, c_f, c_f, c_f, c_f],
    "dawn_temporal_attn": [c_f, _i, _i, _i, _i, _i, c_f, c_f, c_f, c_f, c_f],
    "dawn_temporal_attn_ex": [c_f, _i, _i, _i, _i, _i, c_f, c_f, c_f, c_f, _i, c_f],
    "dawn_temporal_layer_c64": [c_f, _i, _i, _i, _i, _i, c_f, c_f, c_f, c_f, c_f, c_f, _f, c_f, c_f],
    "dawn_temporal_layer_c64_ex": [c_f, _i, _i, _i, _i, _i, c_f, c_f, c_f, c_f, c_f, c_f, c_f, _f, c_f, _i, c_f],
    "dawn_tl16_schedule": [_i, _i, _i, _i, c_f, c_f],
    "dawn_tl13_schedule": [_i, _i, _i, _i, c_f],
    "dawn_sla_context": [c_f, _i, _i, c_f, c_f],
    "dawn_sla_apply": [c_f, c_f, _i, _i, c_f, c_f],
    "dawn_sla_ws_floats": [_i, _i, _i],
    "dawn_gemm1x1_split_ok": [_l, _i, _i, _i],
    "dawn_gemm1x1_ln_inline_ok": [_l, _i, _i, _i],
    "dawn_sla_layer_c64": [c_f, _i, _i, c_f, c_f, c_f, c_f, _f, c_f, c_f, c_f],
    "dawn_frame_attn": [c_f, _i, _i, c_f, c_f],
    "dawn_init_conv_x": [c_f, c_f, c_f, _i, _i, _i, _i, c_f, c_f],
    "dawn_init_conv_x_ex": [c_f, _l, c_f, c_f, _i, _i, _i, _i, c_f, c_f],
    "dawn_head_out": [c_f, c_f, c_f, c_f, c_f, c_f, _l, _i, c_f, c_f],
    "dawn_heads_eps": [c_f, c_f, c_f, c_f, c_f, c_f, c_f, _i, _i, c_f, _i, _i, c_f, c_f, c_f, c_f, _l, _i, c_f, c_f],
    "dawn_fold_heads": [c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, _i, _i, c_f, c_f],      # (host pointers)
    "dawn_linear": [c_f, _i, _i, _i, c_f, c_f, _i, _i, c_f, _i, c_f],
    "dawn_sinusoidal": [_f, _i, c_f, c_f, c_f],
    "dawn_ddim_x0": [c_f, c_f, _f, _f, _l, c_f, c_f, c_f],
    "dawn_select_scan": [c_f, _i, C.c_ulonglong, c_f, _i, c_f],
    "dawn_select_hist": [c_f, _l, c_f, _i, c_f, c_f],
    "dawn_select_finalize": [c_f, c_f, _f, c_f, c_f],
    "dawn_select_ws_reset": [c_f, c_f],
    "dawn_attn_bias32": [c_f, _i, c_f, _i, c_f, _i, _i, _i, _i, c_f, c_f, c_f, _i, _f, c_f, _i, c_f],
    "dawn_attn_win32": [c_f, _i, c_f, _i, c_f, _i, _i, _i, _i, _i, c_f, c_f, c_f, _i, _f, c_f, _i, c_f],
    "dawn_ubench_mfma_bf16": [_i, _i, c_f, c_f, C.POINTER(C.c_float), c_f],
    "dawn_ddim_update": [c_f, c_f, c_f, c_f, _f, _f, _f, _l, c_f, c_f],
    "dawn_cfg_combine": [c_f, c_f, _f, _l, c_f, c_f],
    "dawn_cfg_x0": [c_f, c_f, _f, c_f, _f, _f, _l, c_f, c_f, c_f, c_f],
    # guided whole-path entries (include/dawn_hip.h; the dawn_shard_comm* travels as a void*)
    "dawn_workspace_bytes_guided": [c_f, _i, _i, _i, _i, _i],
    "dawn_unet_forward_guided": [c_f, _i, _i, _i, c_f, c_f, c_f, _f, _f, c_f, c_f, C.c_size_t, c_f, c_f],
    "dawn_sampler_run_guided": [c_f, _i, _i, _i, c_f, c_f, _f, c_f, _i, c_f, C.c_uint64, c_f, c_f, c_f, c_f, C.c_size_t, c_f, c_f],
    # ancestral (DDPM) sampling: step kernel and the whole-path entry (single / guided / sharded in one)
    "dawn_ancestral_update": [c_f, c_f, c_f, c_f, _f, _f, _f, _l, c_f, c_f],
    "dawn_sampler_run_ancestral": [c_f, _i, _i, _i, c_f, c_f, _f, c_f, _i, c_f, C.c_uint64, c_f, c_f, c_f, c_f, C.c_size_t, c_f, c_f],
    # x0 clipping modes: the fused step tails of the modes without a quantile, and the whole-path entries that take a dawn_clip_mode*
    "dawn_ddim_step_fixed": [c_f, c_f, c_f, _f, _f, _f, _f, _f, _i, _l, c_f, c_f, c_f],
    "dawn_ancestral_step_fixed": [c_f, c_f, c_f, _f, _f, _f, _f, _f, _i, _l, c_f, c_f, c_f],
    "dawn_sampler_run_clip": [c_f, _i, _i, _i, c_f, c_f, _f, c_f, _i, c_f, C.c_uint64, c_f, c_f, c_f, c_f, C.c_size_t, c_f, c_f, c_f],
    "dawn_sampler_run_ancestral_clip": [c_f, _i, _i, _i, c_f, c_f, _f, c_f, _i, c_f, C.c_uint64, c_f, c_f, c_f, c_f, C.c_size_t, c_f, c_f,
                                        c_f],
    # DPM-Solver++(2M): the two step tails and the whole-path entry (single / guided / sharded, any clipping mode, in one)
    "dawn_dpmpp_update": [c_f, c_f, c_f, c_f, _f, _f, _f, _l, c_f, c_f, c_f],
    "dawn_dpmpp_step_fixed": [c_f, c_f, c_f, _f, _f, _f, _f, _f, _i, _l, c_f, c_f, c_f],
    "dawn_sampler_run_dpmpp": [c_f, _i, _i, _i, c_f, c_f, _f, c_f, _i, c_f, c_f, c_f, c_f, C.c_size_t, c_f, c_f, c_f],
    "dawn_philox_normal": [c_f, _i, _i, _i, _i, _i, C.c_uint64, C.c_uint32, c_f],
    "dawn_affine_act": [c_f, _i, c_f, c_f, _i, c_f, _l, _i, c_f],
    "dawn_bn_relu_pool2": [c_f, c_f, c_f, c_f, _i, _i, _i, _i, c_f],
    "dawn_warp_blend": [c_f, _i, _i, _i, c_f, _l, c_f, _i, _i, _i, c_f, c_f, c_f, _i, c_f, c_f],
    "dawn_final_conv_blend": [c_f, _i, _i, _i, _i, c_f, c_f, c_f, c_f, _l, c_f, _i, _i, c_f, c_f, _l, c_f],
    "dawn_frames_to_u8": [c_f, _l, _l, _d, _d, _d, _i, c_f, c_f],
    "dawn_final_conv_blend_u8": [c_f, _i, _i, _i, _i, c_f, c_f, c_f, c_f, _l, c_f, _i, _i, _d, _d, _d, _i, c_f, c_f],
    "dawn_frames_to_yuv420": [c_f, _l, _i, _i, _i, _d, _d, _d, c_f, c_f],
    "dawn_final_conv_blend_yuv420": [c_f, _i, _i, _i, _i, c_f, c_f, c_f, c_f, _l, c_f, _i, _i, _d, _d, _d, c_f, c_f],
    # whole-path flow decode (csrc/dawn_decoder.hip; handles, the cfg struct and the named-pointer table travel as void*: ctx.py)
    "dawn_decoder_create": [c_f, c_f, _i, c_f],
    "dawn_decoder_destroy": [c_f],
    "dawn_decoder_skip_bytes": [c_f, _i, _i],
    "dawn_decoder_workspace_bytes": [c_f, _i, _i, _i],
    "dawn_decoder_encode": [c_f, _i, _i, c_f, c_f, C.c_size_t, c_f, c_f, C.c_size_t, c_f],
    "dawn_decode_clip": [c_f, _i, _i, _i, _i, _i, c_f, c_f, c_f, _l, _i, c_f, c_f, _l, c_f, C.POINTER(C.c_double), _i, c_f, C.c_size_t,
                         c_f],
    "dawn_decode_clip_conf": [c_f, _i, _i, _i, _i, _i, c_f, c_f, c_f, _l, c_f, _i, c_f, c_f, _l, c_f, C.POINTER(C.c_double), _i, c_f,
                              C.c_size_t, c_f],
    "dawn_decode_clip_yuv420": [c_f, _i, _i, _i, _i, _i, c_f, c_f, c_f, _l, _i, c_f, C.POINTER(C.c_double), c_f, C.c_size_t, c_f],
    "dawn_decode_clip_conf_yuv420": [c_f, _i, _i, _i, _i, _i, c_f, c_f, c_f, _l, c_f, _i, c_f, C.POINTER(C.c_double), c_f, C.c_size_t,
                                     c_f],
    "dawn_wave_normalize": [c_f, _l, c_f, c_f, c_f],
    "dawn_hubert_conv0": [c_f, _l, c_f, c_f, _i, _i, _i, c_f, c_f],
    "dawn_ln_affine_act": [c_f, _l, _i, c_f, c_f, _f, _i, c_f, c_f],
    "dawn_add_act": [c_f, c_f, _i, _l, c_f, c_f],
    "dawn_attn64": [c_f, _i, _i, c_f, c_f],
    "dawn_interp_linear": [c_f, _l, _i, c_f, _l, c_f, c_f],
    "dawn_hubert_pos_conv": [c_f, _i, _i, _i, _i, c_f, c_f, c_f, c_f],
    # whole-path HuBERT stage (csrc/dawn_hubert.hip; the handle, the cfg struct and the named-pointer table travel as void*: ctx.py)
    "dawn_hubert_create": [c_f, c_f, _i, c_f],
    "dawn_hubert_destroy": [c_f],
    "dawn_hubert_conv_frames": [c_f, _l],
    "dawn_hubert_segments": [c_f, _l, C.POINTER(C.c_long), _i, C.POINTER(C.c_long), C.POINTER(C.c_long)],
    "dawn_hubert_workspace_bytes": [c_f, _l],
    "dawn_hubert_encode": [c_f, c_f, _l, c_f, c_f, C.c_size_t, c_f],
    "dawn_hubert_features": [c_f, c_f, _l, c_f, c_f, c_f, C.c_size_t, c_f],
    # whole-path PBnet pose / blink stage (csrc/dawn_pbnet.hip; handles, the cfg struct and the named-pointer table travel as void*: ctx.py)
    "dawn_pbnet_create": [c_f, c_f, _i, c_f],
    "dawn_pbnet_destroy": [c_f],
    "dawn_pbnet_workspace_bytes": [c_f, _l],
    "dawn_pbnet_generate": [c_f, c_f, c_f, _i, c_f, _l, c_f, _i, c_f, C.c_size_t, c_f],
    "dawn_pose_blink_workspace_bytes": [c_f, c_f, _l],
    "dawn_pose_blink_stage": [c_f, c_f, c_f, _i, _l, C.POINTER(C.c_float), C.POINTER(C.c_float), c_f, c_f, c_f, _i, c_f, _i, c_f,
                              C.c_size_t, c_f],
    # clip inputs (csrc/clip_inputs.hip: bbox6 / init_pose / init_eye are HOST floats), their stage host and the one-call pipeline
    # (csrc/dawn_inputs.hip; the handle, the cfg / args structs and the named-pointer table travel as void*: ctx.py)
    "dawn_face_loc_embed": [C.POINTER(C.c_float), _i, c_f, c_f, c_f, c_f, c_f, _l, c_f],
    "dawn_bbox_mask_bounds": [C.POINTER(C.c_float), _i, C.POINTER(C.c_int)],
    "dawn_cond_rows": [c_f, _i, _i, c_f, _i, _i, c_f, _i, C.POINTER(C.c_float), _i, C.POINTER(C.c_float), _l, c_f, _i, c_f],
    "dawn_inputs_create": [c_f, c_f, _i, c_f],
    "dawn_inputs_destroy": [c_f],
    "dawn_clip_inputs": [c_f, C.POINTER(C.c_float), _i, c_f, _i, c_f, _i, c_f, _i, _i, c_f, _i, C.POINTER(C.c_float), _i,
                         C.POINTER(C.c_float), _l, c_f, _i, c_f],
    "dawn_generate_bytes": [c_f, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)],
    "dawn_generate_clip": [c_f, c_f, C.c_size_t, c_f],
    # media ingest (csrc/media_ingest.hip) and the pipeline from decoded media (csrc/dawn_inputs.hip; the args struct travels as void*: ctx.py)
    "dawn_image_ingest_workspace_bytes": [_i, _i, _i, _i],
    "dawn_image_ingest": [c_f, _i, _i, _l, _i, _i, _i, _i, c_f, _l, c_f, C.c_size_t, c_f],
    "dawn_pcm16_to_samples": [c_f, _l, _i, c_f, c_f],
    "dawn_generate_media_bytes": [c_f, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)],
    "dawn_generate_clip_media": [c_f, c_f, C.c_size_t, c_f],
    # audio at any sample rate (csrc/audio_resample.hip) and the pipeline from PCM at that rate (csrc/dawn_inputs.hip)
    "dawn_resample16k_len": [_l, _i],
    "dawn_resample16k_workspace_bytes": [_i],
    "dawn_resample16k_pcm16": [c_f, _l, _i, _i, c_f, _l, c_f, C.c_size_t, c_f],
    "dawn_resample16k_f32": [c_f, _l, _i, c_f, _l, c_f, C.c_size_t, c_f],
    "dawn_generate_media_rate_bytes": [c_f, _i, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)],
    "dawn_generate_clip_media_rate": [c_f, _i, c_f, C.c_size_t, c_f],
    # LFG motion encode (csrc/motion_encode.hip): driving video -> flow / occlusion latent (motion_encoder.py)
    "dawn_antialias_down": [c_f, _i, _l, _l, _i, _i, _i, _i, c_f, _i, _i, c_f],
    "dawn_region_moments": [c_f, _i, _i, _i, _i, _i, _d, c_f, c_f, c_f, c_f],
    "dawn_bg_params": [c_f, _i, _i, _i, _i, c_f, c_f, c_f, c_f],
    "dawn_motion_inputs": [c_f, c_f, c_f, c_f, c_f, c_f, c_f, _i, c_f, _i, _i, _i, _i, c_f, _i, _i, c_f],
    "dawn_flow_combine": [c_f, _i, c_f, c_f, c_f, c_f, c_f, _i, _i, _i, _i, c_f, _l, c_f, _i, c_f],
    # model bundle (csrc/dawn_bundle.hip; the handle, the table / blob out-pointers and the dawn_generate_args travel as void*: bundle.py, ctx.py)
    "dawn_bundle_open": [C.c_char_p, c_f],
    "dawn_bundle_close": [c_f],
    "dawn_bundle_device_bytes": [c_f],
    "dawn_bundle_verify_workspace_bytes": [c_f],
    "dawn_bundle_upload": [c_f, c_f, C.c_size_t, c_f],
    "dawn_bundle_verify": [c_f, c_f, C.c_size_t, c_f, C.c_size_t, c_f],
    "dawn_bundle_table": [c_f, _i, c_f, c_f, C.POINTER(C.c_int)],
    "dawn_bundle_cfg": [c_f, _i, c_f, C.c_size_t],
    "dawn_bundle_host": [c_f, C.c_char_p, c_f, C.POINTER(C.c_size_t)],
    "dawn_bundle_create_handles": [c_f, c_f, c_f],
    "dawn_bundle_destroy_handles": [c_f],
    "dawn_bundle_create_motion": [c_f, c_f, c_f],
    # yuv420p ingest (csrc/yuv_ingest.hip) and the C-side motion-encode stage (csrc/dawn_motion.hip; handle, cfg and args structs as void*: ctx.py)
    "dawn_yuv420_to_frames": [c_f, _l, _i, _i, _i, c_f, c_f],
    "dawn_motion_create": [c_f, c_f, _i, c_f],
    "dawn_motion_destroy": [c_f],
    "dawn_motion_workspace_bytes": [c_f, _i, _i, _i],
    "dawn_motion_encode_clip": [c_f, _i, _i, _i, c_f, _i, c_f, _i, _l, _l, _i, c_f, _l, c_f, _i, c_f, C.c_size_t, c_f],
    "dawn_reenact_bytes": [c_f, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)],
    "dawn_reenact_clip": [c_f, c_f, C.c_size_t, c_f],
}
# device helpers of the C-side evaluator (csrc/dawn_ctx.hip calls them; from Python only the op tests do)
CTX_HELPER_SIGNATURES = {
    "dawn_chw_to_hwc": [c_f, _i, _l, c_f, c_f],
    "dawn_rotary_tables": [c_f, _i, _i, c_f, c_f, c_f],
}
# whole-path UNet entries (csrc/dawn_ctx.hip; the handle, the cfg / step / dawn_shard_comm structs and the tables travel as void*: ctx.py)
_fwd = [c_f, _i, _i, _i, c_f, c_f, _f, c_f, c_f, C.c_size_t]                               # ctx, F, h, w, clip, x3, t, eps, workspace, bytes
_run = [c_f, _i, _i, _i, c_f, c_f, _i, c_f, C.c_uint64, c_f, c_f, c_f, c_f, C.c_size_t]   # .. clip, x_init, S, steps, seed, noises, x_out, thr, ..
CTX_SIGNATURES = {
    "dawn_ctx_create": [c_f, c_f, _i, c_f],
    "dawn_ctx_destroy": [c_f],
    "dawn_ctx_set_option": [c_f, _i, _i],
    "dawn_clip_bytes": [c_f, _i, _i, _i],
    "dawn_workspace_bytes": [c_f, _i, _i, _i],
    "dawn_workspace_bytes_sharded": [c_f, _i, _i, _i, _i, _i],
    "dawn_clip_prepare": [c_f, _i, _i, _i, c_f, c_f, _i, c_f, c_f, c_f, C.c_size_t, c_f, C.c_size_t, c_f],
    "dawn_unet_forward": _fwd + [c_f],
    "dawn_unet_forward_sharded": _fwd + [c_f, c_f],
    "dawn_sampler_run": _run + [c_f],
    "dawn_sampler_run_sharded": _run + [c_f, c_f],
    "dawn_ctx_profile_read": [c_f, c_f, _i],
    "dawn_rel_pos_bucket": [_i],
}

_lib = None


class DawnHipError(RuntimeError):
    pass


LONG_RESULT = {"dawn_sla_ws_floats", "dawn_workspace_bytes_guided", "dawn_decoder_skip_bytes", "dawn_decoder_workspace_bytes",
               "dawn_hubert_conv_frames", "dawn_hubert_workspace_bytes", "dawn_pbnet_workspace_bytes",
               "dawn_pose_blink_workspace_bytes", "dawn_clip_bytes", "dawn_workspace_bytes",
               "dawn_workspace_bytes_sharded", "dawn_image_ingest_workspace_bytes", "dawn_resample16k_len",
               "dawn_resample16k_workspace_bytes", "dawn_bundle_device_bytes",
               "dawn_bundle_verify_workspace_bytes", "dawn_motion_workspace_bytes"}      # entry points that return a size (long), not a status


def lib() -> C.CDLL:
    """Load libdawn_hip.so once; raise (never fall back) if it is absent."""
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise DawnHipError(
                f"{LIB_PATH} not found: the HIP extension is mandatory (no CPU fallback). "
                "Build it with `python -c 'import __graft_entry__ as g; g.build()'` or ./build_lib.sh")
        L = C.CDLL(str(LIB_PATH))
        L.dawn_last_error.restype = C.c_char_p
        L.dawn_abi_version.restype = _i
        for name, args in {**SIGNATURES, **CTX_HELPER_SIGNATURES, **CTX_SIGNATURES}.items():
            fn = getattr(L, name)
            fn.argtypes = args
            fn.restype = _l if name in LONG_RESULT else _i
        _lib = L
    return _lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise DawnHipError(f"{what} failed with code {rc}: {lib().dawn_last_error().decode()}")
