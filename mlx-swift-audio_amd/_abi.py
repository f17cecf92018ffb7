"""ctypes prototypes and struct mirrors of include/mia.h: the only place they are written down.

`PROTOTYPES` has one entry per function of the header and `STRUCTS` one class per `typedef struct { ... } mia_x;`.  Both are plain
literals; tests/test_abi_table.py parses the header and checks every name, argument, return type, field and array length against them.
`apply(lib)` installs the table on a loaded library, and `_lib.load()` calls it once.

One behaviour follows from binding everything at load: a libmia.so that lacks a symbol of the table (a stale build) fails in
`_lib.load()` with an ImportError naming the symbol, not at the first use of the missing function.

Type rule: `int` / `int32_t` -> c_int, `int64_t` -> c_int64, `float` -> c_float, `double` -> c_double, `const char*` -> c_char_p,
`void` -> None.  Pointers to data and opaque handles are c_void_p, as arguments and as return values (a NumPy `.ctypes.data`, a
tensor's `data_ptr()`, `byref(...)` and None all pass); a pointer to one of the structs below is POINTER(ThatStruct) or c_void_p.

`tensor_views` builds the `mia_tensor_view` array of every load and attach call, and `dtype_tag` is the one rule for the dtype a NumPy
array is handed over as.

Adding an entry point:
  1. declare it in include/mia.h (and a struct it takes as a `typedef struct { ... } mia_x;`);
  2. add its line to PROTOTYPES (and the struct's class to this file and to STRUCTS);
  3. call `lib.mia_x(...)` -- nothing else declares anything.
"""
from __future__ import annotations

import ctypes as C

vp, cs, i32, i64, f32, f64, P = C.c_void_p, C.c_char_p, C.c_int, C.c_int64, C.c_float, C.c_double, C.POINTER


class ConvGemmDesc(C.Structure):
    _fields_ = [("X", vp), ("ldx", i64), ("T_in", i32),
                ("W", vp), ("ldw", i64), ("w_phase_stride", i64),
                ("bias", vp), ("alpha", vp), ("ralpha", vp), ("lrelu_slope", f32),
                ("Y", vp), ("ldy", i64), ("T_out", i32),
                ("y_row_mul", i32), ("y_row_off", i32), ("y_phase_step", i32),
                ("R", vp), ("R2", vp), ("ldr", i64), ("noise", vp), ("out_scale", f32),
                ("M", i32), ("N", i32), ("Cin", i32), ("taps", i32), ("dil", i32), ("pad", i32),
                ("x_row_mul", i32), ("act", i32), ("tanh_out", i32),
                ("phase_len", vp), ("x_phase_step", i32),
                ("n_seq", i32), ("x_seq_step", i64), ("y_seq_step", i64),
                ("seq_len", vp), ("noise_seq_off", vp)]


class SkinnyDesc(C.Structure):
    _fields_ = [("A", vp), ("lda", i64), ("W", vp),
                ("wfrag", vp), ("stfrag", vp), ("bits", i32), ("w_frag", i32),
                ("bias", vp), ("out", vp), ("ldo", i64),
                ("M", i32), ("N", i32), ("K", i32), ("S", i32), ("mode", i32), ("dtype", i32),
                ("xres", vp), ("nw", vp), ("ss_out", vp),
                ("ss_in", vp), ("ss_tiles", i32), ("ss_dim", i32), ("eps", f32), ("rs_scale", f32),
                ("M_cap", i32)]


class GemmQuantDesc(C.Structure):
    """struct mia_gemm_quant_desc of include/mia_gemm_quant.h (mia.h only declares the type, so it is not in STRUCTS)."""
    _fields_ = [("A", vp), ("lda", i64),
                ("wfrag", vp), ("stfrag", vp), ("bits", i32),
                ("C", vp), ("ldc", i64), ("R", vp), ("ldr", i64),
                ("M", i32), ("N", i32), ("K", i32), ("dtype", i32)]


class KokoroConfig(C.Structure):
    """struct mia_kokoro_config of include/mia_kokoro.h (mia.h only declares the type, so it is not in STRUCTS)."""
    _fields_ = [("dim_in", i32), ("style_dim", i32), ("hidden", i32), ("asr_res_dim", i32), ("pred_dim", i32),
                ("up_initial", i32), ("n_ups", i32), ("up_rates", i32 * 4), ("up_kernels", i32 * 4),
                ("n_res_kernels", i32), ("res_kernels", i32 * 4), ("n_dilations", i32), ("dilations", i32 * 4),
                ("n_fft", i32), ("hop", i32), ("n_harmonics", i32), ("voiced_threshold", i32), ("sample_rate", i32)]


class WhisperDims(C.Structure):
    _fields_ = [("n_mels", i32), ("n_audio_ctx", i32), ("n_audio_state", i32), ("n_audio_head", i32), ("n_audio_layer", i32),
                ("n_vocab", i32), ("n_text_ctx", i32), ("n_text_state", i32), ("n_text_head", i32), ("n_text_layer", i32)]


class TensorView(C.Structure):
    _fields_ = [("name", cs), ("dtype", i32), ("ndim", i32), ("shape", i64 * 4), ("data", vp)]


F32, F16, BF16, U32 = 0, 1, 2, 3          # mia_dtype


def dtype_tag(a):
    """The mia_dtype a NumPy array is handed over as, or None when it has none: float32 -> F32, float16 -> F16, uint32 -> U32 (packed
    quantisation codes), uint16 -> BF16.  NumPy has no bfloat16, so a uint16 array IS a bf16 payload here: tagged `.st_dtype == "BF16"`
    (checkpoint.read_safetensors) or untagged; only a uint16 array tagged as something else (a "U16" tensor of a file) has no tag."""
    import numpy as np
    if a.dtype == np.uint16:
        return BF16 if getattr(a, "st_dtype", "BF16") == "BF16" else None
    return {np.dtype(np.float32): F32, np.dtype(np.float16): F16, np.dtype(np.uint32): U32}.get(a.dtype)


def tensor_views(tensors, kinds=(F32,), refuse=None):
    """name -> array dict to the `mia_tensor_view` array every load / attach call takes: (views, count, keep_alive).

    An array whose dtype_tag is in `kinds` is passed as it is (made contiguous).  Any other is converted to contiguous float32 -- the
    dense loads; the fp32-only models pass kinds=(F32,) and so force float32 -- or, with `refuse` (a format of {name} and {dtype}),
    is an INVALID_ARGUMENT MiaError with that text -- the packed tensors of an attach.  Shapes are padded with zeros to four entries.
    `keep_alive` holds the arrays the views point into: keep it until the call has returned."""
    import numpy as np
    from . import _lib
    views = (TensorView * max(len(tensors), 1))()
    keep = []
    for i, (name, arr) in enumerate(tensors.items()):
        tag = dtype_tag(arr)
        if tag in kinds:
            a = np.ascontiguousarray(arr)
        elif refuse is None:
            a, tag = np.ascontiguousarray(arr, np.float32), F32
        else:
            raise _lib.MiaError(_lib.ERR_INVALID_ARGUMENT, refuse.format(name=name, dtype=arr.dtype))
        keep.append(a)
        views[i] = TensorView(name.encode(), tag, a.ndim, (i64 * 4)(*(list(a.shape) + [0] * (4 - a.ndim))), a.ctypes.data)
    return views, len(tensors), keep


class DecodeOpts(C.Structure):
    _fields_ = [("initial_tokens", vp), ("n_initial", i32), ("per_clip_initial", i32), ("sot_index", i32),
                ("suppress_ids", vp), ("n_suppress", i32), ("blank_ids", vp), ("n_blank", i32),
                ("eot", i32), ("no_speech", i32), ("no_timestamps", i32), ("timestamp_begin", i32),
                ("timestamps", i32), ("max_tokens", i32), ("max_initial_timestamp_index", i32), ("max_new_tokens", i32),
                ("temperature", f32), ("uniforms", vp),
                ("n_initial_per_clip", vp), ("sot_index_per_clip", vp), ("clip_temperature", vp), ("clip_active", vp)]


class SnacConfig(C.Structure):
    _fields_ = [("latent_dim", i32), ("decoder_dim", i32), ("n_rates", i32), ("decoder_rates", i32 * 8),
                ("n_vq", i32), ("vq_strides", i32 * 4), ("codebook_size", i32), ("codebook_dim", i32),
                ("noise", i32), ("depthwise", i32)]


class DacConfig(C.Structure):
    _fields_ = [("latent_dim", i32), ("decoder_dim", i32), ("n_rates", i32), ("decoder_rates", i32 * 8),
                ("n_codebooks", i32), ("codebook_size", i32), ("codebook_dim", i32)]


class DacEncoderConfig(C.Structure):
    _fields_ = [("encoder_dim", i32), ("n_rates", i32), ("encoder_rates", i32 * 8)]


class MimiConfig(C.Structure):
    """struct mia_mimi_config of include/mia_mimi.h (mia.h only declares the type, so it is not in STRUCTS)."""
    _fields_ = [("sample_rate", i32), ("upsample_stride", i32), ("nq", i32), ("bins", i32), ("quantizer_dim", i32),
                ("seanet_dimension", i32), ("seanet_nfilters", i32), ("seanet_n_ratios", i32), ("seanet_ratios", i32 * 8),
                ("seanet_ksize", i32), ("seanet_residual_ksize", i32), ("seanet_last_ksize", i32), ("seanet_n_residual_layers", i32),
                ("seanet_dilation_base", i32), ("seanet_compress", i32),
                ("seanet_causal", i32), ("seanet_true_skip", i32), ("seanet_pad_constant", i32),
                ("d_model", i32), ("n_heads", i32), ("n_layers", i32), ("dim_feedforward", i32), ("context", i32), ("kv_repeat", i32),
                ("gating", i32), ("layer_norm", i32), ("layer_scale", i32), ("rope", i32), ("max_period", i32)]


class MarvisConfig(C.Structure):
    """struct mia_marvis_config of include/mia_marvis.h (mia.h only declares the type, so it is not in STRUCTS)."""
    _fields_ = [("text_vocab", i32), ("audio_vocab", i32), ("n_codebooks", i32), ("max_ctx", i32),
                ("bb_hidden", i32), ("bb_inter", i32), ("bb_layers", i32), ("bb_heads", i32), ("bb_kv_heads", i32), ("bb_head_dim", i32),
                ("dec_hidden", i32), ("dec_inter", i32), ("dec_layers", i32), ("dec_heads", i32), ("dec_kv_heads", i32), ("dec_head_dim", i32),
                ("bb_rms_eps", f32), ("dec_rms_eps", f32), ("bb_rope_theta", f32), ("dec_rope_theta", f32),
                ("rope_llama3", i32), ("rope_factor", f32), ("rope_low", f32), ("rope_high", f32), ("rope_old_ctx", f32),
                ("attention_bias", i32), ("mlp_bias", i32)]


class LmConfig(C.Structure):
    _fields_ = [("vocab", i32), ("hidden", i32), ("inter", i32), ("n_layers", i32), ("n_heads", i32), ("n_kv_heads", i32),
                ("head_dim", i32), ("max_ctx", i32),
                ("rms_eps", f32), ("rope_theta", f32), ("rope_llama3", i32),
                ("rope_factor", f32), ("rope_low", f32), ("rope_high", f32), ("rope_old_ctx", i32),
                ("qkv_bias", i32), ("tie_embeddings", i32)]


class LmSampler(C.Structure):
    _fields_ = [("temperature", f32), ("top_p", f32), ("rep_penalty", f32), ("rep_window", i32), ("max_new_tokens", i32),
                ("n_stop", i32), ("stop_ids", i32 * 4), ("reserved", i32)]


class RasParams(C.Structure):
    _fields_ = [("top_p", f32), ("top_k", i32), ("win", i32), ("tau", f32), ("eos", i32), ("min_len", i32), ("max_len", i32)]


class SensevoiceConfig(C.Structure):
    _fields_ = [("input_dim", i32), ("encoder_dim", i32), ("n_heads", i32), ("ffn_dim", i32), ("kernel_size", i32),
                ("sanm_shift", i32), ("n_encoders0", i32), ("n_encoders", i32), ("n_tp_encoders", i32),
                ("adaptor_k", i32), ("llm_dim", i32), ("adaptor_ffn_dim", i32), ("adaptor_layers", i32), ("adaptor_heads", i32)]


class S3Config(C.Structure):
    _fields_ = [("n_mels", i32), ("n_audio_state", i32), ("n_audio_head", i32), ("n_audio_layer", i32)]


class HiftConfig(C.Structure):
    _fields_ = [("in_channels", i32), ("base_channels", i32), ("nb_harmonics", i32), ("sampling_rate", i32),
                ("n_ups", i32), ("up_rates", i32 * 4), ("up_kernels", i32 * 4),
                ("n_res_kernels", i32), ("res_kernels", i32 * 4), ("src_res_kernels", i32 * 4),
                ("n_dilations", i32), ("dilations", i32 * 4),
                ("nsf_alpha", f32), ("nsf_sigma", f32), ("voiced_threshold", f32), ("lrelu_slope", f32), ("audio_limit", f32)]


class FlowConfig(C.Structure):
    _fields_ = [("input_size", i32), ("output_size", i32), ("spk_embed_dim", i32), ("vocab_size", i32),
                ("pre_lookahead_len", i32), ("n_timesteps", i32),
                ("enc_heads", i32), ("enc_linear_units", i32), ("enc_blocks", i32), ("enc_up_blocks", i32), ("upsample_stride", i32),
                ("dec_in_channels", i32), ("dec_channels", i32), ("dec_heads", i32), ("dec_n_blocks", i32), ("dec_mid_blocks", i32),
                ("cfg_rate", f32)]


STRUCTS = {
    "mia_conv_gemm_desc": ConvGemmDesc,
    "mia_skinny_desc": SkinnyDesc,
    "mia_whisper_dims": WhisperDims,
    "mia_tensor_view": TensorView,
    "mia_decode_opts": DecodeOpts,
    "mia_snac_config": SnacConfig,
    "mia_dac_config": DacConfig,
    "mia_dac_encoder_config": DacEncoderConfig,
    "mia_lm_config": LmConfig,
    "mia_lm_sampler": LmSampler,
    "mia_ras_params": RasParams,
    "mia_sensevoice_config": SensevoiceConfig,
    "mia_s3_config": S3Config,
    "mia_hift_config": HiftConfig,
    "mia_flow_config": FlowConfig,
}

TV = P(TensorView)

# name: (restype, [argtypes]) in the order of include/mia.h
PROTOTYPES = {
    # context
    "mia_version": (cs, []),
    "mia_create": (vp, [i32]),
    "mia_create_on_stream": (vp, [i32, vp]),
    "mia_destroy": (None, [vp]),
    "mia_last_error": (cs, [vp]),
    "mia_stream": (vp, [vp]),
    "mia_synchronize": (i32, [vp]),
    # profiling
    "mia_profile_enable": (i32, [vp, i32]),
    "mia_profile_reset": (i32, [vp]),
    "mia_profile_read": (i32, [vp, cs, vp, vp, vp]),
    "mia_profile_codec_bytes": (f64, [i32]),
    # DSP front end
    "mia_logmel_whisper": (i32, [vp, vp, vp, i32, i32, i64, i64, vp, i32, i32]),
    "mia_logmel_s3": (i32, [vp, vp, vp, i32, i32, i64, i64, vp, i32, i32]),
    "mia_mel_s3gen_frames": (i64, [i64]),
    "mia_mel_s3gen": (i32, [vp, vp, i64, vp, i32]),
    "mia_resample_linear_len": (i64, [i64, f32]),
    "mia_resample_linear": (i32, [vp, vp, i64, f32, vp, i32]),
    "mia_resample_sinc_len": (i64, [i64, i32, i32]),
    "mia_resample_sinc_table": (i32, [i32, i32, vp, i32, vp, vp]),
    "mia_resample_sinc": (i32, [vp, vp, i64, i32, i32, vp, i64, vp, i32]),
    # data-parallel exchange
    "mia_dp_shard_range": (i32, [i32, i32, i32, vp, vp]),
    "mia_dp_shard_cap": (i32, [i32, i32]),
    "mia_dp_unpack_host": (i32, [vp, i32, i32, i32, vp]),
    "mia_dp_available": (i32, []),
    "mia_dp_unique_id": (i32, [vp, vp]),
    "mia_dp_init": (i32, [vp, i32, i32, vp]),
    "mia_dp_shutdown": (i32, [vp]),
    "mia_dp_gather_tokens": (i32, [vp, vp, vp, i32, i32, i32, vp, vp]),
    # operator level
    "mia_op_linear": (i32, [vp, vp, i64, vp, vp, vp, i64, vp, i64] + [i32] * 8),
    "mia_op_linear_epi": (i32, [vp, vp, i64, vp, vp, vp, i64, vp] + [i32] * 12),
    "mia_op_attention_h64": (i32, [vp, vp, i64, vp, vp, i64] + [i32] * 6),
    "mia_op_attention_h64_variant": (i32, [vp, vp, i64, vp, vp, i64] + [i32] * 7),
    "mia_op_conv1d_f32": (i32, [vp, vp, i64, i32, vp, vp, vp, vp, i64] + [i32] * 8),
    "mia_dequant_affine": (i32, [vp, vp, vp, vp, i64, i64, i32, i32, i32, vp, i32, i32]),
    "mia_op_attention_f32": (i32, [vp, vp, i64, vp, i64, vp, i64, vp, i64, i32, i32, i32, f32]),
    "mia_op_conv_gemm_f32": (i32, [vp, P(ConvGemmDesc), i32]),
    "mia_op_attention_f32_ex": (i32, [vp, vp, i64, vp, i64, vp, i64, vp, i64, vp, vp, vp, i64, i32, i32, i32, f32, vp, i32]),
    "mia_op_attention_h128": (i32, [vp, vp, i64, vp, i64, vp, i64, vp, i64, i32, i32, i32, f32, vp, i32, i32]),
    "mia_op_fsmn_add": (i32, [vp, vp, i64, vp, i64, vp, i32, i32, i32, i32, i32, vp, i32, i32]),
    "mia_op_funasr_logmel": (i32, [vp, vp, vp, i32, vp, i32]),
    "mia_op_kvq_attention": (i32, [vp, vp, vp, vp, vp] + [i32] * 6),
    "mia_op_lm_prompt_attention": (i32, [vp, vp, vp, vp, vp] + [i32] * 6),
    "mia_op_skinny_gemm": (i32, [vp, P(SkinnyDesc)]),
    "mia_op_gemm_quant": (i32, [vp, vp]),
    # Whisper
    "mia_whisper_load": (vp, [vp, P(WhisperDims), TV, i32, i32]),
    "mia_whisper_free": (None, [vp]),
    "mia_whisper_clone": (vp, [vp, vp]),
    "mia_whisper_attach_quantized": (i32, [vp, TV, i32, i32, i32]),
    "mia_whisper_use_packed": (i32, [vp, i32]),
    "mia_quant_repack": (i32, [vp, vp, vp, i32, i32, i32, i32, i32, vp, vp]),
    "mia_whisper_set_gemm_variant": (i32, [vp, i32]),
    "mia_whisper_set_debug": (i32, [vp, i32]),
    "mia_whisper_trace_logits": (i32, [vp, vp, i32]),
    "mia_whisper_read_logit_trace": (i32, [vp, i32, i32, i32, vp]),
    "mia_whisper_encode": (i32, [vp, vp, i32, i32]),
    "mia_whisper_get_audio_features": (i32, [vp, vp, i32, i32]),
    "mia_whisper_decode_greedy": (i32, [vp, P(DecodeOpts), vp, vp, vp, vp, i32]),
    "mia_whisper_detect_language": (i32, [vp, i32, i32, vp, vp]),
    "mia_whisper_encode_windows": (i32, [vp, vp, vp, i32, i64, i32]),
    "mia_whisper_set_encode_stream": (i32, [vp, vp]),
    "mia_whisper_set_weight_sharing": (i32, [vp, i32]),
    "mia_whisper_transcribe_windows": (i32, [vp, vp, vp, i32, i64, P(DecodeOpts), vp, vp, vp, vp, i32]),
    "mia_whisper_audio_create": (vp, [vp, vp, vp, i32, i64, i32]),
    "mia_whisper_audio_free": (None, [vp]),
    "mia_whisper_audio_frames": (i64, [vp]),
    "mia_whisper_audio_read": (i32, [vp, i32, i64, i64, vp]),
    "mia_whisper_encode_audio_windows": (i32, [vp, vp, vp, vp, vp, i32]),
    "mia_whisper_align": (i32, [vp, vp, i32, vp, vp, i32, vp, i32, i32, vp, vp, vp, vp, i32, vp]),
    # neural codecs
    "mia_snac_load": (vp, [vp, P(SnacConfig), TV, i32]),
    "mia_dac_load": (vp, [vp, P(DacConfig), TV, i32]),
    "mia_codec_free": (None, [vp]),
    "mia_codec_output_len": (i64, [vp, i64]),
    "mia_codec_noise_len": (i64, [vp, i64]),
    "mia_snac_decode": (i32, [vp, vp, vp, i32, vp, i64, vp, i64, vp, i32]),
    "mia_dac_decode": (i32, [vp, vp, i32, i64, vp, i64, vp, i32]),
    "mia_snac_decode_batch": (i32, [vp, i32, vp, vp, i32, vp, i64, vp, vp, vp, i32]),
    "mia_dac_decode_batch": (i32, [vp, i32, vp, i32, vp, vp, vp, vp, i32]),
    "mia_codec_set_stack_budget": (i32, [vp, i64]),
    "mia_dac_load_encoder": (i32, [vp, P(DacEncoderConfig), TV, i32]),
    "mia_dac_code_len": (i64, [vp, i64]),
    "mia_dac_encode": (i32, [vp, vp, i64, i32, vp, i64, vp, i32]),
    # Mimi codec decode
    "mia_mimi_load": (vp, [vp, vp, TV, i32]),
    "mia_mimi_free": (None, [vp]),
    "mia_mimi_output_len": (i64, [vp, i64]),
    "mia_mimi_decode": (i32, [vp, vp, i32, i64, vp, i64, vp, i32]),
    "mia_mimi_stream_create": (vp, [vp]),
    "mia_mimi_stream_free": (None, [vp]),
    "mia_mimi_stream_reset": (i32, [vp]),
    "mia_mimi_stream_decode": (i32, [vp, vp, i32, i64, vp, i64, vp, i32]),
    "mia_mimi_encode_frames": (i64, [vp, i64]),
    "mia_mimi_encode": (i32, [vp, vp, i64, i32, vp, i64, vp, i32]),
    "mia_mimi_encode_latent": (i32, [vp, vp, i64, vp, i64, vp, i32]),
    "mia_mimi_quantize": (i32, [vp, vp, i64, i32, vp, i32]),
    # Kokoro decoder and F0 / N predictor blocks
    "mia_kokoro_load": (vp, [vp, vp, TV, i32]),
    "mia_kokoro_free": (None, [vp]),
    "mia_kokoro_output_len": (i64, [vp, i64]),
    "mia_kokoro_f0n": (i32, [vp, vp, i32, vp, vp, vp, i32]),
    "mia_kokoro_source": (i32, [vp, vp, i32, vp, vp, vp, i32]),
    "mia_kokoro_generate": (i32, [vp, vp, i32, vp, vp, vp, i32]),
    "mia_kokoro_decode": (i32, [vp, vp, i32, vp, vp, vp, vp, vp, i32]),
    "mia_op_instance_norm": (i32, [vp, vp, i64, i64, i32, vp, vp]),
    # OuteTTS speaker-profile audio
    "mia_speaker_audio_create": (vp, [vp, vp, i64, i32, f32, f32]),
    "mia_speaker_audio_free": (None, [vp]),
    "mia_speaker_audio_len": (i64, [vp]),
    "mia_speaker_audio_data": (vp, [vp]),
    "mia_speaker_audio_read": (i32, [vp, i64, i64, vp]),
    "mia_speaker_audio_features": (i32, [vp, vp, vp, i32, vp, vp]),
    "mia_speaker_audio_launches": (i32, [vp]),
    "mia_op_rfft_block": (i64, []),
    "mia_op_rfft_pow2": (i32, [vp, vp, i64, i64, vp]),
    # reference-clip trimming
    "mia_clip_create": (vp, [vp, vp, i64, i32]),
    "mia_clip_free": (None, [vp]),
    "mia_clip_len": (i64, [vp]),
    "mia_clip_data": (vp, [vp]),
    "mia_clip_read": (i32, [vp, i64, i64, vp]),
    "mia_clip_speech_bounds": (i32, [vp, i64, i64, f32, vp, vp, vp]),
    "mia_clip_frame_energy": (i32, [vp, i64, i64, i64, i64, vp]),
    "mia_clip_num_frames": (i64, [i64, i64, i64]),
    "mia_clip_launches": (i32, [vp]),
    # autoregressive LMs
    "mia_lm_load": (vp, [vp, P(LmConfig), TV, i32, i32]),
    "mia_lm_attach_quantized": (i32, [vp, TV, i32, i32, i32]),
    "mia_lm_attach_q4": (i32, [vp, TV, i32, i32]),
    "mia_lm_use_q4": (i32, [vp, i32]),
    "mia_lm_set_prompt_weights": (i32, [vp, i32]),
    "mia_lm_release_dense": (i32, [vp]),
    "mia_lm_weight_bytes": (i32, [vp, vp, vp]),
    "mia_lm_set_debug": (i32, [vp, i32]),
    "mia_lm_set_prompt_attention": (i32, [vp, i32]),
    "mia_lm_free": (None, [vp]),
    "mia_lm_reset": (i32, [vp]),
    "mia_lm_forward": (i32, [vp, vp, i32, vp]),
    "mia_lm_generate": (i32, [vp, vp, i32, P(LmSampler), vp, vp, vp]),
    "mia_lm_set_batch": (i32, [vp, i32]),
    "mia_lm_generate_batch": (i32, [vp, vp, vp, i32, P(LmSampler), vp, vp, vp]),
    "mia_lm_set_kv_quant": (i32, [vp, i32, i32]),
    "mia_lm_read_kv": (i32, [vp, i32, i32, i32, i32, vp, vp]),
    "mia_lm_generate_ras": (i32, [vp, vp, i32, P(RasParams), vp, i32, vp, vp]),
    "mia_lm_generate_ras_batch": (i32, [vp, vp, vp, i32, P(RasParams), vp, i32, vp, i32, vp]),
    "mia_lm_generate_greedy": (i32, [vp, vp, i32, vp, i32, i32, vp, vp]),
    "mia_lm_generate_greedy_batch": (i32, [vp, vp, vp, i32, vp, i32, i32, vp, i32, vp]),
    "mia_lm_generate_topk": (i32, [vp, vp, i32, f32, i32, f32, vp, i32, i32, vp, vp, vp]),
    "mia_lm_generate_topk_batch": (i32, [vp, vp, vp, i32, f32, i32, f32, vp, i32, i32, vp, vp, i32, vp]),
    "mia_sample_top_k_top_p": (i32, [vp, vp, i32, f32, i32, f32, f32, vp, vp, vp]),
    "mia_sample_top_p": (i32, [vp, vp, i32, vp, i32, f32, f32, f32, f32, vp]),
    # Marvis TTS
    "mia_marvis_load": (vp, [vp, vp, TV, i32, i32, vp]),
    "mia_marvis_free": (None, [vp]),
    "mia_marvis_reset": (i32, [vp]),
    "mia_marvis_set_debug": (i32, [vp, i32]),
    "mia_marvis_set_batch": (i32, [vp, i32]),
    "mia_marvis_attach_quantized": (i32, [vp, TV, i32, i32, i32]),
    "mia_marvis_use_packed": (i32, [vp, i32]),
    "mia_marvis_use_packed_prompt": (i32, [vp, i32]),
    "mia_marvis_release_dense": (i32, [vp]),
    "mia_marvis_frame": (i32, [vp, vp, vp, i32, i32, f32, f32, vp, vp, vp, vp]),
    "mia_marvis_generate": (i32, [vp, vp, vp, i32, i32, f32, f32, i32, vp, vp, vp]),
    "mia_marvis_generate_batch": (i32, [vp, vp, vp, vp, i32, i32, f32, f32, i32, vp, vp, vp]),
    "mia_sample_top_p_ascending": (i32, [vp, vp, i32, f32, f32, f32, vp, vp, vp]),
    # Fun-ASR audio half
    "mia_sensevoice_load": (vp, [vp, P(SensevoiceConfig), TV, i32, i32]),
    "mia_sensevoice_free": (None, [vp]),
    "mia_sensevoice_features": (i32, [vp, vp, vp, i32, vp, vp, i64, i32]),
    "mia_sensevoice_feature_rows": (i64, [vp, i32]),
    "mia_sensevoice_encode": (i32, [vp, vp, vp, i32, vp, vp, vp, i32]),
    "mia_sensevoice_encode_audio": (i32, [vp, vp, vp, i32, vp, vp, i32]),
    # S3Tokenizer
    "mia_s3tok_load": (vp, [vp, P(S3Config), TV, i32]),
    "mia_s3tok_free": (None, [vp]),
    "mia_s3tok_encode": (i32, [vp, vp, vp, i32, i32, vp, i32, vp, i32]),
    # HiFT vocoder
    "mia_hift_load": (vp, [vp, P(HiftConfig), TV, i32]),
    "mia_hift_free": (None, [vp]),
    "mia_hift_upsample_factor": (i32, [vp]),
    "mia_hift_f0": (i32, [vp, vp, i32, vp, i32]),
    "mia_hift_source": (i32, [vp, vp, i32, vp, vp, i32]),
    "mia_hift_decode": (i32, [vp, vp, i32, vp, vp, i32]),
    "mia_hift_vocode": (i32, [vp, vp, i32, vp, vp, i32, vp, vp, i32]),
    "mia_hift_vocode_batch": (i32, [vp, vp, vp, i32, vp, vp, i32]),
    # CosyVoice2 flow
    "mia_flow_load": (vp, [vp, P(FlowConfig), TV, i32]),
    "mia_flow_free": (None, [vp]),
    "mia_flow_encode": (i32, [vp, vp, i32, vp, i32]),
    "mia_flow_inference": (i32, [vp, vp, i32, vp, i32, vp, i32, vp, vp, i32, vp, i32]),
    "mia_flow_inference_batch": (i32, [vp, i32] + [vp] * 8 + [i32, vp, i32]),
    "mia_flow_inference_streaming": (i32, [vp, vp, i32, vp, i32, vp, i32, vp, vp, i32, i32, i32, i32, vp, vp, i32]),
    # CAM++ speaker encoder
    "mia_campplus_load": (vp, [vp, TV, i32]),
    "mia_campplus_free": (None, [vp]),
    "mia_kaldi_fbank_frames": (i64, [i64]),
    "mia_campplus_fbank": (i32, [vp, vp, i64, i32, vp, i32]),
    "mia_campplus_forward": (i32, [vp, vp, i32, vp, i32]),
    "mia_campplus_embed": (i32, [vp, vp, i64, vp, i32]),
}


def apply(lib: C.CDLL) -> None:
    """Set restype and argtypes of every table entry on `lib`; a symbol the library does not export is an ImportError."""
    for name, (restype, argtypes) in PROTOTYPES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            raise ImportError(f"{getattr(lib, '_name', 'libmia.so')} does not export {name}: the library is older than "
                              "include/mia.h, rebuild it") from None
        fn.restype, fn.argtypes = restype, argtypes
