"""ctypes binding of the C ABI in include/spittle_hip.h (libspittle_hip.so, in-tree).

The product path has no CPU fallback: if the HIP library is missing this module
raises, loudly, at import of the engine.
"""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libspittle_hip.so")

# status codes
SPT_OK, SPT_ERR_INVALID_ARG, SPT_ERR_LOAD, SPT_ERR_DEVICE, SPT_ERR_OOM, SPT_ERR_UNSUPPORTED, SPT_ERR_INTERNAL = range(7)
STATUS_NAMES = {0: "OK", 1: "INVALID_ARG", 2: "LOAD", 3: "DEVICE", 4: "OOM", 5: "UNSUPPORTED", 6: "INTERNAL"}
SPT_DTYPE_F32, SPT_DTYPE_BF16, SPT_DTYPE_F16, SPT_DTYPE_I8 = 0, 1, 2, 3
SPT_SUPPRESS_BLANK, SPT_NO_TIMESTAMPS, SPT_IGNORE_EOT, SPT_SUPPRESS_NST = 1, 2, 4, 8
SPT_NO_SPEECH_PROB = 16  # SPT_HAS_NO_SPEECH: report each window's no-speech probability without skipping
SPT_BLOCK_PREFILL = 32   # SPT_HAS_BLOCK_PREFILL: the prompt prefix in one block pass per sequence slice
SPT_HAS_BLOCK_PREFILL = 1

# every symbol include/spittle_hip.h declares
EXPORTS = [
    "spt_version", "spt_default_model_params", "spt_default_infer_params", "spt_ctx_create",
    "spt_ctx_destroy", "spt_last_error", "spt_ctx_info", "spt_transcribe", "spt_transcribe_batch",
    "spt_transcribe_batch_device", "spt_result_free", "spt_get_timings", "spt_get_call_stats", "spt_get_xq_stats", "spt_debug_mel",
    "spt_debug_mel_at", "spt_debug_encode", "spt_debug_weight_checksum", "spt_probe_kernel", "spt_language_code",
    "spt_tokenize", "spt_token_to_str", "spt_debug_ggml_tokenize", "spt_debug_ggml_dequant",
    "spt_weights_export", "spt_weights_import", "spt_weights_arena", "spt_weights_commit",
    "spt_ctx_create_replicas", "spt_transcribe_batch_replicas",
    # ABI 6: Parakeet-V3
    "spt_parakeet_default_model_params", "spt_parakeet_default_infer_params", "spt_parakeet_create",
    "spt_parakeet_destroy", "spt_parakeet_last_error", "spt_parakeet_info", "spt_parakeet_tensor_numel",
    "spt_parakeet_set_tensor", "spt_parakeet_set_vocab", "spt_parakeet_transcribe", "spt_parakeet_transcribe_batch",
    "spt_parakeet_transcribe_batch_device", "spt_parakeet_result_free", "spt_parakeet_get_timings",
    "spt_parakeet_debug_mel", "spt_parakeet_debug_encode", "spt_parakeet_debug_decode", "spt_parakeet_debug_last_encoder",
    "spt_parakeet_debug_weight_checksum", "spt_parakeet_onnx_open", "spt_parakeet_onnx_tensor",
    "spt_parakeet_onnx_piece", "spt_parakeet_onnx_close",
    # ABI 7: capture-side resampler
    "spt_resampler_create", "spt_resampler_info", "spt_resample_output_len", "spt_resample",
    "spt_resampler_last_error", "spt_resampler_destroy",
    # ABI 8: voice-activity gate
    "spt_vad_default_params", "spt_vad_create", "spt_vad_push", "spt_vad_result_free", "spt_vad_reset",
    "spt_vad_last_error", "spt_vad_destroy",
    # ABI 10: Parakeet encoder stage profile
    "spt_parakeet_profile_encoder",
    # ABI 13: the Parakeet encoder's int8 mode (SPT_DTYPE_I8)
    "spt_parakeet_onnx_qtensor", "spt_parakeet_debug_qgemm", "spt_parakeet_debug_tap", "spt_parakeet_debug_tap_read",
    # Moonshine (SPT_HAS_MOONSHINE, additive over ABI 14)
    "spt_moonshine_default_model_params", "spt_moonshine_default_infer_params", "spt_moonshine_create",
    "spt_moonshine_destroy", "spt_moonshine_last_error", "spt_moonshine_info", "spt_moonshine_tensor_numel",
    "spt_moonshine_set_tensor", "spt_moonshine_missing_tensors", "spt_moonshine_set_vocab", "spt_moonshine_transcribe",
    "spt_moonshine_transcribe_batch", "spt_moonshine_result_free", "spt_moonshine_get_timings",
    "spt_moonshine_debug_stem", "spt_moonshine_debug_encode", "spt_moonshine_debug_logits",
    # SenseVoice (SPT_HAS_SENSEVOICE, additive over ABI 14)
    "spt_sensevoice_default_model_params", "spt_sensevoice_default_infer_params", "spt_sensevoice_create",
    "spt_sensevoice_destroy", "spt_sensevoice_last_error", "spt_sensevoice_info", "spt_sensevoice_tensor_numel",
    "spt_sensevoice_set_tensor", "spt_sensevoice_missing_tensors", "spt_sensevoice_set_cmvn",
    "spt_sensevoice_set_vocab", "spt_sensevoice_n_rows", "spt_sensevoice_transcribe",
    "spt_sensevoice_transcribe_batch", "spt_sensevoice_result_free", "spt_sensevoice_get_timings",
    "spt_sensevoice_debug_features", "spt_sensevoice_debug_encode", "spt_sensevoice_debug_frames",
    # the sampler kernels alone (test hooks, additive over ABI 14)
    "spt_debug_sample_tokens", "spt_debug_sample_beam", "spt_debug_sample_kv_gather",
    # the attention kernels alone (test hooks, additive over ABI 14)
    "spt_debug_attn_enc", "spt_debug_attn_self", "spt_debug_attn_cross", "spt_debug_xq_fused",
    # the GEMM tiles and LayerNorm kernels alone (test hooks, additive over ABI 14)
    "spt_debug_gemm", "spt_debug_layernorm",
    # quantised decoder weights resident in HBM (SPT_HAS_QUANT_RESIDENT)
    "spt_debug_qgemv", "spt_get_weight_residency",
    # the decoder GEMV and the step's small kernels alone (SPT_HAS_GEMV_KERNELS)
    "spt_debug_gemv", "spt_debug_dec_step",
    # the Parakeet encoder kernels and the TDT bookkeeping alone (SPT_HAS_PK_KERNELS)
    "spt_debug_pk_conv", "spt_debug_pk_relpos", "spt_debug_pk_rel_attn", "spt_debug_pk_tdt",
    "spt_debug_pk_dec_stage", "spt_debug_pk_tdt_steps",
    # the token-alignment kernels alone (SPT_HAS_ALIGN_KERNELS)
    "spt_debug_align_qk", "spt_debug_align_norm", "spt_debug_align_dtw", "spt_debug_align_words",
    # DTW token and word timestamps (SPT_HAS_TOKEN_TIMESTAMPS)
    "spt_set_alignment_heads", "spt_transcribe_aligned", "spt_transcribe_aligned_batch", "spt_alignment_free",
    "spt_debug_align_last", "spt_debug_align_stats",
    # the no-speech probability and the silence skip (SPT_HAS_NO_SPEECH)
    "spt_get_window_info", "spt_debug_no_speech",
    # block prefill of the prompt prefix (SPT_HAS_BLOCK_PREFILL)
    "spt_get_prefill_stats", "spt_debug_attn_prefill_self", "spt_debug_attn_prefill_cross",
    # the fp8 cross K/V cache (SPT_HAS_CROSS_KV_F8)
    "spt_get_cross_kv_info", "spt_debug_cross_kv", "spt_debug_attn_cross_quant",
]


class TokenTime(C.Structure):
    _fields_ = [("t0", C.c_int64), ("t1", C.c_int64), ("p", C.c_float), ("index", C.c_int32)]


class Word(C.Structure):
    _fields_ = [("t0", C.c_int64), ("t1", C.c_int64), ("text", C.c_char_p), ("i0", C.c_int32), ("n_tokens", C.c_int32),
                ("p", C.c_float)]


class Alignment(C.Structure):
    _fields_ = [("tokens", C.POINTER(TokenTime)), ("n_tokens", C.c_int32), ("words", C.POINTER(Word)),
                ("n_words", C.c_int32)]

SPT_MODEL_QUANT_RESIDENT = 2
SPT_MODEL_CROSS_KV_F8 = 4  # SPT_HAS_CROSS_KV_F8: the cross K/V cache in fp8 e4m3 with a scale per key row
SPT_HAS_CROSS_KV_F8 = 1
SPT_GGML_Q4_1, SPT_GGML_Q5_0, SPT_GGML_Q5_1 = 3, 6, 7
SPT_GV_BIAS, SPT_GV_BIAS_GELU, SPT_GV_PARTIAL, SPT_GV_QKV_CACHE, SPT_GV_LOGITS, SPT_GV_BIAS_RESID = range(6)
SPT_QGEMV_A_DIRECT, SPT_QGEMV_A_LN = 0, 1
SPT_GEMV_A_DIRECT, SPT_GEMV_A_LN, SPT_GEMV_A_ATTN = 0, 1, 2
SPT_DEC_STEP_EMBED, SPT_DEC_STEP_FINALIZE, SPT_DEC_STEP_ADVANCE, SPT_DEC_STEP_RESET = range(4)
SPT_ATTN_CROSS_8WAVE, SPT_ATTN_CROSS_VW, SPT_ATTN_CROSS_VW_PQ, SPT_ATTN_CROSS_VW_MERGE, SPT_ATTN_CROSS_VW_PQ_MERGE = range(5)
SPT_LN_PLAIN, SPT_LN_PEND, SPT_LN_PEND2 = range(3)
SPT_SV_LANG_AUTO, SPT_SV_LANG_ZH, SPT_SV_LANG_EN, SPT_SV_LANG_YUE, SPT_SV_LANG_JA, SPT_SV_LANG_KO = range(6)
SPT_PK_WEIGHTS_EMPTY = 1
SPT_PK_TS_TOKEN, SPT_PK_TS_WORD, SPT_PK_TS_SEGMENT = 0, 1, 2
SPT_MODEL_WEIGHTS_EXTERNAL = 1
# spt_pk_stage: encoder stage classes of spt_parakeet_profile_encoder, in order
PK_STAGES = ("subsampling", "pos", "layernorm", "ffn", "qkv_out", "attn", "conv_pw", "conv_dw", "joint_enc")
PROBES = {"dec_cross_attn": 0, "dec_self_attn": 1, "dec_logits": 2, "dec_fc1": 3, "enc_fc1_gemm": 4,
          "enc_attn": 5}


_FP, _I32P = C.POINTER(C.c_float), C.POINTER(C.c_int32)


class GemvDebug(C.Structure):
    """spt_gemv_debug"""
    _fields_ = [(n, _FP) for n in ("W", "A", "ln_w", "ln_b", "pend", "x_out", "apart", "out_merged", "bias", "C",
                                   "p_resid", "cache")] + \
               [("suppress", C.POINTER(C.c_uint32)), ("part", _FP), ("plan", _I32P)] + \
               [(n, C.c_int64) for n in ("a_count", "c_count", "c_split", "suppress_words")] + \
               [(n, C.c_int32) for n in ("dtype", "mode", "a_src", "R", "N", "K", "lda", "a_row0", "n_pend", "S", "H",
                                         "merge_first", "ldc", "ksplit", "B", "Tq", "cache_H", "ctx", "pos0", "blank0",
                                         "blank1", "step", "n_tiles", "reserved0")]


class DecStepDebug(C.Structure):
    """spt_dec_step_debug"""
    _fields_ = [("tok", _I32P), ("part", _FP), ("forced", _I32P), ("done", _I32P), ("emb", _FP),
                ("emb_blocks", C.c_void_p), ("pos", _FP), ("state", _I32P), ("next_tok", _I32P), ("x", _FP),
                ("out_tok", _I32P), ("out_top1", _FP), ("out_top2", _FP), ("emb_blocks_bytes", C.c_size_t)] + \
               [(n, C.c_int32) for n in ("dtype", "op", "B", "Tq", "d", "ctx", "n_vocab", "n_tiles", "n_steps",
                                         "forced_len", "ignore_eot", "out_cap", "eot", "emb_q", "n_advance",
                                         "reserved0")]


SPT_PK_CONV0, SPT_PK_DWCONV1, SPT_PK_DWCONV2, SPT_PK_CONV_MODULE = range(4)
SPT_PK_ATTN_AUTO, SPT_PK_ATTN_VALU, SPT_PK_ATTN_MFMA = range(3)


class PkConvDebug(C.Structure):
    """spt_pk_conv_debug"""
    _fields_ = [("x", _FP), ("lens", _I32P)] + [(n, _FP) for n in ("w", "bias", "bn_g", "bn_b", "bn_m", "bn_v", "y")] + \
               [("y_count", C.c_int64)] + [(n, C.c_int32) for n in ("dtype", "mode", "B", "Tp", "F", "C")]


class PkAttnDebug(C.Structure):
    """spt_pk_attn_debug"""
    _fields_ = [(n, _FP) for n in ("qkv", "p", "pu", "pv")] + [("lens", _I32P), ("out", _FP)] + \
               [(n, C.c_int64) for n in ("p_count", "p_off", "p_bstride", "out_count")] + \
               [(n, C.c_int32) for n in ("dtype", "variant", "B", "Tp", "H", "dk", "ldp", "reserved0")]


SPT_PK_DEC_LSTM, SPT_PK_DEC_PRED, SPT_PK_DEC_JOINT = range(3)


class PkDecDebug(C.Structure):
    """spt_pk_dec_debug"""
    _fields_ = [(n, _FP) for n in ("W", "W2", "b0", "b1")] + [("state", _I32P)] + \
               [(n, _FP) for n in ("xin", "h_in", "c_in", "fe", "gp", "h_out", "c_out", "part", "dur")] + \
               [(n, C.c_int32) for n in ("mode", "B", "P", "V", "n_dur", "reserved0")]


class PkStepsDebug(C.Structure):
    """spt_pk_steps_debug"""
    _fields_ = [("lstm", (_FP * 4) * 2)] + [(n, _FP) for n in ("pred_w", "pred_b", "joint_w", "joint_b", "emb", "fe")] + \
               [("lens", _I32P), ("state", _I32P), ("out_tok", _I32P), ("out_frame", _I32P), ("out_t1", _FP), ("out_t2", _FP)] + \
               [(n, C.c_int32) for n in ("B", "P", "V", "n_dur", "n_steps", "max_symbols", "cap", "T3p")]


class PkTdtDebug(C.Structure):
    """spt_pk_tdt_debug"""
    _fields_ = [("part", _FP), ("dur", _FP), ("lens", _I32P), ("emb", _FP), ("fe", _FP), ("state", _I32P), ("xemb", _FP),
                ("fecur", _FP), ("out_tok", _I32P), ("out_frame", _I32P), ("out_t1", _FP), ("out_t2", _FP)] + \
               [(n, C.c_int32) for n in ("B", "P", "V", "n_dur", "n_tiles", "n_steps", "max_symbols", "cap", "T3p",
                                         "reserved0")]


class ModelParams(C.Structure):
    _fields_ = [("dtype", C.c_int32), ("device", C.c_int32), ("max_batch", C.c_int32),
                ("flags", C.c_uint32), ("seed", C.c_uint64)]


class InferParams(C.Structure):
    _fields_ = [("language", C.c_char_p), ("translate", C.c_int32), ("initial_prompt", C.c_char_p),
                ("flags", C.c_uint32), ("max_new_tokens", C.c_int32), ("temperature", C.c_float),
                ("beam_size", C.c_int32), ("forced_tokens", C.POINTER(C.c_int32)), ("n_forced", C.c_int32),
                ("prompt_tokens", C.POINTER(C.c_int32)), ("n_prompt_tokens", C.c_int32),
                ("temperature_inc", C.c_float), ("best_of", C.c_int32), ("entropy_thold", C.c_float),
                ("logprob_thold", C.c_float), ("max_initial_ts", C.c_float), ("no_speech_thold", C.c_float),
                ("seed", C.c_uint64)]


class WindowInfo(C.Structure):  # spt_window_info
    _fields_ = [(n, C.c_int32) for n in ("utterance", "seek", "seek_delta", "i0", "n_tokens", "n_fallbacks")] + \
               [(n, C.c_float) for n in ("temperature", "avg_logprob", "no_speech_prob")] + [("skipped", C.c_int32)]


class Segment(C.Structure):
    _fields_ = [("t0", C.c_int64), ("t1", C.c_int64), ("text", C.c_char_p), ("i0", C.c_int32),
                ("n_tokens", C.c_int32)]


class Result(C.Structure):
    _fields_ = [("text", C.c_char_p), ("tokens", C.POINTER(C.c_int32)), ("top1", C.POINTER(C.c_float)),
                ("top2", C.POINTER(C.c_float)), ("n_tokens", C.c_int32), ("n_windows", C.c_int32),
                ("language", C.c_int32), ("n_segments", C.c_int32), ("segments", C.POINTER(Segment)),
                ("n_fallbacks", C.c_int32), ("reserved0", C.c_int32)]


class ModelInfo(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("n_mels", "d", "n_head", "n_enc", "n_dec", "n_vocab", "n_audio_ctx",
                                          "n_text_ctx", "dtype", "max_batch")] + \
               [("weight_bytes", C.c_int64), ("workspace_bytes", C.c_int64)]


class Timings(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("mel_ms", "encoder_ms", "cross_kv_ms", "decode_ms", "total_ms",
                                           "h2d_ms")] + [("n_decode_passes", C.c_int32), ("batch", C.c_int32)]


class CallStats(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("engine_calls", "decoder_passes", "beam_steps", "encoder_windows")] + \
               [(n, C.c_double) for n in ("device_ms", "encoder_ms", "decode_ms")] + \
               [(n, C.c_int32) for n in ("pd_passes", "pd_fallbacks")]


class PkModelParams(C.Structure):
    _fields_ = [("dtype", C.c_int32), ("device", C.c_int32), ("max_batch", C.c_int32), ("max_seconds", C.c_float),
                ("seed", C.c_uint64), ("flags", C.c_uint32), ("reserved0", C.c_int32)]


class PkInferParams(C.Structure):
    _fields_ = [("max_symbols", C.c_int32), ("timestamp_granularity", C.c_int32)]


class PkSegment(C.Structure):
    _fields_ = [("start", C.c_double), ("end", C.c_double), ("text", C.c_char_p), ("i0", C.c_int32),
                ("n_tokens", C.c_int32)]


class PkResult(C.Structure):
    _fields_ = [("text", C.c_char_p), ("tokens", C.POINTER(C.c_int32)), ("frames", C.POINTER(C.c_int32)),
                ("logit", C.POINTER(C.c_float)), ("runner_up", C.POINTER(C.c_float)), ("n_tokens", C.c_int32),
                ("n_segments", C.c_int32), ("segments", C.POINTER(PkSegment)), ("n_chunks", C.c_int32),
                ("reserved0", C.c_int32)]


class PkModelInfo(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("n_mels", "d", "n_layers", "n_heads", "ff", "sub_ch", "conv_k", "pred",
                                          "n_vocab", "n_dur", "dtype", "max_batch", "max_samples", "reserved0")] + \
               [("weight_bytes", C.c_int64), ("workspace_bytes", C.c_int64)]


class PkTimings(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("mel_ms", "encoder_ms", "decode_ms", "total_ms", "h2d_ms")] + \
               [(n, C.c_int32) for n in ("n_steps", "batch", "enc_frames", "reserved0")]


class MsModelParams(C.Structure):
    _fields_ = [("dtype", C.c_int32), ("device", C.c_int32), ("max_batch", C.c_int32), ("max_samples", C.c_int32),
                ("seed", C.c_uint64)]


class MsInferParams(C.Structure):
    _fields_ = [("tokens_per_second", C.c_float), ("max_tokens", C.c_int32)]


class MsResult(C.Structure):
    _fields_ = [("text", C.c_char_p), ("tokens", C.POINTER(C.c_int32)), ("top1", C.POINTER(C.c_float)),
                ("top2", C.POINTER(C.c_float)), ("n_tokens", C.c_int32), ("hit_eos", C.c_int32)]


class MsModelInfo(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("d", "n_heads", "head_dim", "rotary_dim", "ff", "n_enc_layers",
                                          "n_dec_layers", "n_vocab", "bos", "eos", "dtype", "max_batch",
                                          "max_samples", "ctx")] + \
               [("weight_bytes", C.c_int64), ("workspace_bytes", C.c_int64)]


class MsTimings(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("stem_ms", "encoder_ms", "cross_kv_ms", "decode_ms", "total_ms")] + \
               [("n_steps", C.c_int32), ("batch", C.c_int32)]


class SvModelParams(C.Structure):
    _fields_ = [("dtype", C.c_int32), ("device", C.c_int32), ("max_batch", C.c_int32), ("max_samples", C.c_int32),
                ("seed", C.c_uint64), ("ln_eps", C.c_float), ("sanm_shift", C.c_int32), ("lfr_m", C.c_int32),
                ("lfr_n", C.c_int32), ("blank_id", C.c_int32), ("n_prefix", C.c_int32), ("lang_rows", C.c_int32 * 6),
                ("event_row", C.c_int32), ("emo_row", C.c_int32), ("itn_row", C.c_int32), ("no_itn_row", C.c_int32)]


class SvInferParams(C.Structure):
    _fields_ = [("language", C.c_int32), ("use_itn", C.c_int32)]


class SvResult(C.Structure):
    _fields_ = [("text", C.c_char_p), ("tokens", C.POINTER(C.c_int32)), ("frames", C.POINTER(C.c_int32)),
                ("top1", C.POINTER(C.c_float)), ("top2", C.POINTER(C.c_float)), ("n_tokens", C.c_int32),
                ("prefix", C.c_int32 * 4)]


class SvModelInfo(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("d", "n_heads", "head_dim", "ff", "n_enc0_layers", "n_enc_layers",
                                          "n_tp_layers", "n_vocab", "input_dim", "dtype", "max_batch",
                                          "max_samples", "max_rows", "reserved")] + \
               [("weight_bytes", C.c_int64), ("workspace_bytes", C.c_int64)]


class SvTimings(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("frontend_ms", "encoder_ms", "ctc_ms", "total_ms")] + \
               [("rows", C.c_int32), ("batch", C.c_int32)]


class SampleParams(C.Structure):
    _fields_ = [("temperature", C.c_float), ("suppress_blank", C.c_int32), ("no_ts", C.c_int32),
                ("max_initial", C.c_int32), ("n_max", C.c_int32), ("max_tokens", C.c_int32), ("seed", C.c_uint64)]


class VadParams(C.Structure):
    _fields_ = [("threshold", C.c_float), ("prefill_frames", C.c_int32), ("hangover_frames", C.c_int32),
                ("onset_frames", C.c_int32), ("device", C.c_int32), ("reserved0", C.c_int32)]


class VadResult(C.Structure):
    _fields_ = [("samples", C.POINTER(C.c_float)), ("n_samples", C.c_size_t), ("prob", C.POINTER(C.c_float)),
                ("kind", C.POINTER(C.c_uint8)), ("n_frames", C.c_int32), ("reserved0", C.c_int32),
                ("device_ms", C.c_double)]


_lib = None


def load():
    """Load libspittle_hip.so (built by __graft_entry__.build / make -C spittle_amd/csrc)."""
    global _lib
    if _lib is not None:
        return _lib
    path = LIB_PATH
    if os.environ.get("SPT_DEBUG_LIB"):  # bounds-checked developer build (make -C spittle_amd/csrc dbg)
        path = os.path.join(os.path.dirname(LIB_PATH), "libspittle_hip_dbg.so")
    if not os.path.exists(path):
        raise ImportError(f"spittle_amd: HIP library not built: {path} (run `make -C spittle_amd/csrc`)")
    L = C.CDLL(path)
    vp, fp = C.c_void_p, C.POINTER(C.c_float)
    L.spt_version.restype = C.c_char_p
    L.spt_default_model_params.argtypes = [C.POINTER(ModelParams)]
    L.spt_default_infer_params.argtypes = [C.POINTER(InferParams)]
    L.spt_ctx_create.argtypes = [C.c_char_p, C.POINTER(ModelParams), C.POINTER(vp), C.c_char_p, C.c_size_t]
    L.spt_ctx_create.restype = C.c_int
    L.spt_ctx_destroy.argtypes = [vp]
    L.spt_last_error.argtypes = [vp]
    L.spt_last_error.restype = C.c_char_p
    L.spt_ctx_info.argtypes = [vp, C.POINTER(ModelInfo)]
    L.spt_transcribe.argtypes = [vp, fp, C.c_size_t, C.POINTER(InferParams), C.POINTER(C.POINTER(Result))]
    L.spt_transcribe_batch.argtypes = [vp, C.POINTER(fp), C.POINTER(C.c_size_t), C.c_size_t,
                                       C.POINTER(InferParams), C.POINTER(C.POINTER(Result))]
    L.spt_transcribe_batch_device.argtypes = [vp, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_size_t,
                                              C.POINTER(InferParams), C.POINTER(C.POINTER(Result))]
    L.spt_result_free.argtypes = [C.POINTER(Result)]
    L.spt_language_code.argtypes = [C.c_int32]
    L.spt_language_code.restype = C.c_char_p
    ip = C.POINTER(C.c_int32)
    L.spt_tokenize.argtypes = [vp, C.c_char_p, ip, C.c_int32, ip]
    L.spt_token_to_str.argtypes = [vp, C.c_int32]
    L.spt_token_to_str.restype = C.c_char_p
    L.spt_debug_ggml_tokenize.argtypes = [C.c_char_p, C.c_char_p, ip, C.c_int32, ip]
    L.spt_debug_ggml_dequant.argtypes = [C.c_int32, C.c_void_p, C.c_int64, fp]
    L.spt_get_timings.argtypes = [vp, C.POINTER(Timings)]
    L.spt_get_call_stats.argtypes = [vp, C.POINTER(CallStats)]
    L.spt_get_xq_stats.argtypes = [vp, ip, ip]
    L.spt_get_prefill_stats.argtypes = [vp, ip, ip, ip]
    L.spt_get_prefill_stats.restype = C.c_int
    L.spt_get_cross_kv_info.argtypes = [vp, ip, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.spt_debug_cross_kv.argtypes = [vp, C.c_int32, C.c_int32, fp, fp]
    L.spt_get_cross_kv_info.restype = L.spt_debug_cross_kv.restype = C.c_int
    L.spt_get_window_info.argtypes = [vp, C.POINTER(WindowInfo), C.c_int32, ip]
    L.spt_get_window_info.restype = C.c_int
    L.spt_debug_mel.argtypes = [vp, fp, C.c_size_t, fp]
    L.spt_debug_mel_at.argtypes = [vp, fp, C.c_size_t, C.c_int32, fp]
    L.spt_debug_encode.argtypes = [vp, fp, fp]
    L.spt_debug_weight_checksum.argtypes = [vp, C.c_int32, C.POINTER(C.c_double)]
    L.spt_probe_kernel.argtypes = [vp, C.c_int32, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                   C.POINTER(C.c_int32)]
    L.spt_weights_export.argtypes = [vp, C.c_void_p, C.c_size_t]
    L.spt_weights_import.argtypes = [vp, C.c_void_p, C.c_size_t]
    L.spt_weights_arena.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.spt_weights_commit.argtypes = [vp]
    L.spt_ctx_create_replicas.argtypes = [C.c_char_p, C.POINTER(ModelParams), C.POINTER(C.c_int32), C.c_int32,
                                          C.POINTER(vp), C.POINTER(C.c_double), C.c_char_p, C.c_size_t]
    L.spt_transcribe_batch_replicas.argtypes = [C.POINTER(vp), C.c_int32, C.POINTER(fp), C.POINTER(C.c_size_t),
                                                C.c_size_t, C.POINTER(InferParams), C.POINTER(C.POINTER(Result))]
    # ABI 6: Parakeet-V3
    PR = C.POINTER(C.POINTER(PkResult))
    L.spt_parakeet_default_model_params.argtypes = [C.POINTER(PkModelParams)]
    L.spt_parakeet_default_infer_params.argtypes = [C.POINTER(PkInferParams)]
    L.spt_parakeet_create.argtypes = [C.c_char_p, C.POINTER(PkModelParams), C.POINTER(vp), C.c_char_p, C.c_size_t]
    L.spt_parakeet_onnx_open.argtypes = [C.c_char_p, C.POINTER(vp), C.POINTER(PkModelInfo), C.c_char_p, C.c_size_t]
    L.spt_parakeet_onnx_tensor.restype = C.c_int64
    L.spt_parakeet_onnx_tensor.argtypes = [vp, C.c_int32, C.POINTER(C.POINTER(C.c_float))]
    L.spt_parakeet_onnx_qtensor.restype = C.c_int64
    L.spt_parakeet_onnx_qtensor.argtypes = [vp, C.c_int32, C.POINTER(C.POINTER(C.c_int16)), C.POINTER(fp),
                                            C.POINTER(C.POINTER(C.c_int32)), C.POINTER(C.c_int32)]
    L.spt_parakeet_onnx_piece.restype = C.c_char_p
    L.spt_parakeet_onnx_piece.argtypes = [vp, C.c_int32]
    L.spt_parakeet_onnx_close.argtypes = [vp]
    L.spt_parakeet_destroy.argtypes = [vp]
    L.spt_parakeet_last_error.argtypes = [vp]
    L.spt_parakeet_last_error.restype = C.c_char_p
    L.spt_parakeet_info.argtypes = [vp, C.POINTER(PkModelInfo)]
    L.spt_parakeet_tensor_numel.argtypes = [vp, C.c_int32, C.POINTER(C.c_int64)]
    L.spt_parakeet_set_tensor.argtypes = [vp, C.c_int32, fp, C.c_int64]
    L.spt_parakeet_set_vocab.argtypes = [vp, C.POINTER(C.c_char_p), C.c_int32]
    L.spt_parakeet_transcribe.argtypes = [vp, fp, C.c_size_t, C.POINTER(PkInferParams), PR]
    L.spt_parakeet_transcribe_batch.argtypes = [vp, C.POINTER(fp), C.POINTER(C.c_size_t), C.c_size_t,
                                                C.POINTER(PkInferParams), PR]
    L.spt_parakeet_transcribe_batch_device.argtypes = [vp, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_size_t,
                                                       C.POINTER(PkInferParams), PR]
    L.spt_parakeet_result_free.argtypes = [C.POINTER(PkResult)]
    L.spt_parakeet_get_timings.argtypes = [vp, C.POINTER(PkTimings)]
    L.spt_parakeet_profile_encoder.argtypes = [vp, C.c_int32, C.POINTER(C.c_double), C.c_int32]
    L.spt_parakeet_debug_mel.argtypes = [vp, fp, C.c_size_t, fp]
    L.spt_parakeet_debug_encode.argtypes = [vp, fp, C.c_int32, fp]
    L.spt_parakeet_debug_decode.argtypes = [vp, fp, C.c_int32, C.c_int32, PR]
    L.spt_parakeet_debug_last_encoder.argtypes = [vp, C.c_int32, fp, C.POINTER(C.c_int32)]
    L.spt_parakeet_debug_weight_checksum.argtypes = [vp, C.c_int32, C.POINTER(C.c_double)]
    i32p = C.POINTER(C.c_int32)
    L.spt_parakeet_debug_qgemm.argtypes = [C.c_int32, fp, C.c_int32, C.c_int32, i32p, C.c_int32, C.POINTER(C.c_int16),
                                           C.c_int32, fp, i32p, C.c_int32, fp, C.c_int32, C.POINTER(C.c_uint8), fp, i32p,
                                           i32p, fp, C.c_char_p, C.c_size_t]
    L.spt_parakeet_debug_tap.argtypes = [vp, C.c_int32]
    L.spt_parakeet_debug_tap_read.argtypes = [vp, i32p, fp, C.c_int64, fp, C.c_int64]
    L.spt_resampler_create.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(vp), C.c_char_p,
                                       C.c_size_t]
    L.spt_resampler_create.restype = C.c_int
    L.spt_resampler_info.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.spt_resampler_info.restype = C.c_int
    L.spt_resample_output_len.argtypes = [vp, C.c_size_t]
    L.spt_resample_output_len.restype = C.c_size_t
    L.spt_resample.argtypes = [vp, fp, C.c_size_t, fp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.spt_resample.restype = C.c_int
    L.spt_resampler_last_error.argtypes = [vp]
    L.spt_resampler_last_error.restype = C.c_char_p
    L.spt_resampler_destroy.argtypes = [vp]
    L.spt_resampler_destroy.restype = None
    L.spt_vad_default_params.argtypes = [C.POINTER(VadParams)]
    L.spt_vad_default_params.restype = None
    L.spt_vad_create.argtypes = [C.c_char_p, C.POINTER(VadParams), C.POINTER(vp), C.c_char_p, C.c_size_t]
    L.spt_vad_create.restype = C.c_int
    L.spt_vad_push.argtypes = [vp, fp, C.c_size_t, C.POINTER(C.POINTER(VadResult))]
    L.spt_vad_push.restype = C.c_int
    L.spt_vad_result_free.argtypes = [C.POINTER(VadResult)]
    L.spt_vad_result_free.restype = None
    L.spt_vad_reset.argtypes = [vp, C.c_int32]
    L.spt_vad_reset.restype = C.c_int
    L.spt_vad_last_error.argtypes = [vp]
    L.spt_vad_last_error.restype = C.c_char_p
    L.spt_vad_destroy.argtypes = [vp]
    L.spt_vad_destroy.restype = None
    # Moonshine
    MR = C.POINTER(C.POINTER(MsResult))
    L.spt_moonshine_default_model_params.argtypes = [C.POINTER(MsModelParams)]
    L.spt_moonshine_default_model_params.restype = None
    L.spt_moonshine_default_infer_params.argtypes = [C.POINTER(MsInferParams)]
    L.spt_moonshine_default_infer_params.restype = None
    L.spt_moonshine_create.argtypes = [C.c_char_p, C.POINTER(MsModelParams), C.POINTER(vp), C.c_char_p, C.c_size_t]
    L.spt_moonshine_destroy.argtypes = [vp]
    L.spt_moonshine_destroy.restype = None
    L.spt_moonshine_last_error.argtypes = [vp]
    L.spt_moonshine_last_error.restype = C.c_char_p
    L.spt_moonshine_info.argtypes = [vp, C.POINTER(MsModelInfo)]
    L.spt_moonshine_tensor_numel.argtypes = [vp, C.c_char_p, C.POINTER(C.c_int64)]
    L.spt_moonshine_set_tensor.argtypes = [vp, C.c_char_p, fp, C.c_int64]
    L.spt_moonshine_missing_tensors.argtypes = [vp]
    L.spt_moonshine_missing_tensors.restype = C.c_int32
    L.spt_moonshine_set_vocab.argtypes = [vp, C.POINTER(C.c_char_p), C.c_int32]
    L.spt_moonshine_transcribe.argtypes = [vp, fp, C.c_size_t, C.POINTER(MsInferParams), MR]
    L.spt_moonshine_transcribe_batch.argtypes = [vp, C.POINTER(fp), C.POINTER(C.c_size_t), C.c_size_t,
                                                 C.POINTER(MsInferParams), MR]
    L.spt_moonshine_result_free.argtypes = [C.POINTER(MsResult)]
    L.spt_moonshine_result_free.restype = None
    L.spt_moonshine_get_timings.argtypes = [vp, C.POINTER(MsTimings)]
    L.spt_moonshine_debug_stem.argtypes = [vp, fp, C.c_size_t, fp]
    L.spt_moonshine_debug_encode.argtypes = [vp, fp, C.c_size_t, fp]
    L.spt_moonshine_debug_logits.argtypes = [vp, fp, C.c_size_t, i32p, C.c_int32, fp]
    for fn in ("spt_moonshine_create", "spt_moonshine_info", "spt_moonshine_tensor_numel", "spt_moonshine_set_tensor",
               "spt_moonshine_set_vocab", "spt_moonshine_transcribe", "spt_moonshine_transcribe_batch",
               "spt_moonshine_get_timings", "spt_moonshine_debug_stem", "spt_moonshine_debug_encode",
               "spt_moonshine_debug_logits"):
        getattr(L, fn).restype = C.c_int
    # SenseVoice
    SR = C.POINTER(C.POINTER(SvResult))
    svip = C.POINTER(SvInferParams)
    L.spt_sensevoice_default_model_params.argtypes = [C.POINTER(SvModelParams)]
    L.spt_sensevoice_default_model_params.restype = None
    L.spt_sensevoice_default_infer_params.argtypes = [svip]
    L.spt_sensevoice_default_infer_params.restype = None
    L.spt_sensevoice_create.argtypes = [C.c_char_p, C.POINTER(SvModelParams), C.POINTER(vp), C.c_char_p, C.c_size_t]
    L.spt_sensevoice_destroy.argtypes = [vp]
    L.spt_sensevoice_destroy.restype = None
    L.spt_sensevoice_last_error.argtypes = [vp]
    L.spt_sensevoice_last_error.restype = C.c_char_p
    L.spt_sensevoice_info.argtypes = [vp, C.POINTER(SvModelInfo)]
    L.spt_sensevoice_tensor_numel.argtypes = [vp, C.c_char_p, C.POINTER(C.c_int64)]
    L.spt_sensevoice_set_tensor.argtypes = [vp, C.c_char_p, fp, C.c_int64]
    L.spt_sensevoice_missing_tensors.argtypes = [vp]
    L.spt_sensevoice_missing_tensors.restype = C.c_int32
    L.spt_sensevoice_set_cmvn.argtypes = [vp, fp, fp, C.c_int32]
    L.spt_sensevoice_set_vocab.argtypes = [vp, C.POINTER(C.c_char_p), C.c_int32]
    L.spt_sensevoice_n_rows.argtypes = [vp, C.c_size_t]
    L.spt_sensevoice_n_rows.restype = C.c_int32
    L.spt_sensevoice_transcribe.argtypes = [vp, fp, C.c_size_t, svip, SR]
    L.spt_sensevoice_transcribe_batch.argtypes = [vp, C.POINTER(fp), C.POINTER(C.c_size_t), C.c_size_t, svip, SR]
    L.spt_sensevoice_result_free.argtypes = [C.POINTER(SvResult)]
    L.spt_sensevoice_result_free.restype = None
    L.spt_sensevoice_get_timings.argtypes = [vp, C.POINTER(SvTimings)]
    L.spt_sensevoice_debug_features.argtypes = [vp, fp, C.c_size_t, fp]
    L.spt_sensevoice_debug_encode.argtypes = [vp, fp, C.c_size_t, svip, fp]
    L.spt_sensevoice_debug_frames.argtypes = [vp, fp, C.c_size_t, svip, i32p, fp, fp]
    for fn in ("spt_sensevoice_create", "spt_sensevoice_info", "spt_sensevoice_tensor_numel", "spt_sensevoice_set_tensor",
               "spt_sensevoice_set_cmvn", "spt_sensevoice_set_vocab", "spt_sensevoice_transcribe",
               "spt_sensevoice_transcribe_batch", "spt_sensevoice_get_timings", "spt_sensevoice_debug_features",
               "spt_sensevoice_debug_encode", "spt_sensevoice_debug_frames"):
        getattr(L, fn).restype = C.c_int
    # the sampler kernels alone
    u32p, spp, i32 = C.POINTER(C.c_uint32), C.POINTER(SampleParams), C.c_int32
    L.spt_debug_sample_tokens.argtypes = [i32, i32, fp, i32, i32, i32, i32, i32, i32, i32, u32p, spp, i32p, i32p, i32p,
                                          i32p, i32p, i32, i32, i32p, i32, i32, i32, fp, fp, i32p, fp, fp, i32p, fp,
                                          u32p, C.c_char_p, C.c_size_t]
    L.spt_debug_sample_beam.argtypes = [i32, fp, i32, i32, i32, i32, i32, i32, u32p, spp, i32p, i32, i32, i32, i32p, fp,
                                        i32p, C.c_char_p, C.c_size_t]
    L.spt_debug_sample_kv_gather.argtypes = [i32, i32, fp, fp, i32p, i32, i32, i32, i32, i32, C.c_char_p, C.c_size_t]
    L.spt_debug_no_speech.argtypes = [i32, fp, i32, i32, i32, i32, fp, C.c_char_p, C.c_size_t]
    for fn in ("spt_debug_sample_tokens", "spt_debug_sample_beam", "spt_debug_sample_kv_gather", "spt_debug_no_speech"):
        getattr(L, fn).restype = C.c_int
    # the attention kernels alone
    L.spt_debug_attn_enc.argtypes = [i32, i32, fp, i32, i32, i32, fp, C.c_char_p, C.c_size_t]
    L.spt_debug_attn_self.argtypes = [i32, i32, fp, fp, i32, i32, i32, i32, i32, fp, C.c_char_p, C.c_size_t]
    L.spt_debug_attn_cross.argtypes = [i32, i32, i32, fp, fp, fp, C.c_float, i32, i32, i32, i32, i32, i32, i32, i32p,
                                       i32, fp, fp, C.c_char_p, C.c_size_t]
    L.spt_debug_xq_fused.argtypes = [i32, i32, fp, fp, fp, fp, fp, fp, fp, C.c_float, i32, i32, i32, i32, i32, fp, fp,
                                     C.c_char_p, C.c_size_t]
    L.spt_debug_attn_prefill_self.argtypes = [i32, i32, fp, fp, i32, i32, i32, i32, fp, C.c_char_p, C.c_size_t]
    L.spt_debug_attn_prefill_cross.argtypes = [i32, i32, fp, fp, fp, C.c_float, i32, i32, i32, i32, i32, i32, i32, i32p,
                                               i32, fp, C.c_char_p, C.c_size_t]
    L.spt_debug_attn_cross_quant.argtypes = [i32, i32, i32, fp, fp, fp, C.c_float, i32, i32, i32, i32, i32, i32, i32p, i32,
                                          fp, fp, fp, fp, fp, fp, C.c_char_p, C.c_size_t]
    for fn in ("spt_debug_attn_enc", "spt_debug_attn_self", "spt_debug_attn_cross", "spt_debug_xq_fused",
               "spt_debug_attn_prefill_self", "spt_debug_attn_prefill_cross", "spt_debug_attn_cross_quant"):
        getattr(L, fn).restype = C.c_int
    # the GEMM tiles and LayerNorm kernels alone
    i64 = C.c_int64
    L.spt_debug_gemm.argtypes = [i32, i32, i32, i32, i32, i32, i32, i32, fp, i64, i64, i32, i64, fp, i32, fp, fp, fp, i64,
                                 i64, i32, i64, C.c_float, i32, i64, i32, i32, i32, C.c_char_p, C.c_size_t]
    L.spt_debug_layernorm.argtypes = [i32, i32, i32, fp, i32, i32, fp, i64, i32, i64, fp, C.c_float, fp, fp, fp, fp, i32,
                                      fp, fp, C.c_char_p, C.c_size_t]
    for fn in ("spt_debug_gemm", "spt_debug_layernorm"):
        getattr(L, fn).restype = C.c_int
    L.spt_debug_qgemv.argtypes = [i32, i32, i32, C.c_void_p, C.c_size_t, i32, i32, fp, i32, fp, fp, fp, fp, i32, i32,
                                  i32, fp, fp, fp, fp, fp, C.c_char_p, C.c_size_t]
    L.spt_debug_qgemv.restype = C.c_int
    L.spt_debug_gemv.argtypes = [i32, C.POINTER(GemvDebug), C.c_char_p, C.c_size_t]
    L.spt_debug_dec_step.argtypes = [i32, C.POINTER(DecStepDebug), C.c_char_p, C.c_size_t]
    L.spt_debug_gemv.restype = L.spt_debug_dec_step.restype = C.c_int
    # the Parakeet encoder kernels alone
    L.spt_debug_pk_conv.argtypes = [i32, C.POINTER(PkConvDebug), C.c_char_p, C.c_size_t]
    L.spt_debug_pk_relpos.argtypes = [i32, i32, i32, i32, fp, i64, C.c_char_p, C.c_size_t]
    L.spt_debug_pk_rel_attn.argtypes = [i32, C.POINTER(PkAttnDebug), C.c_char_p, C.c_size_t]
    L.spt_debug_pk_tdt.argtypes = [i32, C.POINTER(PkTdtDebug), C.c_char_p, C.c_size_t]
    L.spt_debug_pk_conv.restype = L.spt_debug_pk_relpos.restype = L.spt_debug_pk_rel_attn.restype = C.c_int
    L.spt_debug_pk_tdt.restype = C.c_int
    L.spt_debug_pk_dec_stage.argtypes = [i32, C.POINTER(PkDecDebug), C.c_char_p, C.c_size_t]
    L.spt_debug_pk_dec_stage.restype = C.c_int
    L.spt_debug_pk_tdt_steps.argtypes = [i32, C.POINTER(PkStepsDebug), C.c_char_p, C.c_size_t]
    L.spt_debug_pk_tdt_steps.restype = C.c_int
    L.spt_get_weight_residency.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int32)]
    L.spt_get_weight_residency.restype = C.c_int
    # the token-alignment kernels alone
    i64p = C.POINTER(C.c_int64)
    L.spt_debug_align_qk.argtypes = [i32, i32, fp, fp, C.c_float, i32, i32, i32, i32, i32, i32, i32p, i32p, i32, i32p,
                                     i32, i32, fp, C.c_char_p, C.c_size_t]
    L.spt_debug_align_norm.argtypes = [i32, fp, i32, i32, i32, i32, i32p, i32p, fp, fp, C.c_char_p, C.c_size_t]
    L.spt_debug_align_dtw.argtypes = [i32, fp, i32, i32, i32, i32p, i32p, i32p, i32p, i32p, C.c_char_p, C.c_size_t]
    L.spt_debug_align_words.argtypes = [C.POINTER(C.c_char_p), i32p, i64p, i64p, fp, i32, i32p, i32p, i64p, i64p, fp,
                                        i32p, C.c_char_p, C.c_size_t]
    for fn in ("spt_debug_align_qk", "spt_debug_align_norm", "spt_debug_align_dtw", "spt_debug_align_words"):
        getattr(L, fn).restype = C.c_int
    # DTW token and word timestamps
    alp = C.POINTER(Alignment)
    L.spt_set_alignment_heads.argtypes = [vp, i32p, i32]
    L.spt_transcribe_aligned.argtypes = [vp, fp, C.c_size_t, C.POINTER(InferParams), C.POINTER(C.POINTER(Result)),
                                         C.POINTER(alp)]
    L.spt_transcribe_aligned_batch.argtypes = [vp, C.POINTER(fp), C.POINTER(C.c_size_t), C.c_size_t,
                                               C.POINTER(InferParams), C.POINTER(C.POINTER(Result)), C.POINTER(alp)]
    L.spt_alignment_free.argtypes = [alp]
    L.spt_alignment_free.restype = None
    L.spt_debug_align_last.argtypes = [vp, i32p, i32p, i32p, fp, C.c_size_t, fp, C.c_size_t, i32p, C.c_size_t, i32p]
    L.spt_debug_align_stats.argtypes = [vp, i32p, i32p, C.POINTER(C.c_int64)]
    for fn in ("spt_set_alignment_heads", "spt_transcribe_aligned", "spt_transcribe_aligned_batch", "spt_debug_align_last",
               "spt_debug_align_stats"):
        getattr(L, fn).restype = C.c_int
    for fn in EXPORTS:
        if fn.startswith("spt_parakeet_") and fn not in ("spt_parakeet_default_model_params",
                                                          "spt_parakeet_default_infer_params", "spt_parakeet_destroy",
                                                          "spt_parakeet_last_error", "spt_parakeet_result_free",
                                                          "spt_parakeet_onnx_tensor", "spt_parakeet_onnx_piece",
                                                          "spt_parakeet_onnx_close", "spt_parakeet_onnx_qtensor"):
            getattr(L, fn).restype = C.c_int
    for fn in ("spt_weights_arena", "spt_weights_commit", "spt_ctx_create_replicas", "spt_transcribe_batch_replicas",
               "spt_weights_export", "spt_weights_import", "spt_ctx_info", "spt_transcribe", "spt_transcribe_batch", "spt_transcribe_batch_device",
               "spt_get_timings", "spt_get_call_stats", "spt_get_xq_stats", "spt_debug_mel", "spt_debug_mel_at", "spt_debug_encode", "spt_debug_weight_checksum",
               "spt_probe_kernel", "spt_tokenize", "spt_debug_ggml_tokenize", "spt_debug_ggml_dequant"):
        getattr(L, fn).restype = C.c_int
    _lib = L
    return L
