//! Raw bindings to `include/spittle_hip.h` (ABI 14), the C boundary of the MI355X-native Whisper
//! and Parakeet-V3 backend.  One item per declaration of the header, same names, same layouts (x86-64 SysV; the
//! layouts are checked field by field against gcc by tests/test_capi.py).  Safe wrappers live in
//! the `spittle-hip` crate.
#![allow(non_camel_case_types)]

use std::os::raw::{c_char, c_int, c_void};

pub const SPT_ABI_VERSION: c_int = 14;
pub const SPT_PK_STAGE_COUNT: c_int = 9;

pub type spt_status = c_int;
pub const SPT_OK: spt_status = 0;
pub const SPT_ERR_INVALID_ARG: spt_status = 1;
pub const SPT_ERR_LOAD: spt_status = 2;
pub const SPT_ERR_DEVICE: spt_status = 3;
pub const SPT_ERR_OOM: spt_status = 4;
pub const SPT_ERR_UNSUPPORTED: spt_status = 5;
pub const SPT_ERR_INTERNAL: spt_status = 6;

pub type spt_dtype = c_int;
pub const SPT_DTYPE_F32: spt_dtype = 0;
pub const SPT_DTYPE_BF16: spt_dtype = 1;
/// Parakeet's default; ABI 14: also `spt_model_params.dtype`, the Whisper fp16 engine
pub const SPT_DTYPE_F16: spt_dtype = 2;
/// ABI 13, `spt_pk_model_params.dtype` only: the int8 ONNX export's own arithmetic
pub const SPT_DTYPE_I8: spt_dtype = 3;
/// `mode` of `spt_debug_attn_cross`
pub const SPT_ATTN_CROSS_8WAVE: i32 = 0;
pub const SPT_ATTN_CROSS_VW: i32 = 1;
pub const SPT_ATTN_CROSS_VW_PQ: i32 = 2;
pub const SPT_ATTN_CROSS_VW_MERGE: i32 = 3;
pub const SPT_ATTN_CROSS_VW_PQ_MERGE: i32 = 4;
/// `spt_debug_qgemv`: the ggml types with a resident layout, the GEMV modes and A sources
pub const SPT_GGML_Q4_1: i32 = 3;
pub const SPT_GGML_Q5_0: i32 = 6;
pub const SPT_GGML_Q5_1: i32 = 7;
pub const SPT_GV_BIAS: i32 = 0;
pub const SPT_GV_BIAS_GELU: i32 = 1;
pub const SPT_GV_PARTIAL: i32 = 2;
pub const SPT_GV_QKV_CACHE: i32 = 3;
pub const SPT_GV_LOGITS: i32 = 4;
pub const SPT_GV_BIAS_RESID: i32 = 5;
pub const SPT_QGEMV_A_DIRECT: i32 = 0;
pub const SPT_QGEMV_A_LN: i32 = 1;
/// `a_src` of `spt_gemv_debug` and `op` of `spt_dec_step_debug` (SPT_HAS_GEMV_KERNELS)
pub const SPT_GEMV_A_DIRECT: i32 = 0;
pub const SPT_GEMV_A_LN: i32 = 1;
pub const SPT_GEMV_A_ATTN: i32 = 2;
pub const SPT_DEC_STEP_EMBED: i32 = 0;
pub const SPT_DEC_STEP_FINALIZE: i32 = 1;
pub const SPT_DEC_STEP_ADVANCE: i32 = 2;
pub const SPT_DEC_STEP_RESET: i32 = 3;
/// `spt_pk_act` of `spt_parakeet_debug_qgemm`
pub const SPT_PK_ACT_NONE: i32 = 0;
pub const SPT_PK_ACT_RELU: i32 = 1;
pub const SPT_PK_ACT_SWISH: i32 = 2;

pub const SPT_SUPPRESS_BLANK: u32 = 1;
pub const SPT_NO_TIMESTAMPS: u32 = 2;
pub const SPT_IGNORE_EOT: u32 = 4;
pub const SPT_SUPPRESS_NST: u32 = 8;
/// report each window's no-speech probability without skipping (SPT_HAS_NO_SPEECH)
pub const SPT_NO_SPEECH_PROB: u32 = 16;
/// the prompt prefix in one block pass per sequence slice instead of chunks of 4 (SPT_HAS_BLOCK_PREFILL)
pub const SPT_BLOCK_PREFILL: u32 = 32;

pub const SPT_MODEL_WEIGHTS_EXTERNAL: u32 = 1;
/// quantised decoder matrices of a ggml file stay resident in their blocks (SPT_HAS_QUANT_RESIDENT)
pub const SPT_MODEL_QUANT_RESIDENT: u32 = 2;
/// the cross K/V cache in fp8 e4m3 with one f32 scale per key row (SPT_HAS_CROSS_KV_F8)
pub const SPT_MODEL_CROSS_KV_F8: u32 = 4;

/// the arguments of `spt_debug_gemv` (one decoder GEMV launch on caller-supplied arrays)
#[repr(C)]
#[allow(non_snake_case)]
#[derive(Clone, Copy, Debug)]
pub struct spt_gemv_debug {
    pub W: *const f32,
    pub A: *const f32,
    pub ln_w: *const f32,
    pub ln_b: *const f32,
    pub pend: *const f32,
    pub x_out: *mut f32,
    pub apart: *const f32,
    pub out_merged: *mut f32,
    pub bias: *const f32,
    pub C: *mut f32,
    pub p_resid: *const f32,
    pub cache: *mut f32,
    pub suppress: *const u32,
    pub part: *mut f32,
    pub plan: *mut i32,
    pub a_count: i64,
    pub c_count: i64,
    pub c_split: i64,
    pub suppress_words: i64,
    pub dtype: i32,
    pub mode: i32,
    pub a_src: i32,
    pub R: i32,
    pub N: i32,
    pub K: i32,
    pub lda: i32,
    pub a_row0: i32,
    pub n_pend: i32,
    pub S: i32,
    pub H: i32,
    pub merge_first: i32,
    pub ldc: i32,
    pub ksplit: i32,
    pub B: i32,
    pub Tq: i32,
    pub cache_H: i32,
    pub ctx: i32,
    pub pos0: i32,
    pub blank0: i32,
    pub blank1: i32,
    pub step: i32,
    pub n_tiles: i32,
    pub reserved0: i32,
}

/// the arguments of `spt_debug_dec_step` (dec_embed / dec_finalize / dec_advance / dec_reset alone)
#[repr(C)]
#[allow(non_snake_case)]
#[derive(Clone, Copy, Debug)]
pub struct spt_dec_step_debug {
    pub tok: *const i32,
    pub part: *const f32,
    pub forced: *const i32,
    pub done: *mut i32,
    pub emb: *const f32,
    pub emb_blocks: *const c_void,
    pub pos: *const f32,
    pub state: *mut i32,
    pub next_tok: *mut i32,
    pub x: *mut f32,
    pub out_tok: *mut i32,
    pub out_top1: *mut f32,
    pub out_top2: *mut f32,
    pub emb_blocks_bytes: usize,
    pub dtype: i32,
    pub op: i32,
    pub B: i32,
    pub Tq: i32,
    pub d: i32,
    pub ctx: i32,
    pub n_vocab: i32,
    pub n_tiles: i32,
    pub n_steps: i32,
    pub forced_len: i32,
    pub ignore_eot: i32,
    pub out_cap: i32,
    pub eot: i32,
    pub emb_q: i32,
    pub n_advance: i32,
    pub reserved0: i32,
}

/// `spt_debug_pk_conv` modes and `spt_debug_pk_rel_attn` variants (SPT_HAS_PK_KERNELS)
pub const SPT_PK_CONV0: i32 = 0;
pub const SPT_PK_DWCONV1: i32 = 1;
pub const SPT_PK_DWCONV2: i32 = 2;
pub const SPT_PK_CONV_MODULE: i32 = 3;
pub const SPT_PK_ATTN_AUTO: i32 = 0;
pub const SPT_PK_ATTN_VALU: i32 = 1;
pub const SPT_PK_ATTN_MFMA: i32 = 2;

/// the arguments of `spt_debug_pk_conv` (one Parakeet subsampling or convolution-module launch)
#[repr(C)]
#[allow(non_snake_case)]
#[derive(Clone, Copy, Debug)]
pub struct spt_pk_conv_debug {
    pub x: *const f32,
    pub lens: *const i32,
    pub w: *const f32,
    pub bias: *const f32,
    pub bn_g: *const f32,
    pub bn_b: *const f32,
    pub bn_m: *const f32,
    pub bn_v: *const f32,
    pub y: *mut f32,
    pub y_count: i64,
    pub dtype: i32,
    pub mode: i32,
    pub B: i32,
    pub Tp: i32,
    pub F: i32,
    pub C: i32,
}

/// the arguments of `spt_debug_pk_rel_attn` (one Parakeet rel-pos attention launch)
#[repr(C)]
#[allow(non_snake_case)]
#[derive(Clone, Copy, Debug)]
pub struct spt_pk_attn_debug {
    pub qkv: *const f32,
    pub p: *const f32,
    pub pu: *const f32,
    pub pv: *const f32,
    pub lens: *const i32,
    pub out: *mut f32,
    pub p_count: i64,
    pub p_off: i64,
    pub p_bstride: i64,
    pub out_count: i64,
    pub dtype: i32,
    pub variant: i32,
    pub B: i32,
    pub Tp: i32,
    pub H: i32,
    pub dk: i32,
    pub ldp: i32,
    pub reserved0: i32,
}

/// `mode` of `spt_debug_pk_dec_stage`
pub const SPT_PK_DEC_LSTM: i32 = 0;
pub const SPT_PK_DEC_PRED: i32 = 1;
pub const SPT_PK_DEC_JOINT: i32 = 2;

/// the arguments of `spt_debug_pk_dec_stage` (one pk_decode_stage launch on plain weights)
#[repr(C)]
#[allow(non_snake_case)]
#[derive(Clone, Copy, Debug)]
pub struct spt_pk_dec_debug {
    pub W: *const f32,
    pub W2: *const f32,
    pub b0: *const f32,
    pub b1: *const f32,
    pub state: *const i32,
    pub xin: *const f32,
    pub h_in: *const f32,
    pub c_in: *const f32,
    pub fe: *const f32,
    pub gp: *mut f32,
    pub h_out: *mut f32,
    pub c_out: *mut f32,
    pub part: *mut f32,
    pub dur: *mut f32,
    pub mode: i32,
    pub B: i32,
    pub P: i32,
    pub V: i32,
    pub n_dur: i32,
    pub reserved0: i32,
}

/// the arguments of `spt_debug_pk_tdt_steps` (pk_state_init, then whole decode steps on plain weights)
#[repr(C)]
#[allow(non_snake_case)]
#[derive(Clone, Copy, Debug)]
pub struct spt_pk_steps_debug {
    pub lstm: [[*const f32; 4]; 2],
    pub pred_w: *const f32,
    pub pred_b: *const f32,
    pub joint_w: *const f32,
    pub joint_b: *const f32,
    pub emb: *const f32,
    pub fe: *const f32,
    pub lens: *const i32,
    pub state: *mut i32,
    pub out_tok: *mut i32,
    pub out_frame: *mut i32,
    pub out_t1: *mut f32,
    pub out_t2: *mut f32,
    pub B: i32,
    pub P: i32,
    pub V: i32,
    pub n_dur: i32,
    pub n_steps: i32,
    pub max_symbols: i32,
    pub cap: i32,
    pub T3p: i32,
}

/// the arguments of `spt_debug_pk_tdt` (pk_state_init, then pk_joint_fin per step on given partials)
#[repr(C)]
#[allow(non_snake_case)]
#[derive(Clone, Copy, Debug)]
pub struct spt_pk_tdt_debug {
    pub part: *const f32,
    pub dur: *const f32,
    pub lens: *const i32,
    pub emb: *const f32,
    pub fe: *const f32,
    pub state: *mut i32,
    pub xemb: *mut f32,
    pub fecur: *mut f32,
    pub out_tok: *mut i32,
    pub out_frame: *mut i32,
    pub out_t1: *mut f32,
    pub out_t2: *mut f32,
    pub B: i32,
    pub P: i32,
    pub V: i32,
    pub n_dur: i32,
    pub n_tiles: i32,
    pub n_steps: i32,
    pub max_symbols: i32,
    pub cap: i32,
    pub T3p: i32,
    pub reserved0: i32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct spt_model_params {
    pub dtype: i32,
    pub device: i32,
    pub max_batch: i32,
    pub flags: u32,
    pub seed: u64,
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct spt_infer_params {
    pub language: *const c_char,
    pub translate: i32,
    pub initial_prompt: *const c_char,
    pub flags: u32,
    pub max_new_tokens: i32,
    pub temperature: f32,
    pub beam_size: i32,
    pub forced_tokens: *const i32,
    pub n_forced: i32,
    pub prompt_tokens: *const i32,
    pub n_prompt_tokens: i32,
    pub temperature_inc: f32,
    pub best_of: i32,
    pub entropy_thold: f32,
    pub logprob_thold: f32,
    pub max_initial_ts: f32,
    /// the silence skip's threshold (the formerly reserved int32 slot): on iff 0 < value < 1, 0 = off
    pub no_speech_thold: f32,
    pub seed: u64,
}

/// one window of the last `spt_transcribe*` call (`spt_get_window_info`, SPT_HAS_NO_SPEECH)
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct spt_window_info {
    pub utterance: i32,
    pub seek: i32,
    pub seek_delta: i32,
    pub i0: i32,
    pub n_tokens: i32,
    pub n_fallbacks: i32,
    pub temperature: f32,
    pub avg_logprob: f32,
    pub no_speech_prob: f32,
    pub skipped: i32,
}

#[repr(C)]
#[derive(Debug)]
pub struct spt_segment {
    pub t0: i64,
    pub t1: i64,
    pub text: *mut c_char,
    pub i0: i32,
    pub n_tokens: i32,
}

#[repr(C)]
#[derive(Debug)]
pub struct spt_result {
    pub text: *mut c_char,
    pub tokens: *mut i32,
    pub top1: *mut f32,
    pub top2: *mut f32,
    pub n_tokens: i32,
    pub n_windows: i32,
    pub language: i32,
    pub n_segments: i32,
    pub segments: *mut spt_segment,
    pub n_fallbacks: i32,
    pub reserved0: i32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct spt_model_info {
    pub n_mels: i32,
    pub d: i32,
    pub n_head: i32,
    pub n_enc: i32,
    pub n_dec: i32,
    pub n_vocab: i32,
    pub n_audio_ctx: i32,
    pub n_text_ctx: i32,
    pub dtype: i32,
    pub max_batch: i32,
    pub weight_bytes: i64,
    pub workspace_bytes: i64,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct spt_call_stats {
    pub engine_calls: i32,
    pub decoder_passes: i32,
    pub beam_steps: i32,
    /// ABI 11: 30 s windows encoded (one per window, shared by fallbacks and decoders)
    pub encoder_windows: i32,
    pub device_ms: f64,
    pub encoder_ms: f64,
    pub decode_ms: f64,
    /// ABI 12: always 0 (the persistent decoder pass was deleted in round 6)
    pub pd_passes: i32,
    /// ABI 12: always 0
    pub pd_fallbacks: i32,
}

/// decoding parameters of the `spt_debug_sample_*` test hooks
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct spt_sample_params {
    pub temperature: f32,
    pub suppress_blank: i32,
    pub no_ts: i32,
    pub max_initial: i32,
    pub n_max: i32,
    pub max_tokens: i32,
    pub seed: u64,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct spt_timings {
    pub mel_ms: f64,
    pub encoder_ms: f64,
    pub cross_kv_ms: f64,
    pub decode_ms: f64,
    pub total_ms: f64,
    pub h2d_ms: f64,
    pub n_decode_passes: i32,
    pub batch: i32,
}

/// Opaque context (one loaded model on one device).
#[repr(C)]
pub struct spt_ctx {
    _private: [u8; 0],
}

pub type spt_probe_kind = c_int;
pub const SPT_PROBE_DEC_CROSS_ATTN: spt_probe_kind = 0;
pub const SPT_PROBE_DEC_SELF_ATTN: spt_probe_kind = 1;
pub const SPT_PROBE_DEC_LOGITS: spt_probe_kind = 2;
pub const SPT_PROBE_DEC_FC1: spt_probe_kind = 3;
pub const SPT_PROBE_ENC_FC1_GEMM: spt_probe_kind = 4;
pub const SPT_PROBE_ENC_ATTN: spt_probe_kind = 5;

extern "C" {
    pub fn spt_version() -> *const c_char;
    pub fn spt_default_model_params(p: *mut spt_model_params);
    pub fn spt_default_infer_params(p: *mut spt_infer_params);

    pub fn spt_ctx_create(
        model_spec: *const c_char,
        params: *const spt_model_params,
        out: *mut *mut spt_ctx,
        err: *mut c_char,
        errlen: usize,
    ) -> spt_status;
    pub fn spt_ctx_destroy(ctx: *mut spt_ctx);
    pub fn spt_last_error(ctx: *const spt_ctx) -> *const c_char;
    pub fn spt_ctx_info(ctx: *const spt_ctx, info: *mut spt_model_info) -> spt_status;

    pub fn spt_transcribe(
        ctx: *mut spt_ctx,
        pcm16k: *const f32,
        n_samples: usize,
        params: *const spt_infer_params,
        out: *mut *mut spt_result,
    ) -> spt_status;
    pub fn spt_transcribe_batch(
        ctx: *mut spt_ctx,
        pcm: *const *const f32,
        n_samples: *const usize,
        batch: usize,
        params: *const spt_infer_params,
        out: *mut *mut spt_result,
    ) -> spt_status;
    pub fn spt_transcribe_batch_device(
        ctx: *mut spt_ctx,
        pcm_dev: *const f32,
        stride: usize,
        n_samples: *const usize,
        batch: usize,
        params: *const spt_infer_params,
        out: *mut *mut spt_result,
    ) -> spt_status;
    pub fn spt_result_free(r: *mut spt_result);
    pub fn spt_language_code(lang_id: i32) -> *const c_char;

    pub fn spt_tokenize(
        ctx: *mut spt_ctx,
        text: *const c_char,
        tokens: *mut i32,
        n_max: i32,
        n_out: *mut i32,
    ) -> spt_status;
    pub fn spt_token_to_str(ctx: *const spt_ctx, id: i32) -> *const c_char;

    pub fn spt_get_timings(ctx: *const spt_ctx, t: *mut spt_timings) -> spt_status;
    // ---- ABI 9: the whole last call (every window, fallback and beam step)
    pub fn spt_get_call_stats(ctx: *const spt_ctx, s: *mut spt_call_stats) -> spt_status;
    // additive to ABI 14: fused cross-Q + cross-attention launches and chain reruns of the last call
    pub fn spt_get_xq_stats(ctx: *const spt_ctx, fused_launches: *mut i32, fallbacks: *mut i32) -> spt_status;
    // block prefill of the prompt prefix (SPT_HAS_BLOCK_PREFILL, additive over ABI 14): the last call's
    // block passes, the prefix rows they carried, and its chunked prefill passes
    pub fn spt_get_prefill_stats(ctx: *const spt_ctx, block_passes: *mut i32, block_rows: *mut i32, chunk_passes: *mut i32) -> spt_status;
    // the fp8 cross K/V cache (SPT_HAS_CROSS_KV_F8, additive over ABI 14): its format (0 engine dtype, 1 e4m3 +
    // row scales) and bytes, one (layer, window) of it as f32, and its kernels alone
    pub fn spt_get_cross_kv_info(ctx: *const spt_ctx, format: *mut i32, cache_bytes: *mut i64, staging_bytes: *mut i64) -> spt_status;
    pub fn spt_debug_cross_kv(ctx: *mut spt_ctx, layer: i32, window: i32, k: *mut f32, v: *mut f32) -> spt_status;
    pub fn spt_debug_attn_cross_quant(
        device: i32,
        dtype: i32,
        mode: i32,
        q: *const f32,
        k: *const f32,
        v: *const f32,
        pad_value: f32,
        b: i32,
        b_layout: i32,
        b0: i32,
        h: i32,
        t_enc: i32,
        tq: i32,
        kvrow: *const i32,
        share: i32,
        kq: *mut f32,
        vq: *mut f32,
        k_scale: *mut f32,
        v_scale: *mut f32,
        out: *mut f32,
        part: *mut f32,
        err: *mut c_char,
        errlen: usize,
    ) -> spt_status;
    // the block prefill's attention kernels alone (cache: in and out)
    pub fn spt_debug_attn_prefill_self(
        device: i32,
        dtype: i32,
        qkv: *const f32,
        cache: *mut f32,
        B: i32,
        H: i32,
        ctx: i32,
        P: i32,
        out: *mut f32,
        err: *mut c_char,
        errlen: usize,
    ) -> spt_status;
    pub fn spt_debug_attn_prefill_cross(
        device: i32,
        dtype: i32,
        q: *const f32,
        k: *const f32,
        v: *const f32,
        pad_value: f32,
        B: i32,
        B_layout: i32,
        b0: i32,
        H: i32,
        T_enc: i32,
        P: i32,
        ctx: i32,
        kvrow: *const i32,
        share: i32,
        out: *mut f32,
        err: *mut c_char,
        errlen: usize,
    ) -> spt_status;
    // the no-speech probability and the silence skip (SPT_HAS_NO_SPEECH, additive over ABI 14)
    pub fn spt_get_window_info(ctx: *const spt_ctx, out: *mut spt_window_info, cap: i32, n: *mut i32) -> spt_status;
    pub fn spt_debug_no_speech(
        device: i32,
        logits: *const f32,
        B: i32,
        n_vocab: i32,
        ldl: i32,
        nosp: i32,
        prob: *mut f32,
        err: *mut c_char,
        errlen: usize,
    ) -> spt_status;

    pub fn spt_weights_export(ctx: *mut spt_ctx, dev_dst: *mut c_void, bytes: usize) -> spt_status;
    pub fn spt_weights_import(ctx: *mut spt_ctx, dev_src: *const c_void, bytes: usize) -> spt_status;
    pub fn spt_weights_arena(ctx: *mut spt_ctx, dev_ptr: *mut *mut c_void, bytes: *mut usize) -> spt_status;
    pub fn spt_weights_commit(ctx: *mut spt_ctx) -> spt_status;

    pub fn spt_ctx_create_replicas(
        model_spec: *const c_char,
        params: *const spt_model_params,
        devices: *const i32,
        n_devices: i32,
        out: *mut *mut spt_ctx,
        bcast_ms: *mut f64,
        err: *mut c_char,
        errlen: usize,
    ) -> spt_status;
    pub fn spt_transcribe_batch_replicas(
        ctxs: *const *mut spt_ctx,
        n_ctx: i32,
        pcm: *const *const f32,
        n_samples: *const usize,
        batch: usize,
        params: *const spt_infer_params,
        out: *mut *mut spt_result,
    ) -> spt_status;

    pub fn spt_probe_kernel(
        ctx: *mut spt_ctx,
        kind: i32,
        iters: i32,
        avg_us: *mut f64,
        work: *mut f64,
        work_is_flops: *mut i32,
    ) -> spt_status;

    pub fn spt_debug_mel(ctx: *mut spt_ctx, pcm16k: *const f32, n_samples: usize, out: *mut f32) -> spt_status;
    pub fn spt_debug_mel_at(ctx: *mut spt_ctx, pcm16k: *const f32, n_samples: usize, seek: i32, out: *mut f32) -> spt_status;
    pub fn spt_debug_encode(ctx: *mut spt_ctx, mel: *const f32, out: *mut f32) -> spt_status;
    pub fn spt_debug_weight_checksum(ctx: *mut spt_ctx, tensor_id: i32, out2: *mut f64) -> spt_status;
    pub fn spt_debug_ggml_tokenize(
        model_path: *const c_char,
        text: *const c_char,
        tokens: *mut i32,
        n_max: i32,
        n_out: *mut i32,
    ) -> spt_status;
    pub fn spt_debug_ggml_dequant(ggml_type: i32, src: *const c_void, n: i64, dst: *mut f32) -> spt_status;
    // the sampler kernels alone (test hooks, additive over ABI 14)
    pub fn spt_debug_sample_tokens(
        device: i32,
        dtype: i32,
        logits: *const f32,
        n_steps: i32,
        b: i32,
        n_vocab: i32,
        ldl: i32,
        eot: i32,
        beg: i32,
        blank: i32,
        suppress: *const u32,
        prm: *const spt_sample_params,
        seek: *const i32,
        seek_end: *const i32,
        state: *mut i32,
        done: *mut i32,
        forced: *const i32,
        forced_len: i32,
        out_cap: i32,
        dec_state: *mut i32,
        tq: i32,
        d: i32,
        ctx: i32,
        emb: *const f32,
        pos: *const f32,
        out_tok: *mut i32,
        out_plog: *mut f32,
        out_tid: *mut f32,
        next_tok: *mut i32,
        x: *mut f32,
        arrive: *mut u32,
        err: *mut c_char,
        errlen: usize,
    ) -> spt_status;
    pub fn spt_debug_sample_beam(
        device: i32,
        logits: *const f32,
        b: i32,
        n_vocab: i32,
        ldl: i32,
        eot: i32,
        beg: i32,
        blank: i32,
        suppress: *const u32,
        prm: *const spt_sample_params,
        row: *const i32,
        step: i32,
        k: i32,
        chunked: i32,
        cand_id: *mut i32,
        cand_lp: *mut f32,
        tid: *mut i32,
        err: *mut c_char,
        errlen: usize,
    ) -> spt_status;
    pub fn spt_debug_sample_kv_gather(
        device: i32,
        dtype: i32,
        src: *const f32,
        dst: *mut f32,
        rows: *const i32,
        l: i32,
        b: i32,
        h: i32,
        ctx: i32,
        pos0: i32,
        err: *mut c_char,
        errlen: usize,
    ) -> spt_status;
    // the attention kernels alone (test hooks, additive over ABI 14); mode: SPT_ATTN_CROSS_*
    pub fn spt_debug_attn_enc(
        device: i32,
        dtype: i32,
        qkv: *const f32,
        b: i32,
        t: i32,
        h: i32,
        out: *mut f32,
        err: *mut c_char,
        errlen: usize,
    ) -> spt_status;
    pub fn spt_debug_attn_self(
        device: i32,
        dtype: i32,
        q: *const f32,
        cache: *const f32,
        b: i32,
        h: i32,
        ctx: i32,
        tq: i32,
        pos0: i32,
        out: *mut f32,
        err: *mut c_char,
        errlen: usize,
    ) -> spt_status;
    pub fn spt_debug_attn_cross(
        device: i32,
        dtype: i32,
        mode: i32,
        q: *const f32,
        k: *const f32,
        v: *const f32,
        pad_value: f32,
        b: i32,
        b_layout: i32,
        b0: i32,
        h: i32,
        t_enc: i32,
        tq: i32,
        splits: i32,
        kvrow: *const i32,
        share: i32,
        out: *mut f32,
        part: *mut f32,
        err: *mut c_char,
        errlen: usize,
    ) -> spt_status;
    // the fused cross-Q + cross-attention launch alone (lds: 0..2 staged blocks, touch: 0 or 2)
    pub fn spt_debug_xq_fused(
        device: i32,
        dtype: i32,
        x: *const f32,
        ln_w: *const f32,
        ln_b: *const f32,
        wq: *const f32,
        bias: *const f32,
        k: *const f32,
        v: *const f32,
        pad_value: f32,
        b: i32,
        h: i32,
        t_enc: i32,
        lds: i32,
        touch: i32,
        q: *mut f32,
        out: *mut f32,
        err: *mut c_char,
        errlen: usize,
    ) -> spt_status;
    // the GEMM tiles and LayerNorm kernels alone (test hooks, additive over ABI 14); mode: SPT_LN_*
    pub fn spt_debug_gemm(
        device: i32,
        dtype: i32,
        epi: i32,
        variant: i32,
        batch: i32,
        m: i32,
        n: i32,
        k: i32,
        a: *const f32,
        a_count: i64,
        a_off: i64,
        lda: i32,
        s_a: i64,
        w: *const f32,
        ldw: i32,
        bias: *const f32,
        pos: *const f32,
        c: *mut f32,
        c_count: i64,
        c_off: i64,
        ldc: i32,
        s_c: i64,
        alpha: f32,
        ksplit: i32,
        c_split: i64,
        kv_b: i32,
        kv_t: i32,
        kv_h: i32,
        err: *mut c_char,
        errlen: usize,
    ) -> spt_status;
    pub fn spt_debug_layernorm(
        device: i32,
        dtype: i32,
        mode: i32,
        x: *mut f32,
        m: i32,
        d: i32,
        slab: *const f32,
        slab_count: i64,
        ks: i32,
        slab_stride: i64,
        pbias: *const f32,
        alpha: f32,
        w: *const f32,
        b: *const f32,
        w2: *const f32,
        b2: *const f32,
        write_x: i32,
        y: *mut f32,
        y2: *mut f32,
        err: *mut c_char,
        errlen: usize,
    ) -> spt_status;
    // DTW token and word timestamps (SPT_HAS_TOKEN_TIMESTAMPS, additive over ABI 14)
    pub fn spt_set_alignment_heads(ctx: *mut spt_ctx, layer_head: *const i32, n_pairs: i32) -> spt_status;
    pub fn spt_transcribe_aligned(
        ctx: *mut spt_ctx,
        pcm16k: *const f32,
        n_samples: usize,
        params: *const spt_infer_params,
        out: *mut *mut spt_result,
        align: *mut *mut spt_alignment,
    ) -> spt_status;
    pub fn spt_transcribe_aligned_batch(
        ctx: *mut spt_ctx,
        pcm: *const *const f32,
        n_samples: *const usize,
        batch: usize,
        params: *const spt_infer_params,
        out: *mut *mut spt_result,
        align: *mut *mut spt_alignment,
    ) -> spt_status;
    pub fn spt_alignment_free(a: *mut spt_alignment);
    pub fn spt_debug_align_stats(
        ctx: *mut spt_ctx,
        replay_passes: *mut i32,
        n_heads: *mut i32,
        workspace_bytes: *mut i64,
    ) -> spt_status;
    pub fn spt_debug_align_last(
        ctx: *mut spt_ctx,
        n_heads: *mut i32,
        n_rows: *mut i32,
        n_keys: *mut i32,
        p: *mut f32,
        p_cap: usize,
        m: *mut f32,
        m_cap: usize,
        path: *mut i32,
        path_cap: usize,
        path_len: *mut i32,
    ) -> spt_status;
    // the token-alignment kernels alone (SPT_HAS_ALIGN_KERNELS, additive over ABI 14)
    pub fn spt_debug_align_qk(
        device: i32,
        dtype: i32,
        q: *const f32,
        k: *const f32,
        pad_value: f32,
        b: i32,
        b_layout: i32,
        h: i32,
        t_enc: i32,
        tq: i32,
        pos0: i32,
        kvrow: *const i32,
        heads: *const i32,
        n_heads: i32,
        m: *const i32,
        n_cap: i32,
        m_cap: i32,
        p: *mut f32,
        err: *mut c_char,
        errlen: usize,
    ) -> spt_status;
    pub fn spt_debug_align_norm(
        device: i32,
        p: *const f32,
        b: i32,
        a: i32,
        n_cap: i32,
        m_cap: i32,
        n: *const i32,
        m: *const i32,
        stat: *mut f32,
        m_out: *mut f32,
        err: *mut c_char,
        errlen: usize,
    ) -> spt_status;
    pub fn spt_debug_align_dtw(
        device: i32,
        m: *const f32,
        b: i32,
        n_cap: i32,
        m_cap: i32,
        n: *const i32,
        m_len: *const i32,
        jump: *mut i32,
        len: *mut i32,
        path: *mut i32,
        err: *mut c_char,
        errlen: usize,
    ) -> spt_status;
    pub fn spt_debug_align_words(
        pieces: *const *const c_char,
        piece_len: *const i32,
        t0: *const i64,
        t1: *const i64,
        p: *const f32,
        n: i32,
        word_i0: *mut i32,
        word_n: *mut i32,
        word_t0: *mut i64,
        word_t1: *mut i64,
        word_p: *mut f32,
        n_words: *mut i32,
        err: *mut c_char,
        errlen: usize,
    ) -> spt_status;
    pub fn spt_get_weight_residency(
        ctx: *const spt_ctx,
        resident_weights: *mut i64,
        resident_bytes: *mut i64,
        ggml_type: *mut i32,
    ) -> spt_status;
    // the decoder GEMV alone over one quantised matrix, expanded and packed (SPT_HAS_QUANT_RESIDENT)
    pub fn spt_debug_qgemv(
        device: i32,
        dtype: i32,
        ggml_type: i32,
        blocks: *const c_void,
        blocks_bytes: usize,
        n: i32,
        k: i32,
        act: *const f32,
        r: i32,
        ln_w: *const f32,
        ln_b: *const f32,
        bias: *const f32,
        resid: *const f32,
        mode: i32,
        a_src: i32,
        ksplit: i32,
        out_plain: *mut f32,
        out_packed: *mut f32,
        top_plain: *mut f32,
        top_packed: *mut f32,
        unpacked: *mut f32,
        err: *mut c_char,
        errlen: usize,
    ) -> spt_status;

    // the decoder GEMV and the step's small kernels alone (SPT_HAS_GEMV_KERNELS)
    pub fn spt_debug_gemv(device: i32, args: *const spt_gemv_debug, err: *mut c_char, errlen: usize) -> spt_status;
    pub fn spt_debug_dec_step(
        device: i32,
        args: *const spt_dec_step_debug,
        err: *mut c_char,
        errlen: usize,
    ) -> spt_status;

    // the Parakeet encoder kernels and the TDT bookkeeping alone (SPT_HAS_PK_KERNELS)
    pub fn spt_debug_pk_conv(device: i32, args: *const spt_pk_conv_debug, err: *mut c_char, errlen: usize) -> spt_status;
    pub fn spt_debug_pk_relpos(
        device: i32,
        dtype: i32,
        Tp: i32,
        d: i32,
        pe: *mut f32,
        pe_count: i64,
        err: *mut c_char,
        errlen: usize,
    ) -> spt_status;
    pub fn spt_debug_pk_rel_attn(device: i32, args: *const spt_pk_attn_debug, err: *mut c_char, errlen: usize) -> spt_status;

    pub fn spt_debug_pk_tdt(device: i32, args: *const spt_pk_tdt_debug, err: *mut c_char, errlen: usize) -> spt_status;
    pub fn spt_debug_pk_tdt_steps(device: i32, args: *const spt_pk_steps_debug, err: *mut c_char, errlen: usize) -> spt_status;
    pub fn spt_debug_pk_dec_stage(device: i32, args: *const spt_pk_dec_debug, err: *mut c_char, errlen: usize) -> spt_status;

    // ---- ABI 6: Parakeet-V3
    pub fn spt_parakeet_default_model_params(p: *mut spt_pk_model_params);
    pub fn spt_parakeet_default_infer_params(p: *mut spt_pk_infer_params);
    pub fn spt_parakeet_create(
        model_spec: *const c_char,
        params: *const spt_pk_model_params,
        out: *mut *mut spt_pk_ctx,
        err: *mut c_char,
        errlen: usize,
    ) -> spt_status;
    pub fn spt_parakeet_destroy(ctx: *mut spt_pk_ctx);
    pub fn spt_parakeet_last_error(ctx: *const spt_pk_ctx) -> *const c_char;
    pub fn spt_parakeet_info(ctx: *const spt_pk_ctx, info: *mut spt_pk_model_info) -> spt_status;
    pub fn spt_parakeet_tensor_numel(ctx: *const spt_pk_ctx, tensor_id: i32, n: *mut i64) -> spt_status;
    pub fn spt_parakeet_set_tensor(ctx: *mut spt_pk_ctx, tensor_id: i32, data: *const f32, n: i64) -> spt_status;
    pub fn spt_parakeet_set_vocab(ctx: *mut spt_pk_ctx, pieces: *const *const c_char, n: i32) -> spt_status;
    pub fn spt_parakeet_transcribe(
        ctx: *mut spt_pk_ctx,
        pcm16k: *const f32,
        n_samples: usize,
        params: *const spt_pk_infer_params,
        out: *mut *mut spt_pk_result,
    ) -> spt_status;
    pub fn spt_parakeet_transcribe_batch(
        ctx: *mut spt_pk_ctx,
        pcm: *const *const f32,
        n_samples: *const usize,
        batch: usize,
        params: *const spt_pk_infer_params,
        out: *mut *mut spt_pk_result,
    ) -> spt_status;
    pub fn spt_parakeet_transcribe_batch_device(
        ctx: *mut spt_pk_ctx,
        pcm_dev: *const f32,
        stride: usize,
        n_samples: *const usize,
        batch: usize,
        params: *const spt_pk_infer_params,
        out: *mut *mut spt_pk_result,
    ) -> spt_status;
    pub fn spt_parakeet_result_free(r: *mut spt_pk_result);
    pub fn spt_parakeet_get_timings(ctx: *const spt_pk_ctx, t: *mut spt_pk_timings) -> spt_status;
    // ---- ABI 10: encoder stage profile (ms[SPT_PK_STAGE_COUNT], spt_pk_stage order)
    pub fn spt_parakeet_profile_encoder(ctx: *mut spt_pk_ctx, iters: i32, ms: *mut f64, n: i32) -> spt_status;
    pub fn spt_parakeet_debug_mel(ctx: *mut spt_pk_ctx, pcm16k: *const f32, n_samples: usize, out: *mut f32) -> spt_status;
    pub fn spt_parakeet_debug_encode(ctx: *mut spt_pk_ctx, mel: *const f32, t: i32, out: *mut f32) -> spt_status;
    pub fn spt_parakeet_debug_last_encoder(ctx: *mut spt_pk_ctx, b: i32, out: *mut f32, t3: *mut i32) -> spt_status;
    pub fn spt_parakeet_debug_decode(
        ctx: *mut spt_pk_ctx,
        enc: *const f32,
        t3: i32,
        max_symbols: i32,
        out: *mut *mut spt_pk_result,
    ) -> spt_status;
    pub fn spt_parakeet_debug_weight_checksum(ctx: *mut spt_pk_ctx, tensor_id: i32, out2: *mut f64) -> spt_status;
    // ---- ABI 13: test hooks of the int8 mode (SPT_DTYPE_I8)
    pub fn spt_parakeet_debug_qgemm(
        device: i32,
        a: *const f32,
        m: i32,
        k: i32,
        group_len: *const i32,
        n_groups: i32,
        w: *const i16,
        n: i32,
        w_scales: *const f32,
        w_zero_points: *const i32,
        n_scales: i32,
        bias: *const f32,
        act: i32,
        q: *mut u8,
        sa: *mut f32,
        za: *mut i32,
        acc: *mut i32,
        y: *mut f32,
        err: *mut c_char,
        errlen: usize,
    ) -> spt_status;
    pub fn spt_parakeet_debug_tap(ctx: *mut spt_pk_ctx, tensor_id: i32) -> spt_status;
    pub fn spt_parakeet_debug_tap_read(
        ctx: *mut spt_pk_ctx,
        dims: *mut i32,
        a: *mut f32,
        a_cap: i64,
        y: *mut f32,
        y_cap: i64,
    ) -> spt_status;

    // ---- ABI 7: capture-side resampler (audio_toolkit/audio/resampler.rs FrameResampler)
    pub fn spt_resampler_create(
        in_hz: i32,
        out_hz: i32,
        frame_samples: i32,
        device: i32,
        out: *mut *mut spt_resampler,
        err: *mut c_char,
        errlen: usize,
    ) -> spt_status;
    pub fn spt_resampler_info(r: *const spt_resampler, fft_size_in: *mut i32, fft_size_out: *mut i32) -> spt_status;
    pub fn spt_resample_output_len(r: *const spt_resampler, n_samples: usize) -> usize;
    pub fn spt_resample(
        r: *mut spt_resampler,
        pcm: *const f32,
        n_samples: usize,
        out: *mut f32,
        out_cap: usize,
        n_out: *mut usize,
    ) -> spt_status;
    pub fn spt_resampler_last_error(r: *const spt_resampler) -> *const c_char;
    pub fn spt_resampler_destroy(r: *mut spt_resampler);

    // ---- ABI 8: the app's Parakeet model directory without a device (spt_parakeet_create also
    // takes the directory itself)
    pub fn spt_parakeet_onnx_open(
        dir: *const c_char,
        out: *mut *mut spt_pk_onnx,
        info: *mut spt_pk_model_info,
        err: *mut c_char,
        errlen: usize,
    ) -> spt_status;
    pub fn spt_parakeet_onnx_tensor(h: *const spt_pk_onnx, tensor_id: i32, data: *mut *const f32) -> i64;
    // ABI 13: a MatMulInteger / ConvInteger weight as stored ([N][K] integers widened to i16)
    pub fn spt_parakeet_onnx_qtensor(
        h: *const spt_pk_onnx,
        tensor_id: i32,
        q: *mut *const i16,
        scales: *mut *const f32,
        zero_points: *mut *const i32,
        n_scales: *mut i32,
    ) -> i64;
    pub fn spt_parakeet_onnx_piece(h: *const spt_pk_onnx, token_id: i32) -> *const c_char;
    pub fn spt_parakeet_onnx_close(h: *mut spt_pk_onnx);

    // ---- ABI 8: voice-activity gate (audio_toolkit/vad: SmoothedVad over SileroVad)
    pub fn spt_vad_default_params(p: *mut spt_vad_params);
    pub fn spt_vad_create(
        model_path: *const c_char,
        params: *const spt_vad_params,
        out: *mut *mut spt_vad,
        err: *mut c_char,
        errlen: usize,
    ) -> spt_status;
    pub fn spt_vad_push(v: *mut spt_vad, pcm: *const f32, n_samples: usize, out: *mut *mut spt_vad_result) -> spt_status;
    pub fn spt_vad_result_free(r: *mut spt_vad_result);
    pub fn spt_vad_reset(v: *mut spt_vad, reset_model_state: i32) -> spt_status;
    pub fn spt_vad_last_error(v: *const spt_vad) -> *const c_char;
    pub fn spt_vad_destroy(v: *mut spt_vad);

    // ---- Moonshine (SPT_HAS_MOONSHINE, additive over ABI 14)
    pub fn spt_moonshine_default_model_params(p: *mut spt_ms_model_params);
    pub fn spt_moonshine_default_infer_params(p: *mut spt_ms_infer_params);
    pub fn spt_moonshine_create(
        model_spec: *const c_char,
        params: *const spt_ms_model_params,
        out: *mut *mut spt_ms_ctx,
        err: *mut c_char,
        errlen: usize,
    ) -> spt_status;
    pub fn spt_moonshine_destroy(ctx: *mut spt_ms_ctx);
    pub fn spt_moonshine_last_error(ctx: *const spt_ms_ctx) -> *const c_char;
    pub fn spt_moonshine_info(ctx: *const spt_ms_ctx, info: *mut spt_ms_model_info) -> spt_status;
    pub fn spt_moonshine_tensor_numel(ctx: *const spt_ms_ctx, name: *const c_char, n: *mut i64) -> spt_status;
    pub fn spt_moonshine_set_tensor(ctx: *mut spt_ms_ctx, name: *const c_char, data: *const f32, n: i64) -> spt_status;
    pub fn spt_moonshine_missing_tensors(ctx: *const spt_ms_ctx) -> i32;
    pub fn spt_moonshine_set_vocab(ctx: *mut spt_ms_ctx, pieces: *const *const c_char, n: i32) -> spt_status;
    pub fn spt_moonshine_transcribe(
        ctx: *mut spt_ms_ctx,
        pcm16k: *const f32,
        n_samples: usize,
        params: *const spt_ms_infer_params,
        out: *mut *mut spt_ms_result,
    ) -> spt_status;
    pub fn spt_moonshine_transcribe_batch(
        ctx: *mut spt_ms_ctx,
        pcm: *const *const f32,
        n_samples: *const usize,
        batch: usize,
        params: *const spt_ms_infer_params,
        out: *mut *mut spt_ms_result,
    ) -> spt_status;
    pub fn spt_moonshine_result_free(r: *mut spt_ms_result);
    pub fn spt_moonshine_get_timings(ctx: *const spt_ms_ctx, t: *mut spt_ms_timings) -> spt_status;
    pub fn spt_moonshine_debug_stem(ctx: *mut spt_ms_ctx, pcm16k: *const f32, n_samples: usize, out: *mut f32) -> spt_status;
    pub fn spt_moonshine_debug_encode(ctx: *mut spt_ms_ctx, pcm16k: *const f32, n_samples: usize, out: *mut f32) -> spt_status;
    pub fn spt_moonshine_debug_logits(
        ctx: *mut spt_ms_ctx,
        pcm16k: *const f32,
        n_samples: usize,
        prefix: *const i32,
        n_prefix: i32,
        out: *mut f32,
    ) -> spt_status;

    // ---- SenseVoice (SPT_HAS_SENSEVOICE, additive over ABI 14)
    pub fn spt_sensevoice_default_model_params(p: *mut spt_sv_model_params);
    pub fn spt_sensevoice_default_infer_params(p: *mut spt_sv_infer_params);
    pub fn spt_sensevoice_create(
        model_spec: *const c_char,
        params: *const spt_sv_model_params,
        out: *mut *mut spt_sv_ctx,
        err: *mut c_char,
        errlen: usize,
    ) -> spt_status;
    pub fn spt_sensevoice_destroy(ctx: *mut spt_sv_ctx);
    pub fn spt_sensevoice_last_error(ctx: *const spt_sv_ctx) -> *const c_char;
    pub fn spt_sensevoice_info(ctx: *const spt_sv_ctx, info: *mut spt_sv_model_info) -> spt_status;
    pub fn spt_sensevoice_tensor_numel(ctx: *const spt_sv_ctx, name: *const c_char, n: *mut i64) -> spt_status;
    pub fn spt_sensevoice_set_tensor(ctx: *mut spt_sv_ctx, name: *const c_char, data: *const f32, n: i64) -> spt_status;
    pub fn spt_sensevoice_missing_tensors(ctx: *const spt_sv_ctx) -> i32;
    pub fn spt_sensevoice_set_cmvn(ctx: *mut spt_sv_ctx, neg_mean: *const f32, inv_std: *const f32, n: i32) -> spt_status;
    pub fn spt_sensevoice_set_vocab(ctx: *mut spt_sv_ctx, pieces: *const *const c_char, n: i32) -> spt_status;
    pub fn spt_sensevoice_n_rows(ctx: *const spt_sv_ctx, n_samples: usize) -> i32;
    pub fn spt_sensevoice_transcribe(
        ctx: *mut spt_sv_ctx,
        pcm16k: *const f32,
        n_samples: usize,
        params: *const spt_sv_infer_params,
        out: *mut *mut spt_sv_result,
    ) -> spt_status;
    pub fn spt_sensevoice_transcribe_batch(
        ctx: *mut spt_sv_ctx,
        pcm: *const *const f32,
        n_samples: *const usize,
        batch: usize,
        params: *const spt_sv_infer_params,
        out: *mut *mut spt_sv_result,
    ) -> spt_status;
    pub fn spt_sensevoice_result_free(r: *mut spt_sv_result);
    pub fn spt_sensevoice_get_timings(ctx: *const spt_sv_ctx, t: *mut spt_sv_timings) -> spt_status;
    pub fn spt_sensevoice_debug_features(ctx: *mut spt_sv_ctx, pcm16k: *const f32, n_samples: usize, out: *mut f32) -> spt_status;
    pub fn spt_sensevoice_debug_encode(
        ctx: *mut spt_sv_ctx,
        pcm16k: *const f32,
        n_samples: usize,
        params: *const spt_sv_infer_params,
        out: *mut f32,
    ) -> spt_status;
    pub fn spt_sensevoice_debug_frames(
        ctx: *mut spt_sv_ctx,
        pcm16k: *const f32,
        n_samples: usize,
        params: *const spt_sv_infer_params,
        ids: *mut i32,
        top1: *mut f32,
        top2: *mut f32,
    ) -> spt_status;
}

// ---- SenseVoice types
/// The header's feature macro: the spt_sensevoice_* entry points exist.
pub const SPT_HAS_SENSEVOICE: c_int = 1;
/// the token-alignment kernels' test hooks (`spt_debug_align_*`) are present
pub const SPT_HAS_ALIGN_KERNELS: c_int = 1;
/// DTW token and word timestamps (`spt_transcribe_aligned`) are present
pub const SPT_HAS_TOKEN_TIMESTAMPS: c_int = 1;
/// the no-speech probability, the silence skip and `spt_get_window_info` are present
pub const SPT_HAS_NO_SPEECH: c_int = 1;
/// `SPT_BLOCK_PREFILL`, `spt_get_prefill_stats` and the prefill attention hooks are present
pub const SPT_HAS_BLOCK_PREFILL: c_int = 1;
/// `SPT_MODEL_CROSS_KV_F8`, `spt_get_cross_kv_info`, `spt_debug_cross_kv` and the fp8 attention hook are present
pub const SPT_HAS_CROSS_KV_F8: c_int = 1;

/// a text token's start and end (10 ms units), probability and index into `spt_result.tokens`
#[repr(C)]
#[derive(Debug, Clone, Copy)]
pub struct spt_token_time {
    pub t0: i64,
    pub t1: i64,
    pub p: f32,
    pub index: i32,
}

#[repr(C)]
#[derive(Debug, Clone, Copy)]
pub struct spt_word {
    pub t0: i64,
    pub t1: i64,
    pub text: *mut c_char,
    pub i0: i32,
    pub n_tokens: i32,
    pub p: f32,
}

#[repr(C)]
#[derive(Debug)]
pub struct spt_alignment {
    pub tokens: *mut spt_token_time,
    pub n_tokens: i32,
    pub words: *mut spt_word,
    pub n_words: i32,
}
pub const SPT_SV_LANG_AUTO: i32 = 0;
pub const SPT_SV_LANG_ZH: i32 = 1;
pub const SPT_SV_LANG_EN: i32 = 2;
pub const SPT_SV_LANG_YUE: i32 = 3;
pub const SPT_SV_LANG_JA: i32 = 4;
pub const SPT_SV_LANG_KO: i32 = 5;

/// Opaque SenseVoice context.
#[repr(C)]
pub struct spt_sv_ctx {
    _private: [u8; 0],
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct spt_sv_model_params {
    pub dtype: i32,
    pub device: i32,
    pub max_batch: i32,
    pub max_samples: i32,
    pub seed: u64,
    pub ln_eps: f32,
    pub sanm_shift: i32,
    pub lfr_m: i32,
    pub lfr_n: i32,
    pub blank_id: i32,
    pub n_prefix: i32,
    pub lang_rows: [i32; 6],
    pub event_row: i32,
    pub emo_row: i32,
    pub itn_row: i32,
    pub no_itn_row: i32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct spt_sv_infer_params {
    pub language: i32,
    pub use_itn: i32,
}

#[repr(C)]
pub struct spt_sv_result {
    pub text: *mut c_char,
    pub tokens: *mut i32,
    pub frames: *mut i32,
    pub top1: *mut f32,
    pub top2: *mut f32,
    pub n_tokens: i32,
    pub prefix: [i32; 4],
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct spt_sv_model_info {
    pub d: i32,
    pub n_heads: i32,
    pub head_dim: i32,
    pub ff: i32,
    pub n_enc0_layers: i32,
    pub n_enc_layers: i32,
    pub n_tp_layers: i32,
    pub n_vocab: i32,
    pub input_dim: i32,
    pub dtype: i32,
    pub max_batch: i32,
    pub max_samples: i32,
    pub max_rows: i32,
    pub reserved: i32,
    pub weight_bytes: i64,
    pub workspace_bytes: i64,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct spt_sv_timings {
    pub frontend_ms: f64,
    pub encoder_ms: f64,
    pub ctc_ms: f64,
    pub total_ms: f64,
    pub rows: i32,
    pub batch: i32,
}

// ---- Moonshine types
/// The header's feature macro: the spt_moonshine_* entry points exist.
pub const SPT_HAS_MOONSHINE: c_int = 1;

/// Opaque Moonshine context.
#[repr(C)]
pub struct spt_ms_ctx {
    _private: [u8; 0],
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct spt_ms_model_params {
    pub dtype: i32,
    pub device: i32,
    pub max_batch: i32,
    pub max_samples: i32,
    pub seed: u64,
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct spt_ms_infer_params {
    pub tokens_per_second: f32,
    pub max_tokens: i32,
}

#[repr(C)]
pub struct spt_ms_result {
    pub text: *mut c_char,
    pub tokens: *mut i32,
    pub top1: *mut f32,
    pub top2: *mut f32,
    pub n_tokens: i32,
    pub hit_eos: i32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct spt_ms_model_info {
    pub d: i32,
    pub n_heads: i32,
    pub head_dim: i32,
    pub rotary_dim: i32,
    pub ff: i32,
    pub n_enc_layers: i32,
    pub n_dec_layers: i32,
    pub n_vocab: i32,
    pub bos: i32,
    pub eos: i32,
    pub dtype: i32,
    pub max_batch: i32,
    pub max_samples: i32,
    pub ctx: i32,
    pub weight_bytes: i64,
    pub workspace_bytes: i64,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct spt_ms_timings {
    pub stem_ms: f64,
    pub encoder_ms: f64,
    pub cross_kv_ms: f64,
    pub decode_ms: f64,
    pub total_ms: f64,
    pub n_steps: i32,
    pub batch: i32,
}

/// Opaque parsed Parakeet model directory (ABI 8).
#[repr(C)]
pub struct spt_pk_onnx {
    _private: [u8; 0],
}

/// Opaque voice-activity gate (ABI 8).
#[repr(C)]
pub struct spt_vad {
    _private: [u8; 0],
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct spt_vad_params {
    pub threshold: f32,
    pub prefill_frames: i32,
    pub hangover_frames: i32,
    pub onset_frames: i32,
    pub device: i32,
    pub reserved0: i32,
}

#[repr(C)]
pub struct spt_vad_result {
    pub samples: *mut f32,
    pub n_samples: usize,
    pub prob: *mut f32,
    pub kind: *mut u8,
    pub n_frames: i32,
    pub reserved0: i32,
    pub device_ms: f64,
}

/// Opaque capture-side resampler context (ABI 7).
#[repr(C)]
pub struct spt_resampler {
    _private: [u8; 0],
}

// ---- ABI 6: Parakeet-V3 types
pub const SPT_PK_WEIGHTS_EMPTY: u32 = 1;
pub type spt_pk_granularity = c_int;
pub const SPT_PK_TS_TOKEN: spt_pk_granularity = 0;
pub const SPT_PK_TS_WORD: spt_pk_granularity = 1;
pub const SPT_PK_TS_SEGMENT: spt_pk_granularity = 2;

#[repr(C)]
pub struct spt_pk_ctx {
    _private: [u8; 0],
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct spt_pk_model_params {
    pub dtype: i32,
    pub device: i32,
    pub max_batch: i32,
    pub max_seconds: f32,
    pub seed: u64,
    pub flags: u32,
    pub reserved0: i32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct spt_pk_infer_params {
    pub max_symbols: i32,
    pub timestamp_granularity: i32,
}

#[repr(C)]
pub struct spt_pk_segment {
    pub start: f64,
    pub end: f64,
    pub text: *mut c_char,
    pub i0: i32,
    pub n_tokens: i32,
}

#[repr(C)]
pub struct spt_pk_result {
    pub text: *mut c_char,
    pub tokens: *mut i32,
    pub frames: *mut i32,
    pub logit: *mut f32,
    pub runner_up: *mut f32,
    pub n_tokens: i32,
    pub n_segments: i32,
    pub segments: *mut spt_pk_segment,
    pub n_chunks: i32,
    pub reserved0: i32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct spt_pk_model_info {
    pub n_mels: i32,
    pub d: i32,
    pub n_layers: i32,
    pub n_heads: i32,
    pub ff: i32,
    pub sub_ch: i32,
    pub conv_k: i32,
    pub pred: i32,
    pub n_vocab: i32,
    pub n_dur: i32,
    pub dtype: i32,
    pub max_batch: i32,
    pub max_samples: i32,
    pub reserved0: i32,
    pub weight_bytes: i64,
    pub workspace_bytes: i64,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct spt_pk_timings {
    pub mel_ms: f64,
    pub encoder_ms: f64,
    pub decode_ms: f64,
    pub total_ms: f64,
    pub h2d_ms: f64,
    pub n_steps: i32,
    pub batch: i32,
    pub enc_frames: i32,
    pub reserved0: i32,
}
