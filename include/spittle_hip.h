/*
 * spittle_hip.h -- C ABI of the MI355X-native Whisper transcription backend.
 *
 * This is the drop-in boundary for Spittle's transcription hot path.  In the
 * reference, TranscriptionManager owns a transcribe_rs::engines::whisper::WhisperEngine
 * through `LoadedEngine::Whisper` (/root/reference/src-tauri/src/managers/transcription.rs:29-34)
 * and calls, from different OS threads but serialised by one Mutex
 * (transcription.rs:36-47, 437):
 *
 *   WhisperEngine::new() + load_model(&path)     transcription.rs:261-276  -> spt_ctx_create
 *   transcribe_samples(Vec<f32>, Some(params))   transcription.rs:494-503  -> spt_transcribe
 *   unload_model() / Drop                         transcription.rs:175-208  -> spt_ctx_destroy
 *
 * with WhisperInferenceParams { language, translate, initial_prompt, ..Default }
 * (transcription.rs:445-499) -> spt_infer_params, and TranscriptionResult.text
 * (transcription.rs:537-546) -> spt_result.text.  The Rust binding a maintainer
 * adds (spittle-hip-sys / HipWhisperEngine) is shown in INTEGRATION.md.
 *
 * Conventions (same as the in-tree Swift bridge,
 * src-tauri/swift/apple_intelligence_bridge.h:10-24): plain pointers and sizes,
 * status codes plus a message, library-owned results released by
 * spt_result_free.  Input PCM is borrowed for the duration of the call (16 kHz
 * mono f32 in [-1, 1]).  A context is not thread-affine (every entry point
 * selects its device) but is not re-entrant: callers serialise, as the app does.
 */
#ifndef SPITTLE_HIP_H
#define SPITTLE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPT_ABI_VERSION 14

typedef enum {
    SPT_OK = 0,
    SPT_ERR_INVALID_ARG = 1,   /* bad pointer / size / parameter */
    SPT_ERR_LOAD = 2,          /* model spec or file could not be loaded */
    SPT_ERR_DEVICE = 3,        /* HIP runtime / device failure */
    SPT_ERR_OOM = 4,           /* device allocation failed */
    SPT_ERR_UNSUPPORTED = 5,   /* feature not implemented (e.g. beam search) */
    SPT_ERR_INTERNAL = 6
} spt_status;

typedef enum {
    SPT_DTYPE_F32 = 0, SPT_DTYPE_BF16 = 1,
    SPT_DTYPE_F16 = 2 /* Parakeet; ABI 14: also spt_model_params.dtype, the Whisper fp16 engine */,
    SPT_DTYPE_I8 = 3 /* ABI 13, spt_pk_model_params.dtype only: the int8 ONNX export's arithmetic */
} spt_dtype;

/* decode flags (spt_infer_params.flags) */
#define SPT_SUPPRESS_BLANK  1u  /* whisper_full_params.suppress_blank (default on) */
#define SPT_NO_TIMESTAMPS   2u  /* whisper_full_params.no_timestamps */
#define SPT_IGNORE_EOT      4u  /* benchmark protocol: keep decoding past <|endoftext|> */
#define SPT_SUPPRESS_NST    8u  /* whisper_full_params.suppress_non_speech_tokens (ggml models) */
#define SPT_NO_SPEECH_PROB 16u  /* SPT_HAS_NO_SPEECH: compute and report each window's no-speech probability
                                   (spt_get_window_info) without skipping; an enabled no_speech_thold
                                   implies it.  The fast path stays the fast path */
#define SPT_BLOCK_PREFILL  32u  /* SPT_HAS_BLOCK_PREFILL: a prompt prefix ([prev] + prompt tokens) of at least
                                   P_min positions goes through the decoder layers in one block pass per
                                   sequence slice (GEMMs + MFMA attention) instead of ceil(P / 4) chunked
                                   passes.  Off by default; results differ from the chunked path in the low
                                   bits (another accumulation order).  See spt_get_prefill_stats */

typedef struct {
    int32_t dtype;        /* SPT_DTYPE_BF16 (default), SPT_DTYPE_F16 or SPT_DTYPE_F32: weights + activations at
                             the GEMM / GEMV inputs (accumulation, residual stream, logits: always f32).
                             ABI 14: SPT_DTYPE_F16 is an IEEE-half engine with the bf16 engine's layout and
                             weight_bytes (spt_weights_export / _import work unchanged between two f16
                             contexts); an f16 ggml file's matrices are held bit for bit, other types are
                             dequantised in f32 and rounded once (nearest even, subnormals kept).
                             Activations are not saturated (as in whisper.cpp), except that values
                             stored into the decoder's K/V caches are clamped to +-65504 so a cache
                             never holds Inf.  ABI <= 13 rejected SPT_DTYPE_F16 here (bad dtype).
                             SPT_DTYPE_I8 is rejected. */
    int32_t device;       /* HIP device ordinal */
    int32_t max_batch;    /* utterance (30 s window) capacity per call */
    uint32_t flags;       /* SPT_MODEL_* (ABI <= 3: reserved, always 0) */
    uint64_t seed;        /* synthetic weights: PRNG seed */
} spt_model_params;

/* spt_model_params.flags */
#define SPT_MODEL_WEIGHTS_EXTERNAL 1u  /* allocate the weight arena but do not generate / dequantise
                                          into it: spt_weights_import fills it (a multi-GPU load
                                          where rank 0 loads and RCCL broadcasts the arena) */
#define SPT_MODEL_QUANT_RESIDENT 2u    /* SPT_HAS_QUANT_RESIDENT: a ggml file's decoder matrices (per layer
                                          the fused q/k/v, both attention outputs, the cross query, fc1,
                                          fc2) and its token embedding stay in HBM in their quantised
                                          blocks and the decoder GEMVs dequantise them in registers; every
                                          result is bit for bit that of the same file loaded without the
                                          flag.  q4_1, q5_0 and q5_1 tensors are kept; a matrix of any other
                                          type (or a fused one whose parts differ) is dequantised at load as
                                          before, so K-quant and f16 files and synthetic models load with
                                          nothing resident.  bf16 / f16 engines; SPT_DTYPE_F32:
                                          SPT_ERR_UNSUPPORTED at create.  weight_bytes is the smaller arena;
                                          export / import work between contexts of the same file and flag */
#define SPT_MODEL_CROSS_KV_F8 4u       /* SPT_HAS_CROSS_KV_F8: the decoder's cross K/V cache is kept in fp8 e4m3
                                          (OCP) with one f32 scale per 64-element key row, 0.531 of the 16-bit
                                          cache, and the decode-step cross-attention reads it.
                                          Results differ from the unflagged context's within the model's own
                                          tolerances; a row's bits stay its own in any batch.
                                          bf16 / f16 engines; SPT_DTYPE_F32: SPT_ERR_UNSUPPORTED at create.
                                          On such a context spt_transcribe_aligned* return SPT_ERR_UNSUPPORTED,
                                          SPT_BLOCK_PREFILL is ignored (the chunked passes run) and the fused
                                          cross-Q launch is not taken.  Combines with SPT_MODEL_QUANT_RESIDENT */

typedef struct {
    const char* language;        /* ISO-639-1 ("en", "zh", ...); NULL or "auto" = auto-detect
                                    (whisper_lang_auto_detect on the utterance's first 30 s) */
    int32_t translate;           /* task <|translate|> instead of <|transcribe|> */
    const char* initial_prompt;  /* jargon prompt text (src-tauri/src/jargon.rs:594); ggml models */
    uint32_t flags;              /* SPT_SUPPRESS_BLANK | SPT_NO_TIMESTAMPS | SPT_SUPPRESS_NST |
                                    SPT_IGNORE_EOT | SPT_NO_SPEECH_PROB | SPT_BLOCK_PREFILL; default SPT_SUPPRESS_BLANK (whisper_full's
                                    defaults: timestamps on) */
    int32_t max_new_tokens;      /* fast path: generated tokens per 30 s window (<= 220);
                                    whisper_full path: whisper_full_params.max_tokens (0 = none) */
    float temperature;           /* initial temperature (0 = greedy) */
    int32_t beam_size;           /* 1: greedy; 2..8: beam search at temperature 0 (one decoder row
                                    per beam: <= max_batch; whisper_full path) */
    const int32_t* forced_tokens;/* test hook (teacher forcing): [batch][n_forced] or NULL */
    int32_t n_forced;
    const int32_t* prompt_tokens;/* whisper_full_params.prompt_tokens: decoded before [sot ...] as
                                    [prev] + the last min(224, n) of them; NULL = none */
    int32_t n_prompt_tokens;
    /* ABI 3: whisper_full's window loop (timestamps, segments, temperature fallback).  A call
     * takes the device-resident no-timestamp greedy fast path when SPT_NO_TIMESTAMPS is set,
     * temperature_inc == 0, temperature == 0 and beam_size <= 1; every other call runs whisper_full. */
    float temperature_inc;       /* fallback step (0.2); 0 = no fallback */
    int32_t best_of;             /* sampled decoders per window at temperature > 0 (5) */
    float entropy_thold;         /* a decoder whose last 32 tokens' entropy is lower fails (2.4) */
    float logprob_thold;         /* fall back when the average log-probability is lower (-1.0) */
    float max_initial_ts;        /* the first timestamp is at most this many seconds (1.0) */
    /* whisper_full_params.no_speech_thold (SPT_HAS_NO_SPEECH; the former int32 reserved0: same offset
     * and size, and 0 -- every existing caller -- is off).  whisper.cpp 1.7.1 (vendored by
     * whisper-rs-sys 0.11.1, the reference's engine) declares it "TODO: not implemented" and never
     * reads it, so the reference skips no window for no-speech probability; every later whisper.cpp
     * implements it [both recalled; whisper.cpp is not in /root/reference].  Hence off by default:
     * enabled iff 0 < no_speech_thold < 1 (>= 1 is off too: a probability never exceeds it); a
     * negative value or NaN is SPT_ERR_INVALID_ARG.  Enabled, a window of the whisper_full path is
     * dropped when its no-speech probability > no_speech_thold and the kept decoder's average
     * log-probability < logprob_thold; the call takes the whisper_full path.  Unlike whisper.cpp
     * (default 0.6, where 0 means "skip whenever the log-probability is low"), 0 is off here. */
    float no_speech_thold;
    uint64_t seed;               /* temperature sampling stream */
} spt_infer_params;

typedef struct {
    int64_t t0, t1;              /* whisper_full_get_segment_t0 / t1: 10 ms units */
    char* text;                  /* whisper_full_get_segment_text */
    int32_t i0, n_tokens;        /* the segment's tokens in spt_result.tokens */
} spt_segment;

typedef struct {
    char* text;             /* fast path: the text tokens' strings; whisper_full path: the segment
                               texts joined and trimmed (transcribe-rs TranscriptionResult.text);
                               synthetic models spell tokens as "[id]" */
    int32_t* tokens;        /* token ids: fast path every generated token (EOT included, stops
                               after it); whisper_full path each window's chosen decoder's result */
    float* top1;            /* fast path: suppressed logit of the token; whisper_full: its log-prob */
    float* top2;            /* fast path: runner-up suppressed logit; whisper_full: its timestamp id */
    int32_t n_tokens;
    int32_t n_windows;      /* 30 s windows decoded */
    int32_t language;       /* language index decoded with (whisper.cpp order, spt_language_code);
                               -1 for English-only models */
    int32_t n_segments;     /* whisper_full path (0 on the fast path) */
    spt_segment* segments;
    int32_t n_fallbacks;    /* temperature fallbacks taken: decodes repeated at a higher temperature */
    int32_t reserved0;
} spt_result;

typedef struct {
    int32_t n_mels, d, n_head, n_enc, n_dec, n_vocab, n_audio_ctx, n_text_ctx;
    int32_t dtype, max_batch;
    int64_t weight_bytes;
    int64_t workspace_bytes;     /* the workspace arena, plus the block prefill workspaces allocated so far */
} spt_model_info;

/* per-phase device time of the last call, from HIP events on the engine stream; total_ms = the
 * sum of the phases */
typedef struct {
    double mel_ms, encoder_ms, cross_kv_ms, decode_ms, total_ms, h2d_ms;
    int32_t n_decode_passes;  /* of the last engine run: prefix prefill passes (chunked or block), the prompt pass
                                 and the decode steps */
    int32_t batch;
} spt_timings;

typedef struct spt_ctx spt_ctx;

const char* spt_version(void);
void spt_default_model_params(spt_model_params* p);
void spt_default_infer_params(spt_infer_params* p);

/* model_spec: "synthetic:<tiny.en|tiny|base|small|medium|large-v3>[:enc=N][:dec=N][:seed=S]"
 * or the path of a whisper.cpp ggml model file (the catalog's ggml-*.bin; tensor types f32,
 * f16, q4_0, q4_1, q5_0, q5_1, q8_0, q4_K, q5_K, q6_K; dequantised once at load into the engine dtype).
 * Replaces WhisperEngine::load_model(&path) (transcribe-rs; src-tauri/src/managers/
 * transcription.rs:261-276); bad files fail with SPT_ERR_LOAD and a message. */
spt_status spt_ctx_create(const char* model_spec, const spt_model_params* params, spt_ctx** out,
                          char* err, size_t errlen);
void spt_ctx_destroy(spt_ctx* ctx);
const char* spt_last_error(const spt_ctx* ctx);
spt_status spt_ctx_info(const spt_ctx* ctx, spt_model_info* info);

/* one utterance, host PCM (moved Vec<f32> in the app) */
spt_status spt_transcribe(spt_ctx* ctx, const float* pcm16k, size_t n_samples, const spt_infer_params* params,
                          spt_result** out);
/* a batch of utterances, host PCM; out[batch] */
spt_status spt_transcribe_batch(spt_ctx* ctx, const float* const* pcm, const size_t* n_samples, size_t batch,
                                const spt_infer_params* params, spt_result** out);
/* a batch of <= 30 s windows already resident in device memory: pcm_dev[b * stride + i] */
spt_status spt_transcribe_batch_device(spt_ctx* ctx, const float* pcm_dev, size_t stride, const size_t* n_samples,
                                       size_t batch, const spt_infer_params* params, spt_result** out);
void spt_result_free(spt_result* r);
/* ISO-639-1 code of a language index ("en" = 0, "zh" = 1, ...), NULL if out of range */
const char* spt_language_code(int32_t lang_id);

/* whisper_tokenize of the model's vocabulary (ggml models only; SPT_ERR_UNSUPPORTED for
 * synthetic ones).  *n_out = the token count even when it exceeds n_max (then
 * SPT_ERR_INVALID_ARG and nothing is written past n_max). */
spt_status spt_tokenize(spt_ctx* ctx, const char* text, int32_t* tokens, int32_t n_max, int32_t* n_out);
/* whisper_token_to_str: the bytes of token id (owned by the context), NULL without a vocab */
const char* spt_token_to_str(const spt_ctx* ctx, int32_t id);

spt_status spt_get_timings(const spt_ctx* ctx, spt_timings* t);

/* ABI 9: everything the last spt_transcribe* call ran, summed.  spt_timings holds the last engine
 * run only; a whisper_full call (the app's default parameters) runs one decoder run per window
 * batch and temperature, and beam search one decoder pass per step, so its latency reads per
 * decoder pass from here: device_ms / decoder_passes bounds the pass time from above.
 * ABI 11: whisper_full computes the log-mel of each whole utterance once (whisper_pcm_to_mel: its
 * own reflective head, the utterance's global max - 8 clamp) and encodes each 30 s window at
 * `seek` once (whisper_encode_internal), shared by every temperature fallback and by the
 * utterance's beam / best_of decoders: encoder_windows counts those encoder runs.
 * ABI 12: pd_passes / pd_fallbacks counted round 5's opt-in persistent decoder pass; round 6
 * measured it at the persistent-kernel price list's cost, slower than the launch chain at every
 * batch, and deleted it: both counters are always 0 (kept for layout).
 * device_ms (and spt_timings.total_ms) sum the stage intervals (mel, window norm, encoder, cross
 * K/V, decode); host time between the stages is not in them. */
typedef struct {
    int32_t engine_calls;     /* decoder runs (a prompt pass + its steps; ABI <= 10: each with its own
                                 mel + encoder + cross K/V) */
    int32_t decoder_passes;   /* every decoder pass: prefix prefill passes (a chunked pass of <= 4 positions
                                 and a block pass, SPT_BLOCK_PREFILL, count as one pass each), prompt passes,
                                 decode steps, beam steps */
    int32_t beam_steps;       /* host-driven beam steps among them */
    int32_t encoder_windows;  /* ABI 11: 30 s windows encoded (conv stem + encoder + cross K/V): one
                                 per window, shared by every temperature fallback and decoder */
    double device_ms;         /* device time of those runs and steps (HIP events) */
    double encoder_ms;
    double decode_ms;         /* decoder passes incl. prompt prefill and sampling */
    int32_t pd_passes;        /* ABI 12: always 0 (the persistent decoder pass was deleted) */
    int32_t pd_fallbacks;     /* ABI 12: always 0 */
} spt_call_stats;

spt_status spt_get_call_stats(const spt_ctx* ctx, spt_call_stats* s);
/* Additive to ABI 14 (spt_call_stats' layout is unchanged): the last call's fused cross-Q +
 * cross-attention launches (one per decoder layer of every one-token pass that took
 * the fused path) and the engine calls it reran on the two-launch chain because a fused launch's
 * bounded wait ran out (0 in normal operation).  Either pointer may be NULL. */
spt_status spt_get_xq_stats(const spt_ctx* ctx, int32_t* fused_launches, int32_t* fallbacks);

/* Block prefill of the prompt prefix (additive over ABI 14, announced by SPT_HAS_BLOCK_PREFILL and the
 * word "blockprefill" in spt_version()).  With SPT_BLOCK_PREFILL in spt_infer_params.flags
 * the prefix of a decode run ([prev] + the last <= 224 prompt tokens: initial_prompt, prompt_tokens, or
 * whisper_full's prompt_past) of at least P_min = 17 positions (16 prompt tokens; the measured crossover) runs as one pass per slice of a decode
 * group's sequences.  Honoured on the fast path and the whisper_full path (greedy, sampled, beam, the
 * decode of spt_transcribe_aligned; its alignment replay stays chunked).  Ignored -- the prefix then
 * takes the chunked passes, and the statistics say so -- on a context with SPT_MODEL_QUANT_RESIDENT
 * weights resident (no dense decoder matrices) and for a prefix shorter than P_min.  The workspace
 *  is allocated by the first flagged call that takes the block pass; SPT_ERR_OOM if that fails.
 * spt_get_prefill_stats reports the last spt_transcribe* call: block passes run (one per decode-group
 * slice), the prefix rows they carried, and chunked prefill passes of at most 4 positions.  Any pointer
 * may be NULL; a call that fails leaves zeros. */
#define SPT_HAS_BLOCK_PREFILL 1
spt_status spt_get_prefill_stats(const spt_ctx* ctx, int32_t* block_passes, int32_t* block_rows, int32_t* chunk_passes);

/* The fp8 cross K/V cache (additive over ABI 14, announced by SPT_HAS_CROSS_KV_F8 and the word "crosskvf8"
 * in spt_version()).  spt_get_cross_kv_info: format 0 = the engine dtype, 1 = e4m3 codes with
 * a scale per key row; the bytes of the cache in the workspace (max_batch windows) and of the 16-bit staging
 * buffer an fp8 cache is filled through (0 without the flag).  Any pointer may be NULL.
 * spt_debug_cross_kv: layer `layer`, window `window` (of the last call's last encoded window batch) of the
 * cache as f32, k and v [n_head][n_audio_ctx][64] each; an fp8 cache is dequantised on the device by the
 * conversion its kernels use (f32(code) * scale).  SPT_ERR_INVALID_ARG before any window was encoded or
 * for a layer / window out of range. */
#define SPT_HAS_CROSS_KV_F8 1
spt_status spt_get_cross_kv_info(const spt_ctx* ctx, int32_t* format, int64_t* cache_bytes, int64_t* staging_bytes);
spt_status spt_debug_cross_kv(spt_ctx* ctx, int32_t layer, int32_t window, float* k, float* v);

/* The no-speech probability and the silence skip (additive over ABI 14, announced by
 * SPT_HAS_NO_SPEECH and the word "nospeech" in spt_version()).  The probability of
 * a window is softmax(raw logits)[<|nospeech|>] of the last prompt token of the decode run that
 * produced the kept decoder (after any [prev] prefix and the language-detect pass): no suppression
 * mask, no blank rule, no temperature; f32 in every engine dtype, in a summation order fixed by
 * n_vocab, so a row's bits in a batch are its bits alone.  It is computed when SPT_NO_SPEECH_PROB is
 * set or no_speech_thold is enabled; the skip itself is whisper_full-only (an enabled threshold routes
 * the call there; spt_transcribe_batch_device refuses it).
 * spt_get_window_info returns one record per window of the last spt_transcribe* call, in decode order
 * per utterance (utterances ascending); the records are host bookkeeping and always kept (a call that
 * fails leaves none).  *n is the
 * count even when it exceeds cap; the first min(cap, *n) records are written (out may be NULL when
 * cap is 0). */
#define SPT_HAS_NO_SPEECH 1
typedef struct spt_window_info {
    int32_t utterance;          /* index in the call's batch */
    int32_t seek, seek_delta;   /* 10 ms frames */
    int32_t i0, n_tokens;       /* the window's tokens in that utterance's spt_result.tokens (0 tokens when skipped) */
    int32_t n_fallbacks;        /* index of the temperature kept */
    float temperature;
    float avg_logprob;          /* kept decoder's; NaN for a window the fast path decoded (in a fast-path call an
                                   utterance over 30 s or under 1 s takes whisper_full's seek loop: its windows carry
                                   the loop's own avg_logprob and seek_delta) */
    float no_speech_prob;       /* NaN when not computed */
    int32_t skipped;
} spt_window_info;
spt_status spt_get_window_info(const spt_ctx* ctx, spt_window_info* out, int32_t cap, int32_t* n);

/* Multi-GPU load: the weight arena is one device allocation whose layout is a
 * pure function of (model, dtype), spt_model_info.weight_bytes long.  Rank 0 loads the model
 * (file parse + device dequantisation) and exports the arena into a device buffer; the buffer
 * is broadcast over RCCL/xGMI; every other rank, created with SPT_MODEL_WEIGHTS_EXTERNAL on the
 * same model spec, imports it.  Both are synchronous device-to-device copies on the context's
 * device; bytes must equal weight_bytes (else SPT_ERR_INVALID_ARG).  A context created with
 * SPT_MODEL_WEIGHTS_EXTERNAL fails every transcription with SPT_ERR_INVALID_ARG until the
 * import.  The reference loads each engine from disk (transcription.rs:261-276) and has no
 * multi-device path; these two entry points exist for the replica-parallel load only. */
spt_status spt_weights_export(spt_ctx* ctx, void* dev_dst, size_t bytes);
spt_status spt_weights_import(spt_ctx* ctx, const void* dev_src, size_t bytes);
/* ABI 5: the arena itself (device pointer on the context's device, weight_bytes long), so a
 * rank's collective (RCCL broadcast from rank 0) writes straight into it with no staging copy;
 * then spt_weights_commit (synchronises the device) marks an external-weights context usable. */
spt_status spt_weights_arena(spt_ctx* ctx, void** dev_ptr, size_t* bytes);
spt_status spt_weights_commit(spt_ctx* ctx);

/* ABI 5: replica parallelism from ONE host process over several devices, for a
 * host that owns one engine object (the app's TranscriptionManager, transcription.rs:29-47).
 * spt_ctx_create_replicas creates out[i] on devices[i] (distinct ordinals): devices[0] loads the
 * model, one grouped RCCL ncclBroadcast (ncclCommInitAll communicator, xGMI) copies its weight
 * arena into every other context's arena; *bcast_ms (optional) = the broadcast's wall time.
 * Each out[i] is an ordinary context (destroy each with spt_ctx_destroy).
 * spt_transcribe_batch_replicas splits a batch of utterances into n_ctx contiguous balanced
 * shards, transcribes shard i on ctxs[i] in its own host thread (no collective on the data
 * path) and returns out[batch] in input order; on error every result is released and ctxs[0]'s
 * last error names the failing replica. */
spt_status spt_ctx_create_replicas(const char* model_spec, const spt_model_params* params, const int32_t* devices,
                                   int32_t n_devices, spt_ctx** out, double* bcast_ms, char* err, size_t errlen);
spt_status spt_transcribe_batch_replicas(spt_ctx* const* ctxs, int32_t n_ctx, const float* const* pcm,
                                         const size_t* n_samples, size_t batch, const spt_infer_params* params,
                                         spt_result** out);

/* Kernel probe (measurement): re-launch one hot-path kernel `iters` times on the engine
 * stream, on the buffers of the last call.  Decoder kernels (kinds 0-3) are timed between two
 * HIP events after a 512 MB read of other weights (the cold Infinity Cache they meet in the
 * decode loop); kinds 0 and 3 as 8 launches over 8 different layers back to back, like the
 * loop; encoder kernels back to back.  avg_us = mean
 * time per launch; work = algorithmic bytes (HBM-bound kernels) or flops (MFMA-bound kernels)
 * per launch, work_is_flops says which. */
typedef enum {
    SPT_PROBE_DEC_CROSS_ATTN = 0,  /* decoder cross-attention, one layer */
    SPT_PROBE_DEC_SELF_ATTN = 1,   /* decoder self-attention, one layer */
    SPT_PROBE_DEC_LOGITS = 2,      /* final LayerNorm + logits + top-2 partials */
    SPT_PROBE_DEC_FC1 = 3,         /* decoder LayerNorm + fc1 + GELU (weight stream) */
    SPT_PROBE_ENC_FC1_GEMM = 4,    /* encoder fc1 GEMM + bias + GELU */
    SPT_PROBE_ENC_ATTN = 5         /* encoder flash attention, one layer */
} spt_probe_kind;
spt_status spt_probe_kernel(spt_ctx* ctx, int32_t kind, int32_t iters, double* avg_us, double* work,
                            int32_t* work_is_flops);

/* test hooks (parity against the CPU restatement) */
/* normalised log-mel of one window [n_mels][3000] (f32) */
spt_status spt_debug_mel(spt_ctx* ctx, const float* pcm16k, size_t n_samples, float* out);
/* ABI 11: the normalised log-mel [n_mels][3000] the encoder takes for the window at frame `seek` of
 * an utterance of any length: frames [seek, seek + 3000) of the utterance's whole log-mel */
spt_status spt_debug_mel_at(spt_ctx* ctx, const float* pcm16k, size_t n_samples, int32_t seek, float* out);
/* encoder output [1500][d] (f32) from a host mel [n_mels][3000] */
spt_status spt_debug_encode(spt_ctx* ctx, const float* mel, float* out);
/* sum|w| and sum w of the weight tensor with a given id (oracle/wo_model.c table) */
spt_status spt_debug_weight_checksum(spt_ctx* ctx, int32_t tensor_id, double* out2);
/* host-only (no device): whisper_tokenize with the vocabulary of a ggml file */
spt_status spt_debug_ggml_tokenize(const char* model_path, const char* text, int32_t* tokens, int32_t n_max,
                                   int32_t* n_out);
/* host-only: the host reference dequantisation of n elements of one ggml type to f32 */
spt_status spt_debug_ggml_dequant(int32_t ggml_type, const void* src, int64_t n, float* dst);
/* The sampler kernels alone (additive over ABI 14): whisper_full's token rules, the beam candidates
 * and the beam K/V gather on caller-supplied arrays, with no context and no model, on a stream of
 * their own on `device`.  Argument errors and the launchers' own (a vocabulary above 53248 tokens,
 * k outside 1..8) return SPT_ERR_INVALID_ARG with the message in err; no device: SPT_ERR_DEVICE.
 * spt_sample_params is one call's decoding parameters as the kernels read them. */
typedef struct {
    float temperature;       /* 0: greedy; > 0: a draw from softmax(logits / temperature) */
    int32_t suppress_blank;  /* [eot] and the blank token masked at step 0 */
    int32_t no_ts;           /* every timestamp masked */
    int32_t max_initial;     /* step 0: timestamps above beg + max_initial masked; < 0: off */
    int32_t n_max;           /* the repetition guard's step (n_max - 1) */
    int32_t max_tokens;      /* > 0: the segment ends at this token index */
    uint64_t seed;           /* of the (seed, row, step) draw stream */
} spt_sample_params;
/* n_steps decoder steps of the token path: for each step s the statistics launch and the
 * finalize launch on logits [n_steps][B][ldl], as the engine enqueues them, so that the device's
 * own token history feeds the next step's rules.  dtype is the embedding's (emb [n_vocab][d] f32 is
 * rounded to it once; pos [ctx][d] stays f32).  suppress: (n_vocab + 31) / 32 bit words.  In and
 * out (the caller's initial contents are uploaded, the final ones returned): state [B][4] = has_ts,
 * seek_delta, result_len, status; done [B]; out_tok / out_plog / out_tid [B][out_cap]; dec_state =
 * {pos0, step, epoch}.  forced [B][forced_len] may be NULL.  Out: next_tok [B], x [B][d] of the
 * last step, *arrive the last-arriver counter (0 after a complete step). */
spt_status spt_debug_sample_tokens(int32_t device, int32_t dtype, const float* logits, int32_t n_steps, int32_t B,
                                   int32_t n_vocab, int32_t ldl, int32_t eot, int32_t beg, int32_t blank,
                                   const uint32_t* suppress, const spt_sample_params* prm, const int32_t* seek,
                                   const int32_t* seek_end, int32_t* state, int32_t* done, const int32_t* forced,
                                   int32_t forced_len, int32_t out_cap, int32_t* dec_state, int32_t Tq, int32_t d,
                                   int32_t ctx, const float* emb, const float* pos, int32_t* out_tok, float* out_plog,
                                   float* out_tid, int32_t* next_tok, float* x, uint32_t* arrive, char* err,
                                   size_t errlen);
/* one beam candidate launch on logits [B][ldl]: row [B][4] = last token, previous token, has_ts,
 * seek_delta; chunked != 0: the chunk + merge kernels, 0: the one-workgroup kernel.  cand_id /
 * cand_lp [B][8] (in and out: the first k of each row are written), tid [B]. */
spt_status spt_debug_sample_beam(int32_t device, const float* logits, int32_t B, int32_t n_vocab, int32_t ldl,
                                 int32_t eot, int32_t beg, int32_t blank, const uint32_t* suppress,
                                 const spt_sample_params* prm, const int32_t* row, int32_t step, int32_t k,
                                 int32_t chunked, int32_t* cand_id, float* cand_lp, int32_t* tid, char* err,
                                 size_t errlen);
/* the no-speech kernel alone (SPT_HAS_NO_SPEECH; the rules of the hooks above): logits [B][ldl] f32, only
 * columns < n_vocab are read; prob [B].  B 1..1024, n_vocab 1..53248, ldl >= n_vocab, nosp in [0, n_vocab). */
spt_status spt_debug_no_speech(int32_t device, const float* logits, int32_t B, int32_t n_vocab, int32_t ldl,
                               int32_t nosp, float* prob, char* err, size_t errlen);
/* one beam K/V gather: src and dst [L][2][B][H][ctx][64] f32, converted to dtype for the launch
 * and back; dst row b takes positions < pos0 of src row rows[b] and keeps the rest. */
spt_status spt_debug_sample_kv_gather(int32_t device, int32_t dtype, const float* src, float* dst,
                                      const int32_t* rows, int32_t L, int32_t B, int32_t H, int32_t ctx,
                                      int32_t pos0, char* err, size_t errlen);
/* The Whisper attention kernels alone (additive over ABI 14): one launch of the
 * engine's launchers on caller-supplied host f32 arrays, rounded on the host to dtype (f32, bf16 or
 * f16) and returned as f32, on a stream of their own on `device`.  The head dimension is 64.  A shape
 * a launcher would refuse, or that would read outside a buffer, returns SPT_ERR_INVALID_ARG with the
 * message in err before any launch; no device: SPT_ERR_DEVICE.
 * Encoder: qkv [B*T][3*H*64] (q | k | v, head h at h*64) -> out [B*T][H*64]; the SPT_ATTN_* variant
 * switches are read per launch, as the launcher reads them. */
spt_status spt_debug_attn_enc(int32_t device, int32_t dtype, const float* qkv, int32_t B, int32_t T, int32_t H,
                              float* out, char* err, size_t errlen);
/* Decoder self-attention: q [B*Tq][H*64] (row b*Tq + t at position pos0 + t, keys 0..pos0 + t) over
 * the whole cache [2][B][H][ctx][64] as given (rows from pos0 + Tq up are the caller's to poison)
 * -> out [B*Tq][H*64].  Tq 1..4, pos0 >= 0, pos0 + Tq <= ctx. */
spt_status spt_debug_attn_self(int32_t device, int32_t dtype, const float* q, const float* cache, int32_t B,
                               int32_t H, int32_t ctx, int32_t Tq, int32_t pos0, float* out, char* err,
                               size_t errlen);
/* Decoder cross-attention: q [B*Tq][H*64]; k, v [B_layout][H][T_enc][64] are laid out as one layer of
 * the cross K/V cache (32-key blocks, the keys from T_enc to the next multiple of 32 filled with
 * pad_value).  Row b attends to window b0 + b, or with a window map kvrow [B] (required for share >
 * 1) rows j*share .. + share - 1 to window b0 + kvrow[j*share].  splits 2..4 (8-wave mode only): the
 * keys in that many chunks, partials instead of out.  mode: */
enum {
    SPT_ATTN_CROSS_8WAVE = 0,       /* out [B*Tq][H*64], or for splits > 1 part [B*Tq][H][splits][66] */
    SPT_ATTN_CROSS_VW = 1,          /* one wave per workgroup: part [B*Tq][H][8][66] = {o[64], m, l} */
    SPT_ATTN_CROSS_VW_PQ = 2,       /* the same with one query row per workgroup (Tq = 1) */
    SPT_ATTN_CROSS_VW_MERGE = 3,    /* VW, then the partial merge launch: out */
    SPT_ATTN_CROSS_VW_PQ_MERGE = 4  /* VW_PQ, then the partial merge launch: out */
};
spt_status spt_debug_attn_cross(int32_t device, int32_t dtype, int32_t mode, const float* q, const float* k,
                                const float* v, float pad_value, int32_t B, int32_t B_layout, int32_t b0, int32_t H,
                                int32_t T_enc, int32_t Tq, int32_t splits, const int32_t* kvrow, int32_t share,
                                float* out, float* part, char* err, size_t errlen);
/* The fp8 cross K/V kernels alone (SPT_HAS_CROSS_KV_F8): spt_debug_attn_cross's arguments
 * without splits (mode, q, k, v, pad_value, B, B_layout, b0, H, T_enc, Tq, kvrow, share, out, part as there;
 * dtype bf16 or f16, SPT_DTYPE_F32: SPT_ERR_UNSUPPORTED).  k and v are rounded to dtype and quantised per key
 * row; kq, vq [B_layout][H][T_enc][64] receive the dequantised rows and k_scale, v_scale [B_layout][H][T_enc]
 * the scales.  The host quantiser fills the four before the device is looked for, so a valid call without a
 * device returns them with SPT_ERR_DEVICE; on a device they are the device quantiser's, read back through
 * the kernels' conversion, and one launch in the chosen mode gives out / part.  The keys that pad the last
 * 32-key block carry the code of 1.0 in every element and pad_value as their scale (NaN included), so they
 * dequantise to pad_value as spt_debug_attn_cross's do: no result may depend on them. */
spt_status spt_debug_attn_cross_quant(int32_t device, int32_t dtype, int32_t mode, const float* q, const float* k,
                                   const float* v, float pad_value, int32_t B, int32_t B_layout, int32_t b0, int32_t H,
                                   int32_t T_enc, int32_t Tq, const int32_t* kvrow, int32_t share, float* kq, float* vq,
                                   float* k_scale, float* v_scale, float* out, float* part, char* err, size_t errlen);
/* The block prefill's attention kernels alone (SPT_HAS_BLOCK_PREFILL), under the
 * rules of the hooks above; every buffer a kernel writes starts with each byte 0xFF.
 * Self: qkv [B*P][3*H*64] (q | k | v, head h at h*64; rounded to dtype) are positions 0..P-1 of B
 * sequences.  cache [2][B][H][ctx][64] is in and out: uploaded rounded to dtype, rows 0..P-1 receive the
 * K and V of qkv as the engine's cache store holds them (f16: clamped to +-65504), rows from P up come
 * back as given.  Query t attends to keys 0..t -> out [B*P][H*64].  Refused: P < 1, P > ctx, H < 1,
 * B or H outside 1..1024, a null buffer, a buffer above 2^26 elements, a dtype outside f32 / bf16 / f16. */
spt_status spt_debug_attn_prefill_self(int32_t device, int32_t dtype, const float* qkv, float* cache, int32_t B, int32_t H,
                                       int32_t ctx, int32_t P, float* out, char* err, size_t errlen);
/* Cross: q [B*P][H*64]; k, v, pad_value, B_layout, b0, kvrow and share as spt_debug_attn_cross takes
 * them; every one of the T_enc real keys, none of the padded ones -> out [B*P][H*64].  ctx bounds P as
 * the engine's n_text_ctx does.  Also refused: T_enc < 1, b0 + B / share > B_layout, a window map entry
 * outside the layout, share outside 1..8 or not dividing B, share > 1 without a map. */
spt_status spt_debug_attn_prefill_cross(int32_t device, int32_t dtype, const float* q, const float* k, const float* v,
                                        float pad_value, int32_t B, int32_t B_layout, int32_t b0, int32_t H,
                                        int32_t T_enc, int32_t P, int32_t ctx, const int32_t* kvrow, int32_t share,
                                        float* out, char* err, size_t errlen);
/* The fused cross-Q + cross-attention launch alone (dec_xq_fused; additive over
 * ABI 14): x [B][1280] are the f32 residual rows, ln_w / ln_b [1280] the LayerNorm, wq [1280][1280] and
 * bias [1280] the cross-Q projection, k, v [B][20][T_enc][64] and pad_value as spt_debug_attn_cross takes
 * them (row b attends to window b).  wq, k and v are rounded to dtype on the host.  The call builds the
 * step state, the granule buffer and the error word, runs the launch once and returns the projected
 * q [B][1280] and the attention out [B][1280] as f32.  lds: key blocks per attention wave staged in LDS
 * (0..2); touch: key blocks per wave touched before q arrives (0 or 2); neither changes a result bit.
 * SPT_ERR_INVALID_ARG before any launch: dtype f32, H != 20, B outside 1..16, T_enc outside 256..1536,
 * null buffers, lds / touch outside their values, or 80 + B * H above the device's compute units.  A
 * consumer's wait for q that ran out is returned as SPT_ERR_DEVICE, never retried. */
spt_status spt_debug_xq_fused(int32_t device, int32_t dtype, const float* x, const float* ln_w, const float* ln_b,
                              const float* wq, const float* bias, const float* k, const float* v, float pad_value,
                              int32_t B, int32_t H, int32_t T_enc, int32_t lds, int32_t touch, float* q, float* out,
                              char* err, size_t errlen);
/* The GEMM tiles and the LayerNorm kernels alone (additive over ABI 14): one launch of
 * the engine's launcher on caller-supplied host f32 arrays, on a stream of its own on `device`.  A call
 * the launcher would refuse, or that would read or write outside a buffer, returns SPT_ERR_INVALID_ARG
 * with the message in err before any launch; no device: SPT_ERR_DEVICE.
 * spt_debug_gemm: one gemm_nt_variant(dtype, epi, .., batch, variant) call, C = epi(A . W^T).  epi:
 * 0 bias, 1 bias + GELU, 2 bias + GELU + pos (f32), 3 C += alpha (acc + bias) (f32), 4 the head-split
 * store into the cross K/V cache, 5 bias + swish, 6 bias + ReLU, 7 alpha (acc + bias) (f32), 8 split-K
 * slab s at C + s * c_split (f32).  variant: 0 automatic, 1 128 x 128, 2 256 x 256 (bf16 / f16), 3
 * skinny (M <= 64, bf16 / f16, batch 1), 4 64 x 128, 5 64 x 64.  A and C are flat arrays of a_count /
 * c_count elements; batch item z's row m starts at a_off + z * sA + m * lda (rows may overlap: lda < K,
 * the conv stem) and c_off + z * sC + m * ldc.  W [N][ldw], bias [N] or NULL, pos [M][N] or NULL.  A
 * and W are rounded to dtype on the host.  C is in and out: the caller's values are uploaded (rounded
 * to dtype for the epilogues that store dtype: 0, 1, 4, 5, 6), the launch runs, the whole buffer comes
 * back as f32 -- epilogue 3 reads the caller's residual, and every element the kernel must not touch
 * is the caller's to inspect.  Epilogue 4: C is the cache of N / (2 * kv_H * 64) layers of
 * ceil(kv_T / 32) * kv_B * kv_H * 4096 elements from c_off, M == kv_B * kv_T.  Also refused: the 16-byte
 * alignment the kernel that would run needs of A, W, C, pos and their strides, variant 3 with
 * batch != 1, an epilogue a variant lacks, epilogues 4 and 8 with batch != 1. */
spt_status spt_debug_gemm(int32_t device, int32_t dtype, int32_t epi, int32_t variant, int32_t batch, int32_t M,
                          int32_t N, int32_t K, const float* A, int64_t a_count, int64_t a_off, int32_t lda, int64_t sA,
                          const float* W, int32_t ldw, const float* bias, const float* pos, float* C, int64_t c_count,
                          int64_t c_off, int32_t ldc, int64_t sC, float alpha, int32_t ksplit, int64_t c_split,
                          int32_t kv_B, int32_t kv_T, int32_t kv_H, char* err, size_t errlen);
/* spt_debug_layernorm: x [M][d] f32, w, b [d]; eps 1e-5.  mode: */
enum {
    SPT_LN_PLAIN = 0, /* layernorm: y [M][d] = LN(x) w + b, stored as dtype */
    SPT_LN_PEND = 1,  /* layernorm_pend: v = x + alpha (slab_0 + .. + slab_{ks-1} + pbias), y = LN(v) w + b as
                         dtype; x comes back (v where write_x != 0, else as given) */
    SPT_LN_PEND2 = 2  /* layernorm_pend2: y [M][d] f32 = LN(v) w + b, y2 = LN(y) w2 + b2 as dtype; ks 1, 2, 4, 8 */
};
/* The slabs are a flat array of slab_count elements, slab q's row m at q * slab_stride + m * d.  Refused:
 * d % 4, d above 1536 (mode 2: 1024), a NULL pbias in modes 1 and 2, slabs outside the array,
 * slab_stride % 4. */
spt_status spt_debug_layernorm(int32_t device, int32_t dtype, int32_t mode, float* x, int32_t M, int32_t d,
                               const float* slab, int64_t slab_count, int32_t ks, int64_t slab_stride,
                               const float* pbias, float alpha, const float* w, const float* b, const float* w2,
                               const float* b2, int32_t write_x, float* y, float* y2, char* err, size_t errlen);

/* DTW token and word timestamps from the alignment heads' cross-attention (additive over ABI 14,
 * announced by SPT_HAS_TOKEN_TIMESTAMPS): whisper.cpp's dtw_token_timestamps, OpenAI's
 * word_timestamps, HF's return_token_timestamps.  After each window's decoder is chosen, one
 * teacher-forced replay of [sot, (lang, task,) <|notimestamps|>, text tokens] collects the alignment
 * heads' attention probabilities; normalisation, a width-7 median, the head mean and a dynamic time
 * warping (HF transformers' recurrence and tie rule) then give every text token a start and an end. */
#define SPT_HAS_TOKEN_TIMESTAMPS 1
typedef struct spt_token_time {
    int64_t t0, t1;   /* 10 ms units, as spt_segment */
    float p;          /* the token's probability */
    int32_t index;    /* into spt_result.tokens */
} spt_token_time;
typedef struct spt_word {
    int64_t t0, t1;   /* its first token's start, its last token's end */
    char* text;       /* the tokens' bytes */
    int32_t i0, n_tokens;  /* its tokens in spt_alignment.tokens */
    float p;          /* mean of the token probabilities */
} spt_word;
typedef struct spt_alignment {
    spt_token_time* tokens;  /* one per text token (timestamp and eot tokens have none) */
    int32_t n_tokens;
    spt_word* words;         /* ggml models; a synthetic model has no vocabulary and no words */
    int32_t n_words;
} spt_alignment;
/* The alignment heads as n_pairs (layer, head) pairs; n_pairs = 0 restores the default, every head of
 * the top half of the decoder layers.  A pair out of range, a duplicate or more than 512 pairs:
 * SPT_ERR_INVALID_ARG (the heads in use stay). */
spt_status spt_set_alignment_heads(spt_ctx* ctx, const int32_t* layer_head, int32_t n_pairs);
/* spt_transcribe on the whisper_full path (whatever the parameters), plus the alignment of each
 * utterance; *out is what whisper_full gives without the alignment.  Free with spt_result_free and
 * spt_alignment_free.  The test hooks stay allowed here: forced_tokens [batch][n_forced] fixes the token
 * fed after step s of every window of utterance u to forced_tokens[u][s] (the token recorded, and so
 * aligned, is still the sampler's choice at that step; not with beam_size > 1), and SPT_IGNORE_EOT keeps
 * the pass loop from ending early.  With SPT_NO_WINDOW_SHARE set the call is SPT_ERR_INVALID_ARG. */
spt_status spt_transcribe_aligned(spt_ctx* ctx, const float* pcm16k, size_t n_samples, const spt_infer_params* params,
                                  spt_result** out, spt_alignment** align);
spt_status spt_transcribe_aligned_batch(spt_ctx* ctx, const float* const* pcm, const size_t* n_samples, size_t batch,
                                        const spt_infer_params* params, spt_result** out, spt_alignment** align);
void spt_alignment_free(spt_alignment* a);
/* Test hook: what the last aligned call recorded: the replay passes of its last Engine::align, the
 * alignment heads in use, and the bytes of the alignment workspace the context holds.  Any pointer may be NULL. */
spt_status spt_debug_align_stats(spt_ctx* ctx, int32_t* replay_passes, int32_t* n_heads, int64_t* workspace_bytes);
/* Test hook: the last aligned window of the context: the alignment heads' probabilities p
 * [n_heads][n_rows][n_keys] (rows: each text token, then the end), the matrix m [n_rows][n_keys] and
 * the path [path_len][2] of (row, key).  Any buffer may be NULL; the capacities are in elements. */
spt_status spt_debug_align_last(spt_ctx* ctx, int32_t* n_heads, int32_t* n_rows, int32_t* n_keys, float* p, size_t p_cap,
                                float* m, size_t m_cap, int32_t* path, size_t path_cap, int32_t* path_len);

/* The token-alignment kernels alone (additive over ABI 14, announced by SPT_HAS_ALIGN_KERNELS;
 * DESIGN.md 2d / 4.5): align_qk, align_norm and align_dtw of k_align.hip on caller-supplied host
 * arrays, on a stream of their own on `device`, under the rules of the attention hooks above.  N [B]
 * and M [B] are each sequence's text rows and keys in use (0..N_cap, 0..M_cap); what a kernel does not
 * write comes back as NaN (ints: -1).
 * align_qk: q [B*Tq][H*64] (rounded to dtype) are the rows pos0 .. pos0 + Tq - 1 of each sequence,
 * k [B_layout][H][T_enc][64] (rounded to dtype) is laid out as one layer of the cross K/V cache, the V
 * halves and the keys from T_enc to the next multiple of 32 holding pad_value; sequence b attends to
 * window kvrow[b] (NULL: b); heads [n_heads] is any list of heads.  p [B][n_heads][N_cap][M_cap]:
 * p[b][i][pos0 + t][s < M[b]] = softmax over all T_enc keys of q . k / 8 for head heads[i].
 * T_enc <= 3072, M_cap <= T_enc, Tq 1..4, pos0 + Tq <= N_cap. */
#define SPT_HAS_ALIGN_KERNELS 1
spt_status spt_debug_align_qk(int32_t device, int32_t dtype, const float* q, const float* k, float pad_value, int32_t B,
                              int32_t B_layout, int32_t H, int32_t T_enc, int32_t Tq, int32_t pos0,
                              const int32_t* kvrow, const int32_t* heads, int32_t n_heads, const int32_t* M,
                              int32_t N_cap, int32_t M_cap, float* p, char* err, size_t errlen);
/* align_norm: p [B][A][N_cap][M_cap] -> stat [B][A][2][M_cap] (optional: each column's mean and
 * population std over the N rows) and m [B][N_cap][M_cap] = the mean over the heads of the width-7
 * median along the keys (reflect padding; none for M <= 3) of (p - mean) / std, 0 where std == 0. */
spt_status spt_debug_align_norm(int32_t device, const float* p, int32_t B, int32_t A, int32_t N_cap, int32_t M_cap,
                                const int32_t* N, const int32_t* M, float* stat, float* m, char* err, size_t errlen);
/* align_dtw: dynamic time warping of -m (m [B][N_cap][M_cap]; N_cap <= 256, M_cap a multiple of 8, the
 * 2-bit trace within 160 KiB) -> jump [B][N_cap] (the first key of each row on the path), len [B] and,
 * optionally, path [B][N_cap + M_cap][2] = the (row, key) pairs in order, -1 past len. */
spt_status spt_debug_align_dtw(int32_t device, const float* m, int32_t B, int32_t N_cap, int32_t M_cap, const int32_t* N,
                               const int32_t* M, int32_t* jump, int32_t* len, int32_t* path, char* err,
                               size_t errlen);
/* Host only: n aligned tokens (piece bytes with their lengths, start t0, end t1, probability p or
 * NULL) grouped into words: a word starts at the first token and at every token whose piece begins
 * with a space, but a token whose bytes stop inside a UTF-8 sequence joins the next token.  Arrays of
 * n entries receive each word's first token, token count, t0 of its first and t1 of its last token,
 * and (word_p optional) the mean probability; *n_words the count. */
spt_status spt_debug_align_words(const char* const* pieces, const int32_t* piece_len, const int64_t* t0,
                                 const int64_t* t1, const float* p, int32_t n, int32_t* word_i0, int32_t* word_n,
                                 int64_t* word_t0, int64_t* word_t1, float* word_p, int32_t* n_words, char* err,
                                 size_t errlen);

/* Quantised decoder weights resident in HBM (additive over ABI 14, announced by
 * SPT_HAS_QUANT_RESIDENT).  spt_debug_qgemv is the decoder GEMV alone over one
 * quantised matrix, with no context and no model, on a stream of its own on `device`: the launch
 * runs twice, once on the weights expanded to dtype by the loader's dequantisation kernel and once
 * on the matrix packed in its blocks and dequantised in registers, and both results come back as f32.
 *   ggml_type   SPT_GGML_Q4_1, _Q5_0 or _Q5_1 (every other type: SPT_ERR_UNSUPPORTED)
 *   blocks      the file's blocks of W [N][K / 32], blocks_bytes of them (must be the tensor's size)
 *   dtype       SPT_DTYPE_BF16 or SPT_DTYPE_F16 (SPT_DTYPE_F32: SPT_ERR_UNSUPPORTED)
 *   act         f32 [R][K]: SPT_QGEMV_A_DIRECT rounds it to dtype as the activation rows; SPT_QGEMV_A_LN
 *               takes it as the f32 residual rows of the fused LayerNorm (ln_w, ln_b [K]; K <= 1536)
 *   bias [N] (or NULL), resid [R][N] (SPT_GV_BIAS_RESID: required, the rows the product is added to;
 *               SPT_GV_PARTIAL: optional, added into slab 0)
 *   (mode, a_src) one of the decoder's pairs: (BIAS | BIAS_GELU | QKV_CACHE | LOGITS, A_LN),
 *               (PARTIAL | BIAS_RESID, A_DIRECT); ksplit > 1 with SPT_GV_PARTIAL only
 *   out_plain / out_packed   [R][N]; SPT_GV_PARTIAL: [ksplit][R][N]; SPT_GV_QKV_CACHE (N = 3 d, d a
 *               multiple of 64, one token per row at position 0): [R][3 d] = q | the appended k | v
 *   top_plain / top_packed   SPT_GV_LOGITS only: the top-2 partials [R][ceil(N / 16)][4] as stored
 *               (16 bytes each: f32 best, i32 index, f32 runner-up, 0); no token is suppressed
 *   unpacked    optional [N][K]: the packed matrix dequantised back on the host.  It is written before
 *               the device is looked for, so a valid call without a device fills it and returns
 *               SPT_ERR_DEVICE.
 * K must be a multiple of 128, R in 1..64, N >= 1.  Every argument error, and every shape the
 * launcher would refuse, returns SPT_ERR_INVALID_ARG with the message in err before any launch. */
#define SPT_HAS_QUANT_RESIDENT 1
/* what SPT_MODEL_QUANT_RESIDENT kept: the count of weights held quantised, their bytes in the arena
 * (padding included) and their ggml type (-1: none, or matrices of several types).  Any pointer may be NULL. */
spt_status spt_get_weight_residency(const spt_ctx* ctx, int64_t* resident_weights, int64_t* resident_bytes,
                                    int32_t* ggml_type);
enum { SPT_GGML_Q4_1 = 3, SPT_GGML_Q5_0 = 6, SPT_GGML_Q5_1 = 7 };
enum { SPT_GV_BIAS = 0, SPT_GV_BIAS_GELU = 1, SPT_GV_PARTIAL = 2, SPT_GV_QKV_CACHE = 3, SPT_GV_LOGITS = 4,
       SPT_GV_BIAS_RESID = 5 };
enum { SPT_QGEMV_A_DIRECT = 0, SPT_QGEMV_A_LN = 1 };
spt_status spt_debug_qgemv(int32_t device, int32_t dtype, int32_t ggml_type, const void* blocks, size_t blocks_bytes,
                           int32_t N, int32_t K, const float* act, int32_t R, const float* ln_w, const float* ln_b,
                           const float* bias, const float* resid, int32_t mode, int32_t a_src, int32_t ksplit,
                           float* out_plain, float* out_packed, float* top_plain, float* top_packed, float* unpacked,
                           char* err, size_t errlen);

/* The decoder GEMV and the small kernels of the decode step alone (additive over ABI 14, announced by
 * SPT_HAS_GEMV_KERNELS), under the rules of the hooks above: no context, a stream and
 * buffers of the call's own on `device`, host f32 in and out, every refusal made on the host before
 * any launch (SPT_ERR_INVALID_ARG with the reason in err), a valid call without a device
 * SPT_ERR_DEVICE.  Every buffer a kernel writes starts with each byte 0xFF (a NaN in f32, bf16 and
 * f16; -1 in an int) and comes back whole, so what a launch did not write is the caller's to inspect.
 *
 * spt_debug_gemv: one gemv() launch on dense weights W [N][K], given as f32 and rounded to dtype
 * (SPT_DTYPE_F32, _BF16 or _F16) on the host.  R in 1..64.  (mode, a_src) is one of the decoder's pairs.
 *   a_src  SPT_GEMV_A_DIRECT: A [a_count] rounded to dtype, row i at A + i * lda + a_row0.
 *          SPT_GEMV_A_LN: A [a_count] the f32 residual rows in the same layout; pend [n_pend][a_count]
 *            the pending slabs in A's layout (n_pend 0, 1, 2 or 4; the unused ones are a zero slab);
 *            ln_w, ln_b [K]; x_out (optional) [a_count]: the summed rows as workgroup (0, 0) writes them.
 *          SPT_GEMV_A_ATTN: apart [R][H][S][66] = {o[64], m, l}, S in {2, 3, 4, 8}, H * 64 == K.  With
 *            merge_first (S = 8) the call also runs dec_attn_part_merge and the SPT_GEMV_A_DIRECT
 *            projection of its output on the same operands: that second C comes back in out_merged.
 *   C      [c_count] with row i at C + i * ldc (ldc >= N).  SPT_GV_BIAS_RESID: in (the f32 rows the
 *          product is added to) and out; every other mode: out only.  SPT_GV_PARTIAL: slab s at
 *          C + s * c_split, p_resid (optional) [R][ldc] added into slab 0.  SPT_GV_QKV_CACHE (N = 3 d,
 *          d = 64 cache_H, R = B * Tq): q in columns 0..d-1 of C, k and v into cache
 *          [2][B][cache_H][ctx][64] at positions pos0 .. pos0 + Tq - 1 (pos0 + Tq <= ctx).
 *          SPT_GV_LOGITS: the f32 logits; suppress [suppress_words >= ceil(N / 32)] the mask, blank0 /
 *          blank1 the columns also suppressed while step == 0, part [R][n_tiles][4] the top-2 partials as
 *          stored (f32 best, i32 index, f32 runner-up, 0).
 *   plan   (optional) int32 [8]: what gemv_plan() chose: waves, column tiles, super-steps in flight,
 *          exact, row groups, LDS bytes, grid x, grid y.  Written before the device is looked for. */
#define SPT_HAS_GEMV_KERNELS 1
enum { SPT_GEMV_A_DIRECT = 0, SPT_GEMV_A_LN = 1, SPT_GEMV_A_ATTN = 2 };
typedef struct spt_gemv_debug {
    const float* W;
    const float* A;
    const float* ln_w;
    const float* ln_b;
    const float* pend;
    float* x_out;
    const float* apart;
    float* out_merged;
    const float* bias;
    float* C;
    const float* p_resid;
    float* cache;
    const uint32_t* suppress;
    float* part;
    int32_t* plan;
    int64_t a_count, c_count, c_split, suppress_words;
    int32_t dtype, mode, a_src, R, N, K, lda, a_row0, n_pend, S, H, merge_first, ldc, ksplit;
    int32_t B, Tq, cache_H, ctx, pos0, blank0, blank1, step, n_tiles, reserved0;
} spt_gemv_debug;
spt_status spt_debug_gemv(int32_t device, const spt_gemv_debug* args, char* err, size_t errlen);

/* spt_debug_dec_step: the small kernels of the step.
 *   SPT_DEC_STEP_EMBED     dec_embed: x [B * Tq][d] = emb[tok[r]] + pos[pos0 + r % Tq] (tok [B * Tq] in
 *                          0..n_vocab-1, pos0 + Tq <= ctx); the state is not changed.
 *   SPT_DEC_STEP_FINALIZE  dec_finalize n_steps times, step s on part [n_steps][B][n_tiles][4] (the
 *                          partials as spt_debug_gemv returns them): next_tok [n_steps][B] and
 *                          x [n_steps][B][d] per step; out_tok, out_top1, out_top2 [B][out_cap], done [B]
 *                          (in and out) and the state after the last step.  forced [B][forced_len] or
 *                          NULL.  state[0] + n_steps * Tq may pass ctx (the position row is clamped).
 *   SPT_DEC_STEP_ADVANCE   dec_advance by n_advance; SPT_DEC_STEP_RESET  dec_reset.
 *   emb    [n_vocab][d] f32 rounded to dtype on the host, or, with emb_q one of SPT_GGML_Q4_1 / _Q5_0 /
 *          _Q5_1 (16-bit dtypes, d a multiple of 128), emb_blocks: the ggml blocks of [n_vocab][d / 32],
 *          packed as spt_debug_qgemv packs W.  pos [ctx][d] f32.
 *   state  int32 [4] in and out: pos0, step, epoch, arrive. */
enum { SPT_DEC_STEP_EMBED = 0, SPT_DEC_STEP_FINALIZE = 1, SPT_DEC_STEP_ADVANCE = 2, SPT_DEC_STEP_RESET = 3 };
typedef struct spt_dec_step_debug {
    const int32_t* tok;
    const float* part;
    const int32_t* forced;
    int32_t* done;
    const float* emb;
    const void* emb_blocks;
    const float* pos;
    int32_t* state;
    int32_t* next_tok;
    float* x;
    int32_t* out_tok;
    float* out_top1;
    float* out_top2;
    size_t emb_blocks_bytes;
    int32_t dtype, op, B, Tq, d, ctx, n_vocab, n_tiles, n_steps, forced_len, ignore_eot, out_cap, eot, emb_q;
    int32_t n_advance, reserved0;
} spt_dec_step_debug;
spt_status spt_debug_dec_step(int32_t device, const spt_dec_step_debug* args, char* err, size_t errlen);

/* The Parakeet encoder kernels alone (additive over ABI 14, announced by SPT_HAS_PK_KERNELS; DESIGN.md
 * 9.8), under the rules of the hooks above.  lens [B][4] = the frame counts T, T1, T2, T3 of each
 * utterance, as the engine keeps them on the device; every entry >= 0.
 *
 * spt_debug_pk_conv: one launch, by mode (Fo = (F - 1) / 2 + 1 and To = (Tp - 1) / 2 + 1 are the hook's):
 *   SPT_PK_CONV0    pk_conv0: x = mel [B][Tp][F] (f32, not rounded), w [C][9], bias [C]
 *                   -> y [B][To][Fo][C]; frames >= min(lens[b][0], Tp) read as zero.
 *   SPT_PK_DWCONV1 / _DWCONV2  pk_dwconv at stage 1 / 2: x [B][Tp][F][C] (dtype) -> y [B][To][Fo][C];
 *                   frames >= min(lens[b][stage], Tp) read as zero.
 *   SPT_PK_CONV_MODULE  pk_conv_module: x [B * Tp][2 C] (dtype; F is ignored), w [C][9], bias [C],
 *                   bn_g / bn_b / bn_m / bn_v [C] -> y [B * Tp][C]; lens[b][3] <= Tp.
 *   y [y_count]: y_count >= the elements the launch owns; the rest are guards nothing may write.
 * spt_debug_pk_relpos: one pk_relpos launch -> pe [pe_count >= (2 Tp - 1) d] (d even).
 * spt_debug_pk_rel_attn: one pk_rel_attn_variant launch.  qkv [B * Tp][3 d], d = H * dk; p [p_count]
 *   with row r of utterance b at p + p_off + b * p_bstride + r * ldp (2 Tp - 1 rows of d elements;
 *   p_bstride != 0 is f32 only); pu, pv [H][dk] (f32, not rounded); out [out_count >= B * Tp * d].
 *   variant SPT_PK_ATTN_AUTO / _VALU / _MFMA (MFMA: f16 at dk 64 or 128).  lens[b][3] <= Tp: the
 *   kernels index their score row and the position rows from it unguarded.  ldp, p_off and p_bstride
 *   lie on the 16-byte grid of the kernels' vector loads. */
#define SPT_HAS_PK_KERNELS 1
enum { SPT_PK_CONV0 = 0, SPT_PK_DWCONV1 = 1, SPT_PK_DWCONV2 = 2, SPT_PK_CONV_MODULE = 3 };
enum { SPT_PK_ATTN_AUTO = 0, SPT_PK_ATTN_VALU = 1, SPT_PK_ATTN_MFMA = 2 };
typedef struct spt_pk_conv_debug {
    const float* x;
    const int32_t* lens;
    const float* w;
    const float* bias;
    const float* bn_g;
    const float* bn_b;
    const float* bn_m;
    const float* bn_v;
    float* y;
    int64_t y_count;
    int32_t dtype, mode, B, Tp, F, C;
} spt_pk_conv_debug;
spt_status spt_debug_pk_conv(int32_t device, const spt_pk_conv_debug* args, char* err, size_t errlen);
spt_status spt_debug_pk_relpos(int32_t device, int32_t dtype, int32_t Tp, int32_t d, float* pe, int64_t pe_count,
                               char* err, size_t errlen);
typedef struct spt_pk_attn_debug {
    const float* qkv;
    const float* p;
    const float* pu;
    const float* pv;
    const int32_t* lens;
    float* out;
    int64_t p_count, p_off, p_bstride, out_count;
    int32_t dtype, variant, B, Tp, H, dk, ldp, reserved0;
} spt_pk_attn_debug;
spt_status spt_debug_pk_rel_attn(int32_t device, const spt_pk_attn_debug* args, char* err, size_t errlen);

/* spt_debug_pk_tdt: pk_state_init, then n_steps of pk_joint_fin, step s on the caller's partials
 * part [n_steps][B][n_tiles][4] (f32 best, i32 index as stored, f32 runner-up, unused: what the joint stage
 * writes per 64-output tile) and duration logits dur [n_steps][B][n_dur].  emb [V + 1][P], fe [B * T3p][P],
 * lens [B][4] with 0 <= lens[b][3] <= T3p.  Returned for slot 0 (after pk_state_init) and slot s + 1 (after
 * step s): state [n_steps + 1][B][7] = {t, at_t, n_out, done, upd, tok, t3p}, xemb and fecur
 * [n_steps + 1][B][P]; per step the four output arrays whole, out_tok / out_frame (int32) and out_t1 /
 * out_t2 [n_steps][B * cap + 1] (the last element is a guard nothing may write; every element starts as
 * 0xFF bytes).  Refused: a partial whose best is NaN, a best above -inf whose index is outside 0 .. V, and
 * a (step, row) with no best above -inf: the kernel reads the embedding row of the index it finds. */
typedef struct spt_pk_tdt_debug {
    const float* part;
    const float* dur;
    const int32_t* lens;
    const float* emb;
    const float* fe;
    int32_t* state;
    float* xemb;
    float* fecur;
    int32_t* out_tok;
    int32_t* out_frame;
    float* out_t1;
    float* out_t2;
    int32_t B, P, V, n_dur, n_tiles, n_steps, max_symbols, cap, T3p, reserved0;
} spt_pk_tdt_debug;
spt_status spt_debug_pk_tdt(int32_t device, const spt_pk_tdt_debug* args, char* err, size_t errlen);

/* spt_debug_pk_dec_stage: one pk_decode_stage launch of the TDT step, by mode, on plain weights the hook
 * places with pk_place_lstm / pk_place_blocked into a buffer of the padded size that starts as NaN bytes.
 * P up to 640 and a multiple of 64 (LSTM), 128 (PRED) or 32 (JOINT): what pk_decode_stage admits; B in 1..64;
 * state [B][7] are the PkState rows (the stages read upd).
 *   SPT_PK_DEC_LSTM   W = W_ih, W2 = W_hh [4P][P] (gate rows i, f, g, o), b0 = b_ih, b1 = b_hh [4P],
 *                     xin, h_in, c_in [B][P] -> h_out, c_out [B][P] (rows with upd = 0: h_in, c_in as given).
 *   SPT_PK_DEC_PRED   W [P][P], b0 [P], xin [B][P] -> gp [B][P], in and out (rows with upd = 0 untouched).
 *   SPT_PK_DEC_JOINT  W [N][P], b0 [N], N = V + 1 + n_dur; x = ReLU(fe + gp), fe and gp [B][P] ->
 *                     part [B][n_tiles][4] (n_tiles = ceil(N / 64); f32 best, i32 index, f32 runner-up, 0 of
 *                     the tile's outputs n <= V) and dur [B][n_dur]. */
enum { SPT_PK_DEC_LSTM = 0, SPT_PK_DEC_PRED = 1, SPT_PK_DEC_JOINT = 2 };
typedef struct spt_pk_dec_debug {
    const float* W;
    const float* W2;
    const float* b0;
    const float* b1;
    const int32_t* state;
    const float* xin;
    const float* h_in;
    const float* c_in;
    const float* fe;
    float* gp;
    float* h_out;
    float* c_out;
    float* part;
    float* dur;
    int32_t mode, B, P, V, n_dur, reserved0;
} spt_pk_dec_debug;
spt_status spt_debug_pk_dec_stage(int32_t device, const spt_pk_dec_debug* args, char* err, size_t errlen);

/* spt_debug_pk_tdt_steps: pk_state_init, then n_steps of the engine's whole decode step -- LSTM layer 0, LSTM
 * layer 1, the prediction projection, the joint and pk_joint_fin, the five launches of ParakeetEngine's step in
 * its order, with its ping-pong of the LSTM state buffers -- on plain weights (placed as spt_debug_pk_dec_stage
 * places them): lstm [2][4] = W_ih, W_hh [4P][P], b_ih, b_hh [4P] per layer; pred_w [P][P], pred_b [P]; joint_w
 * [N][P], joint_b [N], N = V + 1 + n_dur; emb [V + 1][P]; fe [B * T3p][P]; lens [B][4].  Returns state
 * [n_steps + 1][B][7] (slot 0: after the init) and the four output arrays [B * cap + 1] after the last step. */
typedef struct spt_pk_steps_debug {
    const float* lstm[2][4];
    const float* pred_w;
    const float* pred_b;
    const float* joint_w;
    const float* joint_b;
    const float* emb;
    const float* fe;
    const int32_t* lens;
    int32_t* state;
    int32_t* out_tok;
    int32_t* out_frame;
    float* out_t1;
    float* out_t2;
    int32_t B, P, V, n_dur, n_steps, max_symbols, cap, T3p;
} spt_pk_steps_debug;
spt_status spt_debug_pk_tdt_steps(int32_t device, const spt_pk_steps_debug* args, char* err, size_t errlen);

/* ================================================================================================
 * ABI 6: Parakeet-V3 (NeMo FastConformer-TDT), the app's other local engine;
 * ABI 8: spt_parakeet_create takes the app's model directory (the int8 ONNX export) natively.
 *
 * In the reference TranscriptionManager owns a transcribe_rs ParakeetEngine through
 * LoadedEngine::Parakeet and calls (src-tauri/src/managers/transcription.rs):
 *
 *   ParakeetEngine::new() + load_model_with_params(&path, ParakeetModelParams::int8())
 *                                                   :278-297  -> spt_parakeet_create (+ set_tensor)
 *   transcribe_samples(audio, Some(ParakeetInferenceParams { timestamp_granularity: Segment, .. }))
 *                                                   :505-513  -> spt_parakeet_transcribe
 *   unload_model() / Drop                            :175-208  -> spt_parakeet_destroy
 *
 * and reads TranscriptionResult.text (:537-546).  The encoder runs in fp16 (SPT_DTYPE_F16, the
 * BASELINE config) or f32; the prediction network and joint always in f32.  Weights come from a
 * synthetic spec or tensor by tensor through spt_parakeet_set_tensor (the id table of
 * oracle/po_model.c, NeMo layouts; spittle_amd.parakeet.load_nemo maps a .nemo checkpoint).
 *
 * ABI 13: SPT_DTYPE_I8 runs the encoder as ONNX Runtime runs the app's quantize_dynamic export: the
 * f32 engine, with every encoder Linear and pointwise convolution as DynamicQuantizeLinear (the
 * input to uint8, one range per utterance) -> MatMulInteger / ConvInteger on int8 MFMAs (exact
 * int32 accumulators) -> scale, bias, activation.  A model directory's integers, scales and zero
 * points are used as stored; f32 weights of those layers (synthetic specs, set_tensor, QDQ
 * directories) are quantised at load, symmetric per tensor.  The joint and the TDT decoder stay
 * f32 on dequantised weights.  DESIGN.md §9.7 is the contract.
 * ============================================================================================== */
typedef struct spt_pk_ctx spt_pk_ctx;

typedef struct {
    int32_t dtype;        /* SPT_DTYPE_F16 (default), SPT_DTYPE_F32 or SPT_DTYPE_I8 (bf16 also accepted) */
    int32_t device;
    int32_t max_batch;    /* utterances (chunks) per device pass, <= 64 */
    float max_seconds;    /* workspace size: the longest utterance one pass takes before it grows.
                             A longer recording grows the workspace to its length and is decoded
                             whole (up to 20 min / 96 GiB of workspace); only past that is it cut
                             into chunks (multiples of 80 ms) whose results are concatenated */
    uint64_t seed;        /* synthetic weights */
    uint32_t flags;       /* SPT_PK_WEIGHTS_EMPTY: zero weights, to be filled by set_tensor */
    int32_t reserved0;
} spt_pk_model_params;

#define SPT_PK_WEIGHTS_EMPTY 1u

typedef enum { SPT_PK_TS_TOKEN = 0, SPT_PK_TS_WORD = 1, SPT_PK_TS_SEGMENT = 2 } spt_pk_granularity;

typedef struct {
    int32_t max_symbols;            /* TDT greedy: tokens per encoder frame (NeMo default 10; <= 16) */
    int32_t timestamp_granularity;  /* an spt_pk_granularity; the app asks for SPT_PK_TS_SEGMENT */
} spt_pk_infer_params;

typedef struct {
    double start, end;     /* seconds */
    char* text;
    int32_t i0, n_tokens;  /* the unit's tokens in spt_pk_result.tokens */
} spt_pk_segment;

typedef struct {
    char* text;            /* the pieces joined ("▁" -> space) and trimmed; "[id]" without a vocabulary */
    int32_t* tokens;
    int32_t* frames;       /* encoder frame (80 ms) of each token, utterance-relative */
    float* logit;          /* the token's joint logit */
    float* runner_up;      /* the best other token's (blank included) */
    int32_t n_tokens;
    int32_t n_segments;
    spt_pk_segment* segments;  /* timestamp units of the requested granularity */
    int32_t n_chunks;
    int32_t reserved0;
} spt_pk_result;

typedef struct {
    int32_t n_mels, d, n_layers, n_heads, ff, sub_ch, conv_k, pred, n_vocab, n_dur;
    int32_t dtype, max_batch, max_samples, reserved0;
    int64_t weight_bytes, workspace_bytes;
} spt_pk_model_info;

typedef struct {
    double mel_ms, encoder_ms, decode_ms, total_ms, h2d_ms;
    int32_t n_steps;       /* TDT joint evaluations (graph-replayed decode steps) */
    int32_t batch;
    int32_t enc_frames;    /* padded encoder frames of the pass */
    int32_t reserved0;
} spt_pk_timings;

void spt_parakeet_default_model_params(spt_pk_model_params* p);
void spt_parakeet_default_infer_params(spt_pk_infer_params* p);
/* model_spec: the app's model directory (below; the weights are dequantised and placed, vocab.txt
 * becomes the vocabulary), or "synthetic:parakeet-tdt-0.6b-v3[:layers=N][:seed=S]" /
 * "synthetic:parakeet-test-small[...]" (seeded weights; real ones through spt_parakeet_set_tensor) */
spt_status spt_parakeet_create(const char* model_spec, const spt_pk_model_params* params, spt_pk_ctx** out,
                               char* err, size_t errlen);

/* The model directory the app downloads (parakeet-tdt-0.6b-v3-int8, the onnx-asr export that
 * transcribe-rs reads: encoder-model[.int8].onnx, decoder_joint-model[.int8].onnx, vocab.txt;
 * model_catalog.json:229-241) is also what spt_parakeet_create takes as model_spec -- this is the
 * same loader without a device: parse, dequantise (int8 / uint8 + scale + zero point, per tensor or
 * per channel), map onto the engine's tensor ids (NeMo layouts), infer the dimensions.
 * info->reserved0 receives the number of dequantised initializers.  Host memory only. */
typedef struct spt_pk_onnx spt_pk_onnx;
spt_status spt_parakeet_onnx_open(const char* dir, spt_pk_onnx** out, spt_pk_model_info* info, char* err, size_t errlen);
/* a tensor's f32 values (NeMo layout) by engine tensor id: its element count, or -1 */
int64_t spt_parakeet_onnx_tensor(const spt_pk_onnx* h, int32_t tensor_id, const float** data);
/* ABI 13: a weight consumed by MatMulInteger / ConvInteger exactly as the file stores it: the
 * integers in the engine's [N][K] orientation (int8 or uint8 values, widened to int16), the scales
 * and zero points and their count (1, or N: one per output channel).  Returns the element count, or
 * -1 for a tensor no integer op consumes.  (q - zero_point) * scale is the f32 tensor above. */
int64_t spt_parakeet_onnx_qtensor(const spt_pk_onnx* h, int32_t tensor_id, const int16_t** q, const float** scales,
                                  const int32_t** zero_points, int32_t* n_scales);
/* vocab.txt's piece for a token id (NULL past the vocabulary or without vocab.txt) */
const char* spt_parakeet_onnx_piece(const spt_pk_onnx* h, int32_t token_id);
void spt_parakeet_onnx_close(spt_pk_onnx* h);
void spt_parakeet_destroy(spt_pk_ctx* ctx);
const char* spt_parakeet_last_error(const spt_pk_ctx* ctx);
spt_status spt_parakeet_info(const spt_pk_ctx* ctx, spt_pk_model_info* info);
/* element count of tensor id (SPT_ERR_INVALID_ARG if unknown) and its upload (f32, NeMo layout) */
spt_status spt_parakeet_tensor_numel(const spt_pk_ctx* ctx, int32_t tensor_id, int64_t* n);
spt_status spt_parakeet_set_tensor(spt_pk_ctx* ctx, int32_t tensor_id, const float* data, int64_t n);
/* SentencePiece pieces by id (UTF-8, "▁" marks a word start); copied */
spt_status spt_parakeet_set_vocab(spt_pk_ctx* ctx, const char* const* pieces, int32_t n);
spt_status spt_parakeet_transcribe(spt_pk_ctx* ctx, const float* pcm16k, size_t n_samples,
                                   const spt_pk_infer_params* params, spt_pk_result** out);
spt_status spt_parakeet_transcribe_batch(spt_pk_ctx* ctx, const float* const* pcm, const size_t* n_samples,
                                         size_t batch, const spt_pk_infer_params* params, spt_pk_result** out);
/* batch <= max_batch chunks already in device memory (pcm_dev[b * stride + i], n <= max samples) */
spt_status spt_parakeet_transcribe_batch_device(spt_pk_ctx* ctx, const float* pcm_dev, size_t stride,
                                                const size_t* n_samples, size_t batch,
                                                const spt_pk_infer_params* params, spt_pk_result** out);
void spt_parakeet_result_free(spt_pk_result* r);
spt_status spt_parakeet_get_timings(const spt_pk_ctx* ctx, spt_pk_timings* t);
/* ABI 10: encoder stage profile (measurement).  Re-runs the last call's encoder pass `iters` times
 * eagerly, on the same buffers and shape (bitwise the same output), with a HIP event on the engine
 * stream after every stage's launches; ms[c] = mean time per pass spent in stage class c.
 * n >= SPT_PK_STAGE_COUNT. */
typedef enum {
    SPT_PK_STAGE_SUBSAMPLING = 0, /* conv stem: conv0, two depthwise + pointwise stages, linear */
    SPT_PK_STAGE_POS = 1,         /* relative positions + every layer's linear_pos (one GEMM) */
    SPT_PK_STAGE_LAYERNORM = 2,   /* 5 LayerNorms per layer (pending split-K products folded in) */
    SPT_PK_STAGE_FFN = 3,         /* both half-FFNs' GEMMs (SiLU up-projection, split-K down) */
    SPT_PK_STAGE_QKV_OUT = 4,     /* attention q/k/v and output GEMMs */
    SPT_PK_STAGE_ATTN = 5,        /* relative-position attention */
    SPT_PK_STAGE_CONV_PW = 6,     /* convolution module pointwise GEMMs */
    SPT_PK_STAGE_CONV_DW = 7,     /* GLU + depthwise conv + BatchNorm + SiLU */
    SPT_PK_STAGE_JOINT_ENC = 8,   /* the joint's encoder projection */
    SPT_PK_STAGE_COUNT = 9
} spt_pk_stage;
spt_status spt_parakeet_profile_encoder(spt_pk_ctx* ctx, int32_t iters, double* ms, int32_t n);
/* test hooks: normalised log-mel [n_mels][max(1, n / 160)] (n / 160 valid frames, NeMo get_seq_len); encoder output [T3][d] of a mel
 * [n_mels][T]; sum|w| and sum w of a tensor as stored (transposed tensors: SPT_ERR_UNSUPPORTED) */
spt_status spt_parakeet_debug_mel(spt_pk_ctx* ctx, const float* pcm16k, size_t n_samples, float* out);
spt_status spt_parakeet_debug_encode(spt_pk_ctx* ctx, const float* mel, int32_t T, float* out);
/* the encoder output [T3][d] (f32) of batch row b of the last transcribe call (the production
 * path: graph-replayed or eager); out holds the T3 rows of spt_pk_model_info.max_samples (which grows
 * with the longest recording decoded); *T3 receives the row's count */
spt_status spt_parakeet_debug_last_encoder(spt_pk_ctx* ctx, int32_t b, float* out, int32_t* T3);
/* TDT greedy decoding of a given encoder output [T3][d] (f32): the decoder alone */
spt_status spt_parakeet_debug_decode(spt_pk_ctx* ctx, const float* enc, int32_t T3, int32_t max_symbols,
                                     spt_pk_result** out);
spt_status spt_parakeet_debug_weight_checksum(spt_pk_ctx* ctx, int32_t tensor_id, double* out2);
/* ABI 13 test hooks of the int8 mode.
 * debug_qgemm: the three int8 kernels alone, without a model.  a [m][k] f32 rows in n_groups row
 * groups (utterances: each its own quantisation range) of group_len rows; w [n][k] stored integers
 * (int8 or uint8 values) with n_scales (1 or n) scales / zero points (NULL: zero); optional bias
 * [n]; act an spt_pk_act.  Out: q [m][k] the uint8 quantised input, sa / za [n_groups], acc [m][n]
 * the int32 accumulators, y [m][n].  k a multiple of 64 (<= 4096), n a multiple of 16.
 * debug_tap: arm a capture, in the next spt_parakeet_debug_encode, of the quantised GEMM whose
 * weight is tensor_id (5, 9, 11; per layer 1000 + 64 l + {2, 4, 8, 14, 16, 21, 29, 33, 35}; the
 * stacked q / k / v GEMM is named by linear_q, + 8).  SPT_ERR_INVALID_ARG for any other id,
 * SPT_ERR_UNSUPPORTED on an engine of another dtype.
 * debug_tap_read: dims = {M, K, N, bias_included}; a [M][K] the GEMM's f32 input rows, y [M][N]
 * its stored f32 output (bias_included 0: a residual product, whose bias the next LayerNorm adds).
 * a / y may be NULL to read dims first; capacities in elements. */
typedef enum { SPT_PK_ACT_NONE = 0, SPT_PK_ACT_RELU = 1, SPT_PK_ACT_SWISH = 2 } spt_pk_act;
spt_status spt_parakeet_debug_qgemm(int32_t device, const float* a, int32_t m, int32_t k, const int32_t* group_len,
                                    int32_t n_groups, const int16_t* w, int32_t n, const float* w_scales,
                                    const int32_t* w_zero_points, int32_t n_scales, const float* bias, int32_t act,
                                    uint8_t* q, float* sa, int32_t* za, int32_t* acc, float* y, char* err, size_t errlen);
spt_status spt_parakeet_debug_tap(spt_pk_ctx* ctx, int32_t tensor_id);
spt_status spt_parakeet_debug_tap_read(spt_pk_ctx* ctx, int32_t* dims, float* a, int64_t a_cap, float* y, int64_t y_cap);

/* ================================================================================================
 * ABI 7: the capture-side resampler.
 *
 * Replaces FrameResampler (src-tauri/src/audio_toolkit/audio/resampler.rs:7-104): rubato 0.16.2
 * FftFixedIn<f32>(in_hz, out_hz, RESAMPLER_CHUNK_SIZE = 1024, 1, 1) behind 1024-sample input
 * chunks, its output cut into frames of frame_samples (the recorder's 30 ms = 480 samples at
 * 16 kHz, recorder.rs:264-268).  spt_resample runs one whole capture stream as
 * FrameResampler::new + push(all samples) + finish (recorder.rs:330, 355): the concatenated
 * frames, including finish's zero padding of the last input chunk and of the last frame.
 * in_hz == out_hz: frames of the input, as FrameResampler does without rubato.
 * ============================================================================================== */
typedef struct spt_resampler spt_resampler;
spt_status spt_resampler_create(int32_t in_hz, int32_t out_hz, int32_t frame_samples, int32_t device,
                                spt_resampler** out, char* err, size_t errlen);
/* rubato's unit sizes (0 when in_hz == out_hz) */
spt_status spt_resampler_info(const spt_resampler* r, int32_t* fft_size_in, int32_t* fft_size_out);
/* samples spt_resample writes for an n-sample stream (a multiple of frame_samples) */
size_t spt_resample_output_len(const spt_resampler* r, size_t n_samples);
/* pcm: host samples (borrowed); out: host buffer of at least spt_resample_output_len samples */
spt_status spt_resample(spt_resampler* r, const float* pcm, size_t n_samples, float* out, size_t out_cap,
                        size_t* n_out);
const char* spt_resampler_last_error(const spt_resampler* r);
void spt_resampler_destroy(spt_resampler* r);

/* ================================================================================================
 * ABI 8: the capture-side voice-activity gate.  The recorder's consumer thread
 * pushes every 480-sample (30 ms) frame from the FrameResampler through
 *   SmoothedVad::new(Box::new(SileroVad::new("resources/models/silero_vad_v4.onnx", 0.3)), 15, 15, 2)
 * (src-tauri/src/managers/audio.rs:132-134, 295-307) and appends what it returns as Speech to the
 * recording (audio_toolkit/audio/recorder.rs:284-301); Cmd::Start resets the smoothing (:343-349).
 *
 *   spt_vad_create(model_path, params)  = SileroVad::new + SmoothedVad::new  (the model file the app
 *                                         ships is read natively: ONNX graph, 16 kHz branch)
 *   spt_vad_push(pcm, n)                = push_frame for each 480-sample frame in order (a trailing
 *                                         partial frame is kept as Speech, like the recorder's
 *                                         unwrap_or); result: the kept samples, each frame's speech
 *                                         probability and VadFrame kind (0 Noise, 1 Speech(frame),
 *                                         2 Speech(prefill + frame))
 *   spt_vad_reset(v, 0)                 = SmoothedVad::reset (the Silero LSTM state carries, as in the
 *                                         app); reset_model_state = 1 also zeroes it (a new SileroVad)
 *
 * The network runs on the device: every frame's convolutional front end at once, then the
 * two-layer LSTM recurrence over the frames in one workgroup (its state kept between calls).
 * ============================================================================================== */
typedef struct spt_vad spt_vad;
typedef struct {
    float threshold;          /* speech when prob > threshold (0.3) */
    int32_t prefill_frames;   /* 15 */
    int32_t hangover_frames;  /* 15 */
    int32_t onset_frames;     /* 2 */
    int32_t device;
    int32_t reserved0;
} spt_vad_params;
typedef struct {
    float* samples;           /* the kept audio (Speech frames, prefill at onsets), n_samples long */
    size_t n_samples;
    float* prob;              /* per whole frame: Silero's speech probability */
    uint8_t* kind;            /* per frame (a trailing partial frame included): 0 Noise, 1 Speech, 2 onset */
    int32_t n_frames;
    int32_t reserved0;
    double device_ms;         /* front end + recurrence on the device */
} spt_vad_result;
void spt_vad_default_params(spt_vad_params* p);
spt_status spt_vad_create(const char* model_path, const spt_vad_params* params, spt_vad** out, char* err,
                          size_t errlen);
spt_status spt_vad_push(spt_vad* v, const float* pcm, size_t n_samples, spt_vad_result** out);
void spt_vad_result_free(spt_vad_result* r);
spt_status spt_vad_reset(spt_vad* v, int32_t reset_model_state);
const char* spt_vad_last_error(const spt_vad* v);
void spt_vad_destroy(spt_vad* v);

/* ================================================================================================
 * Moonshine (additive over ABI 14, announced by SPT_HAS_MOONSHINE): the app's third local engine.
 *
 * Replaces transcribe_rs::engines::moonshine::MoonshineEngine as TranscriptionManager drives it
 * through `LoadedEngine::Moonshine` (src-tauri/src/managers/transcription.rs:260-341, 444-534):
 *
 *   load_model_with_params(&path, MoonshineModelParams::variant(ModelVariant::Base))  -> spt_moonshine_create
 *   transcribe_samples(audio, None)                                                   -> spt_moonshine_transcribe
 *   unload_model() / Drop                                                             -> spt_moonshine_destroy
 *
 * The model is an encoder-decoder transformer over raw 16 kHz PCM (no mel): three strided 1-D
 * convolutions with a whole-utterance GroupNorm, partial interleaved rotary positions, head dim 52
 * (Base) or 36 (Tiny), a SiLU-gated decoder MLP, greedy decoding from <s> to </s> or to
 * ceil(tokens_per_second * seconds) tokens.  The arithmetic is HF transformers' modeling_moonshine.py;
 * a batch row computes what it computes alone (the B = 1 semantics the app has).  Engine dtype is
 * fp16 only: f16 weights and GEMM inputs, f32 accumulation, residual stream, norms and softmax.
 * Weights come from a synthetic spec or tensor by tensor, keyed by HF state-dict name.
 * DESIGN.md §12 is the contract.
 * ============================================================================================== */
#define SPT_HAS_MOONSHINE 1

typedef struct spt_ms_ctx spt_ms_ctx;

typedef struct {
    int32_t dtype;        /* SPT_DTYPE_F16 (default); every other dtype: SPT_ERR_UNSUPPORTED */
    int32_t device;
    int32_t max_batch;    /* utterances per device pass, <= 64 (default 8); longer batches run in passes */
    int32_t max_samples;  /* the longest utterance taken: 895..3000000 (187.5 s), default 64 s = 1024000;
                             a longer utterance: SPT_ERR_INVALID_ARG */
    uint64_t seed;        /* synthetic weights (a ":seed=S" in the spec wins) */
} spt_ms_model_params;

typedef struct {
    float tokens_per_second;  /* token limit = ceil(tokens_per_second * n_samples / 16000); default 6.5 */
    int32_t max_tokens;       /* > 0: the limit itself, whatever the length (both are capped at the
                                 context's capacity, spt_ms_model_info.ctx) */
} spt_ms_infer_params;

typedef struct {
    char* text;            /* pieces joined: specials dropped, byte pieces to bytes, "▁" -> space, leading
                              space stripped; "[id]" per token without a vocabulary */
    int32_t* tokens;       /* the generated ids, </s> not included */
    float* top1;           /* each token's logit */
    float* top2;           /* the runner-up's */
    int32_t n_tokens;
    int32_t hit_eos;       /* 1: ended by </s>, 0: by the token limit */
} spt_ms_result;

typedef struct {
    int32_t d, n_heads, head_dim, rotary_dim, ff, n_enc_layers, n_dec_layers, n_vocab, bos, eos;
    int32_t dtype, max_batch, max_samples, ctx;
    int64_t weight_bytes, workspace_bytes;
} spt_ms_model_info;

typedef struct {
    double stem_ms, encoder_ms, cross_kv_ms, decode_ms, total_ms;  /* the last device pass */
    int32_t n_steps;       /* replays of the decode-step graph */
    int32_t batch;
} spt_ms_timings;

void spt_moonshine_default_model_params(spt_ms_model_params* p);
void spt_moonshine_default_infer_params(spt_ms_infer_params* p);
/* model_spec: "synthetic:moonshine-base|moonshine-tiny|moonshine-test-small[:layers=N][:vocab=V][:eos=E][:seed=S]"
 * (seeded weights) or "empty:" + the same grammar (every tensor to be supplied by set_tensor).
 * test-small: Base widths, 2 + 2 layers, vocabulary 1024. */
spt_status spt_moonshine_create(const char* model_spec, const spt_ms_model_params* params, spt_ms_ctx** out,
                                char* err, size_t errlen);
void spt_moonshine_destroy(spt_ms_ctx* ctx);
const char* spt_moonshine_last_error(const spt_ms_ctx* ctx);
spt_status spt_moonshine_info(const spt_ms_ctx* ctx, spt_ms_model_info* info);
/* tensors by HF state-dict name ("model.encoder.conv1.weight", "model.decoder.layers.3.mlp.fc1.bias"):
 * f32 host data in HF's layout.  The tied "proj_out.weight" is accepted after embed_tokens when it
 * rounds to the same f16 values, and is never required. */
spt_status spt_moonshine_tensor_numel(const spt_ms_ctx* ctx, const char* name, int64_t* n);
spt_status spt_moonshine_set_tensor(spt_ms_ctx* ctx, const char* name, const float* data, int64_t n);
/* tensors still to be supplied (transcribing with any missing is an error); -1 for a null context */
int32_t spt_moonshine_missing_tensors(const spt_ms_ctx* ctx);
/* SentencePiece pieces by id (UTF-8); copied */
spt_status spt_moonshine_set_vocab(spt_ms_ctx* ctx, const char* const* pieces, int32_t n);
/* fewer than 895 samples (no encoder frame): SPT_OK, empty text, no device work */
spt_status spt_moonshine_transcribe(spt_ms_ctx* ctx, const float* pcm16k, size_t n_samples,
                                    const spt_ms_infer_params* params, spt_ms_result** out);
/* out: `batch` result pointers, each released by spt_moonshine_result_free */
spt_status spt_moonshine_transcribe_batch(spt_ms_ctx* ctx, const float* const* pcm, const size_t* n_samples,
                                          size_t batch, const spt_ms_infer_params* params, spt_ms_result** out);
void spt_moonshine_result_free(spt_ms_result* r);
spt_status spt_moonshine_get_timings(const spt_ms_ctx* ctx, spt_ms_timings* t);
/* test hooks (one utterance of 895..max_samples samples): the stem's output [T3][d] f32 (before the
 * first encoder layer); the encoder's output [T3][d] f32; the logits [n_prefix][n_vocab] f32 of a
 * forced token prefix (step s is fed prefix[s]; prefix[0] is normally <s>), one row per replay of
 * the step graph the free-running loop uses.  T3 = ((((n - 127) / 64 + 1) - 7) / 3 + 1 - 3) / 2 + 1. */
spt_status spt_moonshine_debug_stem(spt_ms_ctx* ctx, const float* pcm16k, size_t n_samples, float* out);
spt_status spt_moonshine_debug_encode(spt_ms_ctx* ctx, const float* pcm16k, size_t n_samples, float* out);
spt_status spt_moonshine_debug_logits(spt_ms_ctx* ctx, const float* pcm16k, size_t n_samples, const int32_t* prefix,
                                      int32_t n_prefix, float* out);

/* ================================================================================================
 * SenseVoice (additive over ABI 14, announced by SPT_HAS_SENSEVOICE): the app's fourth local engine.
 *
 * Replaces transcribe_rs::engines::sense_voice::SenseVoiceEngine as TranscriptionManager drives it
 * through `LoadedEngine::SenseVoice` (src-tauri/src/managers/transcription.rs:260-341, 444-534):
 *
 *   load_model_with_params(&path, SenseVoiceModelParams::int8())       -> spt_sensevoice_create
 *   transcribe_samples(audio, Some(SenseVoiceInferenceParams{..}))     -> spt_sensevoice_transcribe
 *   unload_model() / Drop                                              -> spt_sensevoice_destroy
 *
 * SenseVoice-Small is non-autoregressive: a Kaldi fbank (80 mels, 25 ms / 10 ms, Hamming) stacked to
 * low-frame-rate rows (7 frames every 6), four query rows (language, event, emotion, text norm) in
 * front, a 70-layer SANM encoder (self-attention with head dim 128 plus an 11-tap FSMN memory) and a
 * CTC head; one forward pass per call, greedy collapse on the device.  A batch row computes what it
 * computes alone.  Engine dtype is fp16 only: f16 weights and GEMM inputs, f32 accumulation, residual
 * stream, norms, softmax and front end.  Weights come from a synthetic spec or tensor by tensor, keyed
 * by FunASR state-dict name.  The encoder's constants recalled from FunASR without a copy to check
 * against are model parameters with the recalled defaults.  DESIGN.md §13 is the contract.
 * ============================================================================================== */
#define SPT_HAS_SENSEVOICE 1

typedef struct spt_sv_ctx spt_sv_ctx;

enum { SPT_SV_LANG_AUTO = 0, SPT_SV_LANG_ZH = 1, SPT_SV_LANG_EN = 2, SPT_SV_LANG_YUE = 3, SPT_SV_LANG_JA = 4,
       SPT_SV_LANG_KO = 5 };

typedef struct {
    int32_t dtype;        /* SPT_DTYPE_F16 (default); every other dtype: SPT_ERR_UNSUPPORTED */
    int32_t device;
    int32_t max_batch;    /* utterances per device pass, <= 64 (default 8); longer batches run in passes */
    int32_t max_samples;  /* the longest utterance taken: 400..4800000 (300 s), default 64 s = 1024000;
                             a longer utterance: SPT_ERR_INVALID_ARG */
    uint64_t seed;        /* synthetic weights (a ":seed=S" in the spec wins) */
    /* recalled from FunASR's SenseVoiceSmall, unverifiable offline: defaults as recalled */
    float ln_eps;         /* LayerNorm epsilon, default 1e-5 */
    int32_t sanm_shift;   /* FSMN padding: 5 + shift frames left, 5 - shift right; default 0 */
    int32_t lfr_m;        /* frames stacked per row, default 7 (the embed / CMVN width is 80 * lfr_m) */
    int32_t lfr_n;        /* frames advanced per row, default 6 */
    int32_t blank_id;     /* CTC blank, default 0 */
    int32_t n_prefix;     /* leading output rows reported as labels, not text: 0..4, default 4 */
    int32_t lang_rows[6]; /* embed row of each SPT_SV_LANG_*: default 0, 3, 4, 7, 11, 12 */
    int32_t event_row;    /* default 1 */
    int32_t emo_row;      /* default 2 */
    int32_t itn_row;      /* text norm row with ITN, default 14 */
    int32_t no_itn_row;   /* without, default 15 */
} spt_sv_model_params;

typedef struct {
    int32_t language;     /* SPT_SV_LANG_*; default AUTO */
    int32_t use_itn;      /* default 0 */
} spt_sv_infer_params;

typedef struct {
    char* text;            /* pieces joined: "<|..|>" tags and specials dropped, byte pieces to bytes, "▁" ->
                              space, leading space stripped; "[id]" per token without a vocabulary */
    int32_t* tokens;       /* collapsed ids, blanks dropped */
    int32_t* frames;       /* the row (after the prefix rows) where each token's run starts: 60 ms units */
    float* top1;           /* that row's top logit */
    float* top2;           /* and its runner-up */
    int32_t n_tokens;
    int32_t prefix[4];     /* argmax of output rows 0..3: language, emotion, event, ITN tags (-1 beyond n_prefix) */
} spt_sv_result;

typedef struct {
    int32_t d, n_heads, head_dim, ff, n_enc0_layers, n_enc_layers, n_tp_layers, n_vocab, input_dim;
    int32_t dtype, max_batch, max_samples, max_rows, reserved;
    int64_t weight_bytes, workspace_bytes;
} spt_sv_model_info;

typedef struct {
    double frontend_ms, encoder_ms, ctc_ms, total_ms;  /* the last device pass */
    int32_t rows;          /* encoder rows per utterance of that pass (the longest) */
    int32_t batch;
} spt_sv_timings;

void spt_sensevoice_default_model_params(spt_sv_model_params* p);
void spt_sensevoice_default_infer_params(spt_sv_infer_params* p);
/* model_spec: "synthetic:sensevoice-small|sensevoice-test-small[:layers=a,b][:vocab=V][:seed=S]" (seeded
 * weights and a fixed CMVN) or "empty:" + the same grammar (every tensor by set_tensor, the CMVN by
 * set_cmvn).  layers=a,b: encoders / tp_encoders.  test-small: d 256, 2 heads, ff 512, 1 + 2 + 1
 * layers, vocabulary 500. */
spt_status spt_sensevoice_create(const char* model_spec, const spt_sv_model_params* params, spt_sv_ctx** out,
                                 char* err, size_t errlen);
void spt_sensevoice_destroy(spt_sv_ctx* ctx);
const char* spt_sensevoice_last_error(const spt_sv_ctx* ctx);
spt_status spt_sensevoice_info(const spt_sv_ctx* ctx, spt_sv_model_info* info);
/* tensors by FunASR state-dict name ("embed.weight", "encoder.encoders.3.self_attn.fsmn_block.weight",
 * "ctc.ctc_lo.bias"): f32 host data in FunASR's layout */
spt_status spt_sensevoice_tensor_numel(const spt_sv_ctx* ctx, const char* name, int64_t* n);
spt_status spt_sensevoice_set_tensor(spt_sv_ctx* ctx, const char* name, const float* data, int64_t n);
/* tensors still to be supplied, the CMVN pair counting as one; -1 for a null context */
int32_t spt_sensevoice_missing_tensors(const spt_sv_ctx* ctx);
/* features = (lfr + neg_mean) * inv_std, n = 80 * lfr_m values each (am.mvn's <AddShift> / <Rescale>) */
spt_status spt_sensevoice_set_cmvn(spt_sv_ctx* ctx, const float* neg_mean, const float* inv_std, int32_t n);
/* SentencePiece pieces by id (UTF-8); copied */
spt_status spt_sensevoice_set_vocab(spt_sv_ctx* ctx, const char* const* pieces, int32_t n);
/* encoder rows of n samples: ceil((1 + (n - 400) / 160) / lfr_n) + 4, or 0 below 400 samples */
int32_t spt_sensevoice_n_rows(const spt_sv_ctx* ctx, size_t n_samples);
/* fewer than 400 samples (no fbank frame): SPT_OK, empty text, no device work */
spt_status spt_sensevoice_transcribe(spt_sv_ctx* ctx, const float* pcm16k, size_t n_samples,
                                     const spt_sv_infer_params* params, spt_sv_result** out);
/* out: `batch` result pointers, each released by spt_sensevoice_result_free */
spt_status spt_sensevoice_transcribe_batch(spt_sv_ctx* ctx, const float* const* pcm, const size_t* n_samples,
                                           size_t batch, const spt_sv_infer_params* params, spt_sv_result** out);
void spt_sensevoice_result_free(spt_sv_result* r);
spt_status spt_sensevoice_get_timings(const spt_sv_ctx* ctx, spt_sv_timings* t);
/* test hooks (one utterance of 400..max_samples samples, R = spt_sensevoice_n_rows): the LFR rows after
 * CMVN, before the queries [R - 4][input_dim] f32; the encoder output after tp_norm [R][d] f32; per row
 * the top-1 id and the top-1 / top-2 logits over the real vocabulary [R] each */
spt_status spt_sensevoice_debug_features(spt_sv_ctx* ctx, const float* pcm16k, size_t n_samples, float* out);
spt_status spt_sensevoice_debug_encode(spt_sv_ctx* ctx, const float* pcm16k, size_t n_samples,
                                       const spt_sv_infer_params* params, float* out);
spt_status spt_sensevoice_debug_frames(spt_sv_ctx* ctx, const float* pcm16k, size_t n_samples,
                                       const spt_sv_infer_params* params, int32_t* ids, float* top1, float* top2);

#ifdef __cplusplus
}
#endif
#endif
