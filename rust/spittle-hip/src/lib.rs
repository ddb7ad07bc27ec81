//! `HipWhisperEngine` and `HipParakeetEngine`: the `transcribe_rs::TranscriptionEngine` surfaces
//! Spittle binds to, backed by the MI355X-native library (`libspittle_hip.so`, C ABI 14), plus `HipFrameResampler` and
//! `HipSmoothedVad` (the capture-side resampler and voice-activity gate).
//!
//! What it replaces in the app (/root/reference/src-tauri/src/managers/transcription.rs):
//!
//! | app call site | transcribe-rs `WhisperEngine` | here |
//! |---|---|---|
//! | `:29-34` `LoadedEngine::Whisper(WhisperEngine)` | engine type | `HipWhisperEngine` (feature swap) |
//! | `:261-276` | `WhisperEngine::new()` + `load_model(&path)` | `new()` + `load_model` (ggml `.bin` from the catalog) |
//! | `:494-503` | `transcribe_samples(audio, Some(WhisperInferenceParams { language, translate, initial_prompt, ..Default::default() }))` | same call |
//! | `:175-208` | `unload_model()` / `Drop` | same |
//!
//! The trait and parameter types come from transcribe-rs 0.2.3 itself, so the app's code at
//! those sites compiles unchanged.  The trait's shape (associated `InferenceParams` /
//! `ModelParams`, `load_model_with_params`, `transcribe_samples(Vec<f32>, Option<_>)`) is
//! restated from the published crate, which is not vendored in the reference
//! [upstream, unverifiable offline].
//!
//! Threading: the app loads from a spawned thread, transcribes from a tokio worker and unloads
//! from the idle watcher, serialised by one Mutex (transcription.rs:36-47, 437).  A context
//! selects its device on every entry point, so the engine is `Send`; it is not `Sync`.

use std::error::Error;
use std::ffi::{CStr, CString};
use std::os::raw::c_char;
use std::path::Path;

use spittle_hip_sys as sys;
use transcribe_rs::engines::parakeet::{ParakeetInferenceParams, TimestampGranularity};
use transcribe_rs::engines::whisper::WhisperInferenceParams;
use transcribe_rs::{TranscriptionEngine, TranscriptionResult, TranscriptionSegment};

/// Device-side model parameters (`spt_model_params`).  The defaults are what the app needs:
/// bf16 weights on device 0, one utterance (and up to 7 more 30 s windows of it) per call.
#[derive(Clone, Copy, Debug)]
pub struct HipModelParams {
    /// true: bf16 weights and activations; false: f32.  The fp16 engine (ABI 14) is asked for with
    /// `HipWhisperEngine::load_model_f16` / `HipWhisperReplicas::load_f16`, which ignore this field.
    pub bf16: bool,
    pub device: i32,
    pub max_batch: i32,
}

impl Default for HipModelParams {
    fn default() -> Self {
        Self { bf16: true, device: 0, max_batch: 8 }
    }
}

/// `model_params` with the fp16 engine (`SPT_DTYPE_F16`, ABI 14): an f16 ggml file's matrices bit
/// for bit, f16 activations at the GEMM inputs, the bf16 engine's memory footprint.
fn model_params_f16(p: &HipModelParams) -> sys::spt_model_params {
    let mut mp = model_params(p);
    mp.dtype = sys::SPT_DTYPE_F16;
    mp
}

fn model_params(p: &HipModelParams) -> sys::spt_model_params {
    let mut mp = std::mem::MaybeUninit::<sys::spt_model_params>::uninit();
    // SAFETY: spt_default_model_params fills every field of the struct
    let mut mp = unsafe {
        sys::spt_default_model_params(mp.as_mut_ptr());
        mp.assume_init()
    };
    mp.dtype = if p.bf16 { sys::SPT_DTYPE_BF16 } else { sys::SPT_DTYPE_F32 };
    mp.device = p.device;
    mp.max_batch = p.max_batch;
    mp
}

fn status_error(what: &str, st: sys::spt_status, msg: String) -> Box<dyn Error> {
    format!("{what} failed (status {st}): {msg}").into()
}

/// The request's parameters, with the CStrings their pointers borrow kept alive beside them.
struct Request {
    ip: sys::spt_infer_params,
    _language: Option<CString>,
    _prompt: Option<CString>,
}

/// whisper_full's defaults (`spt_default_infer_params`) plus the fields the app sets
/// (transcription.rs:445-499): language (None or "auto" = auto-detect), translate,
/// initial_prompt (the jargon prompt, jargon.rs:594), and the two suppression switches
/// `WhisperInferenceParams` carries.
fn request(params: Option<WhisperInferenceParams>) -> Result<Request, Box<dyn Error>> {
    let params = params.unwrap_or_default();
    let language = params.language.clone().map(CString::new).transpose()?;
    let prompt = params.initial_prompt.clone().map(CString::new).transpose()?;
    let mut ip = std::mem::MaybeUninit::<sys::spt_infer_params>::uninit();
    // SAFETY: spt_default_infer_params fills every field of the struct
    let mut ip = unsafe {
        sys::spt_default_infer_params(ip.as_mut_ptr());
        ip.assume_init()
    };
    ip.language = language.as_ref().map_or(std::ptr::null(), |s| s.as_ptr());
    ip.translate = params.translate as i32;
    ip.initial_prompt = prompt.as_ref().map_or(std::ptr::null(), |s| s.as_ptr());
    if params.suppress_non_speech_tokens {
        ip.flags |= sys::SPT_SUPPRESS_NST;
    }
    if !params.suppress_blank {
        ip.flags &= !sys::SPT_SUPPRESS_BLANK;
    }
    Ok(Request { ip, _language: language, _prompt: prompt })
}

/// Copy a library-owned result into transcribe-rs' type and release it.
///
/// SAFETY: `r` must be a result returned by the library and not yet freed.
unsafe fn take_result(r: *mut sys::spt_result) -> TranscriptionResult {
    let res = &*r;
    let text = if res.text.is_null() { String::new() } else { CStr::from_ptr(res.text).to_string_lossy().into_owned() };
    let segments = (0..res.n_segments.max(0) as usize)
        .map(|i| {
            let s = &*res.segments.add(i);
            TranscriptionSegment {
                // whisper_full_get_segment_t0 / t1 are in 10 ms units
                start: s.t0 as f32 / 100.0,
                end: s.t1 as f32 / 100.0,
                text: if s.text.is_null() { String::new() } else { CStr::from_ptr(s.text).to_string_lossy().into_owned() },
            }
        })
        .collect();
    sys::spt_result_free(r);
    TranscriptionResult { text, segments: Some(segments) }
}

/// A text token's time from the alignment heads' cross-attention (`SPT_HAS_TOKEN_TIMESTAMPS`).
#[derive(Debug, Clone, PartialEq)]
pub struct TokenTime {
    /// seconds, as `TranscriptionSegment`
    pub start: f32,
    pub end: f32,
    /// the token's probability
    pub probability: f32,
    /// its index among the call's result tokens
    pub index: usize,
}

/// A word: text tokens joined at leading spaces (a split UTF-8 character kept whole).
#[derive(Debug, Clone, PartialEq)]
pub struct WordTime {
    pub start: f32,
    pub end: f32,
    pub text: String,
    /// mean of its tokens' probabilities
    pub probability: f32,
    /// its tokens: `tokens[first_token .. first_token + n_tokens]` of the `AlignedTranscription`
    pub first_token: usize,
    pub n_tokens: usize,
}

/// `transcribe_samples_aligned`'s result: what `transcribe_samples` returns on the whisper_full path,
/// plus a time for every text token and (ggml models) every word.
pub struct AlignedTranscription {
    pub result: TranscriptionResult,
    pub tokens: Vec<TokenTime>,
    pub words: Vec<WordTime>,
}

/// Copy a library-owned alignment into owned values and release it.
///
/// SAFETY: `a` must be an alignment returned by the library and not yet freed.
unsafe fn take_alignment(a: *mut sys::spt_alignment) -> (Vec<TokenTime>, Vec<WordTime>) {
    let al = &*a;
    let tokens = (0..al.n_tokens.max(0) as usize)
        .map(|i| {
            let t = &*al.tokens.add(i);
            TokenTime { start: t.t0 as f32 / 100.0, end: t.t1 as f32 / 100.0, probability: t.p, index: t.index.max(0) as usize }
        })
        .collect();
    let words = if al.words.is_null() {
        Vec::new()
    } else {
        (0..al.n_words.max(0) as usize)
            .map(|i| {
                let w = &*al.words.add(i);
                WordTime {
                    start: w.t0 as f32 / 100.0,
                    end: w.t1 as f32 / 100.0,
                    text: if w.text.is_null() { String::new() } else { CStr::from_ptr(w.text).to_string_lossy().into_owned() },
                    probability: w.p,
                    first_token: w.i0.max(0) as usize,
                    n_tokens: w.n_tokens.max(0) as usize,
                }
            })
            .collect()
    };
    sys::spt_alignment_free(a);
    (tokens, words)
}

/// One Whisper model on one MI355X.
pub struct HipWhisperEngine {
    ctx: *mut sys::spt_ctx,
    no_speech_thold: f32,
    no_speech_prob: bool,
    block_prefill: bool,
}

/// The last call's prefix prefill (`spt_get_prefill_stats`, `SPT_HAS_BLOCK_PREFILL`).
#[derive(Debug, Clone, Copy, PartialEq, Eq)]
pub struct PrefillStats {
    /// block passes run, one per decode-group slice
    pub block_passes: i32,
    /// prefix rows they carried
    pub block_rows: i32,
    /// chunked prefill passes of at most 4 positions
    pub chunk_passes: i32,
}

/// The cross K/V cache of a loaded model (`spt_get_cross_kv_info`, `SPT_HAS_CROSS_KV_F8`).
#[derive(Debug, Clone, Copy, PartialEq, Eq)]
pub struct CrossKvInfo {
    /// e4m3 codes with a scale per key row (`load_model_cross_kv_f8`), else the engine dtype
    pub fp8: bool,
    /// bytes of the cache in the workspace
    pub cache_bytes: i64,
    /// bytes of the 16-bit staging buffer an fp8 cache is filled through (0 otherwise)
    pub staging_bytes: i64,
}

/// One window of the last call (`spt_get_window_info`, `SPT_HAS_NO_SPEECH`).
#[derive(Debug, Clone, PartialEq)]
pub struct WindowInfo {
    /// index in the call's batch
    pub utterance: usize,
    /// 10 ms frames
    pub seek: i32,
    pub seek_delta: i32,
    /// the window's tokens among the utterance's result tokens (none when skipped)
    pub first_token: usize,
    pub n_tokens: usize,
    /// index of the temperature kept, and that temperature
    pub n_fallbacks: i32,
    pub temperature: f32,
    /// the kept decoder's average log-probability (NaN on the fast path)
    pub avg_logprob: f32,
    /// NaN when not computed
    pub no_speech_prob: f32,
    pub skipped: bool,
}

// SAFETY: a context is not thread-affine (every entry point selects its device); the app
// serialises all calls through one Mutex, which is what `Send` without `Sync` expresses.
unsafe impl Send for HipWhisperEngine {}

impl HipWhisperEngine {
    pub fn new() -> Self {
        Self { ctx: std::ptr::null_mut(), no_speech_thold: 0.0, no_speech_prob: false, block_prefill: false }
    }

    fn last_error(&self) -> String {
        // SAFETY: spt_last_error accepts any context pointer (a static string for null)
        unsafe { CStr::from_ptr(sys::spt_last_error(self.ctx)).to_string_lossy().into_owned() }
    }

    fn need(&self) -> Result<(), Box<dyn Error>> {
        if self.ctx.is_null() {
            return Err("Model is not loaded for transcription.".into());
        }
        Ok(())
    }

    /// whisper.cpp >= 1.7.3's `no_speech_thold` for the calls that follow: a window whose no-speech
    /// probability is above `thold` and whose average log-probability is below `logprob_thold` is
    /// dropped.  On iff 0 < thold < 1; 0 (the default: the reference's whisper.cpp 1.7.1 never reads
    /// the parameter) is off.  `report`: compute each window's probability for `window_info` even
    /// with the threshold off.  A negative or NaN threshold fails the next call.
    pub fn set_no_speech(&mut self, thold: f32, report: bool) {
        self.no_speech_thold = thold;
        self.no_speech_prob = report;
    }

    /// `SPT_BLOCK_PREFILL` for the calls that follow: a prompt prefix (`initial_prompt`, or
    /// whisper_full's `prompt_past` of a later window) of at least 17 positions (16 prompt tokens) runs as one block pass per
    /// sequence slice instead of chunks of 4 positions.  Off by default; the low bits of the results
    /// differ from the chunked path's.  Ignored by a model loaded with `load_model_quant_resident`.
    pub fn set_block_prefill(&mut self, on: bool) {
        self.block_prefill = on;
    }

    /// What the last transcribe call's prefix prefill ran.
    pub fn prefill_stats(&self) -> Result<PrefillStats, Box<dyn Error>> {
        self.need()?;
        let (mut a, mut b, mut c) = (0i32, 0i32, 0i32);
        // SAFETY: a live context and three valid out-pointers
        let st = unsafe { sys::spt_get_prefill_stats(self.ctx, &mut a, &mut b, &mut c) };
        if st != sys::SPT_OK {
            return Err(status_error("prefill stats", st, self.last_error()));
        }
        Ok(PrefillStats { block_passes: a, block_rows: b, chunk_passes: c })
    }

    // the engine's per-call options (set_no_speech, set_block_prefill) into a request
    fn apply_no_speech(&self, rq: &mut Request) {
        rq.ip.no_speech_thold = self.no_speech_thold;
        if self.no_speech_prob {
            rq.ip.flags |= sys::SPT_NO_SPEECH_PROB;
        }
        if self.block_prefill {
            rq.ip.flags |= sys::SPT_BLOCK_PREFILL;
        }
    }

    /// One record per window of the last transcribe call, in decode order per utterance.
    pub fn window_info(&self) -> Result<Vec<WindowInfo>, Box<dyn Error>> {
        self.need()?;
        let mut n = 0i32;
        // SAFETY: a live context; cap 0 writes nothing
        let st = unsafe { sys::spt_get_window_info(self.ctx, std::ptr::null_mut(), 0, &mut n) };
        if st != sys::SPT_OK {
            return Err(status_error("window info", st, self.last_error()));
        }
        let zero = sys::spt_window_info {
            utterance: 0, seek: 0, seek_delta: 0, i0: 0, n_tokens: 0, n_fallbacks: 0, temperature: 0.0,
            avg_logprob: 0.0, no_speech_prob: 0.0, skipped: 0,
        };
        let mut buf = vec![zero; n.max(0) as usize];
        // SAFETY: buf holds `cap` writable records
        let st = unsafe { sys::spt_get_window_info(self.ctx, buf.as_mut_ptr(), buf.len() as i32, &mut n) };
        if st != sys::SPT_OK {
            return Err(status_error("window info", st, self.last_error()));
        }
        buf.truncate(n.max(0) as usize);
        Ok(buf
            .iter()
            .map(|w| WindowInfo {
                utterance: w.utterance as usize,
                seek: w.seek,
                seek_delta: w.seek_delta,
                first_token: w.i0 as usize,
                n_tokens: w.n_tokens as usize,
                n_fallbacks: w.n_fallbacks,
                temperature: w.temperature,
                avg_logprob: w.avg_logprob,
                no_speech_prob: w.no_speech_prob,
                skipped: w.skipped != 0,
            })
            .collect())
    }

    fn load_model_raw(&mut self, model_path: &Path, mp: sys::spt_model_params) -> Result<(), Box<dyn Error>> {
        TranscriptionEngine::unload_model(self);
        // the catalog's ggml-*.bin (managers/model.rs:804-847)
        let spec = CString::new(model_path.to_string_lossy().as_bytes())?;
        let mut err = vec![0 as c_char; 1024];
        let mut ctx = std::ptr::null_mut();
        // SAFETY: valid C strings and out-pointers for the duration of the call
        let st = unsafe { sys::spt_ctx_create(spec.as_ptr(), &mp, &mut ctx, err.as_mut_ptr(), err.len()) };
        if st != sys::SPT_OK {
            // SAFETY: the library NUL-terminates err
            let msg = unsafe { CStr::from_ptr(err.as_ptr()) }.to_string_lossy().into_owned();
            return Err(status_error("model load", st, msg));
        }
        self.ctx = ctx;
        Ok(())
    }

    /// `load_model_with_params` with the fp16 engine (ABI 14, `SPT_DTYPE_F16`): the catalog's f16
    /// files are held bit for bit, at the bf16 engine's memory footprint.  `params.bf16` is ignored.
    pub fn load_model_f16(&mut self, model_path: &Path, params: HipModelParams) -> Result<(), Box<dyn Error>> {
        self.load_model_raw(model_path, model_params_f16(&params))
    }

    /// Load option `SPT_MODEL_QUANT_RESIDENT`: the file's q4_1 / q5_0 / q5_1 decoder matrices and token
    /// embedding stay quantised in HBM (the catalog's `large`, ggml-large-v3-q5_0.bin, and `medium`,
    /// whisper-medium-q4_1.bin, are the files this serves; q5_K `breeze-asr` loads with nothing
    /// resident).  Results are bit for bit those of `load_model_with_params` / `load_model_f16`; the
    /// weight arena shrinks, the decode pass does not get faster.  `f16`: the fp16 engine, else bf16
    /// (`params.bf16` is ignored: the f32 engine keeps no quantised matrices).
    pub fn load_model_quant_resident(&mut self, model_path: &Path, params: HipModelParams, f16: bool) -> Result<(), Box<dyn Error>> {
        let mut mp = model_params_f16(&params);
        if !f16 {
            mp.dtype = sys::SPT_DTYPE_BF16;
        }
        mp.flags |= sys::SPT_MODEL_QUANT_RESIDENT;
        self.load_model_raw(model_path, mp)
    }

    /// Load option `SPT_MODEL_CROSS_KV_F8`: the decoder's cross K/V cache is kept in fp8 e4m3 with one f32
    /// scale per key row, 0.531 of the 16-bit cache.  Results differ from the unflagged model's within
    /// the model's own tolerances; `transcribe_aligned*` is refused, `set_block_prefill` is ignored.
    /// `f16`: the fp16 engine, else bf16; `quant_resident` adds `SPT_MODEL_QUANT_RESIDENT`.
    pub fn load_model_cross_kv_f8(&mut self, model_path: &Path, params: HipModelParams, f16: bool, quant_resident: bool) -> Result<(), Box<dyn Error>> {
        let mut mp = model_params_f16(&params);
        if !f16 {
            mp.dtype = sys::SPT_DTYPE_BF16;
        }
        mp.flags |= sys::SPT_MODEL_CROSS_KV_F8;
        if quant_resident {
            mp.flags |= sys::SPT_MODEL_QUANT_RESIDENT;
        }
        self.load_model_raw(model_path, mp)
    }

    /// The loaded model's cross K/V cache: its format and bytes.
    pub fn cross_kv_info(&self) -> Result<CrossKvInfo, Box<dyn Error>> {
        self.need()?;
        let (mut f, mut c, mut s) = (0i32, 0i64, 0i64);
        // SAFETY: a live context and three valid out-pointers
        let st = unsafe { sys::spt_get_cross_kv_info(self.ctx, &mut f, &mut c, &mut s) };
        if st != sys::SPT_OK {
            return Err(status_error("cross K/V info", st, self.last_error()));
        }
        Ok(CrossKvInfo { fp8: f == 1, cache_bytes: c, staging_bytes: s })
    }

    /// What `load_model_quant_resident` kept: (weights held quantised, their bytes in the arena, their
    /// ggml type or -1 for none / several).
    pub fn weight_residency(&self) -> Result<(i64, i64, i32), Box<dyn Error>> {
        self.need()?;
        let (mut w, mut b, mut t) = (0i64, 0i64, -1i32);
        // SAFETY: a live context and three valid out-pointers
        let st = unsafe { sys::spt_get_weight_residency(self.ctx, &mut w, &mut b, &mut t) };
        if st != sys::SPT_OK {
            return Err(status_error("weight residency", st, self.last_error()));
        }
        Ok((w, b, t))
    }

    /// Several utterances in one call (each <= 30 s window is a batch row).
    pub fn transcribe_batch(
        &mut self,
        batch: &[Vec<f32>],
        params: Option<WhisperInferenceParams>,
    ) -> Result<Vec<TranscriptionResult>, Box<dyn Error>> {
        self.need()?;
        let mut rq = request(params)?;
        self.apply_no_speech(&mut rq);
        let ptrs: Vec<*const f32> = batch.iter().map(|a| a.as_ptr()).collect();
        let lens: Vec<usize> = batch.iter().map(|a| a.len()).collect();
        let mut out = vec![std::ptr::null_mut::<sys::spt_result>(); batch.len()];
        // SAFETY: every pointer is valid for its length for the duration of the call
        let st = unsafe {
            sys::spt_transcribe_batch(self.ctx, ptrs.as_ptr(), lens.as_ptr(), batch.len(), &rq.ip, out.as_mut_ptr())
        };
        if st != sys::SPT_OK {
            return Err(status_error("transcription", st, self.last_error()));
        }
        // SAFETY: on success every out[i] is a live library result
        Ok(out.into_iter().map(|r| unsafe { take_result(r) }).collect())
    }

    /// The alignment heads as (layer, head) pairs; an empty slice restores the default, every head of
    /// the top half of the decoder layers (`spt_set_alignment_heads`).
    pub fn set_alignment_heads(&mut self, pairs: &[(i32, i32)]) -> Result<(), Box<dyn Error>> {
        self.need()?;
        let flat: Vec<i32> = pairs.iter().flat_map(|&(l, h)| vec![l, h]).collect();
        // SAFETY: a live context and 2 * pairs.len() readable values
        let st = unsafe { sys::spt_set_alignment_heads(self.ctx, flat.as_ptr(), pairs.len() as i32) };
        if st != sys::SPT_OK {
            return Err(status_error("alignment heads", st, self.last_error()));
        }
        Ok(())
    }

    /// `transcribe_samples` on the whisper_full path with DTW token and word timestamps (whisper.cpp's
    /// `dtw_token_timestamps`): one extra teacher-forced replay of each window's kept decoder.
    pub fn transcribe_samples_aligned(
        &mut self,
        samples: Vec<f32>,
        params: Option<WhisperInferenceParams>,
    ) -> Result<AlignedTranscription, Box<dyn Error>> {
        let mut v = self.transcribe_batch_aligned(&[samples], params)?;
        v.pop().ok_or_else(|| "no result".into())
    }

    /// Several utterances in one aligned call.
    pub fn transcribe_batch_aligned(
        &mut self,
        batch: &[Vec<f32>],
        params: Option<WhisperInferenceParams>,
    ) -> Result<Vec<AlignedTranscription>, Box<dyn Error>> {
        self.need()?;
        let mut rq = request(params)?;
        self.apply_no_speech(&mut rq);
        let ptrs: Vec<*const f32> = batch.iter().map(|a| a.as_ptr()).collect();
        let lens: Vec<usize> = batch.iter().map(|a| a.len()).collect();
        let mut out = vec![std::ptr::null_mut::<sys::spt_result>(); batch.len()];
        let mut al = vec![std::ptr::null_mut::<sys::spt_alignment>(); batch.len()];
        // SAFETY: every pointer is valid for its length for the duration of the call
        let st = unsafe {
            sys::spt_transcribe_aligned_batch(
                self.ctx,
                ptrs.as_ptr(),
                lens.as_ptr(),
                batch.len(),
                &rq.ip,
                out.as_mut_ptr(),
                al.as_mut_ptr(),
            )
        };
        if st != sys::SPT_OK {
            return Err(status_error("aligned transcription", st, self.last_error()));
        }
        // SAFETY: on success every out[i] and al[i] is live and owned by us until taken (and freed) here
        Ok(out
            .into_iter()
            .zip(al)
            .map(|(r, a)| unsafe {
                let result = take_result(r);
                let (tokens, words) = take_alignment(a);
                AlignedTranscription { result, tokens, words }
            })
            .collect())
    }
}

impl Default for HipWhisperEngine {
    fn default() -> Self {
        Self::new()
    }
}

impl TranscriptionEngine for HipWhisperEngine {
    type InferenceParams = WhisperInferenceParams;
    type ModelParams = HipModelParams;

    fn load_model_with_params(&mut self, model_path: &Path, params: HipModelParams) -> Result<(), Box<dyn Error>> {
        self.load_model_raw(model_path, model_params(&params))
    }

    fn unload_model(&mut self) {
        if !self.ctx.is_null() {
            // SAFETY: the context came from spt_ctx_create and is destroyed once
            unsafe { sys::spt_ctx_destroy(self.ctx) };
            self.ctx = std::ptr::null_mut();
        }
    }

    /// The app's call (transcription.rs:501-503).  `samples` (16 kHz mono f32) is borrowed for
    /// the call and copied to the device; the result's `text` is whisper_full's segment texts
    /// joined and trimmed, `segments` carries their times.
    fn transcribe_samples(
        &mut self,
        samples: Vec<f32>,
        params: Option<WhisperInferenceParams>,
    ) -> Result<TranscriptionResult, Box<dyn Error>> {
        self.need()?;
        let mut rq = request(params)?;
        self.apply_no_speech(&mut rq);
        let mut out = std::ptr::null_mut();
        // SAFETY: samples outlives the call; out receives a library-owned result
        let st = unsafe { sys::spt_transcribe(self.ctx, samples.as_ptr(), samples.len(), &rq.ip, &mut out) };
        if st != sys::SPT_OK {
            return Err(status_error("transcription", st, self.last_error()));
        }
        // SAFETY: a successful call returns a live result
        Ok(unsafe { take_result(out) })
    }
}

impl Drop for HipWhisperEngine {
    fn drop(&mut self) {
        self.unload_model();
    }
}

/// One model replicated over several MI355X of a node: device 0 loads it, one
/// RCCL broadcast over xGMI fills the others; a batch of utterances is split into contiguous
/// shards, one per device, transcribed concurrently.
pub struct HipWhisperReplicas {
    ctxs: Vec<*mut sys::spt_ctx>,
    /// wall time of the weight broadcast at load, ms
    pub broadcast_ms: f64,
}

// SAFETY: as for HipWhisperEngine
unsafe impl Send for HipWhisperReplicas {}

impl HipWhisperReplicas {
    pub fn load(model_path: &Path, params: HipModelParams, devices: &[i32]) -> Result<Self, Box<dyn Error>> {
        Self::load_raw(model_path, model_params(&params), devices)
    }

    /// `load` with the fp16 engine on every device (ABI 14; `params.bf16` is ignored).
    pub fn load_f16(model_path: &Path, params: HipModelParams, devices: &[i32]) -> Result<Self, Box<dyn Error>> {
        Self::load_raw(model_path, model_params_f16(&params), devices)
    }

    fn load_raw(model_path: &Path, mp: sys::spt_model_params, devices: &[i32]) -> Result<Self, Box<dyn Error>> {
        let spec = CString::new(model_path.to_string_lossy().as_bytes())?;
        let mut ctxs = vec![std::ptr::null_mut(); devices.len()];
        let mut ms = 0.0f64;
        let mut err = vec![0 as c_char; 1024];
        // SAFETY: buffers sized for devices.len() contexts
        let st = unsafe {
            sys::spt_ctx_create_replicas(
                spec.as_ptr(),
                &mp,
                devices.as_ptr(),
                devices.len() as i32,
                ctxs.as_mut_ptr(),
                &mut ms,
                err.as_mut_ptr(),
                err.len(),
            )
        };
        if st != sys::SPT_OK {
            // SAFETY: the library NUL-terminates err
            let msg = unsafe { CStr::from_ptr(err.as_ptr()) }.to_string_lossy().into_owned();
            return Err(status_error("replica load", st, msg));
        }
        Ok(Self { ctxs, broadcast_ms: ms })
    }

    pub fn transcribe_batch(
        &mut self,
        batch: &[Vec<f32>],
        params: Option<WhisperInferenceParams>,
    ) -> Result<Vec<TranscriptionResult>, Box<dyn Error>> {
        let rq = request(params)?;
        let ptrs: Vec<*const f32> = batch.iter().map(|a| a.as_ptr()).collect();
        let lens: Vec<usize> = batch.iter().map(|a| a.len()).collect();
        let mut out = vec![std::ptr::null_mut::<sys::spt_result>(); batch.len()];
        // SAFETY: every pointer is valid for its length for the duration of the call
        let st = unsafe {
            sys::spt_transcribe_batch_replicas(
                self.ctxs.as_ptr(),
                self.ctxs.len() as i32,
                ptrs.as_ptr(),
                lens.as_ptr(),
                batch.len(),
                &rq.ip,
                out.as_mut_ptr(),
            )
        };
        if st != sys::SPT_OK {
            // SAFETY: ctxs[0] is live; it carries the failing replica's message
            let msg = unsafe { CStr::from_ptr(sys::spt_last_error(self.ctxs[0])) }.to_string_lossy().into_owned();
            return Err(status_error("replica transcription", st, msg));
        }
        // SAFETY: on success every out[i] is a live library result
        Ok(out.into_iter().map(|r| unsafe { take_result(r) }).collect())
    }
}

impl Drop for HipWhisperReplicas {
    fn drop(&mut self) {
        for c in self.ctxs.drain(..) {
            // SAFETY: each context is destroyed once
            unsafe { sys::spt_ctx_destroy(c) };
        }
    }
}

/// Device-side Parakeet parameters (`spt_pk_model_params`).  `int8()` mirrors the app's
/// `ParakeetModelParams::int8()` (transcription.rs:281); the network runs with an fp16 encoder.
/// `int8_exact()` runs the int8 export's own arithmetic instead (`SPT_DTYPE_I8`: every encoder
/// Linear and pointwise convolution as DynamicQuantizeLinear -> MatMulInteger on the stored
/// integers, the rest f32); it takes precedence over `fp16`.
#[derive(Clone, Copy, Debug)]
pub struct HipParakeetModelParams {
    pub fp16: bool,
    pub int8_exact: bool,
    pub device: i32,
    pub max_batch: i32,
    pub max_seconds: f32,
}

impl HipParakeetModelParams {
    pub fn int8() -> Self {
        Self { fp16: true, int8_exact: false, device: 0, max_batch: 8, max_seconds: 30.0 }
    }
    pub fn int8_exact() -> Self {
        Self { fp16: false, int8_exact: true, device: 0, max_batch: 8, max_seconds: 30.0 }
    }
}

impl Default for HipParakeetModelParams {
    fn default() -> Self {
        Self::int8()
    }
}

/// Parakeet-V3 (FastConformer-TDT) on one MI355X.  What it replaces: `LoadedEngine::Parakeet`
/// (transcription.rs:278-297 load, :505-513 `transcribe_samples` with
/// `TimestampGranularity::Segment`).  The model path is a synthetic spec; a NeMo checkpoint is
/// mapped onto the context tensor by tensor with `set_tensor`.
pub struct HipParakeetEngine {
    ctx: *mut sys::spt_pk_ctx,
}

// SAFETY: as for HipWhisperEngine (calls serialised by the app's Mutex; not thread-affine)
unsafe impl Send for HipParakeetEngine {}

impl HipParakeetEngine {
    pub fn new() -> Self {
        Self { ctx: std::ptr::null_mut() }
    }

    fn last_error(&self) -> String {
        // SAFETY: accepts any context pointer (a static string for null)
        unsafe { CStr::from_ptr(sys::spt_parakeet_last_error(self.ctx)).to_string_lossy().into_owned() }
    }

    /// One weight tensor (f32, NeMo layout) by the id table of oracle/po_model.c.
    pub fn set_tensor(&mut self, tensor_id: i32, data: &[f32]) -> Result<(), Box<dyn Error>> {
        // SAFETY: data is valid for its length during the call
        let st = unsafe { sys::spt_parakeet_set_tensor(self.ctx, tensor_id, data.as_ptr(), data.len() as i64) };
        if st != sys::SPT_OK {
            return Err(status_error("set_tensor", st, self.last_error()));
        }
        Ok(())
    }
}

impl Default for HipParakeetEngine {
    fn default() -> Self {
        Self::new()
    }
}

fn granularity(g: &TimestampGranularity) -> i32 {
    match g {
        TimestampGranularity::Token => sys::SPT_PK_TS_TOKEN,
        TimestampGranularity::Word => sys::SPT_PK_TS_WORD,
        TimestampGranularity::Segment => sys::SPT_PK_TS_SEGMENT,
    }
}

impl TranscriptionEngine for HipParakeetEngine {
    type InferenceParams = ParakeetInferenceParams;
    type ModelParams = HipParakeetModelParams;

    fn load_model_with_params(&mut self, model_path: &Path, params: HipParakeetModelParams) -> Result<(), Box<dyn Error>> {
        self.unload_model();
        let spec = CString::new(model_path.to_string_lossy().as_bytes())?;
        let mut mp = std::mem::MaybeUninit::<sys::spt_pk_model_params>::uninit();
        // SAFETY: fills every field
        let mut mp = unsafe {
            sys::spt_parakeet_default_model_params(mp.as_mut_ptr());
            mp.assume_init()
        };
        mp.dtype = if params.int8_exact {
            sys::SPT_DTYPE_I8
        } else if params.fp16 {
            sys::SPT_DTYPE_F16
        } else {
            sys::SPT_DTYPE_F32
        };
        mp.device = params.device;
        mp.max_batch = params.max_batch;
        mp.max_seconds = params.max_seconds;
        let mut err = vec![0 as c_char; 1024];
        let mut ctx = std::ptr::null_mut();
        // SAFETY: valid C strings and out-pointers for the duration of the call
        let st = unsafe { sys::spt_parakeet_create(spec.as_ptr(), &mp, &mut ctx, err.as_mut_ptr(), err.len()) };
        if st != sys::SPT_OK {
            // SAFETY: the library NUL-terminates err
            let msg = unsafe { CStr::from_ptr(err.as_ptr()) }.to_string_lossy().into_owned();
            return Err(status_error("model load", st, msg));
        }
        self.ctx = ctx;
        Ok(())
    }

    fn unload_model(&mut self) {
        if !self.ctx.is_null() {
            // SAFETY: created by spt_parakeet_create, destroyed once
            unsafe { sys::spt_parakeet_destroy(self.ctx) };
            self.ctx = std::ptr::null_mut();
        }
    }

    fn transcribe_samples(
        &mut self,
        samples: Vec<f32>,
        params: Option<ParakeetInferenceParams>,
    ) -> Result<TranscriptionResult, Box<dyn Error>> {
        if self.ctx.is_null() {
            return Err("Model is not loaded for transcription.".into());
        }
        let mut ip = sys::spt_pk_infer_params { max_symbols: 10, timestamp_granularity: sys::SPT_PK_TS_SEGMENT };
        // SAFETY: fills every field
        unsafe { sys::spt_parakeet_default_infer_params(&mut ip) };
        if let Some(p) = params.as_ref() {
            ip.timestamp_granularity = granularity(&p.timestamp_granularity);
        }
        let mut out = std::ptr::null_mut();
        // SAFETY: samples outlives the call; out receives a library-owned result
        let st = unsafe { sys::spt_parakeet_transcribe(self.ctx, samples.as_ptr(), samples.len(), &ip, &mut out) };
        if st != sys::SPT_OK {
            return Err(status_error("transcription", st, self.last_error()));
        }
        // SAFETY: a successful call returns a live result, read then freed once
        unsafe {
            let res = &*out;
            let text = if res.text.is_null() { String::new() } else { CStr::from_ptr(res.text).to_string_lossy().into_owned() };
            let segments = (0..res.n_segments.max(0) as usize)
                .map(|i| {
                    let s = &*res.segments.add(i);
                    TranscriptionSegment {
                        start: s.start as f32,
                        end: s.end as f32,
                        text: if s.text.is_null() { String::new() } else { CStr::from_ptr(s.text).to_string_lossy().into_owned() },
                    }
                })
                .collect();
            sys::spt_parakeet_result_free(out);
            Ok(TranscriptionResult { text, segments: Some(segments) })
        }
    }
}

impl Drop for HipParakeetEngine {
    fn drop(&mut self) {
        self.unload_model();
    }
}

/// Which Moonshine geometry a model path holds (transcribe-rs' `ModelVariant`).
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum HipMoonshineVariant {
    Tiny,
    Base,
}

/// Counterpart of `MoonshineModelParams::variant(ModelVariant::Base)`.
#[derive(Clone, Copy, Debug)]
pub struct HipMoonshineModelParams {
    pub variant: HipMoonshineVariant,
    pub device: i32,
    pub max_batch: i32,
    /// the longest utterance taken, in 16 kHz samples (default 64 s)
    pub max_samples: i32,
}

impl HipMoonshineModelParams {
    pub fn variant(variant: HipMoonshineVariant) -> Self {
        Self { variant, device: 0, max_batch: 1, max_samples: 64 * 16000 }
    }
}

impl Default for HipMoonshineModelParams {
    fn default() -> Self {
        Self::variant(HipMoonshineVariant::Base)
    }
}

/// `LoadedEngine::Moonshine` over the device (spt_moonshine_*).  `model_path` is a model spec the
/// library takes ("synthetic:moonshine-base", "empty:moonshine-base" + `set_tensor` per HF
/// state-dict name); the app's ONNX download is not read yet.
pub struct HipMoonshineEngine {
    ctx: *mut sys::spt_ms_ctx,
}

// SAFETY: as for HipWhisperEngine (calls serialised by the app's Mutex; not thread-affine)
unsafe impl Send for HipMoonshineEngine {}

impl HipMoonshineEngine {
    pub fn new() -> Self {
        Self { ctx: std::ptr::null_mut() }
    }

    fn last_error(&self) -> String {
        // SAFETY: accepts any context pointer (a static string for null)
        unsafe { CStr::from_ptr(sys::spt_moonshine_last_error(self.ctx)).to_string_lossy().into_owned() }
    }

    /// One weight tensor (f32, HF layout) by HF state-dict name.
    pub fn set_tensor(&mut self, name: &str, data: &[f32]) -> Result<(), Box<dyn Error>> {
        let cname = CString::new(name)?;
        // SAFETY: name and data are valid for the duration of the call
        let st = unsafe { sys::spt_moonshine_set_tensor(self.ctx, cname.as_ptr(), data.as_ptr(), data.len() as i64) };
        if st != sys::SPT_OK {
            return Err(status_error("set_tensor", st, self.last_error()));
        }
        Ok(())
    }

    /// SentencePiece pieces by id (tokenizer.json's model.vocab and added_tokens).
    pub fn set_vocab(&mut self, pieces: &[String]) -> Result<(), Box<dyn Error>> {
        let owned = pieces.iter().map(|p| CString::new(p.as_bytes())).collect::<Result<Vec<_>, _>>()?;
        let ptrs: Vec<*const c_char> = owned.iter().map(|p| p.as_ptr()).collect();
        // SAFETY: the pointers live until the call returns; the library copies the strings
        let st = unsafe { sys::spt_moonshine_set_vocab(self.ctx, ptrs.as_ptr(), ptrs.len() as i32) };
        if st != sys::SPT_OK {
            return Err(status_error("set_vocab", st, self.last_error()));
        }
        Ok(())
    }

    pub fn load_model_with_params(&mut self, model_path: &Path, params: HipMoonshineModelParams) -> Result<(), Box<dyn Error>> {
        self.unload_model();
        let spec = CString::new(model_path.to_string_lossy().as_bytes())?;
        let mut mp = std::mem::MaybeUninit::<sys::spt_ms_model_params>::uninit();
        // SAFETY: fills every field
        let mut mp = unsafe {
            sys::spt_moonshine_default_model_params(mp.as_mut_ptr());
            mp.assume_init()
        };
        mp.device = params.device;
        mp.max_batch = params.max_batch;
        mp.max_samples = params.max_samples;
        let mut err = vec![0 as c_char; 1024];
        let mut ctx = std::ptr::null_mut();
        // SAFETY: valid C strings and out-pointers for the duration of the call
        let st = unsafe { sys::spt_moonshine_create(spec.as_ptr(), &mp, &mut ctx, err.as_mut_ptr(), err.len()) };
        if st != sys::SPT_OK {
            // SAFETY: the library NUL-terminates err
            let msg = unsafe { CStr::from_ptr(err.as_ptr()) }.to_string_lossy().into_owned();
            return Err(status_error("model load", st, msg));
        }
        self.ctx = ctx;
        let mut info = sys::spt_ms_model_info::default();
        // SAFETY: a live context and a valid out-pointer
        unsafe { sys::spt_moonshine_info(self.ctx, &mut info) };
        let want = match params.variant {
            HipMoonshineVariant::Base => 416,
            HipMoonshineVariant::Tiny => 288,
        };
        if info.d != want {
            self.unload_model();
            return Err(format!("model width {} does not match the requested variant ({})", info.d, want).into());
        }
        Ok(())
    }

    pub fn unload_model(&mut self) {
        if !self.ctx.is_null() {
            // SAFETY: created by spt_moonshine_create, destroyed once
            unsafe { sys::spt_moonshine_destroy(self.ctx) };
            self.ctx = std::ptr::null_mut();
        }
    }

    /// `transcribe_samples(audio, None)`: greedy decoding to </s> or ceil(6.5 tokens per second).
    pub fn transcribe_samples(&mut self, samples: Vec<f32>) -> Result<TranscriptionResult, Box<dyn Error>> {
        if self.ctx.is_null() {
            return Err("Model is not loaded for transcription.".into());
        }
        let mut out = std::ptr::null_mut();
        // SAFETY: samples outlives the call; null params = the defaults; out receives a library-owned result
        let st = unsafe { sys::spt_moonshine_transcribe(self.ctx, samples.as_ptr(), samples.len(), std::ptr::null(), &mut out) };
        if st != sys::SPT_OK {
            return Err(status_error("transcription", st, self.last_error()));
        }
        // SAFETY: a successful call returns a live result, read then freed once
        unsafe {
            let res = &*out;
            let text = if res.text.is_null() { String::new() } else { CStr::from_ptr(res.text).to_string_lossy().into_owned() };
            sys::spt_moonshine_result_free(out);
            Ok(TranscriptionResult { text, segments: None })
        }
    }
}

impl Default for HipMoonshineEngine {
    fn default() -> Self {
        Self::new()
    }
}

impl Drop for HipMoonshineEngine {
    fn drop(&mut self) {
        self.unload_model();
    }
}

/// transcribe-rs' `sense_voice::Language`.
#[derive(Clone, Copy, Debug, PartialEq, Eq, Default)]
pub enum HipSenseVoiceLanguage {
    #[default]
    Auto,
    Chinese,
    English,
    Cantonese,
    Japanese,
    Korean,
}

impl HipSenseVoiceLanguage {
    /// The app's `selected_language` mapping (transcription.rs:518-525).
    pub fn from_code(code: &str) -> Self {
        match code {
            "zh" | "zh-Hans" | "zh-Hant" => Self::Chinese,
            "en" => Self::English,
            "ja" => Self::Japanese,
            "ko" => Self::Korean,
            "yue" => Self::Cantonese,
            _ => Self::Auto,
        }
    }

    fn to_sys(self) -> i32 {
        match self {
            Self::Auto => sys::SPT_SV_LANG_AUTO,
            Self::Chinese => sys::SPT_SV_LANG_ZH,
            Self::English => sys::SPT_SV_LANG_EN,
            Self::Cantonese => sys::SPT_SV_LANG_YUE,
            Self::Japanese => sys::SPT_SV_LANG_JA,
            Self::Korean => sys::SPT_SV_LANG_KO,
        }
    }
}

/// Counterpart of `SenseVoiceModelParams::int8()`; the engine itself runs fp16.
#[derive(Clone, Copy, Debug)]
pub struct HipSenseVoiceModelParams {
    pub device: i32,
    pub max_batch: i32,
    /// the longest utterance taken, in 16 kHz samples (default 64 s)
    pub max_samples: i32,
}

impl HipSenseVoiceModelParams {
    pub fn int8() -> Self {
        Self { device: 0, max_batch: 1, max_samples: 64 * 16000 }
    }
}

impl Default for HipSenseVoiceModelParams {
    fn default() -> Self {
        Self::int8()
    }
}

/// Counterpart of `SenseVoiceInferenceParams { language, use_itn }`.
#[derive(Clone, Copy, Debug, Default)]
pub struct HipSenseVoiceInferenceParams {
    pub language: HipSenseVoiceLanguage,
    pub use_itn: bool,
}

/// `LoadedEngine::SenseVoice` over the device (spt_sensevoice_*).  `model_path` is a model spec the
/// library takes ("synthetic:sensevoice-small", "empty:sensevoice-small" + `set_tensor` per FunASR
/// state-dict name + `set_cmvn`); the app's int8 ONNX download is not read.
pub struct HipSenseVoiceEngine {
    ctx: *mut sys::spt_sv_ctx,
}

// SAFETY: as for HipWhisperEngine (calls serialised by the app's Mutex; not thread-affine)
unsafe impl Send for HipSenseVoiceEngine {}

impl HipSenseVoiceEngine {
    pub fn new() -> Self {
        Self { ctx: std::ptr::null_mut() }
    }

    fn last_error(&self) -> String {
        // SAFETY: accepts any context pointer (a static string for null)
        unsafe { CStr::from_ptr(sys::spt_sensevoice_last_error(self.ctx)).to_string_lossy().into_owned() }
    }

    /// One weight tensor (f32, FunASR layout) by FunASR state-dict name.
    pub fn set_tensor(&mut self, name: &str, data: &[f32]) -> Result<(), Box<dyn Error>> {
        let cname = CString::new(name)?;
        // SAFETY: name and data are valid for the duration of the call
        let st = unsafe { sys::spt_sensevoice_set_tensor(self.ctx, cname.as_ptr(), data.as_ptr(), data.len() as i64) };
        if st != sys::SPT_OK {
            return Err(status_error("set_tensor", st, self.last_error()));
        }
        Ok(())
    }

    /// am.mvn's `<AddShift>` and `<Rescale>` vectors: features = (lfr + neg_mean) * inv_std.
    pub fn set_cmvn(&mut self, neg_mean: &[f32], inv_std: &[f32]) -> Result<(), Box<dyn Error>> {
        if neg_mean.len() != inv_std.len() {
            return Err("CMVN vectors differ in length".into());
        }
        // SAFETY: both slices are valid for the duration of the call
        let st = unsafe { sys::spt_sensevoice_set_cmvn(self.ctx, neg_mean.as_ptr(), inv_std.as_ptr(), neg_mean.len() as i32) };
        if st != sys::SPT_OK {
            return Err(status_error("set_cmvn", st, self.last_error()));
        }
        Ok(())
    }

    /// SentencePiece pieces by id.
    pub fn set_vocab(&mut self, pieces: &[String]) -> Result<(), Box<dyn Error>> {
        let owned = pieces.iter().map(|p| CString::new(p.as_bytes())).collect::<Result<Vec<_>, _>>()?;
        let ptrs: Vec<*const c_char> = owned.iter().map(|p| p.as_ptr()).collect();
        // SAFETY: the pointers live until the call returns; the library copies the strings
        let st = unsafe { sys::spt_sensevoice_set_vocab(self.ctx, ptrs.as_ptr(), ptrs.len() as i32) };
        if st != sys::SPT_OK {
            return Err(status_error("set_vocab", st, self.last_error()));
        }
        Ok(())
    }

    pub fn load_model_with_params(&mut self, model_path: &Path, params: HipSenseVoiceModelParams) -> Result<(), Box<dyn Error>> {
        self.unload_model();
        let spec = CString::new(model_path.to_string_lossy().as_bytes())?;
        let mut mp = std::mem::MaybeUninit::<sys::spt_sv_model_params>::uninit();
        // SAFETY: fills every field
        let mut mp = unsafe {
            sys::spt_sensevoice_default_model_params(mp.as_mut_ptr());
            mp.assume_init()
        };
        mp.device = params.device;
        mp.max_batch = params.max_batch;
        mp.max_samples = params.max_samples;
        let mut err = vec![0 as c_char; 1024];
        let mut ctx = std::ptr::null_mut();
        // SAFETY: valid C strings and out-pointers for the duration of the call
        let st = unsafe { sys::spt_sensevoice_create(spec.as_ptr(), &mp, &mut ctx, err.as_mut_ptr(), err.len()) };
        if st != sys::SPT_OK {
            // SAFETY: the library NUL-terminates err
            let msg = unsafe { CStr::from_ptr(err.as_ptr()) }.to_string_lossy().into_owned();
            return Err(status_error("model load", st, msg));
        }
        self.ctx = ctx;
        Ok(())
    }

    pub fn unload_model(&mut self) {
        if !self.ctx.is_null() {
            // SAFETY: created by spt_sensevoice_create, destroyed once
            unsafe { sys::spt_sensevoice_destroy(self.ctx) };
            self.ctx = std::ptr::null_mut();
        }
    }

    /// `transcribe_samples(audio, Some(params))`: one forward pass and the CTC greedy collapse.
    pub fn transcribe_samples(
        &mut self,
        samples: Vec<f32>,
        params: Option<HipSenseVoiceInferenceParams>,
    ) -> Result<TranscriptionResult, Box<dyn Error>> {
        if self.ctx.is_null() {
            return Err("Model is not loaded for transcription.".into());
        }
        let p = params.unwrap_or_default();
        let ip = sys::spt_sv_infer_params { language: p.language.to_sys(), use_itn: p.use_itn as i32 };
        let mut out = std::ptr::null_mut();
        // SAFETY: samples and ip outlive the call; out receives a library-owned result
        let st = unsafe { sys::spt_sensevoice_transcribe(self.ctx, samples.as_ptr(), samples.len(), &ip, &mut out) };
        if st != sys::SPT_OK {
            return Err(status_error("transcription", st, self.last_error()));
        }
        // SAFETY: a successful call returns a live result, read then freed once
        unsafe {
            let res = &*out;
            let text = if res.text.is_null() { String::new() } else { CStr::from_ptr(res.text).to_string_lossy().into_owned() };
            sys::spt_sensevoice_result_free(out);
            Ok(TranscriptionResult { text, segments: None })
        }
    }
}

impl Default for HipSenseVoiceEngine {
    fn default() -> Self {
        Self::new()
    }
}

impl Drop for HipSenseVoiceEngine {
    fn drop(&mut self) {
        self.unload_model();
    }
}

/// The capture-side resampler (ABI 7): `FrameResampler` of
/// /root/reference/src-tauri/src/audio_toolkit/audio/resampler.rs:7-104 over the device.
/// `process_stream` = `FrameResampler::new(in_hz, out_hz, frame_dur)` + `push(all)` + `finish`
/// (recorder.rs:264-268, 330, 355): the concatenated frames of one recorded stream.  The app's
/// streaming `push` per capture buffer stays on the host; a recording-level caller (or a batch
/// re-import of a file) hands the whole stream over at once.
pub struct HipFrameResampler {
    r: *mut sys::spt_resampler,
}

// SAFETY: the context selects its device on every call and holds no thread-local state
unsafe impl Send for HipFrameResampler {}

impl HipFrameResampler {
    pub fn new(in_hz: u32, out_hz: u32, frame_dur: std::time::Duration, device: i32) -> Result<Self, Box<dyn Error>> {
        let frame_samples = (out_hz as f64 * frame_dur.as_secs_f64()).round() as i32;
        if frame_samples <= 0 {
            return Err("frame duration too short".into());
        }
        let mut r = std::ptr::null_mut();
        let mut err = vec![0 as c_char; 512];
        // SAFETY: out-pointer and error buffer are valid for the call
        let st = unsafe {
            sys::spt_resampler_create(in_hz as i32, out_hz as i32, frame_samples, device, &mut r, err.as_mut_ptr(), err.len())
        };
        if st != sys::SPT_OK {
            // SAFETY: the library NUL-terminates the message inside the buffer
            let msg = unsafe { CStr::from_ptr(err.as_ptr()) }.to_string_lossy().into_owned();
            return Err(status_error("resampler", st, msg));
        }
        Ok(Self { r })
    }

    pub fn process_stream(&mut self, samples: &[f32]) -> Result<Vec<f32>, Box<dyn Error>> {
        // SAFETY: a live context; the length query has no other effect
        let need = unsafe { sys::spt_resample_output_len(self.r, samples.len()) };
        let mut out = vec![0f32; need];
        let mut n_out = 0usize;
        // SAFETY: both buffers outlive the call and `out` holds `need` samples
        let st = unsafe { sys::spt_resample(self.r, samples.as_ptr(), samples.len(), out.as_mut_ptr(), out.len(), &mut n_out) };
        if st != sys::SPT_OK {
            // SAFETY: the message lives in the context until its next call
            let msg = unsafe { CStr::from_ptr(sys::spt_resampler_last_error(self.r)) }.to_string_lossy().into_owned();
            return Err(status_error("resample", st, msg));
        }
        out.truncate(n_out);
        Ok(out)
    }
}

impl Drop for HipFrameResampler {
    fn drop(&mut self) {
        // SAFETY: created by spt_resampler_create, destroyed once
        unsafe { sys::spt_resampler_destroy(self.r) };
    }
}

/// The capture-side voice-activity gate (ABI 8): `SmoothedVad::new(Box::new(SileroVad::new(path,
/// 0.3)), 15, 15, 2)` of /root/reference/src-tauri/src/managers/audio.rs:132-134 in one object,
/// the Silero network on the device.  `push_frame` has the app's `VoiceActivityDetector` shape
/// (audio_toolkit/vad/mod.rs); the app-side adapter is three lines.
pub struct HipSmoothedVad {
    v: *mut sys::spt_vad,
    last: Vec<f32>,
}

/// `VadFrame` of audio_toolkit/vad/mod.rs
pub enum HipVadFrame<'a> {
    Speech(&'a [f32]),
    Noise,
}

// SAFETY: the context selects its device on every call and holds no thread-local state
unsafe impl Send for HipSmoothedVad {}

impl HipSmoothedVad {
    pub fn new<P: AsRef<Path>>(model_path: P, threshold: f32, prefill: usize, hangover: usize, onset: usize,
                               device: i32) -> Result<Self, Box<dyn Error>> {
        let path = CString::new(model_path.as_ref().to_string_lossy().as_bytes())?;
        let mut p = sys::spt_vad_params { threshold, prefill_frames: prefill as i32, hangover_frames: hangover as i32,
                                          onset_frames: onset as i32, device, reserved0: 0 };
        if !(0.0..=1.0).contains(&threshold) {
            return Err("threshold must be between 0.0 and 1.0".into());
        }
        let mut v = std::ptr::null_mut();
        let mut err = vec![0 as c_char; 512];
        // SAFETY: every pointer is valid for the call
        let st = unsafe { sys::spt_vad_create(path.as_ptr(), &mut p, &mut v, err.as_mut_ptr(), err.len()) };
        if st != sys::SPT_OK {
            // SAFETY: the library NUL-terminates the message inside the buffer
            let msg = unsafe { CStr::from_ptr(err.as_ptr()) }.to_string_lossy().into_owned();
            return Err(status_error("vad", st, msg));
        }
        Ok(Self { v, last: Vec::new() })
    }

    /// One 30 ms frame (or a whole recorded stream, frame after frame): the kept samples.
    pub fn push_frame<'a>(&'a mut self, frame: &'a [f32]) -> Result<HipVadFrame<'a>, Box<dyn Error>> {
        let mut r = std::ptr::null_mut();
        // SAFETY: the frame outlives the call; the result is library-owned and freed below
        let st = unsafe { sys::spt_vad_push(self.v, frame.as_ptr(), frame.len(), &mut r) };
        if st != sys::SPT_OK {
            // SAFETY: the message lives in the context until its next call
            let msg = unsafe { CStr::from_ptr(sys::spt_vad_last_error(self.v)) }.to_string_lossy().into_owned();
            return Err(status_error("vad push", st, msg));
        }
        // SAFETY: r is a valid result until spt_vad_result_free
        let (kept, speech) = unsafe {
            let res = &*r;
            let kept = if res.n_samples > 0 { std::slice::from_raw_parts(res.samples, res.n_samples).to_vec() } else { Vec::new() };
            (kept, res.n_frames > 0 && *res.kind != 0)
        };
        // SAFETY: freed once
        unsafe { sys::spt_vad_result_free(r) };
        self.last = kept;
        Ok(if speech { HipVadFrame::Speech(&self.last) } else { HipVadFrame::Noise })
    }

    /// `SmoothedVad::reset` (the Silero state carries over, as in the app)
    pub fn reset(&mut self) {
        // SAFETY: a live context
        unsafe { sys::spt_vad_reset(self.v, 0) };
    }
}

impl Drop for HipSmoothedVad {
    fn drop(&mut self) {
        // SAFETY: created by spt_vad_create, destroyed once
        unsafe { sys::spt_vad_destroy(self.v) };
    }
}
