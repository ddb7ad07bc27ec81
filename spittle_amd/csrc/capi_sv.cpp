// capi_sv.cpp -- the spt_sensevoice_* part of include/spittle_hip.h (additive over ABI 14).
//
// Mirrors transcribe-rs' SenseVoiceEngine as Spittle drives it (load_model_with_params,
// transcribe_samples(audio, Some(SenseVoiceInferenceParams { language, use_itn })), unload): status
// codes + message, borrowed PCM, library-owned results.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "../../include/spittle_hip.h"
#include "capi_err.h"
#include "common.h"
#include "sensevoice.h"

struct spt_sv_ctx {
    std::unique_ptr<spt::SenseVoiceEngine> eng;
    std::vector<std::string> pieces;
    std::string spec, err;
};

namespace {

using spt::classify;
using spt::fail;
using spt::guarded;
using spt::set_err;

spt_sv_result* make_result(const spt_sv_ctx* c, const spt::SvUtt& r) {
    spt_sv_result* o = (spt_sv_result*)calloc(1, sizeof(spt_sv_result));
    if (!o) return nullptr;
    const size_t n = r.tok.size();
    const std::string text = spt::sv_detokenize(c->pieces, r.tok.data(), (int)n);
    o->n_tokens = (int32_t)n;
    for (int i = 0; i < 4; i++) o->prefix[i] = r.prefix[i];
    o->tokens = (int32_t*)malloc(4 * (n ? n : 1));
    o->frames = (int32_t*)malloc(4 * (n ? n : 1));
    o->top1 = (float*)malloc(4 * (n ? n : 1));
    o->top2 = (float*)malloc(4 * (n ? n : 1));
    o->text = (char*)malloc(text.size() + 1);
    if (!o->tokens || !o->frames || !o->top1 || !o->top2 || !o->text) {
        spt_sensevoice_result_free(o);
        return nullptr;
    }
    for (size_t i = 0; i < n; i++) {
        o->tokens[i] = r.tok[i];
        o->frames[i] = r.frame[i];
        o->top1[i] = r.top1[i];
        o->top2[i] = r.top2[i];
    }
    memcpy(o->text, text.c_str(), text.size() + 1);
    return o;
}

bool infer_of(spt_sv_ctx* ctx, const spt_sv_infer_params* params, spt::SvInfer* p) {
    spt_sv_infer_params dp;
    spt_sensevoice_default_infer_params(&dp);
    if (!params) params = &dp;
    if (params->language < 0 || params->language >= spt::SV_N_LANG) {
        fail(ctx, SPT_ERR_INVALID_ARG, "language must be one of SPT_SV_LANG_* (0..5), got " + std::to_string(params->language));
        return false;
    }
    p->language = params->language;
    p->use_itn = params->use_itn != 0;
    return true;
}

}  // namespace

extern "C" {

void spt_sensevoice_default_model_params(spt_sv_model_params* p) {
    if (!p) return;
    const spt::SvDims d;
    memset(p, 0, sizeof(*p));
    p->dtype = SPT_DTYPE_F16;
    p->device = 0;
    p->max_batch = 8;
    p->max_samples = 64 * 16000;
    p->seed = 1234;
    p->ln_eps = d.ln_eps;
    p->sanm_shift = d.sanm_shift;
    p->lfr_m = d.lfr_m;
    p->lfr_n = d.lfr_n;
    p->blank_id = d.blank;
    p->n_prefix = d.n_prefix;
    for (int i = 0; i < spt::SV_N_LANG; i++) p->lang_rows[i] = d.lang_rows[i];
    p->event_row = d.event_row;
    p->emo_row = d.emo_row;
    p->itn_row = d.itn_row;
    p->no_itn_row = d.no_itn_row;
}

void spt_sensevoice_default_infer_params(spt_sv_infer_params* p) {
    if (!p) return;
    p->language = SPT_SV_LANG_AUTO;
    p->use_itn = 0;
}

spt_status spt_sensevoice_create(const char* model_spec, const spt_sv_model_params* params, spt_sv_ctx** out, char* err,
                                 size_t errlen) {
    if (!model_spec || !out) {
        set_err(err, errlen, "null argument");
        return SPT_ERR_INVALID_ARG;
    }
    *out = nullptr;
    spt_sv_model_params mp;
    spt_sensevoice_default_model_params(&mp);
    if (params) mp = *params;
    spt::SvSpec spec;
    std::string perr;
    if (!spt::sv_parse_spec(model_spec, &spec, &perr)) {
        set_err(err, errlen, perr);
        return SPT_ERR_LOAD;
    }
    if (mp.dtype != SPT_DTYPE_F16) {
        set_err(err, errlen, "sensevoice: the engine dtype is SPT_DTYPE_F16 only");
        return SPT_ERR_UNSUPPORTED;
    }
    if (mp.max_batch < 1 || mp.max_batch > 64) {
        set_err(err, errlen, "max_batch must be in [1, 64]");
        return SPT_ERR_INVALID_ARG;
    }
    if (mp.max_samples < spt::SV_FRAME || mp.max_samples > spt::SV_MAX_SAMPLES) {
        set_err(err, errlen, "max_samples must be in [400, 4800000]");
        return SPT_ERR_INVALID_ARG;
    }
    spt::SvDims& d = spec.dims;
    d.ln_eps = mp.ln_eps; d.sanm_shift = mp.sanm_shift; d.lfr_m = mp.lfr_m; d.lfr_n = mp.lfr_n;
    d.blank = mp.blank_id; d.n_prefix = mp.n_prefix;
    for (int i = 0; i < spt::SV_N_LANG; i++) d.lang_rows[i] = mp.lang_rows[i];
    d.event_row = mp.event_row; d.emo_row = mp.emo_row; d.itn_row = mp.itn_row; d.no_itn_row = mp.no_itn_row;
    if (!spt::sv_dims_ok(d, &perr)) {
        set_err(err, errlen, perr);
        return SPT_ERR_INVALID_ARG;
    }
    spt_sv_ctx* c = new (std::nothrow) spt_sv_ctx();
    if (!c) return SPT_ERR_OOM;
    c->spec = model_spec;
    try {
        c->eng.reset(new spt::SenseVoiceEngine(d, mp.device, mp.max_batch, mp.max_samples,
                                               spec.has_seed ? spec.seed : mp.seed, spec.synthetic));
    } catch (const std::exception& e) {
        set_err(err, errlen, e.what());
        const spt_status s = classify(e);
        delete c;
        return s == SPT_ERR_INVALID_ARG ? SPT_ERR_LOAD : s;
    }
    *out = c;
    return SPT_OK;
}

void spt_sensevoice_destroy(spt_sv_ctx* ctx) { delete ctx; }

const char* spt_sensevoice_last_error(const spt_sv_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

spt_status spt_sensevoice_info(const spt_sv_ctx* ctx, spt_sv_model_info* info) {
    if (!ctx || !info) return SPT_ERR_INVALID_ARG;
    const spt::SenseVoiceEngine& e = *ctx->eng;
    const spt::SvDims& d = e.dims();
    memset(info, 0, sizeof(*info));
    info->d = d.d; info->n_heads = d.H; info->head_dim = d.dh; info->ff = d.ff;
    info->n_enc0_layers = d.n0; info->n_enc_layers = d.n1; info->n_tp_layers = d.n2; info->n_vocab = d.vocab;
    info->input_dim = d.in(); info->dtype = SPT_DTYPE_F16; info->max_batch = e.max_batch();
    info->max_samples = e.max_samples(); info->max_rows = e.max_rows();
    info->weight_bytes = e.weight_bytes(); info->workspace_bytes = e.workspace_bytes();
    return SPT_OK;
}

spt_status spt_sensevoice_tensor_numel(const spt_sv_ctx* ctx, const char* name, int64_t* n) {
    if (!ctx || !name || !n) return SPT_ERR_INVALID_ARG;
    const int64_t v = ctx->eng->tensor_numel(name);
    if (v < 0) return SPT_ERR_INVALID_ARG;
    *n = v;
    return SPT_OK;
}

spt_status spt_sensevoice_set_tensor(spt_sv_ctx* ctx, const char* name, const float* data, int64_t n) {
    if (!ctx || !name || !data) return fail(ctx, SPT_ERR_INVALID_ARG, "null argument");
    return guarded(ctx, [&] {
        ctx->eng->set_tensor(name, data, n);
        return SPT_OK;
    });
}

int32_t spt_sensevoice_missing_tensors(const spt_sv_ctx* ctx) { return ctx ? ctx->eng->missing() : -1; }

spt_status spt_sensevoice_set_cmvn(spt_sv_ctx* ctx, const float* neg_mean, const float* inv_std, int32_t n) {
    if (!ctx || !neg_mean || !inv_std) return fail(ctx, SPT_ERR_INVALID_ARG, "null argument");
    return guarded(ctx, [&] {
        ctx->eng->set_cmvn(neg_mean, inv_std, n);
        return SPT_OK;
    });
}

spt_status spt_sensevoice_set_vocab(spt_sv_ctx* ctx, const char* const* pieces, int32_t n) {
    if (!ctx || (n > 0 && !pieces) || n < 0) return fail(ctx, SPT_ERR_INVALID_ARG, "null argument");
    std::vector<std::string> v;
    for (int32_t i = 0; i < n; i++) v.push_back(pieces[i] ? pieces[i] : "");
    ctx->pieces.swap(v);
    return SPT_OK;
}

int32_t spt_sensevoice_n_rows(const spt_sv_ctx* ctx, size_t n_samples) {
    if (!ctx || n_samples > (size_t)spt::SV_MAX_SAMPLES) return 0;
    return ctx->eng->rows_of((int64_t)n_samples);
}

spt_status spt_sensevoice_transcribe_batch(spt_sv_ctx* ctx, const float* const* pcm, const size_t* n_samples, size_t batch,
                                           const spt_sv_infer_params* params, spt_sv_result** out) {
    if (!ctx || !out || (batch && (!pcm || !n_samples))) return fail(ctx, SPT_ERR_INVALID_ARG, "null argument");
    spt::SvInfer ip;
    if (!infer_of(ctx, params, &ip)) return SPT_ERR_INVALID_ARG;
    spt::SenseVoiceEngine& e = *ctx->eng;
    for (size_t u = 0; u < batch; u++) {
        out[u] = nullptr;
        if (n_samples[u] && !pcm[u]) return fail(ctx, SPT_ERR_INVALID_ARG, "null pcm");
        if (n_samples[u] > (size_t)e.max_samples())
            return fail(ctx, SPT_ERR_INVALID_ARG, "utterance of " + std::to_string(n_samples[u]) +
                        " samples is longer than max_samples = " + std::to_string(e.max_samples()));
    }
    e.clear_timings();
    return guarded(ctx, [&]() -> spt_status {
        std::vector<spt::SvUtt> acc(batch);
        std::vector<size_t> live;  // utterances with at least one fbank frame
        for (size_t u = 0; u < batch; u++)
            if (n_samples[u] >= (size_t)spt::SV_FRAME) live.push_back(u);
        if (!live.empty() && e.missing() > 0)
            return fail(ctx, SPT_ERR_INVALID_ARG, "sensevoice: " + std::to_string(e.missing()) + " tensors not set");
        for (size_t g0 = 0; g0 < live.size(); g0 += e.max_batch()) {
            const int B = (int)std::min<size_t>(e.max_batch(), live.size() - g0);
            std::vector<const float*> ptr(B);
            std::vector<size_t> ns(B);
            for (int b = 0; b < B; b++) {
                const size_t u = live[g0 + b];
                ptr[b] = pcm[u];
                ns[b] = n_samples[u];
            }
            std::vector<spt::SvUtt> res = e.transcribe(ptr.data(), ns.data(), B, ip);
            for (int b = 0; b < B; b++) acc[live[g0 + b]] = std::move(res[b]);
        }
        for (size_t u = 0; u < batch; u++) {
            out[u] = make_result(ctx, acc[u]);
            if (!out[u]) {
                for (size_t v = 0; v < u; v++) {
                    spt_sensevoice_result_free(out[v]);
                    out[v] = nullptr;
                }
                return fail(ctx, SPT_ERR_OOM, "out of host memory");
            }
        }
        return SPT_OK;
    });
}

spt_status spt_sensevoice_transcribe(spt_sv_ctx* ctx, const float* pcm16k, size_t n_samples,
                                     const spt_sv_infer_params* params, spt_sv_result** out) {
    if (!ctx || !out) return fail(ctx, SPT_ERR_INVALID_ARG, "null argument");
    return spt_sensevoice_transcribe_batch(ctx, &pcm16k, &n_samples, 1, params, out);
}

void spt_sensevoice_result_free(spt_sv_result* r) {
    if (!r) return;
    free(r->text);
    free(r->tokens);
    free(r->frames);
    free(r->top1);
    free(r->top2);
    free(r);
}

spt_status spt_sensevoice_get_timings(const spt_sv_ctx* ctx, spt_sv_timings* t) {
    if (!ctx || !t) return SPT_ERR_INVALID_ARG;
    const spt::SvTimings& m = ctx->eng->timings();
    t->frontend_ms = m.frontend_ms; t->encoder_ms = m.encoder_ms; t->ctc_ms = m.ctc_ms; t->total_ms = m.total_ms;
    t->rows = m.rows; t->batch = m.batch;
    return SPT_OK;
}

static spt_status debug_common(spt_sv_ctx* ctx, const float* pcm, size_t n, const void* out) {
    if (!ctx || !pcm || !out) return fail(ctx, SPT_ERR_INVALID_ARG, "null argument");
    if (n < (size_t)spt::SV_FRAME || n > (size_t)ctx->eng->max_samples())
        return fail(ctx, SPT_ERR_INVALID_ARG, "debug hooks take 400..max_samples samples");
    return SPT_OK;
}

spt_status spt_sensevoice_debug_features(spt_sv_ctx* ctx, const float* pcm16k, size_t n_samples, float* out) {
    const spt_status s = debug_common(ctx, pcm16k, n_samples, out);
    if (s != SPT_OK) return s;
    return guarded(ctx, [&] {
        ctx->eng->debug_features(pcm16k, n_samples, out);
        return SPT_OK;
    });
}

spt_status spt_sensevoice_debug_encode(spt_sv_ctx* ctx, const float* pcm16k, size_t n_samples,
                                       const spt_sv_infer_params* params, float* out) {
    const spt_status s = debug_common(ctx, pcm16k, n_samples, out);
    if (s != SPT_OK) return s;
    spt::SvInfer ip;
    if (!infer_of(ctx, params, &ip)) return SPT_ERR_INVALID_ARG;
    return guarded(ctx, [&] {
        ctx->eng->debug_encode(pcm16k, n_samples, ip, out);
        return SPT_OK;
    });
}

spt_status spt_sensevoice_debug_frames(spt_sv_ctx* ctx, const float* pcm16k, size_t n_samples,
                                       const spt_sv_infer_params* params, int32_t* ids, float* top1, float* top2) {
    const spt_status s = debug_common(ctx, pcm16k, n_samples, ids);
    if (s != SPT_OK) return s;
    if (!top1 || !top2) return fail(ctx, SPT_ERR_INVALID_ARG, "null argument");
    spt::SvInfer ip;
    if (!infer_of(ctx, params, &ip)) return SPT_ERR_INVALID_ARG;
    return guarded(ctx, [&] {
        ctx->eng->debug_frames(pcm16k, n_samples, ip, ids, top1, top2);
        return SPT_OK;
    });
}

}  // extern "C"
