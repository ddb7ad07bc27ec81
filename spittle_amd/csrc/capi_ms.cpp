// capi_ms.cpp -- the spt_moonshine_* part of include/spittle_hip.h (additive over ABI 14).
//
// Mirrors transcribe-rs' MoonshineEngine as Spittle drives it (load_model_with_params with
// ModelVariant::Base, transcribe_samples(audio, None), unload): status codes + message, borrowed
// PCM, library-owned results.
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
#include "moonshine.h"

struct spt_ms_ctx {
    std::unique_ptr<spt::MoonshineEngine> eng;
    std::vector<std::string> pieces;
    std::string spec, err;
};

namespace {

using spt::classify;
using spt::fail;
using spt::guarded;
using spt::set_err;

spt_ms_result* make_result(const spt_ms_ctx* c, const spt::MsUtt& r) {
    spt_ms_result* o = (spt_ms_result*)calloc(1, sizeof(spt_ms_result));
    if (!o) return nullptr;
    const size_t n = r.tok.size();
    const std::string text = spt::ms_detokenize(c->pieces, r.tok.data(), (int)n);
    o->n_tokens = (int32_t)n;
    o->hit_eos = r.hit_eos ? 1 : 0;
    o->tokens = (int32_t*)malloc(4 * (n ? n : 1));
    o->top1 = (float*)malloc(4 * (n ? n : 1));
    o->top2 = (float*)malloc(4 * (n ? n : 1));
    o->text = (char*)malloc(text.size() + 1);
    if (!o->tokens || !o->top1 || !o->top2 || !o->text) {
        spt_moonshine_result_free(o);
        return nullptr;
    }
    for (size_t i = 0; i < n; i++) {
        o->tokens[i] = r.tok[i];
        o->top1[i] = r.top1[i];
        o->top2[i] = r.top2[i];
    }
    memcpy(o->text, text.c_str(), text.size() + 1);
    return o;
}

int token_limit(const spt_ms_infer_params* p, size_t n, int ctx) {
    int64_t lim = p->max_tokens > 0 ? p->max_tokens : (int64_t)ceil((double)p->tokens_per_second * (double)n / 16000.0);
    return (int)std::max<int64_t>(0, std::min<int64_t>(lim, ctx));
}

}  // namespace

extern "C" {

void spt_moonshine_default_model_params(spt_ms_model_params* p) {
    if (!p) return;
    p->dtype = SPT_DTYPE_F16;
    p->device = 0;
    p->max_batch = 8;
    p->max_samples = 64 * 16000;
    p->seed = 1234;
}

void spt_moonshine_default_infer_params(spt_ms_infer_params* p) {
    if (!p) return;
    p->tokens_per_second = 6.5f;
    p->max_tokens = 0;
}

spt_status spt_moonshine_create(const char* model_spec, const spt_ms_model_params* params, spt_ms_ctx** out, char* err,
                                size_t errlen) {
    if (!model_spec || !out) {
        set_err(err, errlen, "null argument");
        return SPT_ERR_INVALID_ARG;
    }
    *out = nullptr;
    spt_ms_model_params mp;
    spt_moonshine_default_model_params(&mp);
    if (params) mp = *params;
    spt::MsSpec spec;
    std::string perr;
    if (!spt::ms_parse_spec(model_spec, &spec, &perr)) {
        set_err(err, errlen, perr);
        return SPT_ERR_LOAD;
    }
    if (mp.dtype != SPT_DTYPE_F16) {
        set_err(err, errlen, "moonshine: the engine dtype is SPT_DTYPE_F16 only");
        return SPT_ERR_UNSUPPORTED;
    }
    if (mp.max_batch < 1 || mp.max_batch > 64) {
        set_err(err, errlen, "max_batch must be in [1, 64]");
        return SPT_ERR_INVALID_ARG;
    }
    if (mp.max_samples < spt::MS_MIN_SAMPLES || mp.max_samples > spt::MS_MAX_SAMPLES) {
        set_err(err, errlen, "max_samples must be in [895, 3000000]");
        return SPT_ERR_INVALID_ARG;
    }
    spt_ms_ctx* c = new (std::nothrow) spt_ms_ctx();
    if (!c) return SPT_ERR_OOM;
    c->spec = model_spec;
    try {
        c->eng.reset(new spt::MoonshineEngine(spec.dims, mp.device, mp.max_batch, mp.max_samples,
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

void spt_moonshine_destroy(spt_ms_ctx* ctx) { delete ctx; }

const char* spt_moonshine_last_error(const spt_ms_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

spt_status spt_moonshine_info(const spt_ms_ctx* ctx, spt_ms_model_info* info) {
    if (!ctx || !info) return SPT_ERR_INVALID_ARG;
    const spt::MoonshineEngine& e = *ctx->eng;
    const spt::MsDims& d = e.dims();
    memset(info, 0, sizeof(*info));
    info->d = d.d; info->n_heads = d.H; info->head_dim = d.dh; info->rotary_dim = d.rot; info->ff = d.ff;
    info->n_enc_layers = d.n_enc; info->n_dec_layers = d.n_dec; info->n_vocab = d.vocab; info->bos = d.bos;
    info->eos = d.eos; info->dtype = SPT_DTYPE_F16; info->max_batch = e.max_batch(); info->max_samples = e.max_samples();
    info->ctx = e.ctx(); info->weight_bytes = e.weight_bytes(); info->workspace_bytes = e.workspace_bytes();
    return SPT_OK;
}

spt_status spt_moonshine_tensor_numel(const spt_ms_ctx* ctx, const char* name, int64_t* n) {
    if (!ctx || !name || !n) return SPT_ERR_INVALID_ARG;
    const int64_t v = ctx->eng->tensor_numel(name);
    if (v < 0) return SPT_ERR_INVALID_ARG;
    *n = v;
    return SPT_OK;
}

spt_status spt_moonshine_set_tensor(spt_ms_ctx* ctx, const char* name, const float* data, int64_t n) {
    if (!ctx || !name || !data) return fail(ctx, SPT_ERR_INVALID_ARG, "null argument");
    return guarded(ctx, [&] {
        ctx->eng->set_tensor(name, data, n);
        return SPT_OK;
    });
}

int32_t spt_moonshine_missing_tensors(const spt_ms_ctx* ctx) { return ctx ? ctx->eng->missing() : -1; }

spt_status spt_moonshine_set_vocab(spt_ms_ctx* ctx, const char* const* pieces, int32_t n) {
    if (!ctx || (n > 0 && !pieces) || n < 0) return fail(ctx, SPT_ERR_INVALID_ARG, "null argument");
    std::vector<std::string> v;
    for (int32_t i = 0; i < n; i++) v.push_back(pieces[i] ? pieces[i] : "");
    ctx->pieces.swap(v);
    return SPT_OK;
}

spt_status spt_moonshine_transcribe_batch(spt_ms_ctx* ctx, const float* const* pcm, const size_t* n_samples, size_t batch,
                                          const spt_ms_infer_params* params, spt_ms_result** out) {
    if (!ctx || !out || (batch && (!pcm || !n_samples))) return fail(ctx, SPT_ERR_INVALID_ARG, "null argument");
    spt_ms_infer_params dp;
    spt_moonshine_default_infer_params(&dp);
    if (!params) params = &dp;
    if (!(params->tokens_per_second >= 0.0f && params->tokens_per_second <= 1000.0f) || params->max_tokens < 0)
        return fail(ctx, SPT_ERR_INVALID_ARG, "tokens_per_second must be in [0, 1000] and max_tokens >= 0");
    spt::MoonshineEngine& e = *ctx->eng;
    for (size_t u = 0; u < batch; u++) {
        out[u] = nullptr;
        if (n_samples[u] && !pcm[u]) return fail(ctx, SPT_ERR_INVALID_ARG, "null pcm");
        if (n_samples[u] > (size_t)e.max_samples())
            return fail(ctx, SPT_ERR_INVALID_ARG, "utterance of " + std::to_string(n_samples[u]) +
                        " samples is longer than max_samples = " + std::to_string(e.max_samples()));
    }
    e.clear_timings();
    return guarded(ctx, [&]() -> spt_status {
        std::vector<spt::MsUtt> acc(batch);
        std::vector<size_t> live;  // utterances with at least one encoder frame
        for (size_t u = 0; u < batch; u++)
            if (n_samples[u] >= (size_t)spt::MS_MIN_SAMPLES) live.push_back(u);
        if (!live.empty() && e.missing() > 0)
            return fail(ctx, SPT_ERR_INVALID_ARG, "moonshine: " + std::to_string(e.missing()) + " tensors not set");
        for (size_t g0 = 0; g0 < live.size(); g0 += e.max_batch()) {
            const int B = (int)std::min<size_t>(e.max_batch(), live.size() - g0);
            std::vector<const float*> ptr(B);
            std::vector<size_t> ns(B);
            std::vector<int> lim(B);
            for (int b = 0; b < B; b++) {
                const size_t u = live[g0 + b];
                ptr[b] = pcm[u];
                ns[b] = n_samples[u];
                lim[b] = token_limit(params, n_samples[u], e.ctx());
            }
            std::vector<spt::MsUtt> res = e.transcribe(ptr.data(), ns.data(), B, lim.data());
            for (int b = 0; b < B; b++) acc[live[g0 + b]] = std::move(res[b]);
        }
        for (size_t u = 0; u < batch; u++) {
            out[u] = make_result(ctx, acc[u]);
            if (!out[u]) {
                for (size_t v = 0; v < u; v++) {
                    spt_moonshine_result_free(out[v]);
                    out[v] = nullptr;
                }
                return fail(ctx, SPT_ERR_OOM, "out of host memory");
            }
        }
        return SPT_OK;
    });
}

spt_status spt_moonshine_transcribe(spt_ms_ctx* ctx, const float* pcm16k, size_t n_samples,
                                    const spt_ms_infer_params* params, spt_ms_result** out) {
    if (!ctx || !out) return fail(ctx, SPT_ERR_INVALID_ARG, "null argument");
    return spt_moonshine_transcribe_batch(ctx, &pcm16k, &n_samples, 1, params, out);
}

void spt_moonshine_result_free(spt_ms_result* r) {
    if (!r) return;
    free(r->text);
    free(r->tokens);
    free(r->top1);
    free(r->top2);
    free(r);
}

spt_status spt_moonshine_get_timings(const spt_ms_ctx* ctx, spt_ms_timings* t) {
    if (!ctx || !t) return SPT_ERR_INVALID_ARG;
    const spt::MsTimings& m = ctx->eng->timings();
    t->stem_ms = m.stem_ms; t->encoder_ms = m.encoder_ms; t->cross_kv_ms = m.cross_kv_ms; t->decode_ms = m.decode_ms;
    t->total_ms = m.total_ms; t->n_steps = m.n_steps; t->batch = m.batch;
    return SPT_OK;
}

static spt_status debug_common(spt_ms_ctx* ctx, const float* pcm, size_t n, const void* out) {
    if (!ctx || !pcm || !out) return fail(ctx, SPT_ERR_INVALID_ARG, "null argument");
    if (n < (size_t)spt::MS_MIN_SAMPLES || n > (size_t)ctx->eng->max_samples())
        return fail(ctx, SPT_ERR_INVALID_ARG, "debug hooks take 895..max_samples samples");
    return SPT_OK;
}

spt_status spt_moonshine_debug_stem(spt_ms_ctx* ctx, const float* pcm16k, size_t n_samples, float* out) {
    const spt_status s = debug_common(ctx, pcm16k, n_samples, out);
    if (s != SPT_OK) return s;
    return guarded(ctx, [&] {
        ctx->eng->debug_encode(pcm16k, n_samples, false, out);
        return SPT_OK;
    });
}

spt_status spt_moonshine_debug_encode(spt_ms_ctx* ctx, const float* pcm16k, size_t n_samples, float* out) {
    const spt_status s = debug_common(ctx, pcm16k, n_samples, out);
    if (s != SPT_OK) return s;
    return guarded(ctx, [&] {
        ctx->eng->debug_encode(pcm16k, n_samples, true, out);
        return SPT_OK;
    });
}

spt_status spt_moonshine_debug_logits(spt_ms_ctx* ctx, const float* pcm16k, size_t n_samples, const int32_t* prefix,
                                      int32_t n_prefix, float* out) {
    const spt_status s = debug_common(ctx, pcm16k, n_samples, out);
    if (s != SPT_OK) return s;
    if (!prefix) return fail(ctx, SPT_ERR_INVALID_ARG, "null prefix");
    return guarded(ctx, [&] {
        ctx->eng->debug_logits(pcm16k, n_samples, prefix, n_prefix, out);
        return SPT_OK;
    });
}

}  // extern "C"
