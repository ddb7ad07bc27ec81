// sensevoice.cpp -- the SenseVoice engine: weights by FunASR state-dict name, the Kaldi fbank / LFR
// front end, the SANM encoder and the CTC head with the greedy collapse on the device.
#include "sensevoice.h"

#include <math.h>
#include <string.h>

#include <algorithm>

#include "common.h"
#include "kernels.h"

namespace spt {

namespace {
constexpr int SV_CTC_CHUNK = 2048;  // rows per CTC GEMM (bounds the f32 logits buffer)
}  // namespace

SenseVoiceEngine::SenseVoiceEngine(const SvDims& dims, int device, int max_batch, int max_samples, uint64_t seed,
                                   bool synthetic)
    : SeqEngine("sensevoice", device, max_batch, max_samples), D_(dims) {
    const SvDims& D = D_;
    std::string derr;
    if (!sv_dims_ok(D, &derr)) throw std::runtime_error(derr);
    if (Bm_ < 1 || Bm_ > 64) throw std::runtime_error("sensevoice: max_batch must be 1..64");
    if (Ns_ < SV_FRAME || Ns_ > SV_MAX_SAMPLES) throw std::runtime_error("sensevoice: max_samples must be 400..4800000");
    in_ = D.in();
    inp_ = sv_pad64(in_);
    Vp_ = (D.vocab + 127) / 128 * 128;
    Tm_ = sv_frames_of(Ns_);
    Rm_ = sv_rows_of(Ns_, D.lfr_n);
    open(4);
    // a throw from here on: ~SeqEngine frees what was allocated
    gemm_prepare();
    const int d = D.d, ff = D.ff;
    // ---- tables and weights
    win_ = (float*)dalloc(SV_FRAME * 4, true);
    basis_ = (float*)dalloc((int64_t)SV_DFT_N * SV_NFFT * 4, true);
    fbT_ = (float*)dalloc((int64_t)SV_NBIN * SV_MELS * 4, true);
    inv_freq_ = (float*)dalloc((int64_t)(in_ / 2) * 4, true);
    neg_mean_ = (float*)dalloc(in_ * 4, true);
    inv_std_ = (float*)dalloc(in_ * 4, true);
    embed_ = (float*)dalloc((int64_t)SV_EMBED_ROWS * in_ * 4, true);
    layers_.resize(D.layers());
    for (int l = 0; l < D.layers(); l++) {
        Layer& L = layers_[l];
        L.din = l < D.n0 ? in_ : d;
        L.ldin = l < D.n0 ? inp_ : d;
        L.n1w = (float*)dalloc(L.din * 4, true);
        L.n1b = (float*)dalloc(L.din * 4, true);
        L.qkv = dalloc((int64_t)3 * d * L.ldin * 2, true);
        L.qkvb = (float*)dalloc(3 * d * 4, true);
        L.fsmn = (float*)dalloc((int64_t)d * SV_FSMN_K * 4, true);
        L.o = dalloc((int64_t)d * d * 2, true);
        L.ob = (float*)dalloc(d * 4, true);
        L.n2w = (float*)dalloc(d * 4, true);
        L.n2b = (float*)dalloc(d * 4, true);
        L.w1 = dalloc((int64_t)ff * d * 2, true);
        L.w1b = (float*)dalloc(ff * 4, true);
        L.w2 = dalloc((int64_t)d * ff * 2, true);
        L.w2b = (float*)dalloc(d * 4, true);
    }
    an_w_ = (float*)dalloc(d * 4, true);
    an_b_ = (float*)dalloc(d * 4, true);
    tn_w_ = (float*)dalloc(d * 4, true);
    tn_b_ = (float*)dalloc(d * 4, true);
    ctc_w_ = dalloc((int64_t)Vp_ * d * 2, true);   // pad rows stay zero
    ctc_b_ = (float*)dalloc(Vp_ * 4, true);
    // ---- workspace (capacity: max_batch utterances of max_samples)
    const int64_t MT = (int64_t)Bm_ * Tm_, MR = (int64_t)Bm_ * Rm_;
    if (MT * SV_DFT_N >= (1ll << 31) || MR * std::max(3 * d, std::max(ff, inp_)) >= (1ll << 31))
        throw std::runtime_error("sensevoice: max_batch x max_samples too large");
    chunk_ = (int)std::min<int64_t>(MR, SV_CTC_CHUNK);
    pcm_ = (float*)dalloc((int64_t)Bm_ * Ns_ * 4, false);
    frames_ = (float*)dalloc(MT * SV_NFFT * 4, false);
    spec_ = (float*)dalloc(MT * SV_DFT_N * 4, false);
    mel_ = (float*)dalloc(MT * SV_MELS * 4, false);
    rows_ = (float*)dalloc(MR * inp_ * 4, false);
    x_ = (float*)dalloc(MR * d * 4, false);
    enc32_ = (float*)dalloc((int64_t)Rm_ * d * 4, false);
    xn16_ = dalloc(MR * std::max(inp_, d) * 2, false);
    qkv16_ = dalloc(MR * 3 * d * 2, false);
    att16_ = dalloc(MR * d * 2, false);
    h16_ = dalloc(MR * ff * 2, false);
    logits_ = (float*)dalloc((int64_t)chunk_ * Vp_ * 4, false);
    ids_ = (int*)dalloc(MR * 4, false);
    top1_ = (float*)dalloc(MR * 4, false);
    top2_ = (float*)dalloc(MR * 4, false);
    out_ = (int*)dalloc((int64_t)Bm_ * (8 + 4 * (int64_t)Rm_) * 4, false);
    lens_ = (int*)dalloc(Bm_ * 4 * 4, false);
    upload_tables();
    build_tensors();
    if (synthetic) {
        gen_synthetic(seed);
        // a log-mel of speech-level PCM x 32768 sits near 10 with a spread of a few units
        std::vector<float> nm((size_t)in_, -10.0f), is((size_t)in_, 0.25f);
        set_cmvn(nm.data(), is.data(), in_);
    }
    HIP_CHECK(hipDeviceSynchronize());
}

void SenseVoiceEngine::upload_tables() {
    std::vector<float> win(SV_FRAME), basis((size_t)SV_DFT_N * SV_NFFT, 0.0f), fbT((size_t)SV_NBIN * SV_MELS, 0.0f);
    for (int i = 0; i < SV_FRAME; i++) win[i] = (float)(0.54 - 0.46 * cos(2.0 * M_PI * i / (SV_FRAME - 1)));
    for (int k = 0; k < SV_NBIN; ++k)
        for (int i = 0; i < SV_NFFT; ++i) {
            const int ph = (k * i) & (SV_NFFT - 1);
            basis[(size_t)k * SV_NFFT + i] = (float)cos(2.0 * M_PI * ph / SV_NFFT);
            basis[(size_t)(SV_NBIN + k) * SV_NFFT + i] = (float)sin(2.0 * M_PI * ph / SV_NFFT);
        }
    // Kaldi-scale mel filters, triangular in mel space, 20 Hz .. 8 kHz, no norm
    auto mel = [](double f) { return 1127.0 * log(1.0 + f / 700.0); };
    const double m0 = mel(20.0), m1 = mel(8000.0);
    for (int j = 0; j < SV_MELS; j++) {
        const double lo = m0 + (m1 - m0) * j / (SV_MELS + 1), ce = m0 + (m1 - m0) * (j + 1) / (SV_MELS + 1),
                     hi = m0 + (m1 - m0) * (j + 2) / (SV_MELS + 1);
        for (int k = 0; k < SV_NBIN; k++) {
            const double m = mel(16000.0 / SV_NFFT * k);
            const double wgt = std::max(0.0, std::min((m - lo) / (ce - lo), (hi - m) / (hi - ce)));
            fbT[(size_t)k * SV_MELS + j] = (float)wgt;
        }
    }
    const int half = in_ / 2;
    std::vector<float> inv((size_t)half);
    const float step = (float)(log(10000.0) / (double)std::max(1, half - 1));
    for (int k = 0; k < half; k++) inv[k] = expf((float)k * -step);
    HIP_CHECK(hipMemcpy(win_, win.data(), win.size() * 4, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(basis_, basis.data(), basis.size() * 4, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(fbT_, fbT.data(), fbT.size() * 4, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(inv_freq_, inv.data(), inv.size() * 4, hipMemcpyHostToDevice));
}

void SenseVoiceEngine::build_tensors() {
    const SvDims& D = D_;
    const int d = D.d, ff = D.ff;
    add_tensor("embed.weight", (int64_t)SV_EMBED_ROWS * in_, T_VEC, embed_, 0, 0, 0);
    for (int l = 0; l < D.layers(); l++) {
        const std::string P = sv_layer_prefix(D, l);
        Layer& L = layers_[l];
        add_tensor(P + "norm1.weight", L.din, T_VEC, L.n1w, 0, 0, 0);
        add_tensor(P + "norm1.bias", L.din, T_VEC, L.n1b, 0, 0, 0);
        add_tensor(P + "self_attn.linear_q_k_v.weight", (int64_t)3 * d * L.din, T_MAT16, L.qkv, 3 * d, L.din, L.ldin);
        add_tensor(P + "self_attn.linear_q_k_v.bias", 3 * d, T_VEC, L.qkvb, 0, 0, 0);
        add_tensor(P + "self_attn.fsmn_block.weight", (int64_t)d * SV_FSMN_K, T_VEC, L.fsmn, 0, 0, 0);
        add_tensor(P + "self_attn.linear_out.weight", (int64_t)d * d, T_MAT16, L.o, d, d, d);
        add_tensor(P + "self_attn.linear_out.bias", d, T_VEC, L.ob, 0, 0, 0);
        add_tensor(P + "norm2.weight", d, T_VEC, L.n2w, 0, 0, 0);
        add_tensor(P + "norm2.bias", d, T_VEC, L.n2b, 0, 0, 0);
        add_tensor(P + "feed_forward.w_1.weight", (int64_t)ff * d, T_MAT16, L.w1, ff, d, d);
        add_tensor(P + "feed_forward.w_1.bias", ff, T_VEC, L.w1b, 0, 0, 0);
        add_tensor(P + "feed_forward.w_2.weight", (int64_t)d * ff, T_MAT16, L.w2, d, ff, ff);
        add_tensor(P + "feed_forward.w_2.bias", d, T_VEC, L.w2b, 0, 0, 0);
    }
    add_tensor("encoder.after_norm.weight", d, T_VEC, an_w_, 0, 0, 0);
    add_tensor("encoder.after_norm.bias", d, T_VEC, an_b_, 0, 0, 0);
    add_tensor("encoder.tp_norm.weight", d, T_VEC, tn_w_, 0, 0, 0);
    add_tensor("encoder.tp_norm.bias", d, T_VEC, tn_b_, 0, 0, 0);
    add_tensor("ctc.ctc_lo.weight", (int64_t)D.vocab * d, T_MAT16, ctc_w_, D.vocab, d, d);
    add_tensor("ctc.ctc_lo.bias", D.vocab, T_VEC, ctc_b_, 0, 0, 0);
    // sv_host.h's table (what the sanitizer harness and the tests see) is this one
    const std::vector<SvTensorName> names = sv_tensor_names(D);
    bool same = names.size() == tensors_.size();
    for (size_t i = 0; same && i < names.size(); i++) same = names[i].name == tensors_[i].name && names[i].numel == tensors_[i].numel;
    if (!same) throw std::runtime_error("sensevoice: tensor table out of step with sv_tensor_names");
}

int SenseVoiceEngine::missing() const {
    return SeqEngine::missing() + (cmvn_set_ ? 0 : 1);
}

void SenseVoiceEngine::require_weights() const {
    SeqEngine::require_weights();
    if (!cmvn_set_) throw std::runtime_error("sensevoice: CMVN not set");
}

void SenseVoiceEngine::set_cmvn(const float* neg_mean, const float* inv_std, int n) {
    if (!neg_mean || !inv_std || n != in_)
        throw std::runtime_error("sensevoice: CMVN vectors have " + std::to_string(in_) + " elements, got " + std::to_string(n));
    select();
    HIP_CHECK(hipStreamSynchronize(st_));
    HIP_CHECK(hipMemcpy(neg_mean_, neg_mean, (size_t)n * 4, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(inv_std_, inv_std, (size_t)n * 4, hipMemcpyHostToDevice));
    cmvn_set_ = true;
}

void SenseVoiceEngine::upload(const float* const* pcm, const size_t* n, int B) {
    const int lfr_n = D_.lfr_n;
    SeqEngine::upload(pcm, n, B, SV_FRAME, [lfr_n](int64_t ns, int* len) {
        len[1] = sv_frames_of(ns); len[2] = sv_lfr_rows_of(len[1], lfr_n); len[3] = len[2] + SV_NQ;
    });
    Tp_ = lens_max_[1]; Rp_ = lens_max_[3];
}

void SenseVoiceEngine::run_frontend(int B, const SvInfer& p, bool feat_only) {
    if (p.language < 0 || p.language >= SV_N_LANG) throw std::runtime_error("sensevoice: language outside 0..5");
    sv_frames(pcm_, stride_, lens_, B, Tp_, win_, frames_, st_);
    gemm(DT_F32, EPI_BIAS, frames_, SV_NFFT, basis_, SV_NFFT, B * Tp_, SV_DFT_N, SV_NFFT, nullptr, spec_, SV_DFT_N, st_);
    sv_melpow(spec_, B * Tp_, fbT_, mel_, st_);
    SvRowsArgs a{};
    a.mel = mel_; a.lens = lens_; a.neg_mean = neg_mean_; a.inv_std = inv_std_; a.embed = embed_; a.inv_freq = inv_freq_;
    a.Tp = Tp_; a.Rp = Rp_; a.in = in_; a.ld = inp_; a.lfr_m = D_.lfr_m; a.lfr_n = D_.lfr_n;
    a.q[0] = D_.lang_rows[p.language]; a.q[1] = D_.event_row; a.q[2] = D_.emo_row;
    a.q[3] = p.use_itn ? D_.itn_row : D_.no_itn_row;
    a.scale = sqrtf((float)D_.d);
    a.feat_only = feat_only ? 1 : 0;
    a.out = rows_;
    sv_lfr_rows(a, B, st_);
}

// LayerNorm into the f16 GEMM input: kernels.h' layernorm where it fits (a contiguous row, its eps)
void SenseVoiceEngine::norm16(const float* x, int M, int d, int ld, const float* w, const float* b, void* y) {
    if (ld == d && D_.ln_eps == 1e-5f) layernorm(DT_F16, x, M, d, w, b, y, st_);
    else sv_layernorm(x, M, d, ld, w, b, D_.ln_eps, y, ld, false, st_);
}

void SenseVoiceEngine::run_encoder(int B) {
    const SvDims& D = D_;
    const int M = B * Rp_, d = D.d, ff = D.ff;
    for (int l = 0; l < D.layers(); l++) {
        const Layer& L = layers_[l];
        const bool first = l < D.n0;  // 560 -> d: no residual around the attention
        norm16(first ? rows_ : x_, M, L.din, L.ldin, L.n1w, L.n1b, xn16_);
        gemm(DT_F16, EPI_BIAS, xn16_, L.ldin, L.qkv, L.ldin, M, 3 * d, L.ldin, L.qkvb, qkv16_, 3 * d, st_);
        sv_fsmn((const f16*)qkv16_ + 2 * d, 3 * d, L.fsmn, lens_, B, Rp_, d, D.sanm_shift, !first, x_, st_);
        sv_attention(qkv16_, lens_, B, Rp_, D.H, att16_, st_);
        gemm(DT_F16, EPI_BIAS_RESID, att16_, d, L.o, d, M, d, d, L.ob, x_, d, st_);
        norm16(x_, M, d, d, L.n2w, L.n2b, xn16_);
        gemm(DT_F16, EPI_BIAS_RELU, xn16_, d, L.w1, d, M, ff, d, L.w1b, h16_, ff, st_);
        gemm(DT_F16, EPI_BIAS_RESID, h16_, ff, L.w2, ff, M, d, ff, L.w2b, x_, d, st_);
        if (l == D.n0 + D.n1 - 1) sv_layernorm(x_, M, d, d, an_w_, an_b_, D.ln_eps, x_, d, true, st_);
    }
}

void SenseVoiceEngine::run_ctc(int B) {
    const int M = B * Rp_, d = D_.d;
    norm16(x_, M, d, d, tn_w_, tn_b_, xn16_);
    for (int m0 = 0; m0 < M; m0 += chunk_) {
        const int m = std::min(chunk_, M - m0);
        gemm(DT_F16, EPI_BIAS_F32, (const f16*)xn16_ + (int64_t)m0 * d, d, ctc_w_, d, m, Vp_, d, ctc_b_, logits_, Vp_, st_);
        sv_ctc_top2(logits_, m, D_.vocab, Vp_, ids_ + m0, top1_ + m0, top2_ + m0, st_);
    }
    SvCollapseArgs c{};
    c.ids = ids_; c.top1 = top1_; c.top2 = top2_; c.lens = lens_;
    c.Rp = Rp_; c.n_prefix = D_.n_prefix; c.blank = D_.blank; c.cap = Rm_; c.out = out_;
    sv_ctc_collapse(c, B, st_);
}

std::vector<SvUtt> SenseVoiceEngine::transcribe(const float* const* pcm, const size_t* n, int B, const SvInfer& p) {
    select();
    require_weights();
    if (p.language < 0 || p.language >= SV_N_LANG) throw std::runtime_error("sensevoice: language outside 0..5");
    upload(pcm, n, B);
    HIP_CHECK(hipEventRecord(ev_[0], st_));  // device work only: the host-to-device copy is not in frontend_ms
    run_frontend(B, p, false);
    HIP_CHECK(hipEventRecord(ev_[1], st_));
    run_encoder(B);
    HIP_CHECK(hipEventRecord(ev_[2], st_));
    run_ctc(B);
    HIP_CHECK(hipEventRecord(ev_[3], st_));
    const int64_t stride = 8 + 4 * (int64_t)Rm_;
    std::vector<int> out((size_t)(B * stride));
    HIP_CHECK(hipMemcpyAsync(out.data(), out_, out.size() * 4, hipMemcpyDeviceToHost, st_));  // the one read-back
    HIP_CHECK(hipStreamSynchronize(st_));
    float ms[3];
    phase_ms(3, ms);
    tm_.frontend_ms = ms[0]; tm_.encoder_ms = ms[1]; tm_.ctc_ms = ms[2];
    tm_.total_ms = (double)ms[0] + ms[1] + ms[2];
    tm_.rows = Rp_; tm_.batch = B;
    std::vector<SvUtt> res(B);
    for (int b = 0; b < B; b++) {
        const int* o = out.data() + b * stride;
        const int k = std::max(0, std::min(o[0], Rm_));
        for (int i = 0; i < SV_NQ; i++) res[b].prefix[i] = o[1 + i];
        res[b].tok.assign(o + 8, o + 8 + k);
        res[b].frame.assign(o + 8 + Rm_, o + 8 + Rm_ + k);
        res[b].top1.resize(k);
        res[b].top2.resize(k);
        if (k) {
            memcpy(res[b].top1.data(), o + 8 + 2 * (int64_t)Rm_, (size_t)k * 4);
            memcpy(res[b].top2.data(), o + 8 + 3 * (int64_t)Rm_, (size_t)k * 4);
        }
    }
    return res;
}

void SenseVoiceEngine::debug_features(const float* pcm, size_t n, float* out) {
    select();
    if (!cmvn_set_) throw std::runtime_error("sensevoice: CMVN not set");
    if (!out) throw std::runtime_error("sensevoice: null output");
    upload(&pcm, &n, 1);
    run_frontend(1, SvInfer(), true);
    HIP_CHECK(hipMemcpy2DAsync(out, (size_t)in_ * 4, rows_ + (int64_t)SV_NQ * inp_, (size_t)inp_ * 4, (size_t)in_ * 4,
                               (size_t)(Rp_ - SV_NQ), hipMemcpyDeviceToHost, st_));
    HIP_CHECK(hipStreamSynchronize(st_));
}

void SenseVoiceEngine::debug_encode(const float* pcm, size_t n, const SvInfer& p, float* out) {
    select();
    require_weights();
    if (!out) throw std::runtime_error("sensevoice: null output");
    upload(&pcm, &n, 1);
    run_frontend(1, p, false);
    run_encoder(1);
    sv_layernorm(x_, Rp_, D_.d, D_.d, tn_w_, tn_b_, D_.ln_eps, enc32_, D_.d, true, st_);
    HIP_CHECK(hipMemcpyAsync(out, enc32_, (size_t)Rp_ * D_.d * 4, hipMemcpyDeviceToHost, st_));
    HIP_CHECK(hipStreamSynchronize(st_));
}

void SenseVoiceEngine::debug_frames(const float* pcm, size_t n, const SvInfer& p, int* ids, float* top1, float* top2) {
    select();
    require_weights();
    if (!ids || !top1 || !top2) throw std::runtime_error("sensevoice: null output");
    upload(&pcm, &n, 1);
    run_frontend(1, p, false);
    run_encoder(1);
    run_ctc(1);
    HIP_CHECK(hipMemcpyAsync(ids, ids_, (size_t)Rp_ * 4, hipMemcpyDeviceToHost, st_));
    HIP_CHECK(hipMemcpyAsync(top1, top1_, (size_t)Rp_ * 4, hipMemcpyDeviceToHost, st_));
    HIP_CHECK(hipMemcpyAsync(top2, top2_, (size_t)Rp_ * 4, hipMemcpyDeviceToHost, st_));
    HIP_CHECK(hipStreamSynchronize(st_));
}

}  // namespace spt
