// moonshine.cpp -- the Moonshine engine: weights by HF state-dict name, the PCM stem, the encoder,
// the cross K/V, and greedy decoding as one captured step graph replayed per token.
#include "moonshine.h"

#include <math.h>
#include <string.h>

#include <algorithm>

#include "common.h"
#include "kernels.h"

namespace spt {

namespace {
enum { T_CONV1 = 2, T_CONVK = 3, T_TIED = 4 };  // the kinds beside SeqEngine's T_VEC and T_MAT16
inline int pad64(int v) { return (v + 63) / 64 * 64; }
}  // namespace

MoonshineEngine::MoonshineEngine(const MsDims& dims, int device, int max_batch, int max_samples, uint64_t seed,
                                 bool synthetic)
    : SeqEngine("moonshine", device, max_batch, max_samples), D_(dims) {
    static_assert(T_CONV1 == T_ENGINE, "the engine's kinds start at T_ENGINE");
    const MsDims& D = D_;
    if (D.d != D.H * D.dh || D.dh > 64 || D.dh % 4 || D.rot % 2 || D.rot > D.dh || D.d % 32 || D.ff % 32 || D.rot < 2)
        throw std::runtime_error("moonshine: unsupported dimensions");
    if (Bm_ < 1 || Bm_ > 64) throw std::runtime_error("moonshine: max_batch must be 1..64");
    if (Ns_ < MS_MIN_SAMPLES || Ns_ > MS_MAX_SAMPLES) throw std::runtime_error("moonshine: max_samples must be 895..3000000");
    dp_ = pad64(D.d);
    n2_ = 2 * D.d;
    n2p_ = pad64(n2_);
    ffp_ = pad64(D.ff);
    T1m_ = frames1(Ns_); T2m_ = frames2(T1m_); T3m_ = frames3(T2m_);
    ctx_ = std::max(448, (int)ceil(6.5 * (double)Ns_ / 16000.0) + 8);
    if (T3m_ > 8192 || ctx_ > 8192) throw std::runtime_error("moonshine: max_samples too large for the decode attention");
    open(5);
    // a throw from here on: ~SeqEngine frees what was allocated
    gemm_prepare();
    const int d = D.d, V = D.vocab, ff = D.ff;
    // ---- weights
    conv1_ = (float*)dalloc((int64_t)dp_ * MS_K1P * 4, true);
    gn_w_ = (float*)dalloc(d * 4, true);
    gn_b_ = (float*)dalloc(d * 4, true);
    conv2_ = dalloc((int64_t)n2p_ * MS_K2 * dp_ * 2, true);
    b2_ = (float*)dalloc(n2p_ * 4, true);
    conv3_ = dalloc((int64_t)dp_ * MS_K3 * n2p_ * 2, true);
    b3_ = (float*)dalloc(dp_ * 4, true);
    enc_.resize(D.n_enc);
    for (auto& L : enc_) {
        L.ln1 = (float*)dalloc(d * 4, true);
        L.ln2 = (float*)dalloc(d * 4, true);
        L.qkv = dalloc((int64_t)3 * dp_ * dp_ * 2, true);
        L.o = dalloc((int64_t)dp_ * dp_ * 2, true);
        L.fc1 = dalloc((int64_t)ffp_ * dp_ * 2, true);
        L.fc1b = (float*)dalloc(ffp_ * 4, true);
        L.fc2 = dalloc((int64_t)dp_ * ffp_ * 2, true);
        L.fc2b = (float*)dalloc(dp_ * 4, true);
    }
    enc_ln_ = (float*)dalloc(d * 4, true);
    emb_ = dalloc((int64_t)V * d * 2, true);
    dec_.resize(D.n_dec);
    for (auto& L : dec_) {
        L.ln1 = (float*)dalloc(d * 4, true);
        L.ln2 = (float*)dalloc(d * 4, true);
        L.ln3 = (float*)dalloc(d * 4, true);
        L.sqkv = dalloc((int64_t)3 * d * d * 2, true);
        L.so = dalloc((int64_t)d * d * 2, true);
        L.cq = dalloc((int64_t)d * d * 2, true);
        L.ckv = dalloc((int64_t)2 * dp_ * dp_ * 2, true);
        L.co = dalloc((int64_t)d * d * 2, true);
        L.fc1 = dalloc((int64_t)2 * ff * d * 2, true);
        L.fc1b = (float*)dalloc(2 * ff * 4, true);
        L.fc2 = dalloc((int64_t)d * ff * 2, true);
        L.fc2b = (float*)dalloc(d * 4, true);
    }
    dec_ln_ = (float*)dalloc(d * 4, true);
    // rotary table [P][rot] = cos | sin, as HF: inv_freq, the angle and cos / sin in f32
    {
        const int P = std::max(T3m_, ctx_), half = D.rot / 2;
        std::vector<float> tab((size_t)P * D.rot);
        for (int i = 0; i < half; i++) {
            const float inv = 1.0f / powf(D.theta, (float)(2 * i) / (float)D.rot);
            for (int p = 0; p < P; p++) {
                const float ang = inv * (float)p;
                tab[(size_t)p * D.rot + i] = cosf(ang);
                tab[(size_t)p * D.rot + half + i] = sinf(ang);
            }
        }
        rope_ = (float*)dalloc((int64_t)tab.size() * 4, true);
        HIP_CHECK(hipMemcpy(rope_, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
    }
    // ---- workspace (capacity: max_batch utterances of max_samples)
    const int64_t M1 = (int64_t)Bm_ * T1m_, M2 = (int64_t)Bm_ * T2m_, M3 = (int64_t)Bm_ * T3m_;
    pcm_ = (float*)dalloc((int64_t)Bm_ * Ns_ * 4, false);
    frames_ = (float*)dalloc(M1 * MS_K1P * 4, false);
    h1_ = (float*)dalloc(M1 * dp_ * 4, false);
    stats_ = (float*)dalloc(Bm_ * 2 * 4, false);
    A2_ = dalloc(M2 * MS_K2 * dp_ * 2, false);
    c2_ = (float*)dalloc(M2 * n2p_ * 4, false);
    A3_ = dalloc(M3 * MS_K3 * n2p_ * 2, false);
    x_ = (float*)dalloc(M3 * dp_ * 4, false);
    xn16_ = dalloc(M3 * dp_ * 2, false);
    qkv32_ = (float*)dalloc(M3 * 3 * dp_ * 4, false);
    qkv16_ = dalloc(M3 * 3 * dp_ * 2, false);
    att16_ = dalloc(M3 * dp_ * 2, false);
    h32_ = (float*)dalloc(M3 * ffp_ * 4, false);
    h16_ = dalloc(M3 * ffp_ * 2, false);
    enc16_ = dalloc(M3 * dp_ * 2, false);
    enc32_ = (float*)dalloc((int64_t)T3m_ * dp_ * 4, false);
    for (int l = 0; l < D.n_dec; l++) ckv_.push_back(dalloc(M3 * 2 * dp_ * 2, false));
    lens_ = (int*)dalloc(Bm_ * 4 * 4, false);
    state_ = (MsState*)dalloc(sizeof(MsState), false);
    cur_tok_ = (int*)dalloc(Bm_ * 4, false);
    done_ = (int*)dalloc(Bm_ * 4, false);
    n_out_ = (int*)dalloc(Bm_ * 4, false);
    hit_eos_ = (int*)dalloc(Bm_ * 4, false);
    limit_ = (int*)dalloc(Bm_ * 4, false);
    forced_ = (int*)dalloc((int64_t)Bm_ * ctx_ * 4, false);
    out_tok_ = (int*)dalloc((int64_t)Bm_ * ctx_ * 4, false);
    out_top1_ = (float*)dalloc((int64_t)Bm_ * ctx_ * 4, false);
    out_top2_ = (float*)dalloc((int64_t)Bm_ * ctx_ * 4, false);
    dx_ = (float*)dalloc((int64_t)Bm_ * d * 4, false);
    dqkv32_ = (float*)dalloc((int64_t)Bm_ * 3 * d * 4, false);
    logits_ = (float*)dalloc((int64_t)Bm_ * V * 4, false);
    dxn16_ = dalloc((int64_t)Bm_ * d * 2, false);
    dq16_ = dalloc((int64_t)Bm_ * d * 2, false);
    datt16_ = dalloc((int64_t)Bm_ * d * 2, false);
    dg16_ = dalloc((int64_t)Bm_ * ff * 2, false);
    cache_ = dalloc((int64_t)D.n_dec * 2 * Bm_ * ctx_ * d * 2, false);
    build_tensors();
    if (synthetic) gen_synthetic(seed);
    HIP_CHECK(hipDeviceSynchronize());
}

MoonshineEngine::~MoonshineEngine() {  // the step graphs and the debug buffer; ~SeqEngine frees the rest
    (void)hipSetDevice(dev_);
    if (st_) (void)hipStreamSynchronize(st_);
    for (auto& kv : graphs_) (void)hipGraphExecDestroy(kv.second);
    if (logits_dbg_) (void)hipFree(logits_dbg_);
}

void MoonshineEngine::build_tensors() {
    const MsDims& D = D_;
    const int d = D.d, ff = D.ff;
    const std::string E = "model.encoder.", Dn = "model.decoder.";
    add_tensor(E + "conv1.weight", (int64_t)d * MS_K1, T_CONV1, conv1_, d, MS_K1, MS_K1P, 0, 0);
    add_tensor(E + "groupnorm.weight", d, T_VEC, gn_w_, d, 1, 1, 0, 0);
    add_tensor(E + "groupnorm.bias", d, T_VEC, gn_b_, d, 1, 1, 0, 0);
    add_tensor(E + "conv2.weight", (int64_t)n2_ * d * MS_K2, T_CONVK, conv2_, n2_, d, dp_, 0, MS_K2);
    add_tensor(E + "conv2.bias", n2_, T_VEC, b2_, n2_, 1, 1, 0, 0);
    add_tensor(E + "conv3.weight", (int64_t)d * n2_ * MS_K3, T_CONVK, conv3_, d, n2_, n2p_, 0, MS_K3);
    add_tensor(E + "conv3.bias", d, T_VEC, b3_, d, 1, 1, 0, 0);
    for (int l = 0; l < D.n_enc; l++) {
        const std::string P = E + "layers." + std::to_string(l) + ".";
        EncLayer& L = enc_[l];
        add_tensor(P + "input_layernorm.weight", d, T_VEC, L.ln1, d, 1, 1, 0, 0);
        add_tensor(P + "self_attn.q_proj.weight", (int64_t)d * d, T_MAT16, L.qkv, d, d, dp_, 0, 0);
        add_tensor(P + "self_attn.k_proj.weight", (int64_t)d * d, T_MAT16, L.qkv, d, d, dp_, dp_, 0);
        add_tensor(P + "self_attn.v_proj.weight", (int64_t)d * d, T_MAT16, L.qkv, d, d, dp_, 2 * dp_, 0);
        add_tensor(P + "self_attn.o_proj.weight", (int64_t)d * d, T_MAT16, L.o, d, d, dp_, 0, 0);
        add_tensor(P + "post_attention_layernorm.weight", d, T_VEC, L.ln2, d, 1, 1, 0, 0);
        add_tensor(P + "mlp.fc1.weight", (int64_t)ff * d, T_MAT16, L.fc1, ff, d, dp_, 0, 0);
        add_tensor(P + "mlp.fc1.bias", ff, T_VEC, L.fc1b, ff, 1, 1, 0, 0);
        add_tensor(P + "mlp.fc2.weight", (int64_t)d * ff, T_MAT16, L.fc2, d, ff, ffp_, 0, 0);
        add_tensor(P + "mlp.fc2.bias", d, T_VEC, L.fc2b, d, 1, 1, 0, 0);
    }
    add_tensor(E + "layer_norm.weight", d, T_VEC, enc_ln_, d, 1, 1, 0, 0);
    add_tensor(Dn + "embed_tokens.weight", (int64_t)D.vocab * d, T_MAT16, emb_, D.vocab, d, d, 0, 0);
    for (int l = 0; l < D.n_dec; l++) {
        const std::string P = Dn + "layers." + std::to_string(l) + ".";
        DecLayer& L = dec_[l];
        add_tensor(P + "input_layernorm.weight", d, T_VEC, L.ln1, d, 1, 1, 0, 0);
        add_tensor(P + "self_attn.q_proj.weight", (int64_t)d * d, T_MAT16, L.sqkv, d, d, d, 0, 0);
        add_tensor(P + "self_attn.k_proj.weight", (int64_t)d * d, T_MAT16, L.sqkv, d, d, d, d, 0);
        add_tensor(P + "self_attn.v_proj.weight", (int64_t)d * d, T_MAT16, L.sqkv, d, d, d, 2 * d, 0);
        add_tensor(P + "self_attn.o_proj.weight", (int64_t)d * d, T_MAT16, L.so, d, d, d, 0, 0);
        add_tensor(P + "post_attention_layernorm.weight", d, T_VEC, L.ln2, d, 1, 1, 0, 0);
        add_tensor(P + "encoder_attn.q_proj.weight", (int64_t)d * d, T_MAT16, L.cq, d, d, d, 0, 0);
        add_tensor(P + "encoder_attn.k_proj.weight", (int64_t)d * d, T_MAT16, L.ckv, d, d, dp_, 0, 0);
        add_tensor(P + "encoder_attn.v_proj.weight", (int64_t)d * d, T_MAT16, L.ckv, d, d, dp_, dp_, 0);
        add_tensor(P + "encoder_attn.o_proj.weight", (int64_t)d * d, T_MAT16, L.co, d, d, d, 0, 0);
        add_tensor(P + "final_layernorm.weight", d, T_VEC, L.ln3, d, 1, 1, 0, 0);
        add_tensor(P + "mlp.fc1.weight", (int64_t)2 * ff * d, T_MAT16, L.fc1, 2 * ff, d, d, 0, 0);
        add_tensor(P + "mlp.fc1.bias", 2 * ff, T_VEC, L.fc1b, 2 * ff, 1, 1, 0, 0);
        add_tensor(P + "mlp.fc2.weight", (int64_t)d * ff, T_MAT16, L.fc2, d, ff, ff, 0, 0);
        add_tensor(P + "mlp.fc2.bias", d, T_VEC, L.fc2b, d, 1, 1, 0, 0);
    }
    add_tensor(Dn + "norm.weight", d, T_VEC, dec_ln_, d, 1, 1, 0, 0);
    add_tensor("proj_out.weight", (int64_t)D.vocab * d, T_TIED, emb_, D.vocab, d, d, 0, 0);
    tensors_.back().set = true;  // tied to embed_tokens: never required
}

void MoonshineEngine::set_special(const Tensor& t, const float* data) {
    const int64_t n = t.numel;
    if (t.kind == T_CONV1) {
        std::vector<float> h((size_t)t.N * MS_K1P, 0.0f);
        for (int r = 0; r < t.N; r++)
            for (int k = 0; k < MS_K1; k++) h[(size_t)r * MS_K1P + k] = data[(size_t)r * MS_K1 + k];
        HIP_CHECK(hipMemcpy(t.dst, h.data(), h.size() * 4, hipMemcpyHostToDevice));
    } else if (t.kind == T_CONVK) {  // [N][C][Kw] -> [N][Kw][Cp]
        const int C = t.K, Cp = t.ld, Kw = t.Kw;
        std::vector<uint16_t> h((size_t)t.N * Kw * Cp, 0);
        for (int r = 0; r < t.N; r++)
            for (int c = 0; c < C; c++)
                for (int k = 0; k < Kw; k++)
                    h[((size_t)r * Kw + k) * Cp + c] = f2h_bits(data[((size_t)r * C + c) * Kw + k]);
        HIP_CHECK(hipMemcpy(t.dst, h.data(), h.size() * 2, hipMemcpyHostToDevice));
    } else {  // T_TIED: must be the embedding already loaded
        const Tensor& e = tensors_[tensor_ix_.at("model.decoder.embed_tokens.weight")];
        if (!e.set) throw std::runtime_error("moonshine: proj_out.weight given before model.decoder.embed_tokens.weight");
        std::vector<uint16_t> h((size_t)n);
        HIP_CHECK(hipMemcpy(h.data(), emb_, (size_t)n * 2, hipMemcpyDeviceToHost));
        for (int64_t i = 0; i < n; i++)
            if (h[(size_t)i] != f2h_bits(data[i])) throw std::runtime_error("moonshine: proj_out.weight is not tied to embed_tokens.weight");
    }
}

void MoonshineEngine::upload(const float* const* pcm, const size_t* n, int B) {
    SeqEngine::upload(pcm, n, B, MS_MIN_SAMPLES, [](int64_t ns, int* len) {
        len[1] = frames1(ns); len[2] = frames2(len[1]); len[3] = frames3(len[2]);
    });
    T1p_ = lens_max_[1]; T2p_ = lens_max_[2]; T3p_ = lens_max_[3];
}

void MoonshineEngine::run_stem(int B) {
    const int d = D_.d;
    ms_frames(pcm_, stride_, lens_, B, T1p_, frames_, st_);
    gemm(DT_F32, EPI_BIAS, frames_, MS_K1P, conv1_, MS_K1P, B * T1p_, dp_, MS_K1P, nullptr, h1_, dp_, st_);
    ms_tanh_gn_stats(h1_, lens_, B, T1p_, d, dp_, 1e-5f, stats_, st_);
    ms_gather2(h1_, stats_, gn_w_, gn_b_, lens_, B, T1p_, T2p_, d, dp_, A2_, st_);
    gemm(DT_F16, EPI_BIAS_F32, A2_, MS_K2 * dp_, conv2_, MS_K2 * dp_, B * T2p_, n2p_, MS_K2 * dp_, b2_, c2_, n2p_, st_);
    ms_gather3(c2_, lens_, B, T2p_, T3p_, n2p_, A3_, st_);
    gemm(DT_F16, EPI_BIAS_F32, A3_, MS_K3 * n2p_, conv3_, MS_K3 * n2p_, B * T3p_, dp_, MS_K3 * n2p_, b3_, x_, dp_, st_);
    ms_gelu_rows(x_, lens_, 3, B, T3p_, dp_, st_);
}

void MoonshineEngine::run_encoder(int B) {
    const MsDims& D = D_;
    const int M = B * T3p_, d = D.d;
    for (const EncLayer& L : enc_) {
        ms_layernorm(x_, M, d, dp_, L.ln1, xn16_, dp_, false, st_);
        gemm(DT_F16, EPI_BIAS_F32, xn16_, dp_, L.qkv, dp_, M, 3 * dp_, dp_, nullptr, qkv32_, 3 * dp_, st_);
        ms_rope_enc(qkv32_, B, T3p_, D.H, D.dh, D.rot, dp_, rope_, qkv16_, st_);
        MsAttnArgs a{};
        a.q = qkv16_; a.ldq = 3 * dp_; a.q_bstride = (int64_t)T3p_ * 3 * dp_;
        a.k = (const f16*)qkv16_ + dp_; a.v = (const f16*)qkv16_ + 2 * dp_; a.ldk = 3 * dp_; a.k_bstride = a.q_bstride;
        a.out = att16_; a.ldo = dp_; a.o_bstride = (int64_t)T3p_ * dp_;
        a.lens = lens_; a.s = state_; a.B = B; a.H = D.H; a.dh = D.dh; a.Tq = T3p_;
        ms_attention(MS_ATT_ENC, a, st_);
        gemm(DT_F16, EPI_BIAS_RESID, att16_, dp_, L.o, dp_, M, dp_, dp_, nullptr, x_, dp_, st_);
        ms_layernorm(x_, M, d, dp_, L.ln2, xn16_, dp_, false, st_);
        gemm(DT_F16, EPI_BIAS_F32, xn16_, dp_, L.fc1, dp_, M, ffp_, dp_, L.fc1b, h32_, ffp_, st_);
        ms_gelu_f16(h32_, (int64_t)M * ffp_, h16_, st_);
        gemm(DT_F16, EPI_BIAS_RESID, h16_, ffp_, L.fc2, ffp_, M, dp_, ffp_, L.fc2b, x_, dp_, st_);
    }
    ms_layernorm(x_, M, d, dp_, enc_ln_, enc16_, dp_, false, st_);
}

void MoonshineEngine::run_cross_kv(int B) {
    for (size_t l = 0; l < dec_.size(); l++)
        gemm(DT_F16, EPI_BIAS, enc16_, dp_, dec_[l].ckv, dp_, B * T3p_, 2 * dp_, dp_, nullptr, ckv_[l], 2 * dp_, st_);
}

void MoonshineEngine::enqueue_step(int R) {
    const MsDims& D = D_;
    const int d = D.d;
    ms_embed(emb_, d, R, cur_tok_, forced_, state_, dx_, st_);
    for (size_t l = 0; l < dec_.size(); l++) {
        const DecLayer& L = dec_[l];
        f16* cache = (f16*)cache_ + (int64_t)l * 2 * Bm_ * ctx_ * d;
        ms_layernorm(dx_, R, d, d, L.ln1, dxn16_, d, false, st_);
        ms_gemv(MS_GV_F32, dxn16_, R, d, L.sqkv, nullptr, 3 * d, dqkv32_, state_, st_);
        ms_rope_dec(dqkv32_, R, D.H, D.dh, D.rot, d, rope_, state_, dq16_, cache, ctx_, st_);
        MsAttnArgs a{};
        a.q = dq16_; a.ldq = d; a.q_bstride = d;
        a.k = cache; a.v = cache + (int64_t)R * ctx_ * d; a.ldk = d; a.k_bstride = (int64_t)ctx_ * d;
        a.out = datt16_; a.ldo = d; a.o_bstride = d;
        a.lens = lens_; a.s = state_; a.B = R; a.H = D.H; a.dh = D.dh; a.Tq = 1;
        ms_attention(MS_ATT_SELF, a, st_);
        ms_gemv(MS_GV_RESID, datt16_, R, d, L.so, nullptr, d, dx_, state_, st_);
        ms_layernorm(dx_, R, d, d, L.ln2, dxn16_, d, false, st_);
        ms_gemv(MS_GV_F16, dxn16_, R, d, L.cq, nullptr, d, dq16_, state_, st_);
        a.k = ckv_[l]; a.v = (const f16*)ckv_[l] + dp_; a.ldk = 2 * dp_; a.k_bstride = 0;
        ms_attention(MS_ATT_CROSS, a, st_);
        ms_gemv(MS_GV_RESID, datt16_, R, d, L.co, nullptr, d, dx_, state_, st_);
        ms_layernorm(dx_, R, d, d, L.ln3, dxn16_, d, false, st_);
        ms_gemv(MS_GV_SILU, dxn16_, R, d, L.fc1, L.fc1b, D.ff, dg16_, state_, st_);
        ms_gemv(MS_GV_RESID, dg16_, R, D.ff, L.fc2, L.fc2b, d, dx_, state_, st_);
    }
    ms_layernorm(dx_, R, d, d, dec_ln_, dxn16_, d, false, st_);
    ms_gemv(MS_GV_LOGITS, dxn16_, R, d, emb_, nullptr, D.vocab, nullptr, state_, st_);
    MsFinArgs f{};
    f.R = R; f.V = D.vocab; f.s = state_;
    f.cur_tok = cur_tok_; f.done = done_; f.n_out = n_out_; f.hit_eos = hit_eos_; f.limit = limit_;
    f.out_tok = out_tok_; f.out_top1 = out_top1_; f.out_top2 = out_top2_;
    ms_finalize(f, st_);
    ms_advance(state_, st_);
}

hipGraphExec_t MoonshineEngine::step_graph(int R) {
    auto it = graphs_.find(R);
    if (it != graphs_.end()) return it->second;
    hipGraph_t graph;
    HIP_CHECK(hipStreamBeginCapture(st_, hipStreamCaptureModeThreadLocal));
    try {
        enqueue_step(R);
    } catch (...) {
        (void)hipStreamEndCapture(st_, &graph);
        throw;
    }
    HIP_CHECK(hipStreamEndCapture(st_, &graph));
    hipGraphExec_t exec;
    HIP_CHECK(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
    HIP_CHECK(hipGraphDestroy(graph));
    graphs_[R] = exec;
    return exec;
}

int MoonshineEngine::run_decode(int R, const int* limit, const int* forced, int forced_len, float* logits_all) {
    int maxlim = 0;
    std::vector<int> lim(R), zero(R, 0), bos(R, D_.bos);
    for (int r = 0; r < R; r++) {
        lim[r] = std::max(0, std::min(limit[r], ctx_));
        maxlim = std::max(maxlim, lim[r]);
    }
    MsState s{};
    s.step = 0; s.t3p = T3p_; s.forced_len = forced_len; s.log_all = logits_all ? 1 : 0;
    s.logits = logits_all ? logits_all : logits_;
    s.eos = D_.eos; s.cap = ctx_;
    hipGraphExec_t exec = step_graph(R);
    HIP_CHECK(hipMemcpyAsync(state_, &s, sizeof(s), hipMemcpyHostToDevice, st_));
    HIP_CHECK(hipMemcpyAsync(cur_tok_, bos.data(), R * 4, hipMemcpyHostToDevice, st_));
    HIP_CHECK(hipMemcpyAsync(done_, zero.data(), R * 4, hipMemcpyHostToDevice, st_));
    HIP_CHECK(hipMemcpyAsync(n_out_, zero.data(), R * 4, hipMemcpyHostToDevice, st_));
    HIP_CHECK(hipMemcpyAsync(hit_eos_, zero.data(), R * 4, hipMemcpyHostToDevice, st_));
    HIP_CHECK(hipMemcpyAsync(limit_, lim.data(), R * 4, hipMemcpyHostToDevice, st_));
    if (forced_len > 0)
        HIP_CHECK(hipMemcpyAsync(forced_, forced, (size_t)R * forced_len * 4, hipMemcpyHostToDevice, st_));
    HIP_CHECK(hipStreamSynchronize(st_));  // the host vectors above have been read
    int steps = 0;
    std::vector<int> done(R);
    while (steps < maxlim) {
        HIP_CHECK(hipGraphLaunch(exec, st_));
        steps++;
        if (steps % 16 == 0 && steps < maxlim) {  // coarse early-out: a finished row records nothing further
            HIP_CHECK(hipMemcpyAsync(done.data(), done_, R * 4, hipMemcpyDeviceToHost, st_));
            HIP_CHECK(hipStreamSynchronize(st_));
            if (std::all_of(done.begin(), done.end(), [](int v) { return v != 0; })) break;
        }
    }
    return steps;
}

std::vector<MsUtt> MoonshineEngine::transcribe(const float* const* pcm, const size_t* n, int B, const int* limit) {
    select();
    require_weights();
    upload(pcm, n, B);
    HIP_CHECK(hipEventRecord(ev_[0], st_));  // the phase times are device work: the host-to-device copy is not in stem_ms
    run_stem(B);
    HIP_CHECK(hipEventRecord(ev_[1], st_));
    run_encoder(B);
    HIP_CHECK(hipEventRecord(ev_[2], st_));
    run_cross_kv(B);
    HIP_CHECK(hipEventRecord(ev_[3], st_));
    const int steps = run_decode(B, limit, nullptr, 0, nullptr);
    HIP_CHECK(hipEventRecord(ev_[4], st_));
    std::vector<int> n_out(B), eos(B), tok((size_t)B * ctx_);
    std::vector<float> t1((size_t)B * ctx_), t2((size_t)B * ctx_);
    HIP_CHECK(hipMemcpyAsync(n_out.data(), n_out_, B * 4, hipMemcpyDeviceToHost, st_));
    HIP_CHECK(hipMemcpyAsync(eos.data(), hit_eos_, B * 4, hipMemcpyDeviceToHost, st_));
    HIP_CHECK(hipMemcpyAsync(tok.data(), out_tok_, tok.size() * 4, hipMemcpyDeviceToHost, st_));
    HIP_CHECK(hipMemcpyAsync(t1.data(), out_top1_, t1.size() * 4, hipMemcpyDeviceToHost, st_));
    HIP_CHECK(hipMemcpyAsync(t2.data(), out_top2_, t2.size() * 4, hipMemcpyDeviceToHost, st_));
    HIP_CHECK(hipStreamSynchronize(st_));
    float ms[4];
    phase_ms(4, ms);
    tm_.stem_ms = ms[0]; tm_.encoder_ms = ms[1]; tm_.cross_kv_ms = ms[2]; tm_.decode_ms = ms[3];
    tm_.total_ms = (double)ms[0] + ms[1] + ms[2] + ms[3];
    tm_.n_steps = steps; tm_.batch = B;
    std::vector<MsUtt> out(B);
    for (int b = 0; b < B; b++) {
        const int k = std::max(0, std::min(n_out[b], ctx_));
        out[b].tok.assign(tok.begin() + (size_t)b * ctx_, tok.begin() + (size_t)b * ctx_ + k);
        out[b].top1.assign(t1.begin() + (size_t)b * ctx_, t1.begin() + (size_t)b * ctx_ + k);
        out[b].top2.assign(t2.begin() + (size_t)b * ctx_, t2.begin() + (size_t)b * ctx_ + k);
        out[b].hit_eos = eos[b] != 0;
    }
    return out;
}

void MoonshineEngine::debug_encode(const float* pcm, size_t n, bool encoded, float* out) {
    select();
    require_weights();
    if (!out) throw std::runtime_error("moonshine: null output");
    upload(&pcm, &n, 1);
    run_stem(1);
    const float* src = x_;
    if (encoded) {
        run_encoder(1);
        ms_layernorm(x_, T3p_, D_.d, dp_, enc_ln_, enc32_, dp_, true, st_);
        src = enc32_;
    }
    HIP_CHECK(hipMemcpy2DAsync(out, (size_t)D_.d * 4, src, (size_t)dp_ * 4, (size_t)D_.d * 4, (size_t)T3p_,
                               hipMemcpyDeviceToHost, st_));
    HIP_CHECK(hipStreamSynchronize(st_));
}

void MoonshineEngine::debug_logits(const float* pcm, size_t n, const int* prefix, int np, float* out) {
    select();
    require_weights();
    if (!prefix || !out || np < 1 || np > ctx_) throw std::runtime_error("moonshine: prefix length outside 1..ctx");
    for (int i = 0; i < np; i++)
        if (prefix[i] < 0 || prefix[i] >= D_.vocab) throw std::runtime_error("moonshine: prefix token outside the vocabulary");
    const int64_t need = (int64_t)np * D_.vocab;
    if (need > logits_dbg_cap_) {
        HIP_CHECK(hipStreamSynchronize(st_));
        if (logits_dbg_) HIP_CHECK(hipFree(logits_dbg_));
        logits_dbg_ = nullptr;
        logits_dbg_cap_ = 0;
        HIP_CHECK(hipMalloc((void**)&logits_dbg_, (size_t)need * 4));
        logits_dbg_cap_ = need;
    }
    upload(&pcm, &n, 1);
    run_stem(1);
    run_encoder(1);
    run_cross_kv(1);
    run_decode(1, &np, prefix, np, logits_dbg_);
    HIP_CHECK(hipMemcpyAsync(out, logits_dbg_, (size_t)need * 4, hipMemcpyDeviceToHost, st_));
    HIP_CHECK(hipStreamSynchronize(st_));
}

}  // namespace spt
