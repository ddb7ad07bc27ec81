// moonshine.h -- the Moonshine engine (encoder-decoder transformer over raw PCM), fp16 on gfx950.
//
// f16 weights and GEMM / GEMV inputs, f32 accumulation, f32 residual stream, norms and softmax.
// Widths are padded to a multiple of 64 (dp) wherever gemm_nt runs: its tiles want N % 64 and
// K % 64, and d = 416 (Base) and 288 (Tiny) are neither; the decode step's GEMVs read unpadded
// copies.  DESIGN.md §12 is the contract.
#pragma once
#include <hip/hip_runtime.h>

#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "ms_host.h"
#include "ms_kernels.h"
#include "seq_engine.h"

namespace spt {

struct MsUtt {
    std::vector<int> tok;
    std::vector<float> top1, top2;
    bool hit_eos = false;
};

struct MsTimings {
    double stem_ms = 0, encoder_ms = 0, cross_kv_ms = 0, decode_ms = 0, total_ms = 0;
    int n_steps = 0, batch = 0;
};

// The tensor names are the HF state dict's (SeqEngine::set_tensor).
class MoonshineEngine : public SeqEngine {
public:
    MoonshineEngine(const MsDims& dims, int device, int max_batch, int max_samples, uint64_t seed, bool synthetic);
    ~MoonshineEngine() override;

    const MsDims& dims() const { return D_; }
    int ctx() const { return ctx_; }
    const MsTimings& timings() const { return tm_; }

    static int frames1(int64_t n) { return n < MS_K1 ? 0 : (int)((n - MS_K1) / MS_S1 + 1); }
    static int frames2(int t1) { return t1 < MS_K2 ? 0 : (t1 - MS_K2) / MS_S2 + 1; }
    static int frames3(int t2) { return t2 < MS_K3 ? 0 : (t2 - MS_K3) / MS_S3 + 1; }
    static int enc_frames(int64_t n) { return frames3(frames2(frames1(n))); }

    // B <= max_batch utterances of MS_MIN_SAMPLES..max_samples samples each; limit[b] tokens at most
    std::vector<MsUtt> transcribe(const float* const* pcm, const size_t* n, int B, const int* limit);
    // one utterance: [T3][d] f32 before the first layer (encoded = false) or the encoder output
    void debug_encode(const float* pcm, size_t n, bool encoded, float* out);
    // one utterance + forced prefix -> logits [np][V] through the step graph
    void debug_logits(const float* pcm, size_t n, const int* prefix, int np, float* out);
    // zero the timings (a call that starts no device pass reports none)
    void clear_timings() { tm_ = MsTimings(); }

private:
    struct EncLayer { float *ln1, *ln2, *fc1b, *fc2b; void *qkv, *o, *fc1, *fc2; };
    struct DecLayer { float *ln1, *ln2, *ln3, *fc1b, *fc2b; void *sqkv, *so, *cq, *ckv, *co, *fc1, *fc2; };

    void build_tensors();
    // conv1's padded rows, the conv2 / conv3 re-layout, and the check of the tied proj_out
    void set_special(const Tensor& t, const float* data) override;
    void upload(const float* const* pcm, const size_t* n, int B);
    void run_stem(int B);
    void run_encoder(int B);
    void run_cross_kv(int B);
    void enqueue_step(int R);
    hipGraphExec_t step_graph(int R);
    int run_decode(int R, const int* limit, const int* forced, int forced_len, float* logits_all);

    MsDims D_;
    int dp_, n2_, n2p_, ffp_, ctx_, T1m_, T2m_, T3m_;
    int T1p_ = 0, T2p_ = 0, T3p_ = 0;  // this call's padded frame counts
    MsTimings tm_;
    // weights
    float *conv1_, *gn_w_, *gn_b_, *b2_, *b3_, *enc_ln_, *dec_ln_, *rope_;
    void *conv2_, *conv3_, *emb_;
    std::vector<EncLayer> enc_;
    std::vector<DecLayer> dec_;
    // workspace
    float *frames_, *h1_, *stats_, *c2_, *x_, *qkv32_, *h32_, *enc32_;
    void *A2_, *A3_, *xn16_, *qkv16_, *att16_, *h16_, *enc16_;
    std::vector<void*> ckv_;
    // decode
    MsState* state_;
    int *cur_tok_, *done_, *n_out_, *hit_eos_, *limit_, *forced_, *out_tok_;
    float *out_top1_, *out_top2_, *dx_, *dqkv32_, *logits_, *logits_dbg_ = nullptr;
    int64_t logits_dbg_cap_ = 0;
    void *dxn16_, *dq16_, *datt16_, *dg16_, *cache_;
    std::map<int, hipGraphExec_t> graphs_;
};

}  // namespace spt
