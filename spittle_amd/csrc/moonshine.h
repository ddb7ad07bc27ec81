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

class MoonshineEngine {
public:
    MoonshineEngine(const MsDims& dims, int device, int max_batch, int max_samples, uint64_t seed, bool synthetic);
    ~MoonshineEngine();
    MoonshineEngine(const MoonshineEngine&) = delete;
    MoonshineEngine& operator=(const MoonshineEngine&) = delete;

    const MsDims& dims() const { return D_; }
    int max_batch() const { return Bm_; }
    int max_samples() const { return Ns_; }
    int ctx() const { return ctx_; }
    int64_t weight_bytes() const { return weight_bytes_; }
    int64_t workspace_bytes() const { return work_bytes_; }
    const MsTimings& timings() const { return tm_; }

    // HF state-dict names; numel -1 for an unknown name
    int64_t tensor_numel(const std::string& name) const;
    void set_tensor(const std::string& name, const float* data, int64_t n);
    int missing() const;

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
    struct Tensor {
        std::string name;
        int64_t numel;
        int kind;
        void* dst;
        int N, K, ld, row0, Kw;
        bool set;
    };
    struct EncLayer { float *ln1, *ln2, *fc1b, *fc2b; void *qkv, *o, *fc1, *fc2; };
    struct DecLayer { float *ln1, *ln2, *ln3, *fc1b, *fc2b; void *sqkv, *so, *cq, *ckv, *co, *fc1, *fc2; };

    void select() const;
    void* dalloc(int64_t bytes, bool weight);
    void add_tensor(const std::string& name, int64_t numel, int kind, void* dst, int N, int K, int ld, int row0, int Kw);
    void build_tensors();
    void gen_synthetic(uint64_t seed);
    void require_weights() const;
    void upload(const float* const* pcm, const size_t* n, int B);
    void run_stem(int B);
    void run_encoder(int B);
    void run_cross_kv(int B);
    void enqueue_step(int R);
    hipGraphExec_t step_graph(int R);
    int run_decode(int R, const int* limit, const int* forced, int forced_len, float* logits_all);

    MsDims D_;
    int dev_, Bm_, Ns_, dp_, n2_, n2p_, ffp_, ctx_, T1m_, T2m_, T3m_;
    int T1p_ = 0, T2p_ = 0, T3p_ = 0;
    int64_t stride_ = 0;
    hipStream_t st_ = nullptr;
    std::vector<hipEvent_t> ev_;
    std::vector<void*> allocs_;
    int64_t weight_bytes_ = 0, work_bytes_ = 0;
    std::vector<Tensor> tensors_;
    std::map<std::string, int> tensor_ix_;
    MsTimings tm_;
    // weights
    float *conv1_, *gn_w_, *gn_b_, *b2_, *b3_, *enc_ln_, *dec_ln_, *rope_;
    void *conv2_, *conv3_, *emb_;
    std::vector<EncLayer> enc_;
    std::vector<DecLayer> dec_;
    // workspace
    float *pcm_, *frames_, *h1_, *stats_, *c2_, *x_, *qkv32_, *h32_, *enc32_;
    void *A2_, *A3_, *xn16_, *qkv16_, *att16_, *h16_, *enc16_;
    std::vector<void*> ckv_;
    int* lens_;
    // decode
    MsState* state_;
    int *cur_tok_, *done_, *n_out_, *hit_eos_, *limit_, *forced_, *out_tok_;
    float *out_top1_, *out_top2_, *dx_, *dqkv32_, *logits_, *logits_dbg_ = nullptr;
    int64_t logits_dbg_cap_ = 0;
    void *dxn16_, *dq16_, *datt16_, *dg16_, *cache_;
    std::map<int, hipGraphExec_t> graphs_;
};

}  // namespace spt
