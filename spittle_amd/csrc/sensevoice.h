// sensevoice.h -- the SenseVoice-Small engine (Kaldi fbank + LFR, SANM encoder, CTC head), fp16 on gfx950.
//
// f16 weights and GEMM inputs, f32 accumulation, f32 residual stream, norms, softmax and front end.
// Non-autoregressive: one forward pass per call, no decode graph.  The LFR width (560) is padded to a
// multiple of 64 for gemm_nt, the vocabulary (25055) to a multiple of 128; pad columns are kept zero
// and the CTC argmax reads the real columns only.  DESIGN.md §13 is the contract.
#pragma once
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>
#include <vector>

#include "seq_engine.h"
#include "sv_host.h"
#include "sv_kernels.h"

namespace spt {

struct SvUtt {
    std::vector<int> tok, frame;
    std::vector<float> top1, top2;
    int prefix[SV_NQ] = {-1, -1, -1, -1};
};

struct SvTimings {
    double frontend_ms = 0, encoder_ms = 0, ctc_ms = 0, total_ms = 0;
    int rows = 0, batch = 0;
};

struct SvInfer {
    int language = 0;  // 0 auto, 1 zh, 2 en, 3 yue, 4 ja, 5 ko
    bool use_itn = false;
};

// The tensor names are the FunASR state dict's (SeqEngine::set_tensor).
class SenseVoiceEngine : public SeqEngine {
public:
    SenseVoiceEngine(const SvDims& dims, int device, int max_batch, int max_samples, uint64_t seed, bool synthetic);

    const SvDims& dims() const { return D_; }
    int max_rows() const { return Rm_; }
    const SvTimings& timings() const { return tm_; }
    void clear_timings() { tm_ = SvTimings(); }

    // (x + neg_mean) * inv_std over the LFR width
    void set_cmvn(const float* neg_mean, const float* inv_std, int n);
    // tensors (and the CMVN pair, counted as one) still to be supplied
    int missing() const override;

    int rows_of(int64_t n) const { return sv_rows_of(n, D_.lfr_n); }

    // B <= max_batch utterances of 400..max_samples samples each
    std::vector<SvUtt> transcribe(const float* const* pcm, const size_t* n, int B, const SvInfer& p);
    // one utterance: the LFR rows after CMVN [T_lfr][in]
    void debug_features(const float* pcm, size_t n, float* out);
    // one utterance: the encoder output after tp_norm [R][d] f32
    void debug_encode(const float* pcm, size_t n, const SvInfer& p, float* out);
    // one utterance: per row the top-1 id and the top-1 / top-2 logits, [R] each
    void debug_frames(const float* pcm, size_t n, const SvInfer& p, int* ids, float* top1, float* top2);

private:
    struct Layer {
        int din, ldin;
        float *n1w, *n1b, *qkvb, *fsmn, *ob, *n2w, *n2b, *w1b, *w2b;
        void *qkv, *o, *w1, *w2;
    };

    void build_tensors();
    void upload_tables();
    void require_weights() const override;
    void upload(const float* const* pcm, const size_t* n, int B);
    void run_frontend(int B, const SvInfer& p, bool feat_only);
    void norm16(const float* x, int M, int d, int ld, const float* w, const float* b, void* y);
    void run_encoder(int B);
    void run_ctc(int B);

    SvDims D_;
    int in_, inp_, Vp_, Tm_, Rm_, chunk_;
    int Tp_ = 0, Rp_ = 0;  // this call's padded fbank frames and encoder rows
    bool cmvn_set_ = false;
    SvTimings tm_;
    // tables and weights
    float *win_, *basis_, *fbT_, *inv_freq_, *neg_mean_, *inv_std_, *embed_;
    float *an_w_, *an_b_, *tn_w_, *tn_b_, *ctc_b_;
    void* ctc_w_;
    std::vector<Layer> layers_;
    // workspace
    float *frames_, *spec_, *mel_, *rows_, *x_, *enc32_, *logits_, *top1_, *top2_;
    void *xn16_, *qkv16_, *att16_, *h16_;
    int *ids_, *out_;
};

}  // namespace spt
