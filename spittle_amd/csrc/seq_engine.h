// seq_engine.h -- what the Moonshine and SenseVoice engines share: the device, stream and events, the
// tracked zero-filled allocations, the table of named weight tensors with its two common kinds, the
// synthetic weights, the PCM / lens upload and the phase times.  An engine derives from SeqEngine;
// `tag` ("moonshine", "sensevoice") prefixes every message.  DESIGN.md §13a.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <functional>
#include <map>
#include <string>
#include <vector>

namespace spt {

class SeqEngine {
public:
    SeqEngine(const SeqEngine&) = delete;
    SeqEngine& operator=(const SeqEngine&) = delete;

    int max_batch() const { return Bm_; }
    int max_samples() const { return Ns_; }
    int64_t weight_bytes() const { return weight_bytes_; }
    int64_t workspace_bytes() const { return work_bytes_; }

    // state-dict names; numel -1 for an unknown name
    int64_t tensor_numel(const std::string& name) const;
    void set_tensor(const std::string& name, const float* data, int64_t n);
    // tensors still to be supplied
    virtual int missing() const;

protected:
    // T_VEC: numel f32 copied as they are.  T_MAT16: f32 [N][K] -> f16 rows of pitch ld (pad columns
    // zero) at row row0 of dst.  Kinds from T_ENGINE on are the engine's own (set_special).
    enum { T_VEC = 0, T_MAT16 = 1, T_ENGINE = 2 };
    struct Tensor {
        std::string name;
        int64_t numel;
        int kind;
        void* dst;
        int N, K, ld, row0, Kw;
        bool set;
    };

    // holds the arguments only: the engine validates them, then open()s the device
    SeqEngine(const char* tag, int device, int max_batch, int max_samples)
        : tag_(tag), dev_(device), Bm_(max_batch), Ns_(max_samples) {}
    // frees every allocation, the events and the stream, also when the engine's constructor throws
    virtual ~SeqEngine();

    // checks the device ordinal, selects it, creates the stream and n_events events
    void open(int n_events);
    void select() const;
    void* dalloc(int64_t bytes, bool weight);
    void add_tensor(const std::string& name, int64_t numel, int kind, void* dst, int N, int K, int ld, int row0 = 0,
                    int Kw = 0);
    // a kind >= T_ENGINE: store data (numel checked, device selected, stream idle)
    virtual void set_special(const Tensor& t, const float* data);
    virtual void require_weights() const;
    // every tensor not yet set, from the PRNG stream of its index: norm weights near 1 (2^-3), biases
    // 2^-5, the rest 2^-4
    void gen_synthetic(uint64_t seed);
    // B utterances of min_samples..max_samples samples -> pcm_ (row stride stride_) and lens_ [B][4];
    // rule fills columns 1..3 of an utterance's lens row from its sample count.  lens_max_[c] is the
    // largest value of column c: the padded row counts of this call.
    void upload(const float* const* pcm, const size_t* n, int B, int min_samples,
                const std::function<void(int64_t, int*)>& rule);
    // ms[i] = time between events i and i + 1 (recorded on st_, completed)
    void phase_ms(int n, float* ms) const;
    // gemm_nt with a named tile, never the automatic choice: the automatic variant wants N % 128 == 0,
    // so a narrower N names the 64 x 64 tile.  The rest name the 128 x 128 tile: k_gemm.hip states its
    // 128 / 64-row tiles bitwise equal, not the 256 x 256 kernel the automatic choice may take at a
    // large M, and a batch row must get what it gets alone
    static void gemm(int dtype, int epi, const void* A, int lda, const void* W, int ldw, int M, int N, int K,
                     const float* bias, void* C, int ldc, hipStream_t st);

    const std::string tag_;
    int dev_, Bm_, Ns_;
    hipStream_t st_ = nullptr;
    std::vector<hipEvent_t> ev_;
    std::vector<Tensor> tensors_;
    std::map<std::string, int> tensor_ix_;
    float* pcm_ = nullptr;  // [max_batch][max_samples], the engine's allocation
    int* lens_ = nullptr;   // [max_batch][4], the engine's allocation
    int64_t stride_ = 0;
    int lens_max_[4] = {0, 0, 0, 0};

private:
    std::vector<void*> allocs_;
    int64_t weight_bytes_ = 0, work_bytes_ = 0;
};

}  // namespace spt
