// seq_engine.cpp -- the core under the Moonshine and SenseVoice engines (seq_engine.h).
#include "seq_engine.h"

#include <algorithm>

#include "common.h"
#include "kernels.h"

namespace spt {

void SeqEngine::gemm(int dtype, int epi, const void* A, int lda, const void* W, int ldw, int M, int N, int K,
                     const float* bias, void* C, int ldc, hipStream_t st) {
    GemmArgs g{};
    g.A = A; g.lda = lda; g.sA = 0;
    g.W = W; g.ldw = ldw;
    g.M = M; g.N = N; g.K = K;
    g.bias = bias;
    g.C = C; g.ldc = ldc; g.sC = 0;
    g.alpha = 1.0f; g.ksplit = 1; g.c_split = 0; g.nmajor = 0; g.groups = 1;
    gemm_nt_variant(dtype, epi, g, 1, N % 128 == 0 ? 1 : 5, st);
}

void SeqEngine::open(int n_events) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || dev_ < 0 || dev_ >= ndev) {
        (void)hipGetLastError();
        throw HipError(tag_ + ": no HIP device " + std::to_string(dev_));
    }
    select();
    HIP_CHECK(hipStreamCreateWithFlags(&st_, hipStreamNonBlocking));
    ev_.resize(n_events);
    for (auto& e : ev_) HIP_CHECK(hipEventCreate(&e));
}

SeqEngine::~SeqEngine() {
    if (!st_) return;  // never opened
    (void)hipSetDevice(dev_);
    (void)hipStreamSynchronize(st_);
    for (void* p : allocs_) (void)hipFree(p);
    for (auto& e : ev_) if (e) (void)hipEventDestroy(e);
    (void)hipStreamDestroy(st_);
}

void SeqEngine::select() const { HIP_CHECK(hipSetDevice(dev_)); }

void* SeqEngine::dalloc(int64_t bytes, bool weight) {
    void* p = nullptr;
    if (bytes <= 0) bytes = 16;
    if (hipMalloc(&p, (size_t)bytes) != hipSuccess) {
        (void)hipGetLastError();
        throw std::runtime_error(tag_ + ": out of device memory (" + std::to_string(bytes) + " bytes)");
    }
    allocs_.push_back(p);
    HIP_CHECK(hipMemset(p, 0, (size_t)bytes));
    (weight ? weight_bytes_ : work_bytes_) += bytes;
    return p;
}

void SeqEngine::add_tensor(const std::string& name, int64_t numel, int kind, void* dst, int N, int K, int ld, int row0,
                           int Kw) {
    tensor_ix_[name] = (int)tensors_.size();
    tensors_.push_back(Tensor{name, numel, kind, dst, N, K, ld, row0, Kw, false});
}

int64_t SeqEngine::tensor_numel(const std::string& name) const {
    auto it = tensor_ix_.find(name);
    return it == tensor_ix_.end() ? -1 : tensors_[it->second].numel;
}

int SeqEngine::missing() const {
    int n = 0;
    for (const Tensor& t : tensors_) n += t.set ? 0 : 1;
    return n;
}

void SeqEngine::require_weights() const {
    for (const Tensor& t : tensors_)
        if (!t.set) throw std::runtime_error(tag_ + ": tensor not set: " + t.name + " (" + std::to_string(missing()) + " missing)");
}

void SeqEngine::set_tensor(const std::string& name, const float* data, int64_t n) {
    auto it = tensor_ix_.find(name);
    if (it == tensor_ix_.end()) throw std::runtime_error(tag_ + ": unknown tensor '" + name + "'");
    Tensor& t = tensors_[it->second];
    if (!data || n != t.numel)
        throw std::runtime_error(tag_ + ": tensor '" + name + "' has " + std::to_string(t.numel) + " elements, got " + std::to_string(n));
    select();
    HIP_CHECK(hipStreamSynchronize(st_));
    if (t.kind == T_VEC) {
        HIP_CHECK(hipMemcpy(t.dst, data, (size_t)n * 4, hipMemcpyHostToDevice));
    } else if (t.kind == T_MAT16) {
        std::vector<uint16_t> h((size_t)t.N * t.ld, 0);
        for (int r = 0; r < t.N; r++)
            for (int k = 0; k < t.K; k++) h[(size_t)r * t.ld + k] = f2h_bits(data[(size_t)r * t.K + k]);
        HIP_CHECK(hipMemcpy((uint16_t*)t.dst + (size_t)t.row0 * t.ld, h.data(), h.size() * 2, hipMemcpyHostToDevice));
    } else
        set_special(t, data);
    t.set = true;
}

void SeqEngine::set_special(const Tensor& t, const float*) {
    throw std::runtime_error(tag_ + ": tensor '" + t.name + "' has no loader");
}

void SeqEngine::gen_synthetic(uint64_t seed) {
    int64_t maxn = 0;
    for (const Tensor& t : tensors_) maxn = std::max(maxn, t.numel);
    float* tmp = nullptr;
    HIP_CHECK(hipMalloc((void**)&tmp, (size_t)maxn * 4));
    std::vector<float> h((size_t)maxn);
    try {
        for (size_t i = 0; i < tensors_.size(); i++) {  // i is the tensor's PRNG stream, skipped tensors keep theirs
            const Tensor t = tensors_[i];
            if (t.set) continue;  // Moonshine's proj_out, tied to the embedding
            const bool is_bias = t.name.find(".bias") != std::string::npos;
            const bool is_norm = !is_bias && t.name.find("norm") != std::string::npos;
            gen_weights(DT_F32, tmp, t.numel, seed, (uint32_t)i, is_norm ? WK_LNW : is_bias ? WK_BIAS : WK_MAT,
                        is_norm ? -3 : is_bias ? -5 : -4, st_);
            HIP_CHECK(hipMemcpyAsync(h.data(), tmp, (size_t)t.numel * 4, hipMemcpyDeviceToHost, st_));
            HIP_CHECK(hipStreamSynchronize(st_));
            set_tensor(t.name, h.data(), t.numel);
        }
    } catch (...) {
        (void)hipFree(tmp);
        throw;
    }
    HIP_CHECK(hipFree(tmp));
}

void SeqEngine::upload(const float* const* pcm, const size_t* n, int B, int min_samples,
                       const std::function<void(int64_t, int*)>& rule) {
    if (B < 1 || B > Bm_) throw std::runtime_error(tag_ + ": batch outside 1..max_batch");
    std::vector<int> lens((size_t)B * 4);
    size_t nmax = 0;
    for (int& m : lens_max_) m = 0;
    for (int b = 0; b < B; b++) {
        if (!pcm[b] || n[b] < (size_t)min_samples || n[b] > (size_t)Ns_)
            throw std::runtime_error(tag_ + ": utterance of " + std::to_string(n[b]) + " samples (takes " +
                                     std::to_string(min_samples) + ".." + std::to_string(Ns_) + ")");
        int* row = &lens[(size_t)b * 4];
        row[0] = (int)n[b];
        rule((int64_t)n[b], row);
        for (int c = 0; c < 4; c++) lens_max_[c] = std::max(lens_max_[c], row[c]);
        nmax = std::max(nmax, n[b]);
    }
    stride_ = (int64_t)nmax;
    for (int b = 0; b < B; b++)
        HIP_CHECK(hipMemcpyAsync(pcm_ + b * stride_, pcm[b], n[b] * 4, hipMemcpyHostToDevice, st_));
    HIP_CHECK(hipMemcpyAsync(lens_, lens.data(), lens.size() * 4, hipMemcpyHostToDevice, st_));
    HIP_CHECK(hipStreamSynchronize(st_));  // lens (a local) has been read
}

void SeqEngine::phase_ms(int n, float* ms) const {
    for (int i = 0; i < n; i++) {
        ms[i] = 0.0f;
        HIP_CHECK(hipEventElapsedTime(&ms[i], ev_[i], ev_[i + 1]));
    }
}

}  // namespace spt
