// capi_gemm.cpp -- spt_debug_gemm and spt_debug_layernorm: one gemm_nt_variant launch (k_gemm.hip) and
// one layernorm / layernorm_pend / layernorm_pend2 launch (k_norm.hip) on caller-supplied arrays (no
// engine, no model), for tests/test_gpu_gemm.py.  Each call owns its stream and its buffers on the
// device the caller names, rounds the f32 operands to the engine dtype on the host and returns f32;
// the launches are the engine's, through the launchers of kernels.h.  Everything a launcher would
// throw on, or that would read or write outside a buffer, is refused here first.
#include <hip/hip_runtime.h>
#include <string.h>

#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/spittle_hip.h"
#include "capi_debug.h"
#include "capi_internal.h"
#include "common.h"
#include "kernels.h"

namespace {

using namespace spt::dbg;

void check_dtype(int32_t dtype, const char* who) {
    if (dtype != spt::DT_F32 && dtype != spt::DT_BF16 && dtype != spt::DT_F16)
        throw std::runtime_error(std::string(who) + ": dtype is f32, bf16 or f16");
}

constexpr int64_t kMaxElems = (int64_t)1 << 26;  // of any one buffer of a call

// the epilogues that store the engine dtype (the others store f32)
bool stores_dtype(int epi) {
    return epi == spt::EPI_BIAS || epi == spt::EPI_BIAS_GELU || epi == spt::EPI_BIAS_SWISH || epi == spt::EPI_BIAS_RELU ||
           epi == spt::EPI_KVSPLIT;
}

// an address with the alignment of element `off` of a device allocation (256-byte aligned), for
// gemm_nt_plan, which reads alignments only
const void* fake_ptr(int64_t off, int esz) { return (const void*)(uintptr_t)((1ull << 32) + (uint64_t)off * esz); }

}  // namespace

extern "C" {

spt_status spt_debug_gemm(int32_t device, int32_t dtype, int32_t epi, int32_t variant, int32_t batch, int32_t M,
                          int32_t N, int32_t K, const float* A, int64_t a_count, int64_t a_off, int32_t lda, int64_t sA,
                          const float* W, int32_t ldw, const float* bias, const float* pos, float* C, int64_t c_count,
                          int64_t c_off, int32_t ldc, int64_t sC, float alpha, int32_t ksplit, int64_t c_split,
                          int32_t kv_B, int32_t kv_T, int32_t kv_H, char* err, size_t errlen) {
    if (!A || !W || !C) {
        set_err(err, errlen, "null argument");
        return SPT_ERR_INVALID_ARG;
    }
    int esz = 4, osz = 4;
    try {
        check_dtype(dtype, "debug_gemm");
        esz = spt::dtype_size(dtype);
        if (epi < spt::EPI_BIAS || epi > spt::EPI_PARTIAL) throw std::runtime_error("debug_gemm: epilogue 0..8");
        osz = stores_dtype(epi) ? esz : 4;
        if (variant < 0 || variant > 5) throw std::runtime_error("debug_gemm: variant 0..5");
        if (M < 1 || N < 1 || K < 1) throw std::runtime_error("debug_gemm: need M, N, K >= 1");
        if (batch < 1 || batch > 65535) throw std::runtime_error("debug_gemm: batch 1..65535 (grid z)");
        if (ksplit < 1 || ksplit > 65535) throw std::runtime_error("debug_gemm: ksplit 1..65535 (grid y)");
        if (a_count < 1 || a_count > kMaxElems || c_count < 1 || c_count > kMaxElems || (int64_t)N * ldw > kMaxElems ||
            (int64_t)M * N > kMaxElems)
            throw std::runtime_error("debug_gemm: buffers above 2^26 elements");
        if (a_off < 0 || c_off < 0 || lda < 1 || sA < 0 || sC < 0 || c_split < 0)
            throw std::runtime_error("debug_gemm: negative offset or stride");
        if (ldw < K) throw std::runtime_error("debug_gemm: W is [N][ldw], ldw >= K");
        if (variant == 2 && dtype == spt::DT_F32) throw std::runtime_error("debug_gemm: the 256 x 256 tile is bf16 / f16");
        if (epi == spt::EPI_BIAS_GELU_POS && !pos) throw std::runtime_error("debug_gemm: EPI_BIAS_GELU_POS needs pos [M][N]");
        if ((epi == spt::EPI_PARTIAL || epi == spt::EPI_KVSPLIT) && batch != 1)
            throw std::runtime_error("debug_gemm: EPI_PARTIAL and EPI_KVSPLIT ignore the batch stride of C: batch == 1");
        // A: the last row's K elements of the last batch item
        if (a_off + (int64_t)(batch - 1) * sA + (int64_t)(M - 1) * lda + K > a_count)
            throw std::runtime_error("debug_gemm: A read beyond a_count");
        // what the launcher refuses (shape, split, epilogue, batch, alignment), on addresses with the
        // alignment the device buffers will have
        spt::GemmArgs g{};
        g.A = fake_ptr(a_off, esz); g.lda = lda; g.sA = sA;
        g.W = fake_ptr(0, esz); g.ldw = ldw;
        g.M = M; g.N = N; g.K = K;
        g.bias = bias; g.C = (void*)fake_ptr(c_off, osz); g.ldc = ldc; g.sC = sC;
        g.pos = pos ? (const float*)fake_ptr(0, 4) : nullptr;
        g.kv_B = kv_B; g.kv_T = kv_T; g.kv_H = kv_H;
        g.alpha = alpha; g.ksplit = ksplit; g.c_split = c_split;
        const int kernel = spt::gemm_nt_plan(dtype, epi, g, batch, variant);
        if (variant == 2 && kernel != 2)
            throw std::runtime_error("debug_gemm: variant 2 would not run the 256 x 256 tile (N % 256, K / ksplit % 64)");
        // C
        if (epi == spt::EPI_KVSPLIT) {
            if (kv_B < 1 || kv_T < 1 || kv_H < 1) throw std::runtime_error("debug_gemm: need kv_B, kv_T, kv_H >= 1");
            if (N % (2 * kv_H * 64)) throw std::runtime_error("debug_gemm: EPI_KVSPLIT needs N % (2 * kv_H * 64) == 0");
            if ((int64_t)kv_B * kv_T != M) throw std::runtime_error("debug_gemm: EPI_KVSPLIT needs M == kv_B * kv_T");
            const int64_t layers = N / (2 * kv_H * 64);
            if (spt::kv_layer_elems(kv_B, kv_H, kv_T) > kMaxElems ||
                c_off + layers * spt::kv_layer_elems(kv_B, kv_H, kv_T) > c_count)
                throw std::runtime_error("debug_gemm: the K/V cache layers reach beyond c_count");
        } else {
            if (ldc < N) throw std::runtime_error("debug_gemm: ldc below N");
            const int64_t item = (int64_t)(M - 1) * ldc + N;  // one batch item or slab of C
            if (batch > 1 && sC < item) throw std::runtime_error("debug_gemm: batch items of C overlap");
            if (epi == spt::EPI_PARTIAL) {
                if (ksplit > 1 && c_split < item) throw std::runtime_error("debug_gemm: split-K slabs of C overlap");
                if (c_off + (int64_t)(ksplit - 1) * c_split + item > c_count)
                    throw std::runtime_error("debug_gemm: the last split-K slab reaches beyond c_count");
            } else if (c_off + (int64_t)(batch - 1) * sC + item > c_count) {
                throw std::runtime_error("debug_gemm: C written beyond c_count");
            }
        }
    } catch (const std::exception& e) {
        set_err(err, errlen, e.what());
        return SPT_ERR_INVALID_ARG;
    }
    if (spt_status s = device_ok(device, err, errlen)) return s;
    try {
        const int cdt = stores_dtype(epi) ? dtype : spt::DT_F32;
        std::vector<uint16_t> a16, w16, c16;
        Scope sc(device);
        spt::gemm_prepare();
        const char* dA = (const char*)up_as(sc, dtype, A, (size_t)a_count, a16);
        const void* dW = up_as(sc, dtype, W, (size_t)N * ldw, w16);
        char* dC = (char*)up_as(sc, cdt, C, (size_t)c_count, c16);
        spt::GemmArgs g{};
        g.A = dA + (size_t)a_off * esz; g.lda = lda; g.sA = sA;
        g.W = dW; g.ldw = ldw;
        g.M = M; g.N = N; g.K = K;
        g.bias = bias ? sc.up(bias, (size_t)N) : nullptr;
        g.C = dC + (size_t)c_off * osz; g.ldc = ldc; g.sC = sC;
        g.pos = pos ? sc.up(pos, (size_t)M * N) : nullptr;
        g.kv_B = kv_B; g.kv_T = kv_T; g.kv_H = kv_H;
        g.alpha = alpha; g.ksplit = ksplit; g.c_split = c_split;
        spt::gemm_nt_variant(dtype, epi, g, batch, variant, sc.st);
        SPT_LAUNCH_CHECK();
        down_f32(sc, cdt, dC, C, (size_t)c_count);
        sc.sync();
        return SPT_OK;
    } catch (const std::exception& e) {
        set_err(err, errlen, e.what());
        return spt_classify(e);
    }
}

spt_status spt_debug_layernorm(int32_t device, int32_t dtype, int32_t mode, float* x, int32_t M, int32_t d,
                               const float* slab, int64_t slab_count, int32_t ks, int64_t slab_stride,
                               const float* pbias, float alpha, const float* w, const float* b, const float* w2,
                               const float* b2, int32_t write_x, float* y, float* y2, char* err, size_t errlen) {
    if (!x || !w || !b || !y) {
        set_err(err, errlen, "null argument");
        return SPT_ERR_INVALID_ARG;
    }
    try {
        check_dtype(dtype, "debug_layernorm");
        if (mode < SPT_LN_PLAIN || mode > SPT_LN_PEND2) throw std::runtime_error("debug_layernorm: mode 0..2");
        if (M < 1 || d < 4) throw std::runtime_error("debug_layernorm: need M >= 1, d >= 4");
        if (d % 4) throw std::runtime_error("layernorm: d % 4");
        if (mode == SPT_LN_PEND2 ? d > 1024 : d > 1536)
            throw std::runtime_error(mode == SPT_LN_PEND2 ? "layernorm_pend2: d too large" : "layernorm: d too large");
        if ((int64_t)M * d > kMaxElems) throw std::runtime_error("debug_layernorm: M * d above 2^26");
        if (mode != SPT_LN_PLAIN) {
            if (!pbias) throw std::runtime_error("layernorm_pend: null pbias (the kernel reads it unconditionally)");
            if (!slab) throw std::runtime_error("debug_layernorm: null slabs");
            if (mode == SPT_LN_PEND2 && ks != 1 && ks != 2 && ks != 4 && ks != 8)
                throw std::runtime_error("layernorm_pend2: split count must be 1, 2, 4 or 8");
            if (ks < 1 || ks > 64) throw std::runtime_error("debug_layernorm: 1..64 slabs");
            if (slab_stride < 0 || slab_stride % 4) throw std::runtime_error("debug_layernorm: slab_stride >= 0, % 4 (16-byte loads)");
            if (slab_count < 1 || slab_count > kMaxElems || (int64_t)(ks - 1) * slab_stride + (int64_t)M * d > slab_count)
                throw std::runtime_error("debug_layernorm: the last slab reaches beyond slab_count");
            if (mode == SPT_LN_PEND2 && (!w2 || !b2 || !y2)) throw std::runtime_error("debug_layernorm: pend2 needs w2, b2 and y2");
        }
    } catch (const std::exception& e) {
        set_err(err, errlen, e.what());
        return SPT_ERR_INVALID_ARG;
    }
    if (spt_status s = device_ok(device, err, errlen)) return s;
    try {
        const size_t n = (size_t)M * d, esz = (size_t)spt::dtype_size(dtype);
        Scope sc(device);
        float* dx = sc.up((const float*)x, n);
        const float* dw = sc.up(w, (size_t)d);
        const float* db = sc.up(b, (size_t)d);
        if (mode == SPT_LN_PLAIN) {
            void* dy = sc.out<char>(n * esz);
            spt::layernorm(dtype, dx, M, d, dw, db, dy, sc.st);
            SPT_LAUNCH_CHECK();
            down_f32(sc, dtype, dy, y, n);
        } else {
            const float* ds = sc.up(slab, (size_t)slab_count);
            const float* dp = sc.up(pbias, (size_t)d);
            if (mode == SPT_LN_PEND) {
                void* dy = sc.out<char>(n * esz);
                spt::layernorm_pend(dtype, dx, M, d, ds, ks, slab_stride, dp, alpha, dw, db, dy, write_x != 0, sc.st);
                down_f32(sc, dtype, dy, y, n);
                sc.down(x, (const float*)dx, n);
            } else {
                float* dy = sc.out<float>(n);
                void* dy2 = sc.out<char>(n * esz);
                spt::layernorm_pend2(dtype, dx, M, d, ds, ks, slab_stride, dp, alpha, dw, db, dy, sc.up(w2, (size_t)d),
                                     sc.up(b2, (size_t)d), dy2, sc.st);
                sc.down(y, (const float*)dy, n);
                down_f32(sc, dtype, dy2, y2, n);
            }
        }
        sc.sync();
        return SPT_OK;
    } catch (const std::exception& e) {
        set_err(err, errlen, e.what());
        return spt_classify(e);
    }
}

}  // extern "C"
