// capi_qgemv.cpp -- spt_debug_qgemv: the decoder GEMV alone over one quantised matrix (no engine, no
// model), for tests/test_qresident_ref.py and tests/test_gpu_qgemv.py.  The call owns its stream and
// buffers (capi_debug.h), checks every argument on the host before any launch, packs the file's blocks
// with the loader's packer (ggml_qpack.h) and runs gemv() of kernels.h twice on the same operands: on
// the weights expanded to the engine dtype by ggml_dequant (what a load without
// SPT_MODEL_QUANT_RESIDENT leaves in the arena) and on the packed matrix.
#include <hip/hip_runtime.h>
#include <string.h>

#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/spittle_hip.h"
#include "capi_debug.h"
#include "capi_internal.h"
#include "common.h"
#include "ggml_qpack.h"
#include "kernels.h"

namespace {

using namespace spt::dbg;

struct Unsupported : std::runtime_error {
    using std::runtime_error::runtime_error;
};

constexpr int64_t kMaxElems = (int64_t)1 << 26;  // of any one buffer of a call

}  // namespace

extern "C" spt_status spt_debug_qgemv(int32_t device, int32_t dtype, int32_t ggml_type, const void* blocks,
                                      size_t blocks_bytes, int32_t N, int32_t K, const float* act, int32_t R,
                                      const float* ln_w, const float* ln_b, const float* bias, const float* resid,
                                      int32_t mode, int32_t a_src, int32_t ksplit, float* out_plain, float* out_packed,
                                      float* top_plain, float* top_packed, float* unpacked, char* err, size_t errlen) {
    using namespace spt;
    if (!blocks || !act || !out_plain || !out_packed) {
        set_err(err, errlen, "null argument");
        return SPT_ERR_INVALID_ARG;
    }
    std::vector<uint8_t> packed;
    int d = 0;  // GV_QKV_CACHE: the model width
    try {
        if (dtype == DT_F32) throw Unsupported("debug_qgemv: the f32 engine keeps no quantised matrices");
        if (dtype != DT_BF16 && dtype != DT_F16) throw std::runtime_error("debug_qgemv: dtype is bf16 or f16");
        if (N < 1 || K < 1 || R < 1 || R > 64) throw std::runtime_error("debug_qgemv: need N, K >= 1 and 1..64 rows");
        if (K % 32) throw std::runtime_error("debug_qgemv: K is not a whole number of 32-element blocks");
        if (K % QPACK_KS) throw std::runtime_error("debug_qgemv: K must be a multiple of 128");
        int blck, bb;
        ggml_block_geom(ggml_type, &blck, &bb);
        QPackGeom qg;
        if (!qpack_geom(ggml_type, &qg)) throw Unsupported("debug_qgemv: no resident layout for this ggml type");
        if ((int64_t)N * K > kMaxElems) throw std::runtime_error("debug_qgemv: N * K above 2^26");
        if (blocks_bytes != (size_t)N * (size_t)(K / 32) * (size_t)bb)
            throw std::runtime_error("debug_qgemv: blocks_bytes is not the size of [N][K / 32] blocks");
        const bool ln = a_src == SPT_QGEMV_A_LN;
        if (a_src != SPT_QGEMV_A_DIRECT && !ln) throw std::runtime_error("debug_qgemv: a_src is A_DIRECT or A_LN");
        const bool ln_mode = mode == GV_BIAS || mode == GV_BIAS_GELU || mode == GV_QKV_CACHE || mode == GV_LOGITS;
        const bool direct_mode = mode == GV_PARTIAL || mode == GV_BIAS_RESID;
        if (!(ln && ln_mode) && !(!ln && direct_mode))
            throw std::runtime_error("debug_qgemv: not one of the decoder's (mode, A source) pairs");
        if (ln && (!ln_w || !ln_b)) throw std::runtime_error("gemv: LayerNorm prologue needs K <= 1536 and LN parameters");
        if (ln && K > 1536) throw std::runtime_error("gemv: LayerNorm prologue needs K <= 1536 and LN parameters");
        if (ln && R > gemv_max_image_rows(dtype, K)) throw std::runtime_error("gemv: A image exceeds the LDS budget");
        if (ksplit < 1) throw std::runtime_error("debug_qgemv: ksplit below 1");
        if (ksplit > 1 && mode != GV_PARTIAL) throw std::runtime_error("gemv: K split needs partial outputs");
        if (ksplit > K / QPACK_KS) throw std::runtime_error("gemv: K split exceeds the super-steps");
        const int nss = (K / QPACK_KS + ksplit - 1) / ksplit;
        if (nss > (ln ? 16 : 48)) throw std::runtime_error("gemv: K too large");
        if (mode == GV_BIAS_RESID && !resid) throw std::runtime_error("debug_qgemv: GV_BIAS_RESID needs the residual rows");
        if (resid && mode != GV_BIAS_RESID && mode != GV_PARTIAL)
            throw std::runtime_error("gemv: residual rows into slab 0 need partial outputs");
        if (mode == GV_QKV_CACHE) {
            if (N % 192) throw std::runtime_error("debug_qgemv: GV_QKV_CACHE needs N = 3 d, d a multiple of 64");
            d = N / 3;
        }
        if (mode == GV_LOGITS && (!top_plain || !top_packed)) throw std::runtime_error("debug_qgemv: GV_LOGITS returns the top-2 partials");
        if ((int64_t)ksplit * R * N > kMaxElems) throw std::runtime_error("debug_qgemv: output above 2^26 elements");
        packed.resize((size_t)qpack_bytes(ggml_type, N, K));
        if (!qpack_rows(ggml_type, (const uint8_t*)blocks, blocks_bytes, N, K, packed.data()))
            throw std::runtime_error("debug_qgemv: packing failed");
        if (unpacked && !qpack_unpack_f32(ggml_type, packed.data(), N, K, unpacked))
            throw std::runtime_error("debug_qgemv: unpacking failed");
    } catch (const Unsupported& e) {
        set_err(err, errlen, e.what());
        return SPT_ERR_UNSUPPORTED;
    } catch (const std::exception& e) {
        set_err(err, errlen, e.what());
        return SPT_ERR_INVALID_ARG;
    }
    if (spt_status s = device_ok(device, err, errlen)) return s;
    try {
        const bool ln = a_src == SPT_QGEMV_A_LN;
        const size_t nA = (size_t)R * K, esz = 2;
        const int n_tiles = (N + 15) / 16;
        const size_t n_out = mode == GV_PARTIAL ? (size_t)ksplit * R * N : (size_t)R * N;
        std::vector<uint16_t> a16;
        Scope sc(device);
        gemv_prepare(dtype);
        gemv_q_prepare(dtype);
        // the weights both ways
        const uint8_t* d_blk = sc.up((const uint8_t*)blocks, blocks_bytes);
        void* d_wplain = sc.out<char>((size_t)N * K * esz);
        ggml_dequant(ggml_type, d_blk, (int64_t)N * K, dtype, d_wplain, sc.st);
        const uint8_t* d_wpack = sc.up(packed.data(), packed.size());
        // operands
        const void* d_A;
        if (ln) d_A = sc.up(act, nA);
        else {
            a16 = to_half_storage(dtype, act, nA);
            d_A = sc.up(a16.data(), nA);
        }
        const float* d_lnw = ln ? sc.up(ln_w, (size_t)K) : nullptr;
        const float* d_lnb = ln ? sc.up(ln_b, (size_t)K) : nullptr;
        float* d_zero = nullptr;
        if (ln) {
            d_zero = sc.alloc<float>(nA);
            HIP_CHECK(hipMemsetAsync(d_zero, 0, nA * sizeof(float), sc.st));
        }
        const float* d_bias = bias ? sc.up(bias, (size_t)N) : nullptr;
        const float* d_resid = resid ? sc.up(resid, (size_t)R * N) : nullptr;
        const DecState ds0{0, 0, 0u};
        const DecState* d_ds = sc.up(&ds0, 1);
        const std::vector<uint32_t> sup0((size_t)(N + 31) / 32, 0u);
        const uint32_t* d_sup = mode == GV_LOGITS ? sc.up(sup0.data(), sup0.size()) : nullptr;

        for (int pass = 0; pass < 2; ++pass) {
            float* h_out = pass ? out_packed : out_plain;
            float* h_top = pass ? top_packed : top_plain;
            GemvArgs a{};
            a.A = d_A; a.lda = K; a.R = R; a.N = N; a.K = K; a.bias = d_bias; a.ksplit = ksplit;
            a.W = pass ? (const void*)d_wpack : (const void*)d_wplain;
            a.wq = pass ? ggml_type : 0;
            if (ln) {
                a.ln_w = d_lnw; a.ln_b = d_lnb;
                for (int p = 0; p < kMaxPend; ++p) a.pend[p] = d_zero;
                a.n_pend = 0;
            }
            a.st = d_ds;
            void* d_C = nullptr;     // storage of the launch's C
            void* d_cache = nullptr;
            void* d_part = nullptr;
            if (mode == GV_BIAS || mode == GV_BIAS_GELU) {
                d_C = sc.out<char>((size_t)R * N * esz);
                a.C = d_C; a.ldc = N;
            } else if (mode == GV_QKV_CACHE) {
                d_C = sc.out<char>((size_t)R * d * esz);
                d_cache = sc.out<char>((size_t)2 * R * d * esz);  // [2][B = R][H][ctx = 1][64]
                a.C = d_C; a.ldc = d;
                a.cache = d_cache; a.cache_B = R; a.cache_H = d / 64; a.cache_ctx = 1; a.Tq = 1;
            } else if (mode == GV_PARTIAL) {
                d_C = sc.out<float>(n_out);
                a.C = d_C; a.ldc = N; a.c_split = (int64_t)R * N; a.p_resid = d_resid;
            } else if (mode == GV_BIAS_RESID) {
                float* c = sc.alloc<float>((size_t)R * N);
                HIP_CHECK(hipMemcpyAsync(c, d_resid, (size_t)R * N * sizeof(float), hipMemcpyDeviceToDevice, sc.st));
                d_C = c;
                a.C = d_C; a.ldc = N;
            } else {  // GV_LOGITS
                d_C = sc.out<float>((size_t)R * N);
                d_part = sc.out<char>((size_t)R * n_tiles * 16);
                a.C = d_C; a.ldc = N; a.suppress = d_sup; a.blank0 = a.blank1 = -1;
                a.part = d_part; a.n_tiles = n_tiles;
            }
            gemv(dtype, mode, ln ? A_LN : A_DIRECT, a, sc.st);
            if (mode == GV_BIAS || mode == GV_BIAS_GELU) {
                float* f = sc.alloc<float>((size_t)R * N);
                to_f32(dtype, d_C, f, (int64_t)R * N, sc.st);
                SPT_LAUNCH_CHECK();
                sc.down(h_out, (const float*)f, (size_t)R * N);
            } else if (mode == GV_QKV_CACHE) {
                float* fq = sc.alloc<float>((size_t)R * d);
                float* fc = sc.alloc<float>((size_t)2 * R * d);
                to_f32(dtype, d_C, fq, (int64_t)R * d, sc.st);
                to_f32(dtype, d_cache, fc, (int64_t)2 * R * d, sc.st);
                SPT_LAUNCH_CHECK();
                for (int r = 0; r < R; ++r) {
                    sc.down(h_out + (size_t)r * N, (const float*)fq + (size_t)r * d, (size_t)d);
                    sc.down(h_out + (size_t)r * N + d, (const float*)fc + (size_t)r * d, (size_t)d);
                    sc.down(h_out + (size_t)r * N + 2 * d, (const float*)fc + ((size_t)R + r) * d, (size_t)d);
                }
            } else {
                sc.down(h_out, (const float*)d_C, n_out);
                if (mode == GV_LOGITS) sc.down(h_top, (const float*)d_part, (size_t)R * n_tiles * 4);
            }
        }
        sc.sync();
        return SPT_OK;
    } catch (const std::exception& e) {
        set_err(err, errlen, e.what());
        return spt_classify(e);
    }
}
