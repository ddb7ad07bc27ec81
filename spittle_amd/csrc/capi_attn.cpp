// capi_attn.cpp -- spt_debug_attn_*: the Whisper attention kernels alone (enc_attention of k_attn.hip;
// dec_self_attn, dec_cross_attn, dec_cross_attn_vw and dec_attn_part_merge of k_dec.hip) on
// caller-supplied arrays (no engine, no model), for tests/test_gpu_attn.py.  Each call owns its stream
// and its buffers on the device the caller names, rounds the f32 inputs to the engine dtype on the
// host and returns f32; the launches are the engine's, through the launchers of kernels.h.  Every
// shape a launcher would throw on, or that would read outside a buffer, is refused here first.
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
#include "prefill_host.h"

namespace {

using namespace spt::dbg;

void check_dtype(int32_t dtype) {
    if (dtype != spt::DT_F32 && dtype != spt::DT_BF16 && dtype != spt::DT_F16)
        throw std::runtime_error("debug_attn: dtype is f32, bf16 or f16");
}

constexpr int64_t kMaxElems = (int64_t)1 << 26;  // of any one buffer of a call

}  // namespace

extern "C" {

spt_status spt_debug_attn_enc(int32_t device, int32_t dtype, const float* qkv, int32_t B, int32_t T, int32_t H,
                              float* out, char* err, size_t errlen) {
    if (!qkv || !out) {
        set_err(err, errlen, "null argument");
        return SPT_ERR_INVALID_ARG;
    }
    try {
        check_dtype(dtype);
        if (B < 1 || T < 1 || H < 1) throw std::runtime_error("debug_attn_enc: need B, T, H >= 1");
        if ((int64_t)B * T * 3 * H * 64 > kMaxElems) throw std::runtime_error("debug_attn_enc: B * T * 3 * H * 64 above 2^26");
        if (H > 65535 || B > 65535) throw std::runtime_error("debug_attn_enc: H, B <= 65535 (grid y / z)");
    } catch (const std::exception& e) {
        set_err(err, errlen, e.what());
        return SPT_ERR_INVALID_ARG;
    }
    if (spt_status s = device_ok(device, err, errlen)) return s;
    try {
        const size_t rows = (size_t)B * T, d = (size_t)H * 64, esz = (size_t)spt::dtype_size(dtype);
        std::vector<uint16_t> h16;
        Scope sc(device);
        const void* d_qkv = up_as(sc, dtype, qkv, rows * 3 * d, h16);
        void* d_out = sc.out<char>(rows * d * esz);
        spt::enc_attention(dtype, d_qkv, B, T, H, d_out, sc.st);
        SPT_LAUNCH_CHECK();
        down_f32(sc, dtype, d_out, out, rows * d);
        sc.sync();
        return SPT_OK;
    } catch (const std::exception& e) {
        set_err(err, errlen, e.what());
        return spt_classify(e);
    }
}

spt_status spt_debug_attn_self(int32_t device, int32_t dtype, const float* q, const float* cache, int32_t B,
                               int32_t H, int32_t ctx, int32_t Tq, int32_t pos0, float* out, char* err,
                               size_t errlen) {
    if (!q || !cache || !out) {
        set_err(err, errlen, "null argument");
        return SPT_ERR_INVALID_ARG;
    }
    try {
        check_dtype(dtype);
        if (B < 1 || H < 1 || ctx < 1) throw std::runtime_error("debug_attn_self: need B, H, ctx >= 1");
        if (Tq < 1 || Tq > 4) throw std::runtime_error("dec_self_attn: 1..4 queries per sequence");
        if (pos0 < 0) throw std::runtime_error("debug_attn_self: negative pos0");
        if ((int64_t)pos0 + Tq > ctx) throw std::runtime_error("debug_attn_self: pos0 + Tq beyond the cache");
        if ((int64_t)2 * B * H * ctx * 64 > kMaxElems) throw std::runtime_error("debug_attn_self: cache above 2^26 elements");
    } catch (const std::exception& e) {
        set_err(err, errlen, e.what());
        return SPT_ERR_INVALID_ARG;
    }
    if (spt_status s = device_ok(device, err, errlen)) return s;
    try {
        const size_t nq = (size_t)B * Tq * H * 64, nc = (size_t)2 * B * H * ctx * 64;
        const size_t esz = (size_t)spt::dtype_size(dtype);
        const spt::DecState ds0{pos0, 0, 0u};
        std::vector<uint16_t> q16, c16;
        Scope sc(device);
        const void* d_q = up_as(sc, dtype, q, nq, q16);
        const void* d_c = up_as(sc, dtype, cache, nc, c16);
        const spt::DecState* ds = sc.up(&ds0, 1);
        void* d_out = sc.out<char>(nq * esz);
        spt::dec_self_attn(dtype, d_q, d_c, B, H, ctx, Tq, ds, d_out, sc.st);
        down_f32(sc, dtype, d_out, out, nq);
        sc.sync();
        return SPT_OK;
    } catch (const std::exception& e) {
        set_err(err, errlen, e.what());
        return spt_classify(e);
    }
}

spt_status spt_debug_attn_cross(int32_t device, int32_t dtype, int32_t mode, const float* q, const float* k,
                                const float* v, float pad_value, int32_t B, int32_t B_layout, int32_t b0, int32_t H,
                                int32_t T_enc, int32_t Tq, int32_t splits, const int32_t* kvrow, int32_t share,
                                float* out, float* part, char* err, size_t errlen) {
    if (!q || !k || !v) {
        set_err(err, errlen, "null argument");
        return SPT_ERR_INVALID_ARG;
    }
    const bool vw = mode >= SPT_ATTN_CROSS_VW;
    const bool per_query = mode == SPT_ATTN_CROSS_VW_PQ || mode == SPT_ATTN_CROSS_VW_PQ_MERGE;
    const bool merge = mode == SPT_ATTN_CROSS_VW_MERGE || mode == SPT_ATTN_CROSS_VW_PQ_MERGE;
    try {
        check_dtype(dtype);
        if (mode < SPT_ATTN_CROSS_8WAVE || mode > SPT_ATTN_CROSS_VW_PQ_MERGE) throw std::runtime_error("debug_attn_cross: mode 0..4");
        if (B < 1 || B > 1024 || H < 1 || B_layout < 1) throw std::runtime_error("debug_attn_cross: need 1..1024 rows, H, B_layout >= 1");
        if (T_enc < 1) throw std::runtime_error("debug_attn_cross: T_enc below 1");
        if (Tq < 1 || Tq > 4) throw std::runtime_error("dec_cross_attn: 1..4 queries per sequence");
        if (splits < 1 || splits > 4) throw std::runtime_error("dec_cross_attn: 1..4 key chunks");
        if (splits > 1 && vw) throw std::runtime_error("debug_attn_cross: key chunks are the 8-wave kernel's");
        if (share < 1 || share > 8 || B % share) throw std::runtime_error("dec_cross_attn: rows per window 1..8, dividing B");
        if (share > 1 && !kvrow) throw std::runtime_error("dec_cross_attn: shared windows need the window map");
        if (per_query && Tq != 1) throw std::runtime_error("debug_attn_cross: per_query is the one-token step's");
        const int nq = share * Tq;
        const int NQ = nq == 1 ? 1 : Tq > 1 ? 4 : (spt::dtype_size(dtype) == 2 ? 5 : 4);
        if (splits > 1 && nq > NQ) throw std::runtime_error("dec_cross_attn: key chunks need one query chunk per window");
        if ((int64_t)((T_enc + 31) / 32) * B_layout * H * 4096 >= (int64_t)INT32_MAX)
            throw std::runtime_error("dec_cross_attn: a layer's cross K/V exceeds 2^31 elements");
        if (spt::kv_layer_elems(B_layout, H, T_enc) > kMaxElems || (int64_t)B * Tq * H * 66 * 8 > kMaxElems)
            throw std::runtime_error("debug_attn_cross: buffers above 2^26 elements");
        if (b0 < 0 || (int64_t)b0 + B / share > B_layout) throw std::runtime_error("debug_attn_cross: b0 + B / share beyond B_layout");
        if (kvrow)
            for (int i = 0; i < B; ++i)
                if (kvrow[i] < 0 || (int64_t)b0 + kvrow[i] >= B_layout)
                    throw std::runtime_error("debug_attn_cross: window map entry outside the layout");
        const bool wants_part = (vw && !merge) || (!vw && splits > 1);
        if (wants_part ? !part : !out) throw std::runtime_error("debug_attn_cross: null output for this mode");
    } catch (const std::exception& e) {
        set_err(err, errlen, e.what());
        return SPT_ERR_INVALID_ARG;
    }
    if (spt_status s = device_ok(device, err, errlen)) return s;
    try {
        // the layer as the K/V GEMM's epilogue writes it (kv_offset), the keys of the last 32-key
        // block past T_enc holding pad_value
        const size_t n_kv = (size_t)spt::kv_layer_elems(B_layout, H, T_enc);
        std::vector<float> lay(n_kv, pad_value);
        const int T32 = (T_enc + 31) / 32 * 32;
        for (int kvi = 0; kvi < 2; ++kvi) {
            const float* src = kvi ? v : k;
            for (int b = 0; b < B_layout; ++b)
                for (int h = 0; h < H; ++h)
                    for (int t = 0; t < T32; ++t) {
                        float* dst = lay.data() + spt::kv_offset(0, kvi, b, h, t, 0, B_layout, H, T_enc);
                        if (t < T_enc) memcpy(dst, src + (((size_t)b * H + h) * T_enc + t) * 64, 64 * sizeof(float));
                    }
        }
        const size_t R = (size_t)B * Tq, nq_el = R * H * 64, esz = (size_t)spt::dtype_size(dtype);
        const int S = vw ? 8 : splits;
        const size_t n_part = R * H * S * 66;
        std::vector<uint16_t> q16, kv16;
        Scope sc(device);
        const void* d_q = up_as(sc, dtype, q, nq_el, q16);
        const char* d_kv = (const char*)up_as(sc, dtype, lay.data(), n_kv, kv16) + (size_t)b0 * H * 4096 * esz;
        const int* d_map = kvrow ? sc.up(kvrow, (size_t)B) : nullptr;
        float* d_part = (vw || splits > 1) ? sc.out<float>(n_part) : nullptr;
        void* d_out = (!vw && splits == 1) || merge ? sc.out<char>(nq_el * esz) : nullptr;
        if (vw) {
            spt::dec_cross_attn_vw(dtype, d_q, d_kv, B, B_layout, H, T_enc, Tq, d_part, sc.st, d_map, share, per_query);
            if (merge) spt::dec_attn_part_merge(dtype, d_part, (int)R, H, d_out, sc.st);
        } else {
            spt::dec_cross_attn(dtype, d_q, d_kv, B, B_layout, H, T_enc, Tq, d_out, sc.st, splits, d_part, d_map, share);
        }
        if (d_out) down_f32(sc, dtype, d_out, out, nq_el);
        else sc.down(part, (const float*)d_part, n_part);
        sc.sync();
        return SPT_OK;
    } catch (const std::exception& e) {
        set_err(err, errlen, e.what());
        return spt_classify(e);
    }
}

spt_status spt_debug_xq_fused(int32_t device, int32_t dtype, const float* x, const float* ln_w, const float* ln_b,
                              const float* wq, const float* bias, const float* k, const float* v, float pad_value,
                              int32_t B, int32_t H, int32_t T_enc, int32_t lds, int32_t touch, float* q, float* out,
                              char* err, size_t errlen) {
    if (!x || !ln_w || !ln_b || !wq || !bias || !k || !v || !q || !out) {
        set_err(err, errlen, "null argument");
        return SPT_ERR_INVALID_ARG;
    }
    const int d = 1280;
    try {
        if (dtype != spt::DT_BF16 && dtype != spt::DT_F16) throw std::runtime_error("debug_xq_fused: dtype is bf16 or f16");
        if (H != d / 64) throw std::runtime_error("debug_xq_fused: the fused launch is d = 1280, H = 20");
        if (B < 1 || B > 16) throw std::runtime_error("debug_xq_fused: 1..16 rows");
        if (T_enc < 256 || T_enc > 1536) throw std::runtime_error("debug_xq_fused: T_enc in 256..1536");
        if (lds < 0 || lds > 2) throw std::runtime_error("debug_xq_fused: 0..2 staged blocks per wave");
        if (touch != 0 && touch != 2) throw std::runtime_error("debug_xq_fused: 0 or 2 touched blocks per wave");
    } catch (const std::exception& e) {
        set_err(err, errlen, e.what());
        return SPT_ERR_INVALID_ARG;
    }
    if (spt_status s = device_ok(device, err, errlen)) return s;
    try {
        hipDeviceProp_t prop;
        HIP_CHECK(hipGetDeviceProperties(&prop, device));
        if (!spt::dec_xq_fused_ok(dtype, B, d, H, T_enc, prop.multiProcessorCount)) {
            // (GV_EXACT_LN=0 also lands here: the chain's cross-Q is then another kernel)
            set_err(err, errlen, "debug_xq_fused: 80 + B * H workgroups are not all resident on this device");
            return SPT_ERR_INVALID_ARG;
        }
        // the layer as the K/V GEMM's epilogue writes it, as spt_debug_attn_cross lays it out
        const size_t n_kv = (size_t)spt::kv_layer_elems(B, H, T_enc);
        std::vector<float> lay(n_kv, pad_value);
        const int T32 = (T_enc + 31) / 32 * 32;
        for (int kvi = 0; kvi < 2; ++kvi) {
            const float* src = kvi ? v : k;
            for (int b = 0; b < B; ++b)
                for (int h = 0; h < H; ++h)
                    for (int t = 0; t < T32; ++t) {
                        float* dst = lay.data() + spt::kv_offset(0, kvi, b, h, t, 0, B, H, T_enc);
                        if (t < T_enc) memcpy(dst, src + (((size_t)b * H + h) * T_enc + t) * 64, 64 * sizeof(float));
                    }
        }
        const size_t nq = (size_t)B * d, esz = (size_t)spt::dtype_size(dtype);
        const spt::DecState ds0{0, 0, 0u};
        std::vector<uint16_t> w16, kv16;
        Scope sc(device);
        spt::gemv_prepare(dtype);
        float* zero = sc.alloc<float>(nq);
        HIP_CHECK(hipMemsetAsync(zero, 0, nq * sizeof(float), sc.st));
        unsigned long long* gran = sc.alloc<unsigned long long>(nq);
        HIP_CHECK(hipMemsetAsync(gran, 0, nq * sizeof(unsigned long long), sc.st));
        unsigned* werr = sc.alloc<unsigned>(1);
        HIP_CHECK(hipMemsetAsync(werr, 0, sizeof(unsigned), sc.st));
        spt::GemvArgs a{};
        a.A = sc.up(x, nq); a.lda = d; a.R = B;
        a.ln_w = sc.up(ln_w, (size_t)d); a.ln_b = sc.up(ln_b, (size_t)d);
        for (int p = 0; p < spt::kMaxPend; ++p) a.pend[p] = zero;
        a.W = up_as(sc, dtype, wq, (size_t)d * d, w16); a.N = d; a.K = d;
        a.bias = sc.up(bias, (size_t)d);
        a.C = sc.out<char>(nq * esz); a.ldc = d;
        spt::XqFuseArgs xa{};
        xa.kv = up_as(sc, dtype, lay.data(), n_kv, kv16); xa.B_layout = B; xa.H = H; xa.T_enc = T_enc;
        xa.out = sc.out<char>(nq * esz); xa.gran = gran; xa.ds = sc.up(&ds0, 1); xa.err = werr; xa.layer = 0;
        xa.lds = lds; xa.touch = touch;
        spt::dec_xq_fused(dtype, a, xa, B, sc.st);
        unsigned herr = 0;
        sc.down(&herr, (const unsigned*)werr, 1);
        down_f32(sc, dtype, a.C, q, nq);
        down_f32(sc, dtype, xa.out, out, nq);
        sc.sync();
        if (herr) {  // never retried: the caller sees the wait that ran out
            set_err(err, errlen, "debug_xq_fused: a consumer's wait for q ran out");
            return SPT_ERR_DEVICE;
        }
        return SPT_OK;
    } catch (const std::exception& e) {
        set_err(err, errlen, e.what());
        return spt_classify(e);
    }
}

// The block prefill's attention kernels alone (k_prefill.hip).  What they refuse is
// prefill_host.h's, decided before the device is looked for.
spt_status spt_debug_attn_prefill_self(int32_t device, int32_t dtype, const float* qkv, float* cache, int32_t B, int32_t H,
                                       int32_t ctx, int32_t P, float* out, char* err, size_t errlen) {
    const std::string why = spt::prefill_self_refusal(dtype, qkv, cache, out, B, H, ctx, P);
    if (!why.empty()) {
        set_err(err, errlen, why);
        return SPT_ERR_INVALID_ARG;
    }
    if (spt_status s = device_ok(device, err, errlen)) return s;
    try {
        const size_t rows = (size_t)B * P, d = (size_t)H * 64, nc = (size_t)2 * B * H * ctx * 64;
        const size_t esz = (size_t)spt::dtype_size(dtype);
        std::vector<uint16_t> q16, c16;
        Scope sc(device);
        const void* d_qkv = up_as(sc, dtype, qkv, rows * 3 * d, q16);
        void* d_c = const_cast<void*>(up_as(sc, dtype, cache, nc, c16));
        void* d_out = sc.out<char>(rows * d * esz);
        spt::dec_prefill_self_attn(dtype, d_qkv, d_c, B, B, H, ctx, P, d_out, sc.st);
        down_f32(sc, dtype, d_out, out, rows * d);
        down_f32(sc, dtype, d_c, cache, nc);
        sc.sync();
        return SPT_OK;
    } catch (const std::exception& e) {
        set_err(err, errlen, e.what());
        return spt_classify(e);
    }
}

spt_status spt_debug_attn_prefill_cross(int32_t device, int32_t dtype, const float* q, const float* k, const float* v,
                                        float pad_value, int32_t B, int32_t B_layout, int32_t b0, int32_t H,
                                        int32_t T_enc, int32_t P, int32_t ctx, const int32_t* kvrow, int32_t share,
                                        float* out, char* err, size_t errlen) {
    const std::string why = spt::prefill_cross_refusal(dtype, q, k, v, out, B, B_layout, b0, H, T_enc, P, ctx, kvrow, share);
    if (!why.empty()) {
        set_err(err, errlen, why);
        return SPT_ERR_INVALID_ARG;
    }
    if (spt_status s = device_ok(device, err, errlen)) return s;
    try {
        // the layer as the K/V GEMM's epilogue writes it, as spt_debug_attn_cross lays it out
        const size_t n_kv = (size_t)spt::kv_layer_elems(B_layout, H, T_enc);
        std::vector<float> lay(n_kv, pad_value);
        for (int kvi = 0; kvi < 2; ++kvi) {
            const float* src = kvi ? v : k;
            for (int b = 0; b < B_layout; ++b)
                for (int h = 0; h < H; ++h)
                    for (int t = 0; t < T_enc; ++t)
                        memcpy(lay.data() + spt::kv_offset(0, kvi, b, h, t, 0, B_layout, H, T_enc),
                               src + (((size_t)b * H + h) * T_enc + t) * 64, 64 * sizeof(float));
        }
        const size_t nq = (size_t)B * P * H * 64, esz = (size_t)spt::dtype_size(dtype);
        std::vector<uint16_t> q16, kv16;
        Scope sc(device);
        const void* d_q = up_as(sc, dtype, q, nq, q16);
        const char* d_kv = (const char*)up_as(sc, dtype, lay.data(), n_kv, kv16) + (size_t)b0 * H * 4096 * esz;
        const int* d_map = kvrow ? sc.up(kvrow, (size_t)B) : nullptr;
        void* d_out = sc.out<char>(nq * esz);
        spt::dec_prefill_cross_attn(dtype, d_q, d_kv, B, B_layout, H, T_enc, P, d_out, sc.st, d_map, share);
        down_f32(sc, dtype, d_out, out, nq);
        sc.sync();
        return SPT_OK;
    } catch (const std::exception& e) {
        set_err(err, errlen, e.what());
        return spt_classify(e);
    }
}

}  // extern "C"
