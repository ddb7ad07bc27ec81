// capi_f8kv.cpp -- spt_debug_attn_cross_quant: the fp8 cross K/V kernels alone (k_dec_f8.hip: kv_quant_f8,
// kv_dequant_f8, dec_cross_attn_f8, dec_cross_attn_vw_f8; format: kv_f8.h) on caller-supplied arrays, for
// tests/test_f8kv_ref.py and tests/test_gpu_f8kv_attn.py.  The rules are capi_attn.cpp's: a stream and
// buffers of its own, f32 inputs rounded to the engine dtype on the host, every refusal before any launch.
// The host quantiser's codes (dequantised) and scales are written before the device is looked for, so a
// valid call without a device returns them with SPT_ERR_DEVICE.
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
#include "kv_f8.h"

namespace {

using namespace spt::dbg;

constexpr int64_t kMaxElems = (int64_t)1 << 26;  // of any one buffer of a call

// IEEE half bits -> f32 on the host (exact)
float h2f_bits(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3FFu;
    uint32_t u;
    if (e == 31) u = sign | 0x7F800000u | (m << 13);
    else if (e) u = sign | ((e + 112u) << 23) | (m << 13);
    else if (!m) u = sign;
    else {
        int s = 0;
        uint32_t mm = m;
        while (!(mm & 0x400u)) { mm <<= 1; ++s; }
        u = sign | ((uint32_t)(113 - s) << 23) | ((mm & 0x3FFu) << 13);
    }
    float f;
    memcpy(&f, &u, 4);
    return f;
}

}  // namespace

extern "C" {

spt_status spt_debug_attn_cross_quant(int32_t device, int32_t dtype, int32_t mode, const float* q, const float* k,
                                   const float* v, float pad_value, int32_t B, int32_t B_layout, int32_t b0, int32_t H,
                                   int32_t T_enc, int32_t Tq, const int32_t* kvrow, int32_t share, float* kq, float* vq,
                                   float* k_scale, float* v_scale, float* out, float* part, char* err, size_t errlen) {
    if (!q || !k || !v || !kq || !vq || !k_scale || !v_scale) {
        set_err(err, errlen, "null argument");
        return SPT_ERR_INVALID_ARG;
    }
    if (dtype == spt::DT_F32) {
        set_err(err, errlen, "debug_attn_cross_quant: the fp8 cross K/V is a bf16 or f16 engine's");
        return SPT_ERR_UNSUPPORTED;
    }
    const bool vw = mode >= SPT_ATTN_CROSS_VW;
    const bool per_query = mode == SPT_ATTN_CROSS_VW_PQ || mode == SPT_ATTN_CROSS_VW_PQ_MERGE;
    const bool merge = mode == SPT_ATTN_CROSS_VW_MERGE || mode == SPT_ATTN_CROSS_VW_PQ_MERGE;
    try {
        if (dtype != spt::DT_BF16 && dtype != spt::DT_F16) throw std::runtime_error("debug_attn_cross_quant: dtype is bf16 or f16");
        if (mode < SPT_ATTN_CROSS_8WAVE || mode > SPT_ATTN_CROSS_VW_PQ_MERGE) throw std::runtime_error("debug_attn_cross_quant: mode 0..4");
        if (B < 1 || B > 1024 || H < 1 || B_layout < 1) throw std::runtime_error("debug_attn_cross_quant: need 1..1024 rows, H, B_layout >= 1");
        if (T_enc < 1) throw std::runtime_error("debug_attn_cross_quant: T_enc below 1");
        if (Tq < 1 || Tq > 4) throw std::runtime_error("dec_cross_attn_f8: 1..4 queries per sequence");
        if (share < 1 || share > 8 || B % share) throw std::runtime_error("dec_cross_attn_f8: rows per window 1..8, dividing B");
        if (share > 1 && !kvrow) throw std::runtime_error("dec_cross_attn_f8: shared windows need the window map");
        if (per_query && Tq != 1) throw std::runtime_error("debug_attn_cross_quant: per_query is the one-token step's");
        if (spt::f8::layer_bytes(B_layout, H, T_enc) >= (int64_t)INT32_MAX)
            throw std::runtime_error("dec_cross_attn_f8: a layer's cross K/V records exceed 2^31 bytes");
        if (spt::kv_layer_elems(B_layout, H, T_enc) > kMaxElems || (int64_t)B * Tq * H * 66 * 8 > kMaxElems)
            throw std::runtime_error("debug_attn_cross_quant: buffers above 2^26 elements");
        if (b0 < 0 || (int64_t)b0 + B / share > B_layout) throw std::runtime_error("debug_attn_cross_quant: b0 + B / share beyond B_layout");
        if (kvrow)
            for (int i = 0; i < B; ++i)
                if (kvrow[i] < 0 || (int64_t)b0 + kvrow[i] >= B_layout)
                    throw std::runtime_error("debug_attn_cross_quant: window map entry outside the layout");
        if ((vw && !merge) ? !part : !out) throw std::runtime_error("debug_attn_cross_quant: null output for this mode");
    } catch (const std::exception& e) {
        set_err(err, errlen, e.what());
        return SPT_ERR_INVALID_ARG;
    }
    // the rows as the 16-bit cache would hold them, and the host quantiser's view of them
    const size_t n_rows = (size_t)B_layout * H * T_enc;
    std::vector<uint16_t> k16 = to_half_storage(dtype, k, n_rows * 64), v16 = to_half_storage(dtype, v, n_rows * 64);
    for (int kvi = 0; kvi < 2; ++kvi) {
        const std::vector<uint16_t>& s16 = kvi ? v16 : k16;
        float* dq = kvi ? vq : kq;
        float* sc = kvi ? v_scale : k_scale;
        for (size_t r = 0; r < n_rows; ++r) {
            float x[64];
            uint8_t code[64];
            for (int e = 0; e < 64; ++e) x[e] = dtype == spt::DT_BF16 ? spt::bf2f(s16[r * 64 + e]) : h2f_bits(s16[r * 64 + e]);
            spt::f8::quant_row_host(x, 64, code, &sc[r]);
            for (int e = 0; e < 64; ++e) dq[r * 64 + e] = spt::f8::decode_soft(code[e]) * sc[r];
        }
    }
    if (spt_status s = device_ok(device, err, errlen)) return s;
    try {
        // the layer as the K/V GEMM's epilogue writes it (kv_offset; the quantiser reads no row past T_enc)
        const size_t n_kv = (size_t)spt::kv_layer_elems(B_layout, H, T_enc);
        std::vector<uint16_t> lay(n_kv, 0);
        for (int kvi = 0; kvi < 2; ++kvi) {
            const std::vector<uint16_t>& s16 = kvi ? v16 : k16;
            for (int b = 0; b < B_layout; ++b)
                for (int h = 0; h < H; ++h)
                    for (int t = 0; t < T_enc; ++t)
                        memcpy(lay.data() + spt::kv_offset(0, kvi, b, h, t, 0, B_layout, H, T_enc),
                               s16.data() + (((size_t)b * H + h) * T_enc + t) * 64, 64 * sizeof(uint16_t));
        }
        const size_t R = (size_t)B * Tq, nq_el = R * H * 64, esz = 2;
        const size_t n_part = R * H * 8 * 66;
        std::vector<uint16_t> q16;
        // what overwrites the padding rows of the last block's records after the quantiser: the code of 1.0 in
        // every element and pad_value as the scale, so they dequantise to pad_value (outlives the stream)
        const int r0 = T_enc & 31, n_pad = r0 ? 32 - r0 : 0;
        const size_t BH = (size_t)B_layout * H;
        const std::vector<uint8_t> pad_codes(BH * (size_t)n_pad * 64, 0x38);
        const std::vector<float> pad_scales(BH, pad_value);
        Scope sc(device);
        const void* d_q = up_as(sc, dtype, q, nq_el, q16);
        const uint16_t* d_lay = sc.up(lay.data(), n_kv);
        char* d_rec = sc.out<char>((size_t)spt::f8::layer_bytes(B_layout, H, T_enc));
        spt::kv_quant_f8(dtype, d_lay, d_rec, 1, B_layout, H, T_enc, sc.st);
        if (n_pad) {  // the last block's records are contiguous: one strided copy per part of a record
            char* last = d_rec + (size_t)(T_enc >> 5) * BH * spt::f8::kRecBytes;
            for (int kvi = 0; kvi < 2; ++kvi) {
                HIP_CHECK(hipMemcpy2DAsync(last + kvi * spt::f8::kRecV + r0 * 64, spt::f8::kRecBytes, pad_codes.data(),
                                           (size_t)n_pad * 64, (size_t)n_pad * 64, BH, hipMemcpyHostToDevice, sc.st));
                for (int r = r0; r < 32; ++r)
                    HIP_CHECK(hipMemcpy2DAsync(last + spt::f8::scale_offset(kvi, r), spt::f8::kRecBytes, pad_scales.data(),
                                               sizeof(float), sizeof(float), BH, hipMemcpyHostToDevice, sc.st));
            }
        }
        const char* d_kv = d_rec + (size_t)b0 * H * spt::f8::kRecBytes;
        const int* d_map = kvrow ? sc.up(kvrow, (size_t)B) : nullptr;
        float* d_part = vw ? sc.out<float>(n_part) : nullptr;
        void* d_out = !vw || merge ? sc.out<char>(nq_el * esz) : nullptr;
        if (vw) {
            spt::dec_cross_attn_vw_f8(dtype, d_q, d_kv, B, B_layout, H, T_enc, Tq, d_part, sc.st, d_map, share, per_query);
            if (merge) spt::dec_attn_part_merge(dtype, d_part, (int)R, H, d_out, sc.st);
        } else {
            spt::dec_cross_attn_f8(dtype, d_q, d_kv, B, B_layout, H, T_enc, Tq, d_out, sc.st, d_map, share);
        }
        float* d_kq = sc.out<float>(n_rows * 64);
        float* d_vq = sc.out<float>(n_rows * 64);
        float* d_ks = sc.out<float>(n_rows);
        float* d_vs = sc.out<float>(n_rows);
        spt::kv_dequant_f8(d_rec, B_layout, H, T_enc, 0, B_layout, d_kq, d_vq, d_ks, d_vs, sc.st);
        sc.down(kq, (const float*)d_kq, n_rows * 64);
        sc.down(vq, (const float*)d_vq, n_rows * 64);
        sc.down(k_scale, (const float*)d_ks, n_rows);
        sc.down(v_scale, (const float*)d_vs, n_rows);
        if (d_out) down_f32(sc, dtype, d_out, out, nq_el);
        else sc.down(part, (const float*)d_part, n_part);
        sc.sync();
        return SPT_OK;
    } catch (const std::exception& e) {
        set_err(err, errlen, e.what());
        return spt_classify(e);
    }
}

}  // extern "C"
