// kv_f8.h -- the fp8 cross K/V cache of SPT_MODEL_CROSS_KV_F8: the record layout, the
// e4m3 code and the row quantiser, one spelling for the host (spt_debug_attn_cross_quant's reference
// arrays, tests) and the device (k_dec_f8.hip).
//
// A key row is the 64 elements of one (layer, window, head, K-or-V, key t), as the 16-bit cache would
// hold them (to_cache<T>, widened to f32).  Per row:
//   amax = max |x|;  amax == 0: scale = 1, every code 0;  otherwise
//   scale = amax / 448,  inv = 448 / amax  (each one correctly rounded f32 division),
//   y = x * inv (one rounding),  code = e4m3fn(y): OCP encoding, round to nearest even, subnormals kept.
// |y| <= 448 (1 + 2^-22) rounds to 448, so the conversion never reaches its overflow case and nothing
// rests on a saturation mode.  Below amax = 2^-64 (bf16 rows near its subnormals; 448 / amax would leave
// f32's range below 1.3e-36) x and amax are first multiplied by 2^64, which is exact, so y is the
// same product with the same single rounding.  The dequantised value is f32(code) * scale.
// Non-finite inputs are outside the contract: a row holding an infinity has inv = 0 and scale = inf
// (codes 0 or NaN, dequantised NaN); a row holding a NaN and no infinity keeps the amax of its other
// elements (fmaxf drops the NaN) and encodes the NaN element as the code 0x7F, NaN again.
//
// Layer layout: records [ceil(T / 32)][B][H], each one 32-key block of one (window, head), contiguous
// and 16-byte aligned, kv_offset's block order:
//   K codes [32][64] | V codes [32][64] | scales [16][4] f32 = {k[s], k[s + 16], v[s], v[s + 16]}
// 4352 bytes against the 8192 of a 16-bit block (0.531).  The scales sit so that the lanes of key slot s
// of the attention wave (keys s and s + 16 of the block) fetch theirs in one 16-byte load.  The rows
// that pad the last block (t >= T) hold code 0 and scale 1; the kernels never use a padded key's scale.
#pragma once
#include <stdint.h>
#include <math.h>
#include <string.h>

#if defined(__HIPCC__)
#define SPT_HD __host__ __device__
#else
#define SPT_HD
#endif

namespace spt {
namespace f8 {

constexpr int kBlockKeys = 32;
constexpr int kRecBytes = 4352;     // one record
constexpr int kRecV = 2048;         // byte offset of the V codes
constexpr int kRecScale = 4096;     // byte offset of the scales
constexpr float kMax = 448.0f;      // largest finite e4m3fn
constexpr float kTinyAmax = 5.421010862427522e-20f;  // 2^-64
constexpr float kTinyUp = 18446744073709551616.0f;   // 2^64

SPT_HD inline int64_t layer_bytes(int B, int H, int T) { return (int64_t)((T + 31) / 32) * B * H * kRecBytes; }
SPT_HD inline int64_t rec_offset(int b, int h, int t, int B, int H) {
    return (((int64_t)(t >> 5) * B + b) * H + h) * kRecBytes;
}
// byte offset inside a record of key row r's (0..31) scale; kvi 0: K, 1: V
SPT_HD inline int scale_offset(int kvi, int r) { return kRecScale + ((r & 15) * 4 + 2 * kvi + (r >> 4)) * 4; }

// f32 -> e4m3fn code, round to nearest even, subnormals kept; above 464 (never reached by the row
// quantiser) and NaN give 0x7F.  The integer form of v_cvt_pk_fp8_f32 for |y| < 464.
SPT_HD inline uint8_t encode_soft(float y) {
    uint32_t u;
    memcpy(&u, &y, 4);
    const uint8_t sign = (uint8_t)((u >> 24) & 0x80u);
    u &= 0x7FFFFFFFu;
    if (u > 0x7F800000u) return (uint8_t)(sign | 0x7Fu);
    float a;
    memcpy(&a, &u, 4);
    if (a < 0.015625f) return (uint8_t)(sign | (uint8_t)(int)rintf(a * 512.0f));  // units of 2^-9; 8 is the least normal
    u += 0x7FFFFu + ((u >> 20) & 1u);  // RNE on the 20 dropped mantissa bits
    u >>= 20;                          // exponent << 3 | mantissa
    if (u > (135u << 3 | 6u)) return (uint8_t)(sign | 0x7Fu);
    return (uint8_t)(sign | (uint8_t)(u - (120u << 3)));
}
SPT_HD inline float decode_soft(uint8_t c) {
    const int e = (c >> 3) & 15, m = c & 7;
    float a;
    if (e == 15 && m == 7) a = NAN;
    else if (e == 0) a = (float)m * 0.001953125f;
    else {
        const uint32_t u = ((uint32_t)(e + 120) << 23) | ((uint32_t)m << 20);
        memcpy(&a, &u, 4);
    }
    return (c & 0x80) ? -a : a;
}

// the row's two factors from its amax: y = (x * up) * inv, dequantised = f32(code) * scale
struct RowScale {
    float up, inv, scale;
};
SPT_HD inline RowScale row_scale(float amax) {
    if (amax == 0.f) return {1.f, 0.f, 1.f};
    const float up = amax < kTinyAmax ? kTinyUp : 1.0f;
    return {up, kMax / (amax * up), amax / kMax};
}

// the quantiser on the host: one row of n <= 64 elements
inline void quant_row_host(const float* x, int n, uint8_t* code, float* scale) {
    float amax = 0.f;
    for (int e = 0; e < n; ++e) amax = fmaxf(amax, fabsf(x[e]));
    const RowScale rs = row_scale(amax);
    for (int e = 0; e < n; ++e) code[e] = amax == 0.f ? (uint8_t)0 : encode_soft((x[e] * rs.up) * rs.inv);
    *scale = rs.scale;
}

}  // namespace f8
}  // namespace spt
