// common.h -- shared device/host helpers for the spittle_amd HIP backend (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdexcept>
#include <string>

namespace spt {

typedef uint16_t bf16;  // raw bf16 storage
typedef _Float16 f16;   // IEEE half (Parakeet's fp16 encoder)
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(8))) short bf16x8;
typedef __attribute__((ext_vector_type(4))) short bf16x4v;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2v;
typedef __attribute__((ext_vector_type(2))) _Float16 f16x2v;

#define SPT_LDS __attribute__((address_space(3)))

struct HipError : std::runtime_error {
    using std::runtime_error::runtime_error;
};

#define HIP_CHECK(expr)                                                                    \
    do {                                                                                   \
        hipError_t _e = (expr);                                                            \
        if (_e != hipSuccess)                                                              \
            throw ::spt::HipError(std::string(#expr) + " failed: " + hipGetErrorString(_e) + \
                                  " (" __FILE__ ":" + std::to_string(__LINE__) + ")");      \
    } while (0)

// surface launch-configuration errors at the launch site (works under stream capture)
#define SPT_LAUNCH_CHECK() HIP_CHECK(hipGetLastError())

__host__ __device__ inline float bf2f(bf16 v) {
    union { uint32_t u; float f; } x;
    x.u = (uint32_t)v << 16;
    return x.f;
}
// round-to-nearest-even; on the device one v_cvt_pk_bf16_f32 (same RNE for finite inputs,
// keeps NaNs NaN), on the host the integer form
__host__ __device__ inline bf16 f2bf(float f) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_bit_cast(bf16, (__bf16)f);
#endif
    union { uint32_t u; float f; } x;
    x.f = f;
    uint32_t u = x.u;
    u += 0x7FFFu + ((u >> 16) & 1u);
    return (bf16)(u >> 16);
}
// packed pair -> one dword
__device__ inline uint32_t pack_bf2(float a, float b) {
    return (uint32_t)f2bf(a) | ((uint32_t)f2bf(b) << 16);
}

// f32 -> IEEE half bits on the host (weight staging, debug inputs): round-to-nearest-even,
// subnormals kept, overflow to infinity, NaN stays NaN -- the device's (f16) conversion
inline uint16_t f2h_bits(float f) {
    union { uint32_t u; float f; } x;
    x.f = f;
    const uint32_t sign = (x.u >> 16) & 0x8000u, a = x.u & 0x7FFFFFFFu;
    if (a >= 0x7F800000u) return (uint16_t)(sign | 0x7C00u | (a > 0x7F800000u ? 0x200u | ((a >> 13) & 0x3FFu) : 0u));
    if (a >= 0x477FF000u) return (uint16_t)(sign | 0x7C00u);  // >= 65520 rounds to infinity
    if (a < 0x38800000u) {                                    // below 2^-14: subnormal half (or zero)
        if (a < 0x33000000u) return (uint16_t)sign;           // below 2^-25 rounds to zero
        const uint32_t shift = 126u - (a >> 23);              // 14..24: mantissa (with hidden bit) >> shift
        const uint32_t m = (a & 0x7FFFFFu) | 0x800000u;
        const uint32_t q = m >> shift, rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1);
        return (uint16_t)(sign | (q + ((rem > half || (rem == half && (q & 1u))) ? 1u : 0u)));
    }
    const uint32_t r = a + 0xFFFu + ((a >> 13) & 1u);         // RNE on the 13 dropped bits
    return (uint16_t)(sign | ((r - 0x38000000u) >> 13));
}

template <typename T> struct TypeTag;
template <> struct TypeTag<float> { static constexpr int id = 0; };
template <> struct TypeTag<bf16> { static constexpr int id = 1; };
template <> struct TypeTag<f16> { static constexpr int id = 2; };

template <typename T> __device__ inline float to_f(T v);
template <> __device__ inline float to_f<float>(float v) { return v; }
template <> __device__ inline float to_f<bf16>(bf16 v) { return bf2f(v); }
template <> __device__ inline float to_f<f16>(f16 v) { return (float)v; }
template <typename T> __device__ inline T from_f(float v);
template <> __device__ inline float from_f<float>(float v) { return v; }
template <> __device__ inline bf16 from_f<bf16>(float v) { return f2bf(v); }
template <> __device__ inline f16 from_f<f16>(float v) { return (f16)v; }  // RNE

// The store into a decoder K/V cache (self: the GV_QKV_CACHE GEMV; cross: the EPI_KVSPLIT GEMM
// epilogue).  f16 clamps to the largest finite f16 first: the decode attention needs finite cache
// rows (engine.cpp, beam_begin), and an f16 activation overflows at 65504 where bf16 needs ~3e38.
// bf16 and f32 are from_f, the same stores as before the f16 mode existed.  (fmaxf returns its
// non-NaN operand, so a NaN is stored as -65504: finite too.)
template <typename T> __device__ inline T to_cache(float v) {
    if constexpr (TypeTag<T>::id == TypeTag<f16>::id)
        return (f16)__builtin_fminf(__builtin_fmaxf(v, -65504.0f), 65504.0f);
    else
        return from_f<T>(v);
}

// GELU, tanh form (ggml / whisper.cpp): 0.5 x (1 + tanh(u)), u = sqrt(2/pi) (x + 0.044715 x^3),
// evaluated as x * sigmoid(2u) = x / (1 + 2^(-2u log2 e)): one v_exp_f32 + one v_rcp_f32
// instead of tanhf (the same function; differs from libm tanhf by a few f32 ulp)
// (contraction off: every kernel that inlines it -- the decoder's fc1 GEMV, the encoder's GEMM
// epilogues -- computes the same bits, whatever the surrounding code)
__device__ inline float gelu_tanh(float x) {
#pragma clang fp contract(off)
    const float c2 = -2.0f * 0.7978845608028654f * 1.4426950408889634f;
    const float e = __builtin_amdgcn_exp2f(c2 * (x + 0.044715f * x * x * x));
    return x * __builtin_amdgcn_rcpf(1.0f + e);
}

// the decoder rows' LayerNorm arithmetic (gemv_kernel's A_LN prologue), spelled out with
// contraction off so every instance computes the same bits: the squared deviations of four elements,
// and one normalised element
__device__ inline float ln_sq4(float4 v, float mean) {
#pragma clang fp contract(off)
    const float p = v.x - mean, q = v.y - mean, u = v.z - mean, w = v.w - mean;
    return (p * p + q * q) + (u * u + w * w);
}
__device__ inline float ln_out(float v, float mean, float rstd, float g, float b) {
#pragma clang fp contract(off)
    return (v - mean) * rstd * g + b;
}

// Swish / SiLU x * sigmoid(x) (NeMo's Swish activation): one v_exp_f32 + one v_rcp_f32
__device__ inline float swish(float x) {
    return x * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * x));
}
__device__ inline float sigmoidf_(float x) {
    return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * x));
}

__device__ inline float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ inline float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

__host__ __device__ inline int cdiv(int a, int b) { return (a + b - 1) / b; }

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) for the calling thread's current device, once
// per (kernel, device): the attribute is per device, and replica threads drive several devices
// from one process (r2 advisor finding).  Thread-safe.  Call outside stream capture.
void ensure_lds_attr(const void* kernel, int bytes);

}  // namespace spt
