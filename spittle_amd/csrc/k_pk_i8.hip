// k_pk_i8.hip -- the Parakeet encoder's int8 mode (DT_I8): ONNX DynamicQuantizeLinear followed by
// MatMulInteger / 1 x 1 ConvInteger, as ONNX Runtime's quantize_dynamic export runs every encoder
// Linear and pointwise convolution (DESIGN.md §9.7 is the arithmetic contract).
//
//   pk_i8_minmax    per-utterance min / max of a GEMM input's valid rows, as order-preserving keys
//                   (atomic min / max of integers: order-independent, so deterministic)
//   pk_i8_quantize  s_a = (hi - lo) / 255, z_a, q = clamp(rint(x / s_a) + z_a, 0, 255); stores
//                   q - 128 (the MFMA operands are signed) and each row's sum of q - 128
//   pk_i8_gemm      acc = sum_k (q - z_a)(w - z_w) with v_mfma_i32_16x16x64_i8, restored from the
//                   shifted operands' product by the row / column sums, then
//                   y = float(acc) * (s_a * s_w[n]) (+ bias, activation, alpha)
//
// Everything stays in int32 until the accumulator is complete; the float steps are single rounded
// f32 operations in a fixed order (no contraction), so y is reproducible to the bit.
#include <algorithm>

#include "common.h"
#include "kernels.h"
#include "pk_kernels.h"

namespace spt {

namespace {

typedef int __attribute__((ext_vector_type(4))) i32x4;

// order-preserving float <-> unsigned keys
__device__ inline unsigned f2key(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ inline float key2f(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

// group g's valid rows of the GEMM input: first row (of A, and of the group's own row block) and count
__device__ inline void group_rows(const PkI8Groups& G, int g, int* a_row0, int* n) {
    const int len = G.lens ? G.lens[g * G.lens_stride + G.lens_off] : G.rows;
    if (G.mode == PK_I8_POS) {  // relative positions |r| < len of a table of 2 Tp - 1 rows (Tp = (rows + 1) / 2)
        *a_row0 = (G.rows + 1) / 2 - len;
        *n = len > 0 ? 2 * len - 1 : 0;
    } else {
        *a_row0 = g * G.rows;
        *n = min(len * G.rpf, G.rows);
    }
}

__global__ __launch_bounds__(256) void i8_minmax_kernel(const float* __restrict__ A, int K, PkI8Groups G,
                                                        unsigned* __restrict__ keys) {
    const int g = blockIdx.y;
    int r0, n;
    group_rows(G, g, &r0, &n);
    const float4* p = (const float4*)(A + (size_t)r0 * K);
    const int64_t n4 = (int64_t)n * K / 4;
    float lo = 0.0f, hi = 0.0f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const float4 v = p[i];
        lo = fminf(fminf(lo, v.x), fminf(v.y, fminf(v.z, v.w)));
        hi = fmaxf(fmaxf(hi, v.x), fmaxf(v.y, fmaxf(v.z, v.w)));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, o, 64));
        hi = fmaxf(hi, __shfl_xor(hi, o, 64));
    }
    if ((threadIdx.x & 63) == 0 && n4 > 0) {
        atomicMin(&keys[2 * g], f2key(lo));
        atomicMax(&keys[2 * g + 1], f2key(hi));
    }
}

// The float steps below are the contract's single f32 operations in its order: contraction is off
// (the __f*_rn spellings alone do not stop the compiler from fusing a multiply into an add).

// DynamicQuantizeLinear's scale and zero point from the range keys
__device__ inline void quant_params(const unsigned* keys, int g, float* s, int* z) {
#pragma clang fp contract(off)
    const float lo = fminf(key2f(keys[2 * g]), 0.0f), hi = fmaxf(key2f(keys[2 * g + 1]), 0.0f);
    const float sa = __fdiv_rn(__fsub_rn(hi, lo), 255.0f);
    *s = sa;
    *z = sa > 0.0f ? (int)fminf(fmaxf(rintf(__fdiv_rn(__fsub_rn(0.0f, lo), sa)), 0.0f), 255.0f) : 0;
}

// q - 128 of one element
__device__ inline int quant_one(float x, float s, float zf) {
#pragma clang fp contract(off)
    int q = 0;
    if (s > 0.0f) q = (int)fminf(fmaxf(__fadd_rn(rintf(__fdiv_rn(x, s)), zf), 0.0f), 255.0f);
    return q - 128;
}

// y = act(float(acc) * (s_a * s_w) + bias) * alpha
__device__ inline float i8_tail(int t, float sa, float sw, bool has_bias, float bias, int act, float alpha) {
#pragma clang fp contract(off)
    float y = (float)t * (sa * sw);
    if (has_bias) y = y + bias;
    if (act == PK_I8_RELU) y = fmaxf(y, 0.0f);
    else if (act == PK_I8_SWISH) y = y / (1.0f + expf(-y));
    if (alpha != 1.0f) y = y * alpha;
    return y;
}

// one wave per row: 4 floats per lane and step -> 4 bytes of q - 128
__global__ __launch_bounds__(256) void i8_quantize_kernel(const float* __restrict__ A, int K, PkI8Groups G,
                                                          const unsigned* __restrict__ keys, int M,
                                                          int8_t* __restrict__ Q, int* __restrict__ rowsum,
                                                          float* __restrict__ sa_out, int* __restrict__ za_out) {
    const int m = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (m >= M) return;
    const int g = m / G.rows, r = m - g * G.rows;
    float s;
    int z;
    quant_params(keys, g, &s, &z);
    if (r == 0 && lane == 0) {
        sa_out[g] = s;
        za_out[g] = z;
    }
    const float* a = A + (size_t)(G.mode == PK_I8_POS ? r : m) * K;
    const float zf = (float)z;
    int sum = 0;
    for (int k = lane * 4; k < K; k += 256) {
        const float4 v = *(const float4*)(a + k);
        const float x[4] = {v.x, v.y, v.z, v.w};
        unsigned pk = 0;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int q = quant_one(x[u], s, zf);
            sum += q;
            pk |= (unsigned)(q & 0xFF) << (8 * u);
        }
        *(unsigned*)(Q + (size_t)m * K + k) = pk;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if (lane == 0) rowsum[m] = sum;
}

// C tile of (2 * WM * 16) x (2 * WN * 16) per workgroup of 2 x 2 waves, each wave WM x WN MFMA
// tiles.  Operands come straight from global memory (16 bytes per lane and tile: lane l holds
// A[row l & 15][k = 16 (l >> 4) ..] and W[col l & 15][the same k]: both operands use one k map, so
// the product does not depend on the order of k inside the instruction), the next K step's loads
// issued before this step's MFMAs.  Rows and columns past M / N re-read the last one and are not
// stored.
template <int WM, int WN>
__global__ __launch_bounds__(256) void i8_gemm_kernel(PkI8Gemm a) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int m0 = (blockIdx.y * 2 + (wave >> 1)) * (WM * 16), n0 = (blockIdx.x * 2 + (wave & 1)) * (WN * 16);
    if (m0 >= a.M || n0 >= a.N) return;
    const int fr = lane & 15, fq = lane >> 4;
    const int8_t* ap[WM];
    const int8_t* wp[WN];
#pragma unroll
    for (int i = 0; i < WM; ++i) ap[i] = a.Q + (size_t)min(m0 + i * 16 + fr, a.M - 1) * a.K + fq * 16;
#pragma unroll
    for (int j = 0; j < WN; ++j) wp[j] = a.W + (size_t)min(n0 + j * 16 + fr, a.N - 1) * a.K + fq * 16;
    i32x4 acc[WM][WN];
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int j = 0; j < WN; ++j) acc[i][j] = i32x4{0, 0, 0, 0};
    i32x4 af[WM], wf[WN];
#pragma unroll
    for (int i = 0; i < WM; ++i) af[i] = *(const i32x4*)ap[i];
#pragma unroll
    for (int j = 0; j < WN; ++j) wf[j] = *(const i32x4*)wp[j];
    for (int k0 = 0; k0 < a.K; k0 += 64) {
        i32x4 an[WM], wn[WN];
        const int kn = k0 + 64 < a.K ? k0 + 64 : k0;  // the last step re-reads its own operands
#pragma unroll
        for (int i = 0; i < WM; ++i) an[i] = *(const i32x4*)(ap[i] + kn);
#pragma unroll
        for (int j = 0; j < WN; ++j) wn[j] = *(const i32x4*)(wp[j] + kn);
#pragma unroll
        for (int i = 0; i < WM; ++i)
#pragma unroll
            for (int j = 0; j < WN; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(af[i], wf[j], acc[i][j], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < WM; ++i) af[i] = an[i];
#pragma unroll
        for (int j = 0; j < WN; ++j) wf[j] = wn[j];
    }
    // C / D layout: col = lane & 15, row = 4 (lane >> 4) + reg
#pragma unroll
    for (int j = 0; j < WN; ++j) {
        const int n = n0 + j * 16 + fr;
        if (n >= a.N) continue;
        const int zw = a.zw[n], cs = a.cs[n];
        const float sw = a.sw[n];
        const float bias = a.bias ? a.bias[n] : 0.0f;
#pragma unroll
        for (int i = 0; i < WM; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + i * 16 + fq * 4 + r;
                if (m >= a.M) continue;
                const int g = m / a.rows;
                const int za = a.za[g] - 128;
                // sum (qs - za)(ws - zw) = sum qs ws - zw sum qs - za sum ws + K za zw
                const int t = acc[i][j][r] - zw * a.rowsum[m] - za * cs + a.K * za * zw;
                const float y = i8_tail(t, a.sa[g], sw, a.bias != nullptr, bias, a.act, a.alpha);
                a.C[(size_t)m * a.ldc + n] = y;
                if (a.acc_out) a.acc_out[(size_t)m * a.N + n] = t;
            }
    }
}

}  // namespace

void pk_i8_minmax(const float* A, int K, const PkI8Groups& G, int n_groups, unsigned* keys, hipStream_t st) {
    if (K % 64) throw std::runtime_error("pk_i8_minmax: K must be a multiple of 64");
    const int64_t span = (int64_t)G.rows * K;
    const int nb = (int)std::min<int64_t>(128, std::max<int64_t>(1, span / 16384));
    hipLaunchKernelGGL(i8_minmax_kernel, dim3(nb, n_groups), dim3(256), 0, st, A, K, G, keys);
    SPT_LAUNCH_CHECK();
}

void pk_i8_quantize(const float* A, int K, const PkI8Groups& G, int n_groups, const unsigned* keys, int8_t* Q,
                    int* rowsum, float* sa, int* za, hipStream_t st) {
    if (K % 64) throw std::runtime_error("pk_i8_quantize: K must be a multiple of 64");
    const int M = n_groups * G.rows;
    hipLaunchKernelGGL(i8_quantize_kernel, dim3(cdiv(M, 4)), dim3(256), 0, st, A, K, G, keys, M, Q, rowsum, sa, za);
    SPT_LAUNCH_CHECK();
}

void pk_i8_gemm(const PkI8Gemm& a, hipStream_t st) {
    if (a.K % 64 || a.K > 4096) throw std::runtime_error("pk_i8_gemm: K must be a multiple of 64, <= 4096");
    if (a.N % 16) throw std::runtime_error("pk_i8_gemm: N must be a multiple of 16");
    if (a.M < 1 || a.rows < 1) throw std::runtime_error("pk_i8_gemm: empty product");
    // 64 x 64 workgroup tiles until they fill the chip several times over, then 128 x 128
    if ((int64_t)cdiv(a.M, 128) * cdiv(a.N, 128) >= 1024)
        hipLaunchKernelGGL((i8_gemm_kernel<4, 4>), dim3(cdiv(a.N, 128), cdiv(a.M, 128)), dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL((i8_gemm_kernel<2, 2>), dim3(cdiv(a.N, 64), cdiv(a.M, 64)), dim3(256), 0, st, a);
    SPT_LAUNCH_CHECK();
}

}  // namespace spt
