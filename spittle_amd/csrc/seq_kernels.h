// seq_kernels.h -- the kernels Moonshine and SenseVoice both run (gfx950): the MFMA flash attention
// over a head tile of 64 or 128, the one-wave-per-row LayerNorm, the top-1 / top-2 row reduction and
// block_sum.  Device text only, in an unnamed namespace: k_ms.hip and k_sv.hip each include it and
// instantiate their own copies (as k_dec.hip and k_dec_q.hip do with dec_gemv.h), because the two
// files compile their f32 arithmetic differently -- k_sv.hip has contraction off for the whole file
// and includes this header below that pragma, k_ms.hip only in named functions -- and each model
// keeps the bits it had.
#pragma once
#include "common.h"

namespace spt {

// q / k / v / out are f16; batch item b's rows start at base + b * bstride, head h at column h * dh
struct SeqAttnArgs {
    const void* q; int ldq; int64_t q_bstride;
    const void* k; const void* v; int ldk; int64_t k_bstride;
    void* out; int ldo; int64_t o_bstride;
    const int* lens;   // [B][4]; column 3 is the number of valid queries = keys of batch item b
    int B, H, dh, Tq;  // Tq: padded query rows per batch item (grid)
};

namespace {

__device__ inline float block_sum(float v, float* red) {  // blockDim.x a multiple of 64, <= 1024
    v = wave_sum(v);
    const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[w] = v;
    __syncthreads();
    float s = 0.0f;
    for (int i = 0; i < nw; i++) s += red[i];  // the same order in every thread
    return s;
}

// LayerNorm of x [M][ldx] over its first d columns, one wave per row; bs may be null (no bias: + 0.0f).
// Columns d .. ldy - 1 of y are zeroed.  A lane writes only the columns it read (y may be x).
template <typename OutT>
__global__ void layernorm_kernel(const float* x, int M, int d, int ldx, const float* w, const float* bs, float eps, OutT* y,
                                 int ldy) {
    const int m = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (m >= M) return;
    const float* xr = x + (int64_t)m * ldx;
    float s = 0.0f;
    for (int c = lane; c < d; c += 64) s += xr[c];
    const float mean = wave_sum(s) / (float)d;
    float q = 0.0f;
    for (int c = lane; c < d; c += 64) {
        const float v = xr[c] - mean;
        q += v * v;
    }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)d + eps);
    OutT* yr = y + (int64_t)m * ldy;
    for (int c = lane; c < ldy; c += 64)
        yr[c] = c < d ? (OutT)ln_out(xr[c], mean, rstd, w[c], bs ? bs[c] : 0.0f) : (OutT)0.0f;
}

// y is f32 [M][ldy] when out_f32, else f16
inline void layernorm_launch(const float* x, int M, int d, int ldx, const float* w, const float* bs, float eps, void* y,
                             int ldy, bool out_f32, hipStream_t st) {
    if (out_f32) layernorm_kernel<float><<<cdiv(M, 4), 256, 0, st>>>(x, M, d, ldx, w, bs, eps, (float*)y, ldy);
    else layernorm_kernel<f16><<<cdiv(M, 4), 256, 0, st>>>(x, M, d, ldx, w, bs, eps, (f16*)y, ldy);
    SPT_LAUNCH_CHECK();
}

// The largest and second largest of lg[0 .. V) and the lowest index of the largest, by a workgroup of
// 256 threads: a strided scan, then a merge through LDS.  Every thread returns the row's result; a row
// of NaNs gives token 0.
struct RowTop2 {
    int tok;
    float v1, v2;
};
__device__ inline RowTop2 row_top2(const float* lg, int V) {
    __shared__ float v1s[256], v2s[256];
    __shared__ int i1s[256];
    const int tid = threadIdx.x;
    float v1 = -INFINITY, v2 = -INFINITY;
    int i1 = 0x7FFFFFFF;
    for (int i = tid; i < V; i += 256) {  // ascending: a tie keeps the lower index
        const float v = lg[i];
        if (v > v1) { v2 = v1; v1 = v; i1 = i; }
        else if (v > v2) v2 = v;
    }
    v1s[tid] = v1; v2s[tid] = v2; i1s[tid] = i1;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
            const float b1 = v1s[tid + o], b2 = v2s[tid + o];
            const int bi = i1s[tid + o];
            if (b1 > v1s[tid] || (b1 == v1s[tid] && bi < i1s[tid])) {
                v2s[tid] = fmaxf(v1s[tid], b2);
                v1s[tid] = b1;
                i1s[tid] = bi;
            } else
                v2s[tid] = fmaxf(v2s[tid], b1);
        }
        __syncthreads();
    }
    int tok = i1s[0];
    if (tok < 0 || tok >= V) tok = 0;  // a row of NaNs
    return RowTop2{tok, v1s[0], v2s[0]};
}

// ---------------------------------------------------------------- flash attention (MFMA)
// Workgroup = 4 waves = 64 queries of one (b, h); 64-key tiles of K (row-major) and V (transposed)
// staged in LDS with the head dim zero-padded to the head tile DT (64: any dh <= 64 with dh % 4 == 0;
// 128: dh == 128) and keys >= nk stored as zero; a masked key's probability is set to 0 (not
// multiplied to 0), so nothing a masked key holds reaches the output.  Query rows >= nk write zeros.
// CLAMP: nk = min(lens[b][3], Tq).
// v_mfma_f32_16x16x32_f16: A[row l&15][k = 8 (l>>4) + j], B[k = 8 (l>>4) + j][col l&15],
// C[row 4 (l>>4) + reg][col l&15].
constexpr int ATT_VLD = 72;  // V^T / P row pitch (f16): 64 + 8, rows stay 16-byte aligned

template <int DT, bool CLAMP>
__global__ void __launch_bounds__(256) flash_attn_kernel(SeqAttnArgs a, float scale) {
    static_assert(DT == 64 || DT == 128, "head tile");
    constexpr int KLD = DT + 8;  // K tile row pitch (f16)
    constexpr int KS = DT / 32;  // k-steps of q . k
    constexpr int ND = DT / 16;  // O fragments
    __shared__ __attribute__((aligned(16))) f16 Ks[64 * KLD];
    __shared__ __attribute__((aligned(16))) f16 Vt[DT * ATT_VLD];
    __shared__ __attribute__((aligned(16))) f16 Ps[4 * 16 * ATT_VLD];
    const int b = blockIdx.z, h = blockIdx.y, q0 = blockIdx.x * 64;
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, lr = l & 15, lg = l >> 4;
    const int nk = CLAMP ? min(a.lens[b * 4 + 3], a.Tq) : a.lens[b * 4 + 3];
    const int dh = DT == 128 ? 128 : a.dh;
    const f16* qb = (const f16*)a.q + b * a.q_bstride + h * dh;
    const f16* kb = (const f16*)a.k + b * a.k_bstride + h * dh;
    const f16* vb = (const f16*)a.v + b * a.k_bstride + h * dh;
    f16* ob = (f16*)a.out + b * a.o_bstride + h * dh;
    if (q0 >= nk) {  // a padded query block: zero rows
        for (int o = tid; o < 64 * dh; o += 256) {
            const int q = q0 + o / dh;
            if (q < a.Tq) ob[(int64_t)q * a.ldo + o % dh] = (f16)0.0f;
        }
        return;
    }
    f16x8 qa[KS];
    {
        const int q = q0 + w * 16 + lr;
        for (int ks = 0; ks < KS; ks++) {
            if constexpr (DT == 128) {
                for (int j = 0; j < 8; j++) qa[ks][j] = (f16)0.0f;
                if (q < nk) qa[ks] = *(const f16x8*)&qb[(int64_t)q * a.ldq + ks * 32 + lg * 8];
            } else {  // a head at h * dh is only 8-byte aligned
                for (int j = 0; j < 8; j++) {
                    const int e = ks * 32 + lg * 8 + j;
                    qa[ks][j] = (q < nk && e < dh) ? qb[(int64_t)q * a.ldq + e] : (f16)0.0f;
                }
            }
        }
    }
    f32x4 O[ND];
    float m_run[4], l_run[4];
    for (int i = 0; i < ND; i++) O[i] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    for (int i = 0; i < 4; i++) {
        m_run[i] = -INFINITY;
        l_run[i] = 0.0f;
    }
    f16* Pw = Ps + w * 16 * ATT_VLD;
    for (int k0 = 0; k0 < nk; k0 += 64) {
        __syncthreads();  // the previous tile's reads are done
        {
            const int key = tid >> 2;
            const bool kvalid = k0 + key < nk;
            if constexpr (DT == 128) {
                const int part = (tid & 3) * 32;
                for (int c = 0; c < 4; c++) {
                    const int e = part + c * 8;
                    f16x8 kv, vv;
                    for (int j = 0; j < 8; j++) kv[j] = vv[j] = (f16)0.0f;
                    if (kvalid) {
                        const int64_t at = (int64_t)(k0 + key) * a.ldk + e;
                        kv = *(const f16x8*)&kb[at];
                        vv = *(const f16x8*)&vb[at];
                    }
                    *(f16x8*)&Ks[key * KLD + e] = kv;
                    for (int j = 0; j < 8; j++) Vt[(e + j) * ATT_VLD + key] = vv[j];
                }
            } else {
                const int e0 = (tid & 3) * 16;
                for (int c = 0; c < 16; c += 4) {
                    const int e = e0 + c;
                    f16 kv[4] = {(f16)0.0f, (f16)0.0f, (f16)0.0f, (f16)0.0f}, vv[4] = {(f16)0.0f, (f16)0.0f, (f16)0.0f, (f16)0.0f};
                    if (kvalid && e < dh) {  // dh % 4 == 0: a group of 4 dims is inside or outside the head
                        const int64_t at = (int64_t)(k0 + key) * a.ldk + e;
                        for (int j = 0; j < 4; j++) {
                            kv[j] = kb[at + j];
                            vv[j] = vb[at + j];
                        }
                    }
                    for (int j = 0; j < 4; j++) {
                        Ks[key * KLD + e + j] = kv[j];
                        Vt[(e + j) * ATT_VLD + key] = vv[j];
                    }
                }
            }
        }
        __syncthreads();
        f32x4 S[4];
        for (int n = 0; n < 4; n++) {
            S[n] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            for (int ks = 0; ks < KS; ks++) {
                const f16x8 kf = *(const f16x8*)&Ks[(n * 16 + lr) * KLD + ks * 32 + lg * 8];
                S[n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(qa[ks], kf, S[n], 0, 0, 0);
            }
        }
        for (int r = 0; r < 4; r++) {  // query row 4 lg + r; its 64 keys: 4 tiles x the 16 lanes of this lane group
            float mx = -INFINITY;
            bool valid[4];
            for (int n = 0; n < 4; n++) {
                valid[n] = k0 + n * 16 + lr < nk;
                S[n][r] = valid[n] ? S[n][r] * scale : -INFINITY;
                mx = fmaxf(mx, S[n][r]);
            }
            for (int o = 1; o < 16; o <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
            const float m_new = fmaxf(m_run[r], mx);  // finite: key k0 of this tile is valid
            const float alpha = m_run[r] == -INFINITY ? 0.0f : __expf(m_run[r] - m_new);
            float ps = 0.0f;
            for (int n = 0; n < 4; n++) {
                const float p = valid[n] ? __expf(S[n][r] - m_new) : 0.0f;
                ps += p;
                Pw[(lg * 4 + r) * ATT_VLD + n * 16 + lr] = (f16)p;
            }
            for (int o = 1; o < 16; o <<= 1) ps += __shfl_xor(ps, o, 64);
            l_run[r] = l_run[r] * alpha + ps;
            m_run[r] = m_new;
            for (int dn = 0; dn < ND; dn++) O[dn][r] *= alpha;
        }
        __syncthreads();  // P visible to the whole wave
        for (int ks = 0; ks < 2; ks++) {
            const f16x8 pf = *(const f16x8*)&Pw[lr * ATT_VLD + ks * 32 + lg * 8];
            for (int dn = 0; dn < ND; dn++) {
                const f16x8 vf = *(const f16x8*)&Vt[(dn * 16 + lr) * ATT_VLD + ks * 32 + lg * 8];
                O[dn] = __builtin_amdgcn_mfma_f32_16x16x32_f16(pf, vf, O[dn], 0, 0, 0);
            }
        }
    }
    for (int r = 0; r < 4; r++) {
        const int q = q0 + w * 16 + lg * 4 + r;
        if (q >= a.Tq) continue;
        const float inv = q < nk ? 1.0f / l_run[r] : 0.0f;
        for (int dn = 0; dn < ND; dn++) {
            const int e = dn * 16 + lr;
            if (e < dh) ob[(int64_t)q * a.ldo + e] = (f16)(q < nk ? O[dn][r] * inv : 0.0f);
        }
    }
}

template <int DT, bool CLAMP>
void flash_attn_launch(const SeqAttnArgs& a, hipStream_t st) {
    const float scale = 1.0f / sqrtf((float)a.dh);
    flash_attn_kernel<DT, CLAMP><<<dim3(cdiv(a.Tq, 64), a.H, a.B), 256, 0, st>>>(a, scale);
    SPT_LAUNCH_CHECK();
}

}  // namespace
}  // namespace spt
