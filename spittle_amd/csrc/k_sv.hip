// k_sv.hip -- SenseVoice kernels (gfx950): Kaldi framing and the mel / log floor around the DFT GEMM,
// the LFR / CMVN / query / position rows, LayerNorm with bias, the FSMN depthwise memory, the MFMA
// flash attention for head dim 128, and CTC argmax + greedy collapse.  The GEMMs are gemm_nt.
#include "common.h"
#include "sv_host.h"
#include "sv_kernels.h"

#include <algorithm>
#include <cmath>

// contraction off for the whole file: every instance of a per-element formula (each kernel, each
// unrolled copy of a loop) computes the same bits, so a batch row is what it is alone
#pragma clang fp contract(off)

namespace spt {

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

__global__ void __launch_bounds__(512) frames_kernel(const float* pcm, int64_t stride, const int* lens, int Tp,
                                                     const float* window, float* frames) {
    __shared__ float xs[SV_NFFT];
    __shared__ float red[8];
    const int t = blockIdx.x, b = blockIdx.y, i = threadIdx.x;  // 512 threads
    const int T = lens[b * 4 + 1];
    float* row = frames + ((int64_t)b * Tp + t) * SV_NFFT;
    if (t >= T) {  // the whole workgroup
        row[i] = 0.0f;
        return;
    }
    // 160 t + 399 < n by T's definition
    const float v = i < SV_FRAME ? pcm[b * stride + (int64_t)t * SV_HOP + i] * 32768.0f : 0.0f;
    const float mean = block_sum(v, red) / (float)SV_FRAME;
    xs[i] = v - mean;
    __syncthreads();
    float o = 0.0f;
    if (i < SV_FRAME) {
        const float y = xs[i];
        const float z = i ? y - 0.97f * xs[i - 1] : y * (float)(1.0 - 0.97);
        o = z * window[i];
    }
    row[i] = o;
}

__global__ void __launch_bounds__(128) melpow_kernel(const float* spec, const float* fbT, float* mel) {
    __shared__ float pw[SV_NBIN];
    const int64_t m = blockIdx.x;
    const float* s = spec + m * SV_DFT_N;
    for (int k = threadIdx.x; k < SV_NBIN; k += 128) {
        const float re = s[k], im = s[SV_NBIN + k];
        pw[k] = re * re + im * im;
    }
    __syncthreads();
    const int j = threadIdx.x;
    if (j >= SV_MELS) return;
    float acc = 0.0f;
    for (int k = 0; k < SV_NBIN; k++) acc += fbT[k * SV_MELS + j] * pw[k];
    mel[m * SV_MELS + j] = logf(fmaxf(acc, 1.1920929e-07f));
}

__global__ void __launch_bounds__(256) lfr_rows_kernel(SvRowsArgs a) {
    const int r = blockIdx.x, b = blockIdx.y;
    const int T = a.lens[b * 4 + 1], R = a.lens[b * 4 + 3];
    float* row = a.out + ((int64_t)b * a.Rp + r) * a.ld;
    const int half = a.in >> 1;
    for (int c = threadIdx.x; c < a.ld; c += 256) {
        float o = 0.0f;
        if (r < R && c < a.in) {
            float v;
            if (r < SV_NQ) v = a.feat_only ? 0.0f : a.embed[a.q[r] * a.in + c];
            else {
                const int f = sv_lfr_frame(r - SV_NQ, c / SV_MELS, T, a.lfr_m, a.lfr_n);  // 0 <= f < T
                v = (a.mel[((int64_t)b * a.Tp + f) * SV_MELS + c % SV_MELS] + a.neg_mean[c]) * a.inv_std[c];
            }
            if (a.feat_only) o = v;
            else {
                const float ang = (float)(r + 1) * a.inv_freq[c < half ? c : c - half];
                o = v * a.scale + (c < half ? sinf(ang) : cosf(ang));
            }
        }
        row[c] = o;
    }
}

// one wave per row
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
    // a lane writes only the columns it read (y may be x)
    for (int c = lane; c < ldy; c += 64) yr[c] = c < d ? (OutT)((xr[c] - mean) * rstd * w[c] + bs[c]) : (OutT)0.0f;
}

__global__ void __launch_bounds__(256) fsmn_kernel(const f16* v, int ldv, const float* w, const int* lens, int Rp, int d,
                                                   int shift, int add, float* x) {
    const int t = blockIdx.x, b = blockIdx.y;
    const int R = lens[b * 4 + 3];
    float* xr = x + ((int64_t)b * Rp + t) * d;
    const f16* vb = v + (int64_t)b * Rp * ldv;
    const int left = (SV_FSMN_K - 1) / 2 + shift;
    for (int c = threadIdx.x; c < d; c += 256) {
        if (t >= R) {
            xr[c] = 0.0f;
            continue;
        }
        float acc = 0.0f;
        for (int j = 0; j < SV_FSMN_K; j++) {
            const int tt = t + j - left;
            const float vv = (tt >= 0 && tt < R) ? (float)vb[(int64_t)tt * ldv + c] : 0.0f;
            acc += w[c * SV_FSMN_K + j] * vv;
        }
        acc += (float)vb[(int64_t)t * ldv + c];
        xr[c] = add ? xr[c] + acc : acc;
    }
}

// ---------------------------------------------------------------- attention (MFMA, head dim 128)
// Workgroup = 4 waves = 64 queries of one (b, h); 64-key tiles of K (row-major, 128 dims) and V
// (transposed) staged in LDS with keys >= R_b stored as zero; a masked key's probability is set to 0
// (not multiplied to 0), so nothing a masked key holds reaches the output.
// v_mfma_f32_16x16x32_f16: A[row l&15][k = 8 (l>>4) + j], B[k = 8 (l>>4) + j][col l&15],
// C[row 4 (l>>4) + reg][col l&15].
constexpr int SVA_KLD = 136;  // K tile row pitch (f16): 128 + 8, rows stay 16-byte aligned
constexpr int SVA_VLD = 72;   // V^T / P row pitch: 64 + 8

__global__ void __launch_bounds__(256) attn128_kernel(const f16* qkv, const int* lens, int Rp, int d, f16* out, float scale) {
    __shared__ __attribute__((aligned(16))) f16 Ks[64 * SVA_KLD];
    __shared__ __attribute__((aligned(16))) f16 Vt[128 * SVA_VLD];
    __shared__ __attribute__((aligned(16))) f16 Ps[4 * 16 * SVA_VLD];
    const int b = blockIdx.z, h = blockIdx.y, q0 = blockIdx.x * 64;
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, lr = l & 15, lg = l >> 4;
    const int nk = min(lens[b * 4 + 3], Rp);
    const int ld = 3 * d;
    const f16* qb = qkv + (int64_t)b * Rp * ld + h * 128;
    const f16* kb = qb + d;
    const f16* vb = qb + 2 * d;
    f16* ob = out + (int64_t)b * Rp * d + h * 128;
    if (q0 >= nk) {  // a padded query block: zero rows
        for (int o = tid; o < 64 * 128; o += 256) {
            const int q = q0 + (o >> 7);
            if (q < Rp) ob[(int64_t)q * d + (o & 127)] = (f16)0.0f;
        }
        return;
    }
    f16x8 qa[4];
    {
        const int q = q0 + w * 16 + lr;
        for (int ks = 0; ks < 4; ks++) {
            for (int j = 0; j < 8; j++) qa[ks][j] = (f16)0.0f;
            if (q < nk) qa[ks] = *(const f16x8*)&qb[(int64_t)q * ld + ks * 32 + lg * 8];
        }
    }
    f32x4 O[8];
    float m_run[4], l_run[4];
    for (int i = 0; i < 8; i++) O[i] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    for (int i = 0; i < 4; i++) {
        m_run[i] = -INFINITY;
        l_run[i] = 0.0f;
    }
    f16* Pw = Ps + w * 16 * SVA_VLD;
    for (int k0 = 0; k0 < nk; k0 += 64) {
        __syncthreads();  // the previous tile's reads are done
        {
            const int key = tid >> 2, part = (tid & 3) * 32;
            const bool kvalid = k0 + key < nk;
            for (int c = 0; c < 4; c++) {
                const int e = part + c * 8;
                f16x8 kv, vv;
                for (int j = 0; j < 8; j++) kv[j] = vv[j] = (f16)0.0f;
                if (kvalid) {
                    const int64_t at = (int64_t)(k0 + key) * ld + e;
                    kv = *(const f16x8*)&kb[at];
                    vv = *(const f16x8*)&vb[at];
                }
                *(f16x8*)&Ks[key * SVA_KLD + e] = kv;
                for (int j = 0; j < 8; j++) Vt[(e + j) * SVA_VLD + key] = vv[j];
            }
        }
        __syncthreads();
        f32x4 S[4];
        for (int n = 0; n < 4; n++) {
            S[n] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            for (int ks = 0; ks < 4; ks++) {
                const f16x8 kf = *(const f16x8*)&Ks[(n * 16 + lr) * SVA_KLD + ks * 32 + lg * 8];
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
                Pw[(lg * 4 + r) * SVA_VLD + n * 16 + lr] = (f16)p;
            }
            for (int o = 1; o < 16; o <<= 1) ps += __shfl_xor(ps, o, 64);
            l_run[r] = l_run[r] * alpha + ps;
            m_run[r] = m_new;
            for (int dn = 0; dn < 8; dn++) O[dn][r] *= alpha;
        }
        __syncthreads();  // P visible to the whole wave
        for (int ks = 0; ks < 2; ks++) {
            const f16x8 pf = *(const f16x8*)&Pw[lr * SVA_VLD + ks * 32 + lg * 8];
            for (int dn = 0; dn < 8; dn++) {
                const f16x8 vf = *(const f16x8*)&Vt[(dn * 16 + lr) * SVA_VLD + ks * 32 + lg * 8];
                O[dn] = __builtin_amdgcn_mfma_f32_16x16x32_f16(pf, vf, O[dn], 0, 0, 0);
            }
        }
    }
    for (int r = 0; r < 4; r++) {
        const int q = q0 + w * 16 + lg * 4 + r;
        if (q >= Rp) continue;
        const float inv = q < nk ? 1.0f / l_run[r] : 0.0f;
        for (int dn = 0; dn < 8; dn++)
            ob[(int64_t)q * d + dn * 16 + lr] = (f16)(q < nk ? O[dn][r] * inv : 0.0f);
    }
}

// ---------------------------------------------------------------- CTC
__global__ void __launch_bounds__(256) ctc_top2_kernel(const float* logits, int V, int ld, int* ids, float* top1, float* top2) {
    __shared__ float v1s[256], v2s[256];
    __shared__ int i1s[256];
    const int64_t m = blockIdx.x;
    const int tid = threadIdx.x;
    const float* lg = logits + m * ld;
    float v1 = -INFINITY, v2 = -INFINITY;
    int i1 = 0x7FFFFFFF;
    for (int i = tid; i < V; i += 256) {  // the real columns only; ascending: a tie keeps the lower index
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
    if (tid != 0) return;
    int tok = i1s[0];
    if (tok < 0 || tok >= V) tok = 0;  // a row of NaNs
    ids[m] = tok;
    top1[m] = v1s[0];
    top2[m] = v2s[0];
}

__global__ void __launch_bounds__(256) ctc_collapse_kernel(SvCollapseArgs a) {
    __shared__ int scan[256];
    __shared__ int base;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int R = min(a.lens[b * 4 + 3], a.Rp);
    const int* ids = a.ids + (int64_t)b * a.Rp;
    const float* t1 = a.top1 + (int64_t)b * a.Rp;
    const float* t2 = a.top2 + (int64_t)b * a.Rp;
    int* out = a.out + (int64_t)b * (8 + 4 * (int64_t)a.cap);
    if (tid < SV_NQ) out[1 + tid] = (tid < a.n_prefix && tid < R) ? ids[tid] : -1;
    if (tid == 0) base = 0;
    __syncthreads();
    for (int r0 = a.n_prefix; r0 < R; r0 += 256) {
        const int r = r0 + tid;
        int flag = 0, id = 0;
        if (r < R) {
            id = ids[r];
            flag = (r == a.n_prefix || id != ids[r - 1]) && id != a.blank;
        }
        scan[tid] = flag;
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {
            const int add = tid >= o ? scan[tid - o] : 0;
            __syncthreads();
            scan[tid] += add;
            __syncthreads();
        }
        const int pos = base + scan[tid] - 1;
        if (flag && pos < a.cap) {
            out[8 + pos] = id;
            out[8 + a.cap + pos] = r - a.n_prefix;
            out[8 + 2 * a.cap + pos] = __float_as_int(t1[r]);
            out[8 + 3 * a.cap + pos] = __float_as_int(t2[r]);
        }
        __syncthreads();
        if (tid == 255) base += scan[255];
        __syncthreads();
    }
    if (tid == 0) out[0] = min(base, a.cap);
}

}  // namespace

void sv_frames(const float* pcm, int64_t stride, const int* lens, int B, int Tp, const float* window, float* frames,
               hipStream_t st) {
    frames_kernel<<<dim3(Tp, B), SV_NFFT, 0, st>>>(pcm, stride, lens, Tp, window, frames);
    SPT_LAUNCH_CHECK();
}
void sv_melpow(const float* spec, int M, const float* fbT, float* mel, hipStream_t st) {
    melpow_kernel<<<M, 128, 0, st>>>(spec, fbT, mel);
    SPT_LAUNCH_CHECK();
}
void sv_lfr_rows(const SvRowsArgs& a, int B, hipStream_t st) {
    if (a.in > a.ld || a.in % 2) throw std::runtime_error("sv_lfr_rows: bad widths");
    lfr_rows_kernel<<<dim3(a.Rp, B), 256, 0, st>>>(a);
    SPT_LAUNCH_CHECK();
}
void sv_layernorm(const float* x, int M, int d, int ldx, const float* w, const float* b, float eps, void* y, int ldy,
                  bool out_f32, hipStream_t st) {
    if (d > ldx || d > ldy) throw std::runtime_error("sv_layernorm: d above a row pitch");
    if (out_f32) layernorm_kernel<float><<<cdiv(M, 4), 256, 0, st>>>(x, M, d, ldx, w, b, eps, (float*)y, ldy);
    else layernorm_kernel<f16><<<cdiv(M, 4), 256, 0, st>>>(x, M, d, ldx, w, b, eps, (f16*)y, ldy);
    SPT_LAUNCH_CHECK();
}
void sv_fsmn(const void* v, int ldv, const float* w, const int* lens, int B, int Rp, int d, int shift, bool add, float* x,
             hipStream_t st) {
    fsmn_kernel<<<dim3(Rp, B), 256, 0, st>>>((const f16*)v, ldv, w, lens, Rp, d, shift, add ? 1 : 0, x);
    SPT_LAUNCH_CHECK();
}
void sv_attention(const void* qkv, const int* lens, int B, int Rp, int H, void* out, hipStream_t st) {
    const float scale = 1.0f / sqrtf(128.0f);
    attn128_kernel<<<dim3(cdiv(Rp, 64), H, B), 256, 0, st>>>((const f16*)qkv, lens, Rp, H * 128, (f16*)out, scale);
    SPT_LAUNCH_CHECK();
}
void sv_ctc_top2(const float* logits, int M, int V, int ld, int* ids, float* top1, float* top2, hipStream_t st) {
    if (V > ld) throw std::runtime_error("sv_ctc_top2: V above the row pitch");
    ctc_top2_kernel<<<M, 256, 0, st>>>(logits, V, ld, ids, top1, top2);
    SPT_LAUNCH_CHECK();
}
void sv_ctc_collapse(const SvCollapseArgs& a, int B, hipStream_t st) {
    ctc_collapse_kernel<<<B, 256, 0, st>>>(a);
    SPT_LAUNCH_CHECK();
}

}  // namespace spt
