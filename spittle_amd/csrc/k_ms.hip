// k_ms.hip -- Moonshine kernels (gfx950): the PCM stem's framing / GroupNorm / gathers,
// partial interleaved rotary, and the decode step's GEMV / attention / argmax.  The LayerNorm, the
// encoder's flash attention (head tile 64) and the top-2 reduction are seq_kernels.h' text,
// instantiated here.  The GEMMs themselves are gemm_nt (k_gemm.hip).
#include "common.h"
#include "ms_kernels.h"
#include "seq_kernels.h"

#include <algorithm>
#include <cmath>

namespace spt {

namespace {

// contraction off: every kernel (and every unrolled copy of a loop) that inlines it computes the same bits
__device__ inline float gelu_erf(float x) {
#pragma clang fp contract(off)
    return 0.5f * x * (1.0f + erff(x * 0.70710678118654752f));
}

__global__ void frames_kernel(const float* pcm, int64_t stride, const int* lens, int T1p, float* frames) {
    const int t = blockIdx.x, b = blockIdx.y, i = threadIdx.x;  // 128 threads
    const int T1 = lens[b * 4 + 1];
    float v = 0.0f;
    if (t < T1 && i < MS_K1) v = pcm[b * stride + (int64_t)t * MS_S1 + i];  // t * 64 + 126 < n by T1's definition
    frames[((int64_t)b * T1p + t) * MS_K1P + i] = v;
}

__global__ void __launch_bounds__(1024) tanh_gn_kernel(float* h, const int* lens, int T1p, int d, int dp, float eps,
                                                       float* stats) {
    __shared__ float red[16];
    const int b = blockIdx.x, T1 = lens[b * 4 + 1];
    float* hb = h + (int64_t)b * T1p * dp;
    const int64_t n = (int64_t)T1 * d;
    float s = 0.0f;
    for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {
        const int64_t o = (i / d) * dp + (i % d);
        const float v = tanhf(hb[o]);
        hb[o] = v;
        s += v;
    }
    const float cnt = (float)(n > 0 ? n : 1);
    const float mean = block_sum(s, red) / cnt;
    float q = 0.0f;
    for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {  // each thread re-reads what it wrote
        const float v = hb[(i / d) * dp + (i % d)] - mean;
        q += v * v;
    }
    const float var = block_sum(q, red) / cnt;
    if (threadIdx.x == 0) {
        stats[b * 2] = mean;
        stats[b * 2 + 1] = 1.0f / sqrtf(var + eps);
    }
}

__global__ void gather2_kernel(const float* h, const float* stats, const float* gw, const float* gb, const int* lens,
                               int T1p, int T2p, int d, int dp, f16* A) {
    const int t2 = blockIdx.x, b = blockIdx.y;
    const int T2 = lens[b * 4 + 2];
    f16* row = A + ((int64_t)b * T2p + t2) * (MS_K2 * dp);
    const float mean = stats[b * 2], rstd = stats[b * 2 + 1];
    for (int o = threadIdx.x; o < MS_K2 * dp; o += blockDim.x) {
        const int k = o / dp, c = o % dp;
        float v = 0.0f;
        if (t2 < T2 && c < d)  // 3 t2 + k <= 3 (T2 - 1) + 6 < T1
            v = ln_out(h[((int64_t)b * T1p + t2 * MS_S2 + k) * dp + c], mean, rstd, gw[c], gb[c]);
        row[o] = (f16)v;
    }
}

__global__ void gather3_kernel(const float* c2, const int* lens, int T2p, int T3p, int n2p, f16* A) {
    const int t3 = blockIdx.x, b = blockIdx.y;
    const int T3 = lens[b * 4 + 3];
    f16* row = A + ((int64_t)b * T3p + t3) * (MS_K3 * n2p);
    for (int o = threadIdx.x; o < MS_K3 * n2p; o += blockDim.x) {
        const int k = o / n2p, c = o % n2p;
        float v = 0.0f;
        if (t3 < T3) v = gelu_erf(c2[((int64_t)b * T2p + t3 * MS_S3 + k) * n2p + c]);  // pad columns: gelu(0) = 0
        row[o] = (f16)v;
    }
}

__global__ void gelu_rows_kernel(float* x, const int* lens, int li, int Tp, int ld) {
    const int t = blockIdx.x, b = blockIdx.y;
    const bool valid = t < lens[b * 4 + li];
    float* row = x + ((int64_t)b * Tp + t) * ld;
    for (int c = threadIdx.x; c < ld; c += blockDim.x) row[c] = valid ? gelu_erf(row[c]) : 0.0f;
}

__global__ void gelu_f16_kernel(const float* x, int64_t n, f16* y) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        y[i] = (f16)gelu_erf(x[i]);
}

// the pair (x[2i], x[2i+1]) of a head's first `rot` dims rotated by the angle of (pos, i)
__device__ inline void rope_pair(float a, float b, const float* tab, int pos, int rot, int i, float& oa, float& ob) {
#pragma clang fp contract(off)
    const float c = tab[(int64_t)pos * rot + i], s = tab[(int64_t)pos * rot + (rot >> 1) + i];
    oa = a * c - b * s;
    ob = b * c + a * s;
}

__global__ void rope_enc_kernel(const float* qkv32, int Tp, int H, int dh, int rot, int dp, const float* tab, f16* qkv16) {
    const int t = blockIdx.x, b = blockIdx.y;
    const int64_t base = ((int64_t)b * Tp + t) * (3 * dp);
    const int d = H * dh, half = dh >> 1;
    for (int o = threadIdx.x; o < 2 * H * half; o += blockDim.x) {  // q and k pairs
        const int which = o / (H * half), r = o % (H * half), h = r / half, i = r % half;
        const int64_t at = base + (int64_t)which * dp + h * dh + 2 * i;
        float a = qkv32[at], c = qkv32[at + 1];
        if (2 * i < rot) rope_pair(a, c, tab, t, rot, i, a, c);
        qkv16[at] = (f16)a;
        qkv16[at + 1] = (f16)c;
    }
    for (int c = threadIdx.x; c < d; c += blockDim.x) qkv16[base + 2 * dp + c] = (f16)qkv32[base + 2 * dp + c];
}

__global__ void rope_dec_kernel(const float* qkv32, int R, int H, int dh, int rot, int d, const float* tab,
                                const MsState* s, f16* q16, f16* cache, int ctx) {
    const int r = blockIdx.x, half = dh >> 1;
    const int pos = s->step;
    if (pos >= ctx) return;  // the host never replays past ctx steps
    const float* src = qkv32 + (int64_t)r * 3 * d;
    f16* kdst = cache + ((int64_t)r * ctx + pos) * d;
    f16* vdst = cache + ((int64_t)R * ctx + (int64_t)r * ctx + pos) * d;
    for (int o = threadIdx.x; o < 2 * H * half; o += blockDim.x) {
        const int which = o / (H * half), rr = o % (H * half), h = rr / half, i = rr % half;
        const int at = h * dh + 2 * i;
        float a = src[which * d + at], c = src[which * d + at + 1];
        if (2 * i < rot) rope_pair(a, c, tab, pos, rot, i, a, c);
        f16* dst = which == 0 ? q16 + (int64_t)r * d : kdst;
        dst[at] = (f16)a;
        dst[at + 1] = (f16)c;
    }
    for (int c = threadIdx.x; c < d; c += blockDim.x) vdst[c] = (f16)src[2 * d + c];
}

// ---------------------------------------------------------------- decode attention (one query per row)
// One workgroup (256 threads) per (row, head).  Scores of all keys in LDS (f32), then the
// probability-weighted sum of V with each thread owning one dim for a quarter of the keys.
constexpr int DEC_ATT_MAXK = 8192;

__global__ void __launch_bounds__(256) dec_attn_kernel(int mode, MsAttnArgs a, float scale) {
    extern __shared__ float sc[];  // [nk_cap]
    __shared__ float red[4];
    __shared__ float qs[64];
    __shared__ float part[4][64];
    const int h = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, dh = a.dh;
    int nk;
    int64_t kbs = a.k_bstride;
    if (mode == MS_ATT_SELF) nk = a.s->step + 1;
    else {
        nk = a.lens[b * 4 + 3];
        kbs = (int64_t)a.s->t3p * a.ldk;
    }
    if (nk > DEC_ATT_MAXK) nk = DEC_ATT_MAXK;  // the engine's capacities keep nk below this
    const f16* qb = (const f16*)a.q + b * a.q_bstride + h * dh;
    const f16* kb = (const f16*)a.k + b * kbs + h * dh;
    const f16* vb = (const f16*)a.v + b * kbs + h * dh;
    f16* ob = (f16*)a.out + b * a.o_bstride + h * dh;
    if (tid < 64) qs[tid] = tid < dh ? (float)qb[tid] : 0.0f;
    __syncthreads();
    float mx = -INFINITY;
    for (int t = tid; t < nk; t += 256) {
        const f16* kr = kb + (int64_t)t * a.ldk;
        float s = 0.0f;
        for (int e = 0; e < dh; e += 4) {
            const f16x2v k01 = *(const f16x2v*)(kr + e), k23 = *(const f16x2v*)(kr + e + 2);
            s += qs[e] * (float)k01[0] + qs[e + 1] * (float)k01[1] + qs[e + 2] * (float)k23[0] + qs[e + 3] * (float)k23[1];
        }
        s *= scale;
        sc[t] = s;
        mx = fmaxf(mx, s);
    }
    mx = wave_max(mx);
    if ((tid & 63) == 0) red[tid >> 6] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    float ls = 0.0f;
    for (int t = tid; t < nk; t += 256) {
        const float p = __expf(sc[t] - mx);
        sc[t] = p;
        ls += p;
    }
    ls = wave_sum(ls);
    if ((tid & 63) == 0) red[tid >> 6] = ls;
    __syncthreads();  // also makes every sc[] visible
    ls = (red[0] + red[1]) + (red[2] + red[3]);
    const int e = tid & 63, g = tid >> 6;
    float acc = 0.0f;
    if (e < dh)
        for (int t = g; t < nk; t += 4) acc += sc[t] * (float)vb[(int64_t)t * a.ldk + e];
    part[g][e] = acc;
    __syncthreads();
    if (tid < dh) ob[tid] = (f16)(((part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid])) / ls);
}

// ---------------------------------------------------------------- decode GEMV
// One wave per output column (SILU: its two weight rows), 8 activation rows at a time.
template <int MODE>
__global__ void __launch_bounds__(256) gemv_kernel(const f16* x, int R, int K, const f16* W, const float* bias, int N,
                                                   void* out, const MsState* s) {
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (n >= N) return;
    const f16* w0 = W + (int64_t)n * K;
    const f16* w1 = W + (int64_t)(n + N) * K;  // SILU: the gate row
    for (int r0 = 0; r0 < R; r0 += 8) {
        float acc[8], acg[8];
        for (int i = 0; i < 8; i++) acc[i] = acg[i] = 0.0f;
        for (int k = lane * 8; k < K; k += 512) {
            const f16x8 wv = *(const f16x8*)(w0 + k);
            f16x8 gv = wv;
            if (MODE == MS_GV_SILU) gv = *(const f16x8*)(w1 + k);
            for (int i = 0; i < 8; i++) {
                if (r0 + i >= R) break;
                const f16x8 xv = *(const f16x8*)(x + (int64_t)(r0 + i) * K + k);
                float t = 0.0f, u = 0.0f;
                for (int j = 0; j < 8; j++) {
                    t += (float)xv[j] * (float)wv[j];
                    if (MODE == MS_GV_SILU) u += (float)xv[j] * (float)gv[j];
                }
                acc[i] += t;
                acg[i] += u;
            }
        }
        for (int i = 0; i < 8 && r0 + i < R; i++) {
            float v = wave_sum(acc[i]) + (bias ? bias[n] : 0.0f);
            const int r = r0 + i;
            if (MODE == MS_GV_SILU) {
                const float g = wave_sum(acg[i]) + (bias ? bias[n + N] : 0.0f);
                v = g / (1.0f + __expf(-g)) * v;
            }
            if (lane != 0) continue;
            if (MODE == MS_GV_F32) ((float*)out)[(int64_t)r * N + n] = v;
            else if (MODE == MS_GV_RESID) ((float*)out)[(int64_t)r * N + n] += v;
            else if (MODE == MS_GV_LOGITS) s->logits[(s->log_all ? (int64_t)s->step * R * N : 0) + (int64_t)r * N + n] = v;
            else ((f16*)out)[(int64_t)r * N + n] = (f16)v;
        }
    }
}

__global__ void embed_kernel(const f16* emb, int d, const int* cur_tok, const int* forced, const MsState* s, float* x) {
    const int r = blockIdx.x;
    int tok = cur_tok[r];
    if (s->forced_len > 0) tok = forced[r * s->forced_len + min(s->step, s->forced_len - 1)];
    for (int c = threadIdx.x; c < d; c += blockDim.x) x[(int64_t)r * d + c] = (float)emb[(int64_t)tok * d + c];
}

__global__ void __launch_bounds__(256) finalize_kernel(MsFinArgs a) {
    const int r = blockIdx.x;
    const MsState* s = a.s;
    const RowTop2 t = row_top2(s->logits + (s->log_all ? (int64_t)s->step * a.R * a.V : 0) + (int64_t)r * a.V, a.V);
    if (threadIdx.x != 0) return;
    const int tok = t.tok;
    a.cur_tok[r] = tok;
    if (a.done[r]) return;
    if (tok == s->eos && s->forced_len == 0) {
        a.done[r] = 1;
        a.hit_eos[r] = 1;
        return;
    }
    const int n = a.n_out[r];
    if (n < s->cap) {
        a.out_tok[(int64_t)r * s->cap + n] = tok;
        a.out_top1[(int64_t)r * s->cap + n] = t.v1;
        a.out_top2[(int64_t)r * s->cap + n] = t.v2;
    }
    a.n_out[r] = n + 1;
    if (n + 1 >= a.limit[r]) a.done[r] = 1;
}

__global__ void advance_kernel(MsState* s) { s->step += 1; }

}  // namespace

void ms_frames(const float* pcm, int64_t stride, const int* lens, int B, int T1p, float* frames, hipStream_t st) {
    frames_kernel<<<dim3(T1p, B), MS_K1P, 0, st>>>(pcm, stride, lens, T1p, frames);
    SPT_LAUNCH_CHECK();
}
void ms_tanh_gn_stats(float* h, const int* lens, int B, int T1p, int d, int dp, float eps, float* stats, hipStream_t st) {
    tanh_gn_kernel<<<B, 1024, 0, st>>>(h, lens, T1p, d, dp, eps, stats);
    SPT_LAUNCH_CHECK();
}
void ms_gather2(const float* h, const float* stats, const float* gw, const float* gb, const int* lens, int B, int T1p,
                int T2p, int d, int dp, void* A, hipStream_t st) {
    gather2_kernel<<<dim3(T2p, B), 256, 0, st>>>(h, stats, gw, gb, lens, T1p, T2p, d, dp, (f16*)A);
    SPT_LAUNCH_CHECK();
}
void ms_gather3(const float* c2, const int* lens, int B, int T2p, int T3p, int n2p, void* A, hipStream_t st) {
    gather3_kernel<<<dim3(T3p, B), 256, 0, st>>>(c2, lens, T2p, T3p, n2p, (f16*)A);
    SPT_LAUNCH_CHECK();
}
void ms_gelu_rows(float* x, const int* lens, int li, int B, int Tp, int ld, hipStream_t st) {
    gelu_rows_kernel<<<dim3(Tp, B), 256, 0, st>>>(x, lens, li, Tp, ld);
    SPT_LAUNCH_CHECK();
}
void ms_gelu_f16(const float* x, int64_t n, void* y, hipStream_t st) {
    // one element per thread: no grid-stride second trip whose code could round differently
    gelu_f16_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(x, n, (f16*)y);
    SPT_LAUNCH_CHECK();
}
void ms_layernorm(const float* x, int M, int d, int ldx, const float* w, void* y, int ldy, bool out_f32, hipStream_t st) {
    layernorm_launch(x, M, d, ldx, w, nullptr, 1e-5f, y, ldy, out_f32, st);
}
void ms_rope_enc(const float* qkv32, int B, int Tp, int H, int dh, int rot, int dp, const float* tab, void* qkv16,
                 hipStream_t st) {
    rope_enc_kernel<<<dim3(Tp, B), 256, 0, st>>>(qkv32, Tp, H, dh, rot, dp, tab, (f16*)qkv16);
    SPT_LAUNCH_CHECK();
}
void ms_rope_dec(const float* qkv32, int R, int H, int dh, int rot, int d, const float* tab, const MsState* s, void* q16,
                 void* cache, int ctx, hipStream_t st) {
    rope_dec_kernel<<<R, 256, 0, st>>>(qkv32, R, H, dh, rot, d, tab, s, (f16*)q16, (f16*)cache, ctx);
    SPT_LAUNCH_CHECK();
}
void ms_attention(int mode, const MsAttnArgs& a, hipStream_t st) {
    if (a.dh > 64 || a.dh % 4) throw std::runtime_error("ms_attention: head dim must be a multiple of 4, <= 64");
    if (mode == MS_ATT_ENC) {
        flash_attn_launch<64, false>(SeqAttnArgs{a.q, a.ldq, a.q_bstride, a.k, a.v, a.ldk, a.k_bstride, a.out, a.ldo,
                                                 a.o_bstride, a.lens, a.B, a.H, a.dh, a.Tq}, st);
        return;
    }
    dec_attn_kernel<<<dim3(a.H, a.B), 256, DEC_ATT_MAXK * sizeof(float), st>>>(mode, a, 1.0f / sqrtf((float)a.dh));
    SPT_LAUNCH_CHECK();
}
void ms_gemv(int mode, const void* x16, int R, int K, const void* W, const float* bias, int N, void* out,
             const MsState* s, hipStream_t st) {
    if (K % 8) throw std::runtime_error("ms_gemv: K % 8");
    const dim3 grid(cdiv(N, 4));
#define MS_GV(M) gemv_kernel<M><<<grid, 256, 0, st>>>((const f16*)x16, R, K, (const f16*)W, bias, N, out, s)
    switch (mode) {
        case MS_GV_F32: MS_GV(MS_GV_F32); break;
        case MS_GV_RESID: MS_GV(MS_GV_RESID); break;
        case MS_GV_F16: MS_GV(MS_GV_F16); break;
        case MS_GV_SILU: MS_GV(MS_GV_SILU); break;
        case MS_GV_LOGITS: MS_GV(MS_GV_LOGITS); break;
        default: throw std::runtime_error("ms_gemv: bad mode");
    }
#undef MS_GV
    SPT_LAUNCH_CHECK();
}
void ms_embed(const void* emb, int d, int R, const int* cur_tok, const int* forced, const MsState* s, float* x,
              hipStream_t st) {
    embed_kernel<<<R, 256, 0, st>>>((const f16*)emb, d, cur_tok, forced, s, x);
    SPT_LAUNCH_CHECK();
}
void ms_finalize(const MsFinArgs& a, hipStream_t st) {
    finalize_kernel<<<a.R, 256, 0, st>>>(a);
    SPT_LAUNCH_CHECK();
}
void ms_advance(MsState* s, hipStream_t st) {
    advance_kernel<<<1, 1, 0, st>>>(s);
    SPT_LAUNCH_CHECK();
}

}  // namespace spt
