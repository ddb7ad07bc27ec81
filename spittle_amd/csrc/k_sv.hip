// k_sv.hip -- SenseVoice kernels (gfx950): Kaldi framing and the mel / log floor around the DFT GEMM,
// the LFR / CMVN / query / position rows, the FSMN depthwise memory and the CTC greedy collapse.  The
// LayerNorm, the flash attention (head tile 128) and the CTC top-2 are seq_kernels.h' text,
// instantiated here.  The GEMMs are gemm_nt.
#include "common.h"
#include "sv_host.h"
#include "sv_kernels.h"

#include <algorithm>
#include <cmath>

// contraction off for the whole file: every instance of a per-element formula (each kernel, each
// unrolled copy of a loop) computes the same bits, so a batch row is what it is alone
#pragma clang fp contract(off)

#include "seq_kernels.h"  // below the pragma: this file's instantiations have contraction off too

namespace spt {

namespace {

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

// ---------------------------------------------------------------- CTC
__global__ void __launch_bounds__(256) ctc_top2_kernel(const float* logits, int V, int ld, int* ids, float* top1, float* top2) {
    const int64_t m = blockIdx.x;
    const RowTop2 t = row_top2(logits + m * ld, V);  // the real columns only
    if (threadIdx.x != 0) return;
    ids[m] = t.tok;
    top1[m] = t.v1;
    top2[m] = t.v2;
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
    layernorm_launch(x, M, d, ldx, w, b, eps, y, ldy, out_f32, st);
}
void sv_fsmn(const void* v, int ldv, const float* w, const int* lens, int B, int Rp, int d, int shift, bool add, float* x,
             hipStream_t st) {
    fsmn_kernel<<<dim3(Rp, B), 256, 0, st>>>((const f16*)v, ldv, w, lens, Rp, d, shift, add ? 1 : 0, x);
    SPT_LAUNCH_CHECK();
}
void sv_attention(const void* qkv, const int* lens, int B, int Rp, int H, void* out, hipStream_t st) {
    const int d = H * 128, ld = 3 * d;
    const f16* q = (const f16*)qkv;
    flash_attn_launch<128, true>(SeqAttnArgs{q, ld, (int64_t)Rp * ld, q + d, q + 2 * d, ld, (int64_t)Rp * ld, out, d,
                                             (int64_t)Rp * d, lens, B, H, 128, Rp}, st);
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
