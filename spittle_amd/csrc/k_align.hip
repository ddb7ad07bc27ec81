// k_align.hip -- token alignment from the decoder's cross-attention: the attention
// probabilities of the alignment heads (align_qk), their per-column normalisation, 7-tap median and
// head mean (align_norm), and the dynamic time warping of the result (align_dtw).  Everything after
// the 16-bit loads of q and K is f32 (statistics and the head mean accumulate in f64); no kernel
// waits on another workgroup.
#include <hip/hip_runtime.h>

#include "common.h"
#include "dec_attn.h"
#include "kernels.h"

namespace spt {

namespace {

constexpr int kQkThreads = 512;     // align_qk: 8 waves per (head, sequence)
constexpr int kNormThreads = 256;   // align_norm: one column per thread
constexpr int kMedTile = kNormThreads - 6;  // output columns of a median workgroup (3 halo columns a side)
constexpr int kDtwThreads = 256;    // align_dtw: one text row per thread
constexpr int kDtwCostStride = kDtwThreads + 8;

// ------------------------------------------------------------------ align_qk
// One workgroup per (alignment head of this layer, sequence).  A key row is 64 elements = LPK lanes
// of 16 bytes, so a wave's load instruction sweeps 64 / LPK whole keys, fully coalesced; the Tq <= 4
// query rows sit pre-scaled in registers and share every key read.  The scores (log2 units) of all
// T_enc real keys go to LDS, then wave r turns row r into probabilities: maximum, sum of
// exp2(s - max) over every real key in a fixed order, and p = exp2(s - max) / sum for the first M.
template <typename T>
__global__ __launch_bounds__(kQkThreads) void align_qk_kernel(AlignQkArgs a) {
    constexpr int EPL = 16 / (int)sizeof(T);   // elements per lane
    constexpr int LPK = 64 / EPL;              // lanes per key
    constexpr int KPP = kQkThreads / LPK;      // keys per pass of the workgroup
    extern __shared__ __attribute__((aligned(16))) float s_sc[];  // [Tq][T32]
    const int tid = threadIdx.x, b = blockIdx.y;
    const int h = a.heads[blockIdx.x];
    const int w = a.kvrow ? a.kvrow[b] : b;
    if ((unsigned)h >= (unsigned)a.H || (unsigned)w >= (unsigned)a.B_layout) return;  // (uniform)
    const int T32 = (a.T_enc + 31) / 32 * 32;
    const int g = tid / LPK, sub = tid % LPK;

    float qf[4][EPL];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const T* qr = (const T*)a.q + ((size_t)(b * a.Tq + (r < a.Tq ? r : 0)) * a.H + h) * 64 + sub * EPL;
#pragma unroll
        for (int e = 0; e < EPL; ++e) qf[r][e] = r < a.Tq ? to_f<T>(qr[e]) * kLog2Scale : 0.0f;
    }
    const T* kbase = (const T*)a.kv + ((size_t)w * a.H + h) * 4096 + sub * EPL;
    const size_t blk = (size_t)a.B_layout * a.H * 4096;  // elements from one 32-key block to the next
    // four key loads per lane in flight: the loop is latency-bound otherwise (one workgroup streams a head's K)
    constexpr int U = 4;
    for (int t0 = 0; t0 < a.T_enc; t0 += KPP * U) {
        uint4 raw[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int t = t0 + u * KPP + g;
            const int tc = t < a.T_enc ? t : a.T_enc - 1;
            raw[u] = *(const uint4*)(kbase + (size_t)(tc >> 5) * blk + (tc & 31) * 64);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int t = t0 + u * KPP + g;
            const T* kv = (const T*)&raw[u];
            float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int e = 0; e < EPL; ++e) {
                const float ke = to_f<T>(kv[e]);
#pragma unroll
                for (int r = 0; r < 4; ++r) s[r] = fmaf(qf[r][e], ke, s[r]);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
#pragma unroll
                for (int o = 1; o < LPK; o <<= 1) s[r] += __shfl_xor(s[r], o, 64);
            }
            if (t < a.T_enc && sub == 0) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (r < a.Tq) s_sc[r * T32 + t] = s[r];
            }
        }
    }
    __syncthreads();

    const int r = tid >> 6, lane = tid & 63;
    const int rr = a.pos0 + r;  // the text row; a pass may begin before row 0 (the prompt's inputs)
    if (r >= a.Tq || rr < 0 || rr >= a.N_cap) return;
    const float* row = s_sc + r * T32;
    float mx = -INFINITY;
    for (int t = lane; t < a.T_enc; t += 64) mx = fmaxf(mx, row[t]);
    mx = wave_max(mx);
    float l = 0.0f;
    for (int t = lane; t < a.T_enc; t += 64) l += exp2f(row[t] - mx);
    l = wave_sum(l);
    int M = a.M[b];
    M = M < a.M_cap ? M : a.M_cap;
    M = M < a.T_enc ? M : a.T_enc;
    float* out = a.p + (((size_t)b * a.A + a.a0 + blockIdx.x) * a.N_cap + rr) * a.M_cap;
    for (int t = lane; t < M; t += 64) out[t] = exp2f(row[t] - mx) / l;
}

// ------------------------------------------------------------------ align_norm
// mean and population standard deviation of every (sequence, head, key) column over the N rows:
// stat [B][A][2][M_cap] = {mean, std} (f64 sums, rounded once)
__global__ __launch_bounds__(kNormThreads) void align_stat_kernel(const float* p, int A, int N_cap, int M_cap,
                                                                  const int* Ns, const int* Ms, float* stat) {
    const int b = blockIdx.z, a = blockIdx.y, s = blockIdx.x * kNormThreads + threadIdx.x;
    const int N = min(Ns[b], N_cap), M = min(Ms[b], M_cap);
    if (s >= M || N < 1) return;
    const float* col = p + ((size_t)b * A + a) * N_cap * M_cap + s;
    double sum = 0.0;
    for (int r = 0; r < N; ++r) sum += (double)col[(size_t)r * M_cap];
    const double mean = sum / N;
    double sq = 0.0;
    for (int r = 0; r < N; ++r) {
        const double d = (double)col[(size_t)r * M_cap] - mean;
        sq += d * d;
    }
    float* o = stat + ((size_t)b * A + a) * 2 * M_cap + s;
    o[0] = (float)mean;
    o[M_cap] = (float)sqrt(sq / N);
}

__device__ __forceinline__ void cswap(float& x, float& y) {
    const float lo = fminf(x, y), hi = fmaxf(x, y);
    x = lo;
    y = hi;
}
// the median of seven by a 13-exchange selection network, in registers
__device__ __forceinline__ float median7(float v0, float v1, float v2, float v3, float v4, float v5, float v6) {
    cswap(v0, v5); cswap(v0, v3); cswap(v1, v6); cswap(v2, v4); cswap(v0, v1); cswap(v3, v5); cswap(v2, v6);
    cswap(v2, v3); cswap(v3, v6); cswap(v4, v5); cswap(v1, v4); cswap(v1, v3); cswap(v3, v4);
    return v3;
}

// m[b][r][s] = mean over the heads, in head order, of the width-7 median along s (reflect padding;
// none for M <= 3) of z = (p - mean) / std (0 where std == 0).  One workgroup per (column tile, row,
// sequence): thread i holds z of column c0 - 3 + i of one head in LDS (two images, one barrier a head).
__global__ __launch_bounds__(kNormThreads) void align_median_kernel(const float* p, const float* stat, int A, int N_cap,
                                                                    int M_cap, const int* Ns, const int* Ms, float* m) {
    __shared__ float s_z[2][kNormThreads];
    const int b = blockIdx.z, r = blockIdx.y, c0 = blockIdx.x * kMedTile, i = threadIdx.x;
    const int N = min(Ns[b], N_cap), M = min(Ms[b], M_cap);
    if (r >= N || c0 >= M) return;  // (uniform)
    int j = c0 - 3 + i;             // this thread's column, reflected into [0, M)
    if (j < 0) j = -j;
    if (j >= M) j = 2 * (M - 1) - j;
    j = max(0, min(j, M - 1));
    const bool filt = M > 3;
    const int s = c0 + i - 3;
    const bool writes = i >= 3 && i < 3 + kMedTile && s < M;
    double acc = 0.0;
    for (int a = 0; a < A; ++a) {
        const size_t ba = (size_t)b * A + a;
        const float pv = p[(ba * N_cap + r) * M_cap + j];
        const float mean = stat[ba * 2 * M_cap + j], sd = stat[ba * 2 * M_cap + M_cap + j];
        const float z = sd > 0.0f ? (pv - mean) / sd : 0.0f;
        float* img = s_z[a & 1];
        img[i] = z;
        __syncthreads();
        if (writes)
            acc += (double)(filt ? median7(img[i - 3], img[i - 2], img[i - 1], z, img[i + 1], img[i + 2], img[i + 3]) : z);
    }
    if (writes) m[((size_t)b * N_cap + r) * M_cap + s] = (float)(acc / A);
}

// ------------------------------------------------------------------ align_dtw
// One workgroup per sequence; thread i - 1 owns text row i of the (N + 1) x (M + 1) cost grid and
// walks it along the anti-diagonals d = i + j, one barrier per diagonal.  cost(i, j - 1) stays in a
// register, cost(i - 1, j) comes from the neighbour through LDS, cost(i - 1, j - 1) is what that read
// returned one diagonal earlier.  The step taken is packed at 2 bits per cell into the row's own LDS
// words, so the backtrace (lane 0) never leaves the CU.  Recurrence and tie rule are the reference's:
// step 0 only if c0 < c1 && c0 < c2, step 1 only if c1 < c0 && c1 < c2, else step 2 at cost c2.
__global__ __launch_bounds__(kDtwThreads) void align_dtw_kernel(const float* m, int N_cap, int M_cap, const int* Ns,
                                                                const int* Ms, int* jump, int* len, int* path) {
    extern __shared__ __attribute__((aligned(16))) unsigned s_dtw[];
    float* cbuf = (float*)s_dtw;                     // [2][kDtwCostStride]: cost of row i on the last two diagonals
    unsigned* tr = s_dtw + 2 * kDtwCostStride;       // [N_cap][W]: 16 cells per word
    const int W = (M_cap + 15) / 16;
    const int b = blockIdx.x, tid = threadIdx.x, i = tid + 1;
    const int N = min(min(Ns[b], N_cap), kDtwThreads), M = min(Ms[b], M_cap);
    if (N < 1 || M < 1) {  // (uniform)
        if (tid == 0) len[b] = 0;
        return;
    }
    if (tid == 0) cbuf[0] = cbuf[kDtwCostStride] = INFINITY;  // row 0: cost(0, j >= 1)
    const float* mrow = m + ((size_t)b * N_cap + (tid < N ? tid : 0)) * M_cap;
    // the row's values, 8 columns at a time, the next 8 in flight (M_cap is a multiple of 8)
    float4 cur0, cur1, nxt0 = *(const float4*)mrow, nxt1 = *(const float4*)(mrow + 4);
    cur0 = nxt0;
    cur1 = nxt1;
    float c0 = i == 1 ? 0.0f : INFINITY, c2 = INFINITY;
    unsigned bits = 0;
    __syncthreads();
    for (int d = 2; d <= N + M; ++d) {
        const int j = d - i;
        if (tid < N && j >= 1 && j <= M) {
            const int jj = j - 1;
            if ((jj & 7) == 0) {
                cur0 = nxt0;
                cur1 = nxt1;
                if (jj + 8 < M_cap) {
                    nxt0 = *(const float4*)(mrow + jj + 8);
                    nxt1 = *(const float4*)(mrow + jj + 12);
                }
            }
            const float4 q = (jj & 4) ? cur1 : cur0;
            const float mv = (jj & 2) ? ((jj & 1) ? q.w : q.z) : ((jj & 1) ? q.y : q.x);
            const float c1 = cbuf[((d - 1) & 1) * kDtwCostStride + i - 1];
            float c;
            unsigned t;
            if (c0 < c1 && c0 < c2) {
                c = c0; t = 0u;
            } else if (c1 < c0 && c1 < c2) {
                c = c1; t = 1u;
            } else {
                c = c2; t = 2u;
            }
            c = -mv + c;
            cbuf[(d & 1) * kDtwCostStride + i] = c;
            bits |= t << (2 * (jj & 15));
            if ((jj & 15) == 15 || j == M) {
                tr[(size_t)tid * W + (jj >> 4)] = bits;
                bits = 0;
            }
            c0 = c1;
            c2 = c;
        }
        __syncthreads();
    }
    if (tid != 0) return;
    // the reference's backtrace: trace(0, j) = 2, trace(i, 0) = 1
    int bi = N, bj = M, n = 0;
    int* pth = path ? path + (size_t)b * (N_cap + M_cap) : nullptr;
    int* jmp = jump + (size_t)b * N_cap;
    while (bi > 0 || bj > 0) {
        if (pth) pth[n] = (int)(((unsigned)(bi - 1) << 16) | ((unsigned)(bj - 1) & 0xFFFFu));
        ++n;
        unsigned t;
        if (bi == 0) t = 2u;
        else if (bj == 0) t = 1u;
        else {
            jmp[bi - 1] = bj - 1;  // backwards along the path: the last write is the row's first frame
            t = (tr[(size_t)(bi - 1) * W + ((bj - 1) >> 4)] >> (2 * ((bj - 1) & 15))) & 3u;
        }
        if (t == 0u) { --bi; --bj; }
        else if (t == 1u) --bi;
        else --bj;
    }
    len[b] = n;
}

size_t dtw_lds_bytes(int N_cap, int M_cap) {
    return ((size_t)2 * kDtwCostStride + (size_t)N_cap * ((M_cap + 15) / 16)) * sizeof(unsigned);
}

}  // namespace

void align_qk(int dtype, const AlignQkArgs& a, int B, hipStream_t st) {
    if (a.Tq < 1 || a.Tq > 4) throw std::runtime_error("align_qk: 1..4 queries per sequence");
    if (B < 1 || a.n_heads < 1 || a.pos0 + a.Tq <= 0) return;  // (a pass wholly before row 0)
    if (a.T_enc < 1 || a.T_enc > kAlignMaxKeys) throw std::runtime_error("align_qk: 1..3072 keys");
    if (a.pos0 + a.Tq > a.N_cap) throw std::runtime_error("align_qk: rows beyond the workspace");
    if (a.a0 < 0 || a.a0 + a.n_heads > a.A) throw std::runtime_error("align_qk: heads beyond the workspace");
    if (B > 65535) throw std::runtime_error("align_qk: B <= 65535 (grid y)");
    const int T32 = (a.T_enc + 31) / 32 * 32;
    const size_t lds = (size_t)a.Tq * T32 * sizeof(float);  // <= 48 KiB
    const dim3 grid(a.n_heads, B);
    if (dtype == DT_F32) align_qk_kernel<float><<<grid, kQkThreads, lds, st>>>(a);
    else if (dtype == DT_BF16) align_qk_kernel<bf16><<<grid, kQkThreads, lds, st>>>(a);
    else if (dtype == DT_F16) align_qk_kernel<f16><<<grid, kQkThreads, lds, st>>>(a);
    else throw std::runtime_error("align_qk: dtype is f32, bf16 or f16");
    SPT_LAUNCH_CHECK();
}

void align_norm(const float* p, int B, int A, int N_cap, int M_cap, const int* N, const int* M, float* stat, float* m,
                hipStream_t st) {
    if (B < 1) return;
    if (A < 1 || N_cap < 1 || M_cap < 1) throw std::runtime_error("align_norm: need A, N_cap, M_cap >= 1");
    if (A > 65535 || N_cap > 65535 || B > 65535) throw std::runtime_error("align_norm: A, N_cap, B <= 65535 (grid y / z)");
    align_stat_kernel<<<dim3(cdiv(M_cap, kNormThreads), A, B), kNormThreads, 0, st>>>(p, A, N_cap, M_cap, N, M, stat);
    SPT_LAUNCH_CHECK();
    align_median_kernel<<<dim3(cdiv(M_cap, kMedTile), N_cap, B), kNormThreads, 0, st>>>(p, stat, A, N_cap, M_cap, N, M, m);
    SPT_LAUNCH_CHECK();
}

void align_prepare(int N_cap, int M_cap) {
    if (N_cap < 1 || N_cap > kAlignMaxRows || M_cap < 8 || M_cap % 8 || dtw_lds_bytes(N_cap, M_cap) > 160 * 1024)
        throw std::runtime_error("align_dtw: N_cap 1..256, M_cap a multiple of 8, trace within 160 KiB of LDS");
    ensure_lds_attr((const void*)align_dtw_kernel, 160 * 1024);  // one value: contexts of several sizes share it
}

void align_dtw(const float* m, int B, int N_cap, int M_cap, const int* N, const int* M, int* jump, int* len, int* path,
               hipStream_t st) {
    if (B < 1) return;
    align_prepare(N_cap, M_cap);
    align_dtw_kernel<<<B, kDtwThreads, dtw_lds_bytes(N_cap, M_cap), st>>>(m, N_cap, M_cap, N, M, jump, len, path);
    SPT_LAUNCH_CHECK();
}

}  // namespace spt
