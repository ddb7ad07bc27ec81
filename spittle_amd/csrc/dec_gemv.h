// dec_gemv.h -- the decoder's GEMV: body, kernel, launch geometry.  Included by k_dec.hip (weights in
// the engine dtype: QW = false) and by k_dec_q.hip (QW = true: a matrix resident in its packed ggml
// blocks, ggml_qpack.h, dequantised in registers).  The two differ in the weight fetch alone: the K
// order, the MFMA sequence, the reductions, prologues, epilogues and the geometry chosen per shape
// are one text, so a row's result is bitwise the same from either.
#pragma once
#include "common.h"
#include "ggml_qpack.h"
#include "kernels.h"

#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <type_traits>

#ifndef SPT_STAMP
#define SPT_STAMP 0
#endif

namespace spt {
namespace {

// ------------------------------------------------------------------ GEMV
template <typename T> struct GV;
template <> struct GV<bf16> {
    static constexpr int KS = 128;  // K per super-step: 4 lane groups x 32 elements
    typedef bf16x8 frag;
};
template <> struct GV<f16> {
    static constexpr int KS = 128;  // bf16's geometry: 4 lane groups x 32 elements
    typedef f16x8 frag;
};
template <> struct GV<float> {
    static constexpr int KS = 64;   // 4 lane groups x 16 elements
    typedef f32x4 frag;
};

constexpr int GV_LDS_BYTES = 98304;  // LN image budget: rows x (K + pad) x sizeof(T)
__host__ __device__ inline int gv_img_bytes(int R, int K, int esz) {
    return ((R * (K + 16 / esz) * esz) + 15) & ~15;
}

struct alignas(16) TopP { float v1; int i1; float v2; int pad; };
__device__ __forceinline__ TopP top_merge(TopP a, TopP b) {
    const bool aw = (a.v1 > b.v1) || (a.v1 == b.v1 && a.i1 < b.i1);
    TopP r;
    r.pad = 0;
    if (aw) { r.v1 = a.v1; r.i1 = a.i1; r.v2 = fmaxf(a.v2, b.v1); }
    else { r.v1 = b.v1; r.i1 = b.i1; r.v2 = fmaxf(b.v2, a.v1); }
    return r;
}
__device__ __forceinline__ TopP top_shfl(TopP t, int mask) {
    TopP u;
    u.v1 = __shfl_xor(t.v1, mask, 64);
    u.i1 = __shfl_xor(t.i1, mask, 64);
    u.v2 = __shfl_xor(t.v2, mask, 64);
    u.pad = 0;
    return u;
}

// weight loads: default cache policy. Non-temporal (SPT_GV_NT=1) measured slower on MI355X
// (r1 ubench: logits 36.8 -> 58.6 us, one decoder layer 59.6 -> 76.9 us)
#ifndef SPT_GV_NT
#define SPT_GV_NT 0
#endif
template <typename F>
__device__ __forceinline__ F load_w(const F* p) {
#if SPT_GV_NT
    return __builtin_nontemporal_load(p);
#else
    return *p;
#endif
}

// NWV waves; CT column tiles of 16 per workgroup; KSPLIT = NWV / CT waves share a tile
// and split its K.  Each wave keeps up to MAXJ super-steps of weights in flight.
// blockIdx.y splits K across workgroups (GV_PARTIAL only: each split writes its own
// partial slab, summed in split order by the consumer's A_LN prologue).
// ASRC selects the A operand:
//   A_DIRECT  activation rows [R][lda] of type T read straight into MFMA fragments;
//   A_LN      LayerNorm of the f32 residual rows x + pend[0..np-1] (the pending partial slabs
//             of the previous GV_PARTIAL launch), staged as a bank-padded LDS image;
//             workgroup (0, 0) also writes the combined rows to x_out;
//   A_ATTN    the cross-attention output merged from its S key-chunk partials
//             [R][H][S][66] = {o[64], m, l} (rows of this workgroup's K range), staged in LDS.
// kernel-side A source codes: A_DIRECT, LN_SRC(np) = A_LN with np pending slabs (0, 1, 2, 4), or
// ATTN_SRC(s) = A_ATTN combining s cross-attention key chunks
constexpr int LN_SRC(int np) { return 16 + np; }
constexpr bool is_ln(int asrc) { return asrc >= 16 && asrc < 32; }
constexpr int ln_np(int asrc) { return asrc - 16; }
constexpr int ATTN_SRC(int s) { return 32 + s; }
constexpr bool is_attn(int asrc) { return asrc >= 32; }
constexpr int attn_s(int asrc) { return asrc - 32; }

// developer timeline (SPT_STAMP=1 builds): thread 0's view of its workgroup's start / end
#define GV_STAMP(i)                                                                                       \
    do {                                                                                                  \
        if (SPT_STAMP && a.stamp && threadIdx.x == 0)                                                     \
            a.stamp[2 * (blockIdx.x + blockIdx.y * gridDim.x) + (i)] = __builtin_amdgcn_s_memrealtime(); \
    } while (0)

// The body is a device function so that the fused cross-Q + cross-attention launch (xq_fused_kernel)
// runs the stand-alone kernel's instructions in its producer workgroups.  PUB (GV_BIAS only): each
// output element is also published to the launch's consumers as an 8-byte granule {tag, the
// element's stored bits} at gran[row * N + n], one relaxed agent-scope (write-through) store.
//
// QW: W is a packed quantised matrix of type a.wq (wave-uniform, read at run time: one kernel per
// configuration serves every resident type).  A lane fetches, per super-step, the 32 nibble bytes it
// shares with lane group fq ^ 2, its dword of fifth bits and the 4 scales and minima of the row's 4
// blocks -- 52 bytes in 5 aligned loads, all of them unconditional where the plain kernel's are -- and
// converts block i into the fragment of MFMA step i just before that step.  Each element is
// from_f<T>(gq_dequant_elem(..)): the bits dequant_kernel<T> stores for it at load.
struct QRaw {      // one super-step of one lane, as fetched
    uint4 nib[2];  // blocks 0, 1 | 2, 3: two dwords (8 bytes) each
    uint32_t qh;   // byte i: the fifth bits of the lane's 8 elements of block i
    uint2 d, m;    // 4 x f16 each
};

// f16 bits -> f32 (exact).  The hardware conversion differs from gq_half in one thing: it sets a
// signalling NaN's quiet bit, which the product of gq_dequant_elem does to its result either way.
__device__ __forceinline__ float q_half(uint32_t bits16) {
    return (float)__builtin_bit_cast(_Float16, (unsigned short)bits16);
}

template <typename T>
__device__ __forceinline__ typename GV<T>::frag q_convert(const QRaw& r, int i, int fq, const QPackGeom& g) {
    const uint32_t lo = i & 1 ? r.nib[i >> 1].z : r.nib[i >> 1].x, hi = i & 1 ? r.nib[i >> 1].w : r.nib[i >> 1].y;
    const int sh = fq < 2 ? 0 : 4;
    const uint32_t hb = (r.qh >> (8 * i)) & 0xffu;
    const uint32_t dd = i < 2 ? r.d.x : r.d.y, mm = i < 2 ? r.m.x : r.m.y;
    const float d = q_half((dd >> (16 * (i & 1))) & 0xffffu), m = q_half((mm >> (16 * (i & 1))) & 0xffffu);
    typename GV<T>::frag f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const uint32_t w = e < 4 ? lo : hi;
        const int x = (int)(((w >> (8 * (e & 3) + sh)) & 0xfu) | (((hb >> e) << 4) & (uint32_t)g.q5));
        const T t = from_f<T>(gq_dequant_elem(x, g.sub, d, g.has_m != 0, m));
        if constexpr (std::is_same<T, f16>::value) f[e] = t;
        else f[e] = (short)t;
    }
    return f;
}

template <typename T, int MODE, int ASRC, int RG, int NWV, int CT, int MAXJ, bool EXACT = false, bool PUB = false,
          bool QW = false>
__device__ __forceinline__ void gemv_body(const GemvArgs& a, unsigned long long* gran = nullptr, unsigned tag = 0) {
    static_assert(!PUB || (MODE == GV_BIAS && sizeof(T) == 2), "gemv: granules carry one 16-bit GV_BIAS element");
    static_assert(!QW || sizeof(T) == 2, "gemv: resident quantised weights are the 16-bit engines'");
    GV_STAMP(0);
    constexpr int KS = GV<T>::KS;
    constexpr int CPE = 16 / sizeof(T);  // elements per 16-byte chunk
    constexpr int KSPLIT = NWV / CT;
    constexpr bool IMG = ASRC != A_DIRECT;
    typedef typename GV<T>::frag frag;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int fr = lane & 15, fq = lane >> 4;
    const int ct = wid % CT, ks = wid / CT;
    const int tile = blockIdx.x * CT + ct;
    const int n0 = tile * 16;
    const int K = a.K;
    const int lds_ld = K + CPE;  // padded row stride (elements): rows land 4 banks apart
    // K split across the grid's y dimension: this workgroup owns super-steps [ss0, ss1)
    const int kz = blockIdx.y, kzc = gridDim.y;
    const int nss_all = K / KS, per = (nss_all + kzc - 1) / kzc;
    const int ss0 = kz * per, ss1 = min(nss_all, ss0 + per);
    // K order inside a super-step: MFMA step i, lane group fq takes the 16-byte chunk 4 i + fq,
    // so the four lanes of a weight row read 64 contiguous bytes per load instruction (16 rows x
    // 64 B per wave-instruction instead of 64 scattered 16-byte pieces); A uses the same order
    const T* wrow = (const T*)a.W + (size_t)min(n0 + fr, a.N - 1) * K + fq * CPE;
    // QW: the row's records, one per super-step (the same row clamp, so every lane reads inside W)
    QPackGeom qg{};
    const uint8_t* qrow = nullptr;
    if constexpr (QW) {
        qpack_geom(a.wq, &qg);
        qrow = (const uint8_t*)a.W + (size_t)min(n0 + fr, a.N - 1) * nss_all * qg.rec;
    }

    typename std::conditional<QW, QRaw, frag>::type w[MAXJ][QW ? 1 : 4];
    // EXACT (every wave's K slice is exactly MAXJ super-steps, checked at launch): the weight
    // loads are unconditional, so the compiler can wait for the LayerNorm rows and prefetched
    // operands (issued before them) with a counted vmcnt that leaves the weight stream in flight.
    // Otherwise a predicated load makes every such wait a vmcnt(0) (r2: the LayerNorm then ran
    // only after the weights had landed); forcing unconditional loads there instead (waves
    // re-reading a super-step) measured slower (r2 exp_r2c).
    auto load_chunk = [&](int j0) {
#pragma unroll
        for (int j = 0; j < MAXJ; ++j) {
            const int ss = ss0 + ks + (j0 + j) * KSPLIT;
            if (EXACT || ss < ss1) {
                if constexpr (QW) {
                    const uint8_t* r = qrow + (size_t)ss * qg.rec;
                    w[j][0].nib[0] = load_w((const uint4*)(r + 32 * (fq & 1)));
                    w[j][0].nib[1] = load_w((const uint4*)(r + 32 * (fq & 1) + 16));
                    w[j][0].qh = load_w((const uint32_t*)(r + qg.off_qh + 4 * fq));
                    w[j][0].d = load_w((const uint2*)(r + qg.off_d));
                    w[j][0].m = load_w((const uint2*)(r + qg.off_m));
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) w[j][i] = load_w((const frag*)(wrow + (size_t)ss * KS + i * 4 * CPE));
                }
            }
        }
    };
    // LayerNorm input rows (x and the pending slabs) are fetched BEFORE the weight stream:
    // loads retire in issue order, so the prologue then waits only for its own row.  The slab
    // count is a template constant: loads under a runtime select are serialised by hipcc.
    constexpr int NP = is_ln(ASRC) ? ln_np(ASRC) : 0;
    float4 x0[NP + 1][6];
    if constexpr (is_ln(ASRC)) {
        if (wid < a.R) {
            const size_t ro = (size_t)wid * a.lda + a.a_row0;
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                const int k = lane * 4 + 256 * i;
                if (k < K) {
                    x0[0][i] = *(const float4*)((const float*)a.A + ro + k);
#pragma unroll
                    for (int p = 0; p < NP; ++p) x0[p + 1][i] = *(const float4*)(a.pend[p] + ro + k);
                }
            }
        }
    }
    // Every operand of the LayerNorm and of the epilogue is fetched here, up front, beside the
    // LayerNorm rows and before the weight stream: a workgroup then pays one memory round trip
    // (kernel arguments aside) instead of one per dependent stage (r2 chain timeline: the
    // epilogue's bias / residual loads and the LayerNorm's gain / shift loads were each a round
    // trip after the weights had arrived).
    const int n_ep = n0 + fr;  // the output column this lane finishes
    const bool ep_lane = ks == 0 && n_ep < a.N;
    float bias_pre = 0.f;
    if constexpr (MODE != GV_LOGITS) {
        if (ep_lane && a.bias && kz == 0) bias_pre = a.bias[n_ep];
    }
    float resid_pre[RG][4];
    // GV_PARTIAL with p_resid: split 0 adds the residual rows into its slab, so the consumer's
    // prologue sums one slab fewer (x + p0 is formed here instead of there: the same operation)
    const float* resid = MODE == GV_BIAS_RESID ? (const float*)a.C
                         : MODE == GV_PARTIAL && kz == 0 ? a.p_resid : nullptr;
    if constexpr (MODE == GV_BIAS_RESID || MODE == GV_PARTIAL) {
#pragma unroll
        for (int g = 0; g < RG; ++g)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = g * 16 + 4 * fq + r;
                resid_pre[g][r] = (resid && ep_lane && row < a.R) ? resid[(size_t)row * a.ldc + n_ep] : 0.f;
            }
    }
    int st_pre = 0;  // decoder step state: GV_QKV_CACHE appends at pos0, GV_LOGITS reads step
    if constexpr (MODE == GV_QKV_CACHE) st_pre = a.st->pos0;
    if constexpr (MODE == GV_LOGITS) st_pre = a.st->step;
    uint32_t sup_pre = 0;
    if constexpr (MODE == GV_LOGITS) {
        if (n_ep < a.N) sup_pre = a.suppress[n_ep >> 5];
    }
    float4 lnw_pre[6], lnb_pre[6];
    if constexpr (is_ln(ASRC)) {
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const int k = lane * 4 + 256 * i;
            if (k < K) {
                lnw_pre[i] = *(const float4*)(a.ln_w + k);
                lnb_pre[i] = *(const float4*)(a.ln_b + k);
            }
        }
    }
    load_chunk(0);  // the first weight fetch overlaps the prologue

    if constexpr (is_ln(ASRC)) {
        T* img = (T*)smem;
        const bool wr_x = a.x_out && blockIdx.x == 0 && blockIdx.y == 0;
        for (int r = wid; r < a.R; r += NWV) {
            const size_t ro = (size_t)r * a.lda + a.a_row0;
            float4 v[6];
            float s = 0.f;
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                const int k = lane * 4 + 256 * i;
                if (k < K) {
                    float4 u[NP + 1];
                    if (r == wid) {
#pragma unroll
                        for (int p = 0; p <= NP; ++p) u[p] = x0[p][i];
                    } else {
                        u[0] = *(const float4*)((const float*)a.A + ro + k);
#pragma unroll
                        for (int p = 0; p < NP; ++p) u[p + 1] = *(const float4*)(a.pend[p] + ro + k);
                    }
                    // x + p0 + p1 + ..., always in this order (deterministic)
                    v[i] = u[0];
#pragma unroll
                    for (int p = 1; p <= NP; ++p) {
                        v[i].x += u[p].x; v[i].y += u[p].y; v[i].z += u[p].z; v[i].w += u[p].w;
                    }
                    if (wr_x) *(float4*)(a.x_out + ro + k) = v[i];
                    s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
                }
            }
            const float mean = wave_sum(s) / (float)K;
            float s2 = 0.f;
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                const int k = lane * 4 + 256 * i;
                if (k < K) {
                    s2 += ln_sq4(v[i], mean);
                }
            }
            const float rstd = 1.0f / sqrtf(wave_sum(s2) / (float)K + 1e-5f);
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                const int k = lane * 4 + 256 * i;
                if (k < K) {
                    const float4 g = lnw_pre[i];
                    const float4 b = lnb_pre[i];
                    T* o = img + (size_t)r * lds_ld + k;
                    o[0] = from_f<T>(ln_out(v[i].x, mean, rstd, g.x, b.x));
                    o[1] = from_f<T>(ln_out(v[i].y, mean, rstd, g.y, b.y));
                    o[2] = from_f<T>(ln_out(v[i].z, mean, rstd, g.z, b.z));
                    o[3] = from_f<T>(ln_out(v[i].w, mean, rstd, g.w, b.w));
                }
            }
        }
        __syncthreads();
    }

    if constexpr (is_attn(ASRC)) {
        // flash-decoding merge of the S chunks: heads covering this workgroup's K range;
        // thread <-> (row r, head h, element e)
        constexpr int S = attn_s(ASRC);
        SPT_LDS T* img = (SPT_LDS T*)smem;  // LDS-typed: the stores cannot alias the partials' loads
        const int H = a.a_heads;
        const int h0 = (ss0 * KS) >> 6, h1 = min(H, (ss1 * KS + 63) >> 6);
        const int nh = h1 - h0;
        const int total = a.R * nh * 64;
        // one element per thread per round: the engine takes this prologue for one row only (B = 1:
        // 1280 elements over 512 threads); several rows merge once in attn_part_merge_kernel (r4:
        // batching four elements per round here cost the one-row pass 1.5 %, 189 VGPRs)
        for (int idx = tid; idx < total; idx += 64 * NWV) {
            const int r = idx / (nh * 64), rem = idx - r * nh * 64;
            const int h = h0 + (rem >> 6), e = rem & 63;
            const float* pp = a.apart + ((size_t)r * H + h) * S * 66;
            float mc[S], lc[S], oc[S];
#pragma unroll
            for (int c = 0; c < S; ++c) {
                mc[c] = pp[c * 66 + 64];
                lc[c] = pp[c * 66 + 65];
                oc[c] = pp[c * 66 + e];
            }
            float M = mc[0];
#pragma unroll
            for (int c = 1; c < S; ++c) M = fmaxf(M, mc[c]);
            float L = 0.f, O = 0.f;
#pragma unroll
            for (int c = 0; c < S; ++c) {  // attn_merge's operations (bitwise): skip empty chunks
                if (mc[c] == -INFINITY) continue;
                const float f = exp2f(mc[c] - M);
                L = __builtin_fmaf(lc[c], f, L);
                O = __builtin_fmaf(oc[c], f, O);
            }
            img[(size_t)r * lds_ld + h * 64 + e] = from_f<T>(O / L);
        }
        __syncthreads();
    }

    f32x4 acc[RG];
#pragma unroll
    for (int g = 0; g < RG; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
    auto compute_chunk = [&](int j0) {
#pragma unroll
        for (int j = 0; j < MAXJ; ++j) {
            const int ss = ss0 + ks + (j0 + j) * KSPLIT;
            if (!EXACT && ss >= ss1) break;
            const int kb = ss * KS + fq * CPE;
            frag wf[4];  // the B fragments of this super-step's four MFMA steps
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if constexpr (QW) wf[i] = q_convert<T>(w[j][0], i, fq, qg);
                else wf[i] = w[j][i];
            }
#pragma unroll
            for (int g = 0; g < RG; ++g) {
                const int row = g * 16 + fr;
                frag af[4];
                if (row < a.R) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        if constexpr (IMG)
                            af[i] = *(const frag*)((const T*)smem + (size_t)row * lds_ld + kb + i * 4 * CPE);
                        else
                            af[i] = *(const frag*)((const T*)a.A + (size_t)row * a.lda + a.a_row0 + kb + i * 4 * CPE);
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) af[i] = frag{};
                }
                if constexpr (std::is_same<T, f16>::value) {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[i], wf[i], acc[g], 0, 0, 0);
                } else if constexpr (sizeof(T) == 2) {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], wf[i], acc[g], 0, 0, 0);
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i][e], wf[i][e], acc[g], 0, 0, 0);
                }
            }
        }
    };
    if constexpr (EXACT) {
        compute_chunk(0);
    } else {
        for (int j0 = 0; ss0 + ks + j0 * KSPLIT < ss1; j0 += MAXJ) {
            if (j0 > 0) load_chunk(j0);
            compute_chunk(j0);
        }
    }

    // cross-wave K reduction (waves sharing a column tile)
    if constexpr (KSPLIT > 1) {
        f32x4* red = (f32x4*)(smem + (IMG ? gv_img_bytes(a.R, K, sizeof(T)) : 0));
        if (IMG) __syncthreads();  // the image region is not reused, but keep waves in step
#pragma unroll
        for (int g = 0; g < RG; ++g) red[(wid * RG + g) * 64 + lane] = acc[g];
        __syncthreads();
        if (ks != 0) return;
#pragma unroll
        for (int g = 0; g < RG; ++g) {
            f32x4 v = acc[g];
#pragma unroll
            for (int s = 1; s < KSPLIT; ++s) v += red[(((s * CT) + ct) * RG + g) * 64 + lane];
            acc[g] = v;
        }
    }
    const int n = n0 + fr;
    if constexpr (MODE == GV_LOGITS) {
        // logits + this tile's suppressed top-2 per row (finished by dec_finalize)
        const int step = st_pre;
        const bool nvalid = n < a.N;
        bool sup = !nvalid;
        if (nvalid) {
            sup = (sup_pre >> (n & 31)) & 1u;
            if (step == 0 && (n == a.blank0 || n == a.blank1)) sup = true;
        }
#pragma unroll
        for (int g = 0; g < RG; ++g) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = g * 16 + 4 * fq + r;
                const float v = acc[g][r];
                if (nvalid && row < a.R) ((float*)a.C)[(size_t)row * a.ldc + n] = v;
                TopP t{sup ? -INFINITY : v, nvalid ? n : 0x7fffffff, -INFINITY, 0};
                t = top_merge(t, top_shfl(t, 1));
                t = top_merge(t, top_shfl(t, 2));
                t = top_merge(t, top_shfl(t, 4));
                t = top_merge(t, top_shfl(t, 8));
                if (fr == 0 && row < a.R && tile < a.n_tiles) ((TopP*)a.part)[(size_t)row * a.n_tiles + tile] = t;
            }
        }
        GV_STAMP(1);
        return;
    }
    if (n >= a.N) return;
    const float bv = bias_pre;
#pragma unroll
    for (int g = 0; g < RG; ++g) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = g * 16 + 4 * fq + r;
            if (row >= a.R) continue;
            const float y = acc[g][r] + bv;
            if constexpr (MODE == GV_BIAS) {
                const T yt = from_f<T>(y);
                ((T*)a.C)[(size_t)row * a.ldc + n] = yt;
                if constexpr (PUB) {
                    unsigned short bits;
                    __builtin_memcpy(&bits, &yt, 2);
                    __hip_atomic_store(gran + (size_t)row * a.N + n, ((unsigned long long)tag << 32) | bits,
                                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            } else if constexpr (MODE == GV_BIAS_GELU) {
                ((T*)a.C)[(size_t)row * a.ldc + n] = from_f<T>(gelu_tanh(y));
            } else if constexpr (MODE == GV_PARTIAL) {
                ((float*)a.C + (size_t)kz * a.c_split)[(size_t)row * a.ldc + n] = resid ? resid_pre[g][r] + y : y;
            } else if constexpr (MODE == GV_BIAS_RESID) {
                ((float*)a.C)[(size_t)row * a.ldc + n] = resid_pre[g][r] + y;
            } else if constexpr (MODE == GV_QKV_CACHE) {
                const int d = a.cache_H * 64;
                if (n < d) {
                    ((T*)a.C)[(size_t)row * a.ldc + n] = from_f<T>(y);
                } else {
                    const int part = n / d - 1;  // 0 = K, 1 = V
                    const int rem = n - (part + 1) * d;
                    const int hh = rem >> 6, e = rem & 63;
                    const int bb = row / a.Tq, t = row - bb * a.Tq;
                    const int pos = st_pre + t;
                    const size_t off = ((((size_t)part * a.cache_B + bb) * a.cache_H + hh) * a.cache_ctx + pos) * 64 + e;
                    ((T*)a.cache)[off] = to_cache<T>(y);
                }
            }
        }
    }
    GV_STAMP(1);
}

// the weight format of this translation unit's kernels and launchers: k_dec_q.hip defines SPT_GEMV_QW 1
#ifndef SPT_GEMV_QW
#define SPT_GEMV_QW 0
#endif
constexpr bool GV_QW = SPT_GEMV_QW != 0;

template <typename T, int MODE, int ASRC, int RG, int NWV, int CT, int MAXJ, bool EXACT = false, bool QW = GV_QW>
__global__ __launch_bounds__(64 * NWV) void gemv_kernel(GemvArgs a) {
    gemv_body<T, MODE, ASRC, RG, NWV, CT, MAXJ, EXACT, false, QW>(a);
}

template <typename T, int MODE, int ASRC, int RG, int NWV, int CT, int MAXJ, bool EXACT = false>
void gemv_attr() {  // per kernel and device (ensure_lds_attr)
    const int red = NWV * RG * 64 * (int)sizeof(f32x4);
    ensure_lds_attr((const void*)gemv_kernel<T, MODE, ASRC, RG, NWV, CT, MAXJ, EXACT>, GV_LDS_BYTES + red);
}

template <typename T, int MODE, int ASRC, int RG, int NWV, int CT, int MAXJ, bool EXACT = false>
void gemv_launch_cfg(const GemvArgs& a, hipStream_t st) {
    if (EXACT && cdiv(a.K / GV<T>::KS, a.ksplit) != MAXJ * (NWV / CT))
        throw std::runtime_error("gemv: exact configuration does not match the K slice");
    const int red = NWV * RG * 64 * (int)sizeof(f32x4);
    const int lds = (ASRC != A_DIRECT ? gv_img_bytes(a.R, a.K, sizeof(T)) : 0) + (NWV / CT > 1 ? red : 0);
    hipLaunchKernelGGL((gemv_kernel<T, MODE, ASRC, RG, NWV, CT, MAXJ, EXACT>), dim3(cdiv(a.N, 16 * CT), a.ksplit),
                       dim3(64 * NWV), lds, st, a);
    SPT_LAUNCH_CHECK();
}

// geometry per shape (nss = super-steps of K per workgroup): every wave's whole K slice in
// flight at once where registers allow; logits: 4 column tiles x 1 wave each (4, 4, 4)
#define SPT_GV_CONFIGS(X)   \
    X(4, 1, 2)  /* nss <= 8  */ \
    X(8, 1, 2)  /* nss <= 16 */ \
    X(16, 1, 3) /* nss <= 48 */

// the (mode, A source) pairs the decoder uses
#define SPT_GV_PAIRS(X)                 \
    X(GV_QKV_CACHE, LN_SRC(0))          \
    X(GV_QKV_CACHE, LN_SRC(1))          \
    X(GV_QKV_CACHE, LN_SRC(2))          \
    X(GV_QKV_CACHE, LN_SRC(4))          \
    X(GV_BIAS, LN_SRC(0))               \
    X(GV_BIAS, LN_SRC(2))               \
    X(GV_BIAS_GELU, LN_SRC(0))          \
    X(GV_LOGITS, LN_SRC(0))             \
    X(GV_LOGITS, LN_SRC(1))             \
    X(GV_LOGITS, LN_SRC(2))             \
    X(GV_LOGITS, LN_SRC(4))             \
    X(GV_PARTIAL, A_DIRECT)             \
    X(GV_BIAS_RESID, A_DIRECT)          \
    X(GV_BIAS_RESID, ATTN_SRC(2))       \
    X(GV_BIAS_RESID, ATTN_SRC(3))       \
    X(GV_BIAS_RESID, ATTN_SRC(4))       \
    X(GV_BIAS_RESID, ATTN_SRC(8))

// > 64 KiB of dynamic LDS must be enabled per kernel, outside any stream capture
template <typename T, int MODE, int ASRC>
void gemv_attr_all() {
#define SPT_ATTR(NWV, CT, MAXJ)                          \
    gemv_attr<T, MODE, ASRC, 1, NWV, CT, MAXJ>();         \
    gemv_attr<T, MODE, ASRC, 2, NWV, CT, MAXJ>();         \
    gemv_attr<T, MODE, ASRC, 4, NWV, CT, MAXJ>();
    if constexpr (MODE == GV_LOGITS) {
        SPT_ATTR(4, 4, 4)
        SPT_ATTR(8, 8, 4)
    } else if constexpr (ASRC == A_DIRECT || is_attn(ASRC)) {
        SPT_GV_CONFIGS(SPT_ATTR)
        gemv_attr<T, MODE, ASRC, 1, 12, 1, 1, true>();
        gemv_attr<T, MODE, ASRC, 2, 12, 1, 1, true>();
        gemv_attr<T, MODE, ASRC, 4, 12, 1, 1, true>();
    } else {
        SPT_ATTR(4, 1, 2)
        SPT_ATTR(8, 1, 2)
        SPT_ATTR(8, 2, 3)
        gemv_attr<T, MODE, ASRC, 1, 10, 1, 1, true>();
        gemv_attr<T, MODE, ASRC, 2, 10, 1, 1, true>();
        gemv_attr<T, MODE, ASRC, 4, 10, 1, 1, true>();
        gemv_attr<T, MODE, ASRC, 1, 10, 2, 2, true>();
        gemv_attr<T, MODE, ASRC, 2, 10, 2, 2, true>();
        gemv_attr<T, MODE, ASRC, 4, 10, 2, 2, true>();
        gemv_attr<T, MODE, ASRC, 1, 12, 1, 1, true>();
        gemv_attr<T, MODE, ASRC, 2, 12, 1, 1, true>();
        gemv_attr<T, MODE, ASRC, 4, 12, 1, 1, true>();
    }
#undef SPT_ATTR
}
template <typename T>
void gemv_attr_modes() {
#define SPT_PAIR(M, S) gemv_attr_all<T, M, S>();
    SPT_GV_PAIRS(SPT_PAIR)
#undef SPT_PAIR
}

// The geometry of one launch (host only): waves, column tiles per workgroup, super-steps in flight per
// wave, whether every wave's K slice is exact, the row groups and the dynamic LDS.  esz: the dtype's
// element size (KS = 128 / 64); code: the kernel-side A source; nss = super-steps of K per workgroup.
// Throws where no configuration holds the K slice.  gemv_launch_rg launches what this returns, and
// gemv_plan() (kernels.h) returns it to callers that only ask.
inline GemvPlan gemv_shape(int esz, int mode, int code, int R, int N, int K, int ksplit) {
    GemvPlan p{};
    p.code = code;
    p.rg = R <= 16 ? 1 : R <= 32 ? 2 : 4;
    auto cfg = [&](int nwv, int ct, int maxj, bool exact) {
        p.nwv = nwv; p.ct = ct; p.maxj = maxj; p.exact = exact;
        const int red = nwv * p.rg * 64 * (int)sizeof(f32x4);
        p.lds_bytes = (code != A_DIRECT ? gv_img_bytes(R, K, esz) : 0) + (nwv / ct > 1 ? red : 0);
        p.grid_x = cdiv(N, 16 * ct);
        p.grid_y = ksplit;
        return p;
    };
    const int nss = cdiv(K / (esz == 2 ? 128 : 64), ksplit);  // super-steps per workgroup
    if (mode == GV_LOGITS) {
        // one wave per 16-column tile over all of K either way (bitwise the same logits); wider
        // workgroups stage each LayerNorm image for more tiles (SPT_GV_LOGITS_CT = 4 / 8, r4)
        static const int lct = getenv("SPT_GV_LOGITS_CT") ? atoi(getenv("SPT_GV_LOGITS_CT")) : 4;
        return lct == 8 ? cfg(8, 8, 4, false) : cfg(4, 4, 4, false);
    }
    // Wide LayerNorm-prologue GEMVs (fc1, N = 4d >= 4096): two column tiles per workgroup,
    // so half as many workgroups re-read the residual rows for their LayerNorm image (r1
    // exp23: fc1 9.4 -> 8.6 us, RTFx +1.2 %; the QKV and cross-Q projections lose with it)
    // an attention-merge prologue (A_ATTN) takes A_DIRECT's geometry: the same waves and K
    // slices, so the cross output projection of merged key partials is bitwise the projection
    // of the 8-wave kernel's output (dec_cross_attn_vw)
    if (is_ln(code)) {
        // K = 10 super-steps (large-v3's d = 1280 in bf16): 10 waves, each an exact slice, so
        // the LayerNorm does not wait for the weight stream (GV_EXACT_LN=0 restores r1's shapes)
        static const bool exact_ln = !getenv("GV_EXACT_LN") || atoi(getenv("GV_EXACT_LN")) != 0;
        // SPT_GV_CT2_MIN: the smallest N given two column tiles per workgroup (experiments)
        static const int ct2_min = getenv("SPT_GV_CT2_MIN") ? atoi(getenv("SPT_GV_CT2_MIN")) : 4096;
        if (exact_ln && nss == 10) return N >= ct2_min ? cfg(10, 2, 2, true) : cfg(10, 1, 1, true);
        // K = 12 super-steps (Whisper-small's d = 768 in f32, the C2 decoder): 12 waves, one exact
        // super-step each (experiment; SPT_GV_EXACT12=0: the 8-wave shape)
        static const bool exact12 = !getenv("SPT_GV_EXACT12") || atoi(getenv("SPT_GV_EXACT12")) != 0;
        if (exact_ln && exact12 && nss == 12) return cfg(12, 1, 1, true);
        if (N >= 4096 && nss <= 24) return cfg(8, 2, 3, false);
    } else {
        // the directly-read / attention-merge GEMVs of 12 super-steps (C2's self-out and cross-out) on
        // the same exact 12-wave split (r6ac: pass 0.623 -> 0.618 ms; SPT_GV_EXACT12_DIRECT=0: 8 waves).
        // A_DIRECT and A_ATTN keep one geometry, so the merged-partials projection stays bitwise the
        // merge kernel's
        static const bool exact12_direct = !getenv("SPT_GV_EXACT12_DIRECT") || atoi(getenv("SPT_GV_EXACT12_DIRECT")) != 0;
        if (exact12_direct && nss == 12) return cfg(12, 1, 1, true);
    }
    if (nss <= 8) return cfg(4, 1, 2, false);
    if (nss <= 16) return cfg(8, 1, 2, false);
    // 16 waves: no room for a staged A image's registers
    if (is_ln(code)) throw std::runtime_error("gemv: K too large for a staged A operand");
    if (nss <= 48) return cfg(16, 1, 3, false);
    throw std::runtime_error("gemv: K too large");
}

template <typename T, int MODE, int ASRC, int RG>
void gemv_launch_rg(const GemvArgs& a, hipStream_t st) {
    const GemvPlan p = gemv_shape((int)sizeof(T), MODE, ASRC, a.R, a.N, a.K, a.ksplit);
    // the configurations gemv_shape gives this (mode, A source) class: no other is instantiated
#define SPT_CFG(NWV, CT, MAXJ, EX)                                            \
    if (p.nwv == NWV && p.ct == CT && p.maxj == MAXJ && p.exact == EX) {      \
        gemv_launch_cfg<T, MODE, ASRC, RG, NWV, CT, MAXJ, EX>(a, st);         \
        return;                                                               \
    }
    if constexpr (MODE == GV_LOGITS) {
        SPT_CFG(4, 4, 4, false)
        SPT_CFG(8, 8, 4, false)
    } else {
        if constexpr (is_ln(ASRC)) {
            SPT_CFG(10, 2, 2, true)
            SPT_CFG(10, 1, 1, true)
            SPT_CFG(8, 2, 3, false)
        } else {
            SPT_CFG(16, 1, 3, false)
        }
        SPT_CFG(12, 1, 1, true)
        SPT_CFG(4, 1, 2, false)
        SPT_CFG(8, 1, 2, false)
    }
#undef SPT_CFG
    throw std::runtime_error("gemv: no kernel of the planned geometry");
}

template <typename T, int MODE, int ASRC>
void gemv_launch(const GemvArgs& a, hipStream_t st) {
    if (a.R <= 16) gemv_launch_rg<T, MODE, ASRC, 1>(a, st);
    else if (a.R <= 32) gemv_launch_rg<T, MODE, ASRC, 2>(a, st);
    else gemv_launch_rg<T, MODE, ASRC, 4>(a, st);
}

}  // namespace
}  // namespace spt
