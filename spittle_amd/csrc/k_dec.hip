// k_dec.hip -- the autoregressive decoder step (whisper.cpp whisper_build_graph_decoder
// + whisper_process_logits + greedy whisper_sample_token), entirely on the device:
// no per-step logits copy to the host, the next token is written straight into
// the next step's input, and the per-step state (position, step index) lives in
// device memory so one captured hipGraph replays every step.
//
// At <= 64 rows every projection is a weight stream (HBM-bound), so projections
// are "GEMV" kernels: a workgroup owns 16 x CT output columns; its 4 waves split
// the column tiles and K; each lane streams 64 contiguous bytes of one weight
// row per step straight into registers (two steps in flight, no LDS round trip)
// and the rows x 16 tile is an MFMA (16x16x32 bf16 or f16 / 16x16x4 f32) with the
// activations as the A operand.  A fused pre-LayerNorm is computed once per
// workgroup into a bank-padded LDS image that the MFMA A fragments read;
// bias / GELU / residual / KV-cache append are fused epilogues.
//
// Attention over the caches (self: <= 448 keys, cross: 1500 keys) is a
// flash-decoding kernel: one workgroup of 8 waves per (batch, head), 8 lanes per
// key so every load is a fully coalesced 16-byte-per-lane sweep of the K/V rows,
// online softmax per wave, a one-shot cross-wave merge in LDS.
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

#if SPT_STAMP
// developer timeline of the decode-step cross-attention (SPT_STAMP=1 builds): per workgroup
// {entry, streaming done, exit} in s_memrealtime ticks
__device__ unsigned long long* g_xattn_stamp;
void set_xattn_stamp(void* p) { HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(g_xattn_stamp), &p, sizeof(p))); }
#define XA_STAMP(i)                                                                          \
    do {                                                                                     \
        if (g_xattn_stamp && threadIdx.x == 0)                                               \
            g_xattn_stamp[3 * blockIdx.x + (i)] = __builtin_amdgcn_s_memrealtime();          \
    } while (0)
// and of the fused cross-Q + cross-attention launch: per workgroup {entry, q seen, staged blocks
// ready, streaming done, exit} (producers: entry and exit only), thread 0's view
__device__ unsigned long long* g_xq_stamp;
void set_xq_stamp(void* p) { HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(g_xq_stamp), &p, sizeof(p))); }
#define XQ_STAMP(i)                                                                          \
    do {                                                                                     \
        if (g_xq_stamp && threadIdx.x == 0)                                                  \
            g_xq_stamp[5 * blockIdx.x + (i)] = __builtin_amdgcn_s_memrealtime();             \
    } while (0)
#else
#define XA_STAMP(i) do {} while (0)
#define XQ_STAMP(i) do {} while (0)
#endif

namespace {

// ------------------------------------------------------------------ embed
// QE: the embedding is resident in its packed ggml blocks (emb_q: its type); emb_row_read, ggml_qpack.h
template <typename T, bool QE = false>
__global__ void embed_kernel(const int* __restrict__ tok, int Tq, int d, const T* __restrict__ emb, int emb_q,
                             const float* __restrict__ pos, const DecState* __restrict__ ds, float* __restrict__ x) {
    const int r = blockIdx.x, t = r % Tq;
    const int p = ds->pos0 + t;
    const int tk = tok[r];
    const float* pp = pos + (size_t)p * d;
    for (int i = threadIdx.x; i < d; i += blockDim.x) x[(size_t)r * d + i] = emb_row_read<T, QE>(emb, emb_q, d, tk, i) + pp[i];
}

}  // namespace
}  // namespace spt

// the GEMV body, kernel and launch geometry (shared with k_dec_q.hip, the quantised-weight instances)
#include "dec_gemv.h"
#include "dec_attn.h"

namespace spt {
namespace {

// Self-attention over the cache (keys 0..pos0+t), one workgroup per (b, h).
// q rows: q + (b*Tq + t)*q_ld + h*64; K/V rows of (b, h): base + ((kv*B + b)*H + h)*ctx*64.
template <typename T, int NQ, int NIX = 0>
__global__ __launch_bounds__(64 * AW) void self_attn_kernel(const T* __restrict__ q, int q_ld,
                                                            const T* __restrict__ kv, int B, int H, int ctx, int Tq,
                                                            const DecState* __restrict__ ds, T* __restrict__ out) {
    __shared__ float s_m[AW][NQ], s_l[AW][NQ];
    __shared__ float s_o[AW][NQ][64];
    const int bh = blockIdx.x, b = bh / H, h = bh - b * H;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, g = lane & 7;
    AttnWave<T, NQ, NIX> aw;
    // the wave's first key block is fetched before the position is known (every cache row is
    // readable): the K/V stream no longer waits behind the DecState round trip (run_pre)
    aw.init(kv + (((size_t)0 * B + b) * H + h) * (size_t)ctx * 64 + 8 * g,
            kv + (((size_t)1 * B + b) * H + h) * (size_t)ctx * 64 + 8 * g, ctx, lane);
    aw.load_blk(aw.kc_[0], aw.vc_[0], wid);
    const int pos0 = ds->pos0;
    const int n_keys = pos0 + Tq;
    aw.n_keys = n_keys;
    float qv[NQ][8];
    int lim[NQ];
#pragma unroll
    for (int t = 0; t < NQ; ++t) {
        const int tt = t < Tq ? t : Tq - 1;
        const T* qr = q + (size_t)(b * Tq + tt) * q_ld + h * 64 + 8 * g;
#pragma unroll
        for (int e = 0; e < 8; ++e) qv[t][e] = to_f<T>(qr[e]) * kLog2Scale;
        lim[t] = pos0 + tt + 1;
    }
    aw.template run_pre<(448 / AttnWave<T, NQ, NIX>::KB + 1 + AW - 1) / AW>(wid, cdiv(n_keys, AttnWave<T, NQ, NIX>::KB), qv, lim, Tq);
    aw.to_lds(s_m, s_l, s_o, wid, lane);
    __syncthreads();
    if (tid < 64 * Tq) {
        const int t = tid >> 6, e = tid & 63;
        float M, L, O;
        attn_merge<NQ>(s_m, s_l, s_o, t, e, M, L, O);
        out[(size_t)(b * Tq + t) * (H * 64) + h * 64 + e] = from_f<T>(O / L);
    }
}

// Cross-attention over the cached encoder K/V (all T_enc keys), one workgroup per (row run, h).
// kv: one layer in the kv_offset layout of B_layout windows, at the group's first window (no map)
// or at the layer (kvrow: the window of each run of `share` rows).  A workgroup takes queries
// [blockIdx.y * NQ, + NQ) of its run's share * Tq query rows (rows j * share .. + share - 1, Tq
// each), so the decoders of one utterance (beam / best_of) read its window's K/V once per chunk.
// (A fused LayerNorm + cross-Q projection prologue, every workgroup projecting its own q, and key-chunk
// splits were measured slower on MI355X: r1 exp_fused_xattn_pending_slabs.txt.  xq_fused_kernel below
// fuses the two launches with the projection done once.)
template <typename T, int NQ, bool SPLIT, int NW = AW, int NIX = 0, int PF = 2>
__global__ __launch_bounds__(64 * NW) void cross_attn_kernel(const T* __restrict__ q, const T* __restrict__ kv,
                                                             int B_layout, int H, int T_enc, int Tq,
                                                             T* __restrict__ out, float* __restrict__ part,
                                                             const int* __restrict__ kvrow, int share) {
    typedef AttnWave<T, NQ, NIX, NW, PF> W;
    XA_STAMP(0);
    __shared__ float s_m[NW][NQ], s_l[NW][NQ];
    __shared__ float s_o[NW][NQ][64];
    const int bh = blockIdx.x, j = bh / H, h = bh - j * H;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, g = lane & 7;
    const int nq_all = share * Tq;                          // query rows of this run
    const int c0 = SPLIT ? 0 : (int)blockIdx.y * NQ;        // first query of this workgroup
    const int nq = min(NQ, nq_all - c0);
    const int kb = kvrow ? kvrow[j * share] : j;            // the run's window
    W aw;  // kv_offset layout: 32-key blocks [T/32][B][H][2][32][64]
    const size_t kvo = ((size_t)kb * H + h) * 4096 + 8 * g;
    aw.init(kv + kvo, kv + kvo + 2048, T_enc, lane, (int64_t)B_layout * H * 4096);
    const size_t qrow0 = (size_t)j * nq_all + c0;           // = (j * share) * Tq + c0
    float qv[NQ][8];
    int lim[NQ];
#pragma unroll
    for (int t = 0; t < NQ; ++t) {
        const int tt = t < nq ? t : nq - 1;
        const T* qr = q + (qrow0 + tt) * (H * 64) + h * 64 + 8 * g;
#pragma unroll
        for (int e = 0; e < 8; ++e) qv[t][e] = to_f<T>(qr[e]) * kLog2Scale;
        lim[t] = T_enc;
    }
    // SPLIT: this workgroup's chunk of the key blocks (gridDim.y chunks, block-aligned)
    const int nblk_all = cdiv(T_enc, W::KB);
    const int S = SPLIT ? (int)gridDim.y : 1, sp = SPLIT ? (int)blockIdx.y : 0;
    const int per = cdiv(nblk_all, S), blk0 = sp * per, nblk = min(nblk_all, blk0 + per);
    aw.template run<(1500 / W::KB + 1 + NW - 1) / NW>(blk0 + wid, nblk, qv, lim, nq);
    if (wid == 0) XA_STAMP(1);
    aw.to_lds(s_m, s_l, s_o, wid, lane);
    __syncthreads();
    XA_STAMP(2);
    for (int i = tid; i < 64 * nq; i += 64 * NW) {
        const int t = i >> 6, e = i & 63;
        float M, L, O;
        attn_merge<NQ, NW>(s_m, s_l, s_o, t, e, M, L, O);
        if constexpr (SPLIT) {  // partial {o[64], m, l} for the output projection's merge prologue
            float* pp = part + (((qrow0 + t) * H + h) * S + sp) * 66;
            pp[e] = O;
            if (e == 0) {
                pp[64] = M;
                pp[65] = L;
            }
        } else {
            out[(qrow0 + t) * (H * 64) + h * 64 + e] = from_f<T>(O / L);
        }
    }
}

// LN2 + cross-Q projection and the one-row cross-attention in one launch.  The cross
// K/V of a layer depend on nothing in the pass; only q does.  Workgroups [0, N / 16) are the cross-Q
// GEMV's, unchanged (gemv_body, 10 exact waves), and publish each q element as a tagged granule
// beside the q row they store; the following B x H workgroups are cross_attn_kernel<T, 1, false, 8>'s:
// waves 0..7 put their first PF - 1 key blocks in flight at once, wave 8 sweeps the head's 64 granules
// (one relaxed agent-scope 8-byte load per lane, s_sleep between sweeps) until every tag is this
// pass's, and hands the bits over in LDS, so the attention waves' wait for q is a barrier, not a
// load behind their K/V stream.  Producers wait on nothing and have the lowest workgroup indices;
// the launcher admits the grid only if every workgroup is resident at once (> 128 VGPRs at 10 waves:
// one workgroup per CU).  The wait is bounded by the wall clock (XqFuseArgs).
// PF = 3: the deepest ring without scratch at this workgroup's 168 VGPRs per wave (4 spills: 20 / 36 bytes
// per lane for bf16 / f16)
// TOUCH: beside the ring, each attention wave also pulls the cache lines of its next TOUCH key blocks
// towards L2 while it waits for q, one dword per line (a block of one wave is 32 K rows + 32 V rows of
// 128 bytes: one line per lane, one load instruction, one register); the ring's own loads of those
// blocks, issued once q is there, then find the lines in flight or in L2.
// QW: the cross-Q matrix is resident in its packed ggml blocks (gemv_body's quantised fetch).
// LDSB: the blocks number 2 .. 2 + LDSB - 1 of every attention wave's schedule are staged
// in LDS by the tenth wave, which requests them at launch by LDS-DMA (no register destination, every byte
// fetched once): block s of wave w at kXqStage + (w * LDSB + s) * 8 KiB, four K pieces then four V
// pieces of 1 KiB, each lane-linear with load_blk's per-lane source, so that lane L's ds_read_b128 at
// piece + 16 L returns the 16 bytes load_blk would have put in its registers.  The attention waves
// issue no LDS-DMA themselves (their ring's counted waits stay counted) and read the staged blocks only
// past a barrier that the loader reaches after its vmcnt(0): nothing else orders a ds_read behind
// another wave's LDS-DMA.  The loader shares the q hand-off barrier (every live wave must arrive at every
// barrier) without waiting for its DMA there, takes the give-up path with the others, and drains its
// DMA before it ends on either path.  LDSB = 0 is the kernel without any of this.
constexpr int kXqStage = 4096;  // the consumer's merge scratch, q bits and s_ok live below (2244 bytes)
template <typename T, int TOUCH, bool QW = false, int LDSB = 0, int PF = 3>
__global__ __launch_bounds__(640) void xq_fused_kernel(GemvArgs a, XqFuseArgs x) {
    const int n_prod = a.N / 16;
    // a vector load: a scalar one would hold every workgroup's first kernel-argument wait for its round trip
    const unsigned tag =
        (__hip_atomic_load(&x.ds->epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) + 1u) * 64u + (unsigned)x.layer;
    XQ_STAMP(0);
    if ((int)blockIdx.x < n_prod) {
        gemv_body<T, GV_BIAS, LN_SRC(0), 1, 10, 1, 1, true, true, QW>(a, x.gran, tag);
        XQ_STAMP(4);
        return;
    }
    typedef AttnWave<T, 1, 0, AW, PF> W;
    constexpr int MAXB = (1500 / W::KB + 1 + AW - 1) / AW;
    // LDS carved from the dynamic region the producers size (statics would shift its base)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float (*s_o)[1][64] = (float (*)[1][64])smem;
    float (*s_m)[1] = (float (*)[1])(smem + AW * 256);
    float (*s_l)[1] = (float (*)[1])(smem + AW * 256 + AW * 4);
    unsigned short* s_q = (unsigned short*)(smem + AW * 256 + AW * 8);  // the head's 64 q elements (bits)
    int* s_ok = (int*)(smem + AW * 256 + AW * 8 + 128);
    const int cb = (int)blockIdx.x - n_prod, j = cb / x.H, h = cb - j * x.H;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, g = lane & 7;
    const int nblk = cdiv(x.T_enc, W::KB);
    if (wid > AW) {  // the producer geometry's tenth wave: the LDS loader, or no part here
        if constexpr (LDSB > 0) {
            typedef const __attribute__((address_space(1))) void* GP;
            typedef __attribute__((address_space(3))) void* LP;
            const T* kb = (const T*)x.kv + ((size_t)j * x.H + h) * 4096 + 8 * g;
            const int bstride = x.B_layout * x.H * 4096, slot = lane >> 3;
#pragma unroll
            for (int s = 0; s < LDSB; ++s) {
#pragma unroll
                for (int w = 0; w < AW; ++w) {
                    const int mine = w + (nblk - 1 - w) / AW * AW;  // wave w's last block (nblk >= AW)
                    const int blk = min(w + (2 + s) * AW, mine);    // ring_run's clamp
#pragma unroll
                    for (int i = 0; i < W::NI; ++i) {  // load_blk's addresses
                        const int key = min(blk * W::KB + 8 * i + slot, x.T_enc - 1);
                        const uint32_t off = (uint32_t)((key >> 5) * bstride + (key & 31) * 64);
                        char* dst = smem + kXqStage + ((w * LDSB + s) * 8 + i) * 1024;
                        __builtin_amdgcn_global_load_lds((GP)(kb + off), (LP)dst, 16, 0, 0);
                        __builtin_amdgcn_global_load_lds((GP)(kb + 2048 + off), (LP)(dst + 4096), 16, 0, 0);
                    }
                }
            }
            // the q hand-off barrier, raw: a __syncthreads() here would wait for the DMA first
            asm volatile("s_barrier" ::: "memory");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every staged byte is in LDS (and none lands later)
            // the staged blocks' barrier, unless wave 8 gave up (the attention waves then end without it)
            if (__builtin_amdgcn_readfirstlane(*s_ok)) asm volatile("s_barrier" ::: "memory");
        }
        return;
    }
    W aw;
    unsigned touch[TOUCH > 0 ? TOUCH : 1] = {};
    if (wid < AW) {
        const size_t kvo = ((size_t)j * x.H + h) * 4096 + 8 * g;
        aw.init((const T*)x.kv + kvo, (const T*)x.kv + kvo + 2048, x.T_enc, lane, (int64_t)x.B_layout * x.H * 4096);
        aw.template ring_fill<MAXB>(wid, nblk);
        if constexpr (TOUCH > 0) {
            const T* base = (const T*)x.kv + ((size_t)j * x.H + h) * 4096 + (lane < 32 ? 0 : 2048);
#pragma unroll
            for (int t = 0; t < TOUCH; ++t) {
                const int key = min((wid + (PF - 1 + t) * AW) * W::KB + (lane & 31), x.T_enc - 1);
                touch[t] = *(const unsigned*)(base + (uint32_t)((key >> 5) * aw.bstride + (key & 31) * 64));
            }
        }
    } else {
        unsigned long long* gp = x.gran + ((size_t)j * x.H + h) * 64 + lane;
        bool ok = false;
        if (__hip_atomic_load(x.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) {
            const long long t0 = wall_clock64();
            for (;;) {
                const unsigned long long v = __hip_atomic_load(gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (__all((unsigned)(v >> 32) == tag)) {
                    s_q[lane] = (unsigned short)v;
                    ok = true;
                    break;
                }
                if (wall_clock64() - t0 > kXqTimeoutTicks) break;
                __builtin_amdgcn_s_sleep(2);
            }
        }
        if (lane == 0) {
            *s_ok = ok ? 1 : 0;
            if (!ok) __hip_atomic_store(x.err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    __syncthreads();
    if (wid >= AW || !*s_ok) return;
    XQ_STAMP(1);
    float qv[1][8];
    int lim[1] = {x.T_enc};
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        T qt;
        __builtin_memcpy(&qt, &s_q[8 * g + e], 2);
        qv[0][e] = to_f<T>(qt) * kLog2Scale;
    }
    if constexpr (LDSB > 0) {
        aw.template staged_head<MAXB, LDSB>(wid, nblk, qv, lim, 1);
        // the staged blocks' barrier: the loader arrives behind its vmcnt(0).  Raw, and reached by all 8
        // waves whatever their block counts; these waves have written nothing the others wait for.
        asm volatile("s_barrier" ::: "memory");
        XQ_STAMP(2);
        aw.template staged_tail<MAXB, LDSB>(wid, nblk, qv, lim, 1, smem + kXqStage + wid * LDSB * 8192 + lane * 16);
    } else {
        aw.template ring_run<MAXB>(wid, nblk, qv, lim, 1);
    }
    XQ_STAMP(3);
    aw.to_lds(s_m, s_l, s_o, wid, lane);
    __syncthreads();
    if (tid < 64) {
        float M, L, O;
        attn_merge<1, AW>(s_m, s_l, s_o, 0, tid, M, L, O);
        ((T*)x.out)[((size_t)j * x.H + h) * 64 + tid] = from_f<T>(O / L);
    }
    XQ_STAMP(4);
    if constexpr (TOUCH > 0) {
        // the touched dwords are used nowhere; this keeps their loads (layer is never negative)
        unsigned u = 0;
#pragma unroll
        for (int t = 0; t < TOUCH; ++t) u ^= touch[t];
        if (x.layer < 0 && u == 0x9e3779b9u) __hip_atomic_store(x.err, 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// The same cross-attention with each of the 8 waves of a (row run, h) workgroup as a workgroup
// of its own (grid.y = the wave index w, grid.z = the query chunk): wave w of the 8-wave kernel
// and workgroup w here run the same AttnWave over the same key blocks (w, w + 8, ...), and each
// writes its {o[64], m, l} as partial w of [rows][H][8][66]; the cross output projection's A_ATTN
// prologue merges the 8 partials in order w = 0..7 with attn_merge's arithmetic.  A row's result
// is therefore bitwise the 8-wave kernel's, and the choice between the two is free: this one runs
// when the 8-wave grid is small (B = 1, or the decoders of one utterance sharing a window), where
// 20 workgroups would stream 7.7 MB per layer through 20 CUs.
template <typename T, int NQ, int NIX = 0, int PF = 2>
__global__ __launch_bounds__(64) void cross_attn_vw_kernel(const T* __restrict__ q, const T* __restrict__ kv,
                                                           int B_layout, int H, int T_enc, int Tq,
                                                           float* __restrict__ part, const int* __restrict__ kvrow,
                                                           int share) {
    typedef AttnWave<T, NQ, NIX, AW, PF> W;  // block stride AW = the 8-wave kernel's waves
    __shared__ float s_m[1][NQ], s_l[1][NQ];
    __shared__ float s_o[1][NQ][64];
    const int bh = blockIdx.x, j = bh / H, h = bh - j * H;
    const int vw = blockIdx.y;                              // the 8-wave kernel's wave index
    const int lane = threadIdx.x, g = lane & 7;
    const int nq_all = share * Tq;
    const int c0 = (int)blockIdx.z * NQ;
    const int nq = min(NQ, nq_all - c0);
    const int kb = kvrow ? kvrow[j * share] : j;
    W aw;
    const size_t kvo = ((size_t)kb * H + h) * 4096 + 8 * g;
    aw.init(kv + kvo, kv + kvo + 2048, T_enc, lane, (int64_t)B_layout * H * 4096);
    const size_t qrow0 = (size_t)j * nq_all + c0;
    float qv[NQ][8];
    int lim[NQ];
#pragma unroll
    for (int t = 0; t < NQ; ++t) {
        const int tt = t < nq ? t : nq - 1;
        const T* qr = q + (qrow0 + tt) * (H * 64) + h * 64 + 8 * g;
#pragma unroll
        for (int e = 0; e < 8; ++e) qv[t][e] = to_f<T>(qr[e]) * kLog2Scale;
        lim[t] = T_enc;
    }
    aw.template run<(1500 / W::KB + 1 + AW - 1) / AW>(vw, cdiv(T_enc, W::KB), qv, lim, nq);
    aw.to_lds(s_m, s_l, s_o, 0, lane);
    __syncthreads();
    for (int i = lane; i < 64 * nq; i += 64) {
        const int t = i >> 6, e = i & 63;
        float* pp = part + (((qrow0 + t) * H + h) * AW + vw) * 66;
        pp[e] = s_o[0][t][e];
        if (e == 0) {
            pp[64] = s_m[0][t];
            pp[65] = s_l[0][t];
        }
    }
}

// The 8 partials {o[64], m, l} of each (query row, head) written by cross_attn_vw_kernel, merged
// once into the bf16 / f32 attention output: attn_merge's operations in the same order, so the
// result is bitwise the 8-wave kernel's.  Used when the cross output projection has several rows:
// its A_ATTN prologue would merge every row and head in each of its 80 workgroups (15 us at a
// beam's 5 rows, profiles/r4/exp_beam_step.txt).
template <typename T>
__global__ __launch_bounds__(64) void attn_part_merge_kernel(const float* __restrict__ part, int H, T* __restrict__ out) {
#pragma clang fp contract(off)
    const int rh = blockIdx.x, e = threadIdx.x;
    const float* pp = part + (size_t)rh * AW * 66;
    float mw[AW], lw[AW], ow[AW];
#pragma unroll
    for (int w = 0; w < AW; ++w) {
        mw[w] = pp[w * 66 + 64];
        lw[w] = pp[w * 66 + 65];
        ow[w] = pp[w * 66 + e];
    }
    float M = -INFINITY;
#pragma unroll
    for (int w = 0; w < AW; ++w) M = fmaxf(M, mw[w]);
    float L = 0.f, O = 0.f;
#pragma unroll
    for (int w = 0; w < AW; ++w) {
        if (mw[w] == -INFINITY) continue;
        const float f = exp2f(mw[w] - M);
        L = __builtin_fmaf(lw[w], f, L);
        O = __builtin_fmaf(ow[w], f, O);
    }
    out[(size_t)rh * 64 + e] = from_f<T>(O / L);  // row r, head h: out[r][h * 64 + e], rh = r * H + h
}

// ------------------------------------------------------------------ finalize
// Per sequence: reduce the logits tiles' top-2, record the token, choose the next
// input (argmax or forced), embed it for the next pass; the last block advances
// the step state (every block reads it before arriving).
constexpr int FIN_T = 1024;  // finalize threads per sequence: the 3.2k top-2 partials in ~3 loads each
template <typename T, bool QE = false>
__global__ __launch_bounds__(FIN_T) void finalize_kernel(FinalizeArgs a) {
    __shared__ TopP s_top[FIN_T / 64];
    __shared__ int s_tok;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int step = a.ds->step, pos0 = a.ds->pos0;
    const unsigned epoch = a.ds->epoch;
    TopP t{-INFINITY, 0x7fffffff, -INFINITY, 0};
    const TopP* p = (const TopP*)a.part + (size_t)b * a.n_tiles;
    for (int i = tid; i < a.n_tiles; i += FIN_T) t = top_merge(t, p[i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) t = top_merge(t, top_shfl(t, o));
    if ((tid & 63) == 0) s_top[tid >> 6] = t;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < FIN_T / 64; ++w) t = top_merge(t, s_top[w]);
        // non-finite logits leave no valid winner: record the sentinel, never index with it
        if (t.i1 < 0 || t.i1 >= a.n_vocab) {
            t.i1 = -2;
            t.v1 = t.v2 = __builtin_nanf("");
        }
        int nxt = a.eot;
        if (step < a.out_cap) {
            const int oi = b * a.out_cap + step;
            if (a.done[b]) {
                a.out_tok[oi] = -1;
                a.out_top1[oi] = -INFINITY;
                a.out_top2[oi] = -INFINITY;
            } else {
                a.out_tok[oi] = t.i1;
                a.out_top1[oi] = t.v1;
                a.out_top2[oi] = t.v2;
                nxt = t.i1;
                if (a.forced && step < a.forced_len) nxt = a.forced[b * a.forced_len + step];
                if (!a.ignore_eot && t.i1 == a.eot) a.done[b] = 1;
                if (nxt < 0 || nxt >= a.n_vocab) nxt = a.eot;
            }
        }
        a.next_tok[b] = nxt;
        s_tok = nxt;
    }
    __syncthreads();
    const int tok = s_tok;
    const int pn = min(pos0 + a.Tq, a.ctx - 1);
    const float* pp = a.pos + (size_t)pn * a.d;
    for (int i = tid; i < a.d; i += FIN_T)
        a.x[(size_t)b * a.d + i] = emb_row_read<T, QE>(a.emb, a.emb_q, a.d, tok, i) + pp[i];
    if (tid == 0) {
        // relaxed: every block's reads of the step state were consumed before it arrives, and the next
        // kernel sees the last arriver's plain stores across the launch boundary (an acq_rel RMW cost
        // an L2 write-back and invalidate in every block's tail)
        const unsigned prev = __hip_atomic_fetch_add(a.arrive, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (prev == (unsigned)gridDim.x - 1) {
            a.ds->pos0 = pos0 + a.Tq;
            a.ds->step = step + 1;
            a.ds->epoch = epoch + 1u;
            __hip_atomic_store(a.arrive, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

__global__ void advance_kernel(DecState* ds, int n) {
    ds->pos0 += n;
    ds->epoch += 1u;
}

__global__ void reset_kernel(DecState* ds, unsigned* arrive) {
    ds->pos0 = 0;
    ds->step = 0;
    *arrive = 0u;
}

}  // namespace

void gemv_prepare(int dtype) {
    dec_xq_fused_prepare(dtype);
    if (dtype == DT_BF16) gemv_attr_modes<bf16>();
    else if (dtype == DT_F16) gemv_attr_modes<f16>();
    else gemv_attr_modes<float>();
}

int gemv_max_image_rows(int dtype, int K) {
    const int esz = dtype_size(dtype);
    int r = 64;
    while (r > 1 && gv_img_bytes(r, K, esz) > GV_LDS_BYTES) --r;
    return r;
}

GemvPlan gemv_plan(int dtype, int mode, int asrc, const GemvArgs& a_in) {
    if (a_in.R > 64 || a_in.R <= 0) throw std::runtime_error("gemv: rows must be in 1..64");
    const int ks = dtype_size(dtype) == 2 ? 128 : 64;
    if (a_in.K % ks) throw std::runtime_error("gemv: K alignment");
    GemvArgs a = a_in;
    a.ksplit = std::max(1, a.ksplit);
    if (a.ksplit > 1 && mode != GV_PARTIAL) throw std::runtime_error("gemv: K split needs partial outputs");
    if (a.ksplit > a.K / ks) throw std::runtime_error("gemv: K split exceeds the super-steps");
    const int esz = dtype_size(dtype);
    if (asrc != A_DIRECT && gv_img_bytes(a.R, a.K, esz) > GV_LDS_BYTES)
        throw std::runtime_error("gemv: A image exceeds the LDS budget");
    if (asrc == A_LN && (a.K > 1536 || !a.ln_w || !a.ln_b))
        throw std::runtime_error("gemv: LayerNorm prologue needs K <= 1536 and LN parameters");
    if (asrc == A_LN && (a.n_pend < 0 || a.n_pend > 4 || a.n_pend == 3))
        throw std::runtime_error("gemv: pending slab count must be 0, 1, 2 or 4");
    if (a.p_resid && mode != GV_PARTIAL) throw std::runtime_error("gemv: residual rows into slab 0 need partial outputs");
    if (asrc == A_LN)
        for (int p = 0; p < 4; ++p)
            if (!a.pend[p]) throw std::runtime_error("gemv: LayerNorm prologue needs 4 pending slabs (zero slab if none)");
    if (asrc == A_ATTN && (!a.apart || a.a_splits < 2 || (a.a_splits > 4 && a.a_splits != 8) || a.a_heads * 64 != a.K))
        throw std::runtime_error("gemv: attention-merge prologue needs 2..4 or 8 chunks over all heads");
    const int code = asrc == A_LN ? LN_SRC(a.n_pend) : asrc == A_ATTN ? ATTN_SRC(a.a_splits) : asrc;
    if (a.wq) {  // a matrix resident in its packed blocks: the same checks, geometry and body (k_dec_q.hip)
        QPackGeom qg;
        if (esz != 2 || !qpack_geom(a.wq, &qg)) throw std::runtime_error("gemv: no resident layout for this weight type / dtype");
    }
#define SPT_GV(M, S) \
    if (mode == M && code == S) return gemv_shape(esz, mode, code, a.R, a.N, a.K, a.ksplit);
    SPT_GV_PAIRS(SPT_GV)
#undef SPT_GV
    throw std::runtime_error("gemv: unsupported mode / A source");
}

void gemv(int dtype, int mode, int asrc, const GemvArgs& a_in, hipStream_t st) {
    const int code = gemv_plan(dtype, mode, asrc, a_in).code;
    GemvArgs a = a_in;
    a.ksplit = std::max(1, a.ksplit);
    if (a.wq) {
        gemv_q(dtype, mode, code, a, st);
        return;
    }
#define SPT_GV(M, S)                                                      \
    if (mode == M && code == S) {                                         \
        if (dtype == DT_BF16) gemv_launch<bf16, M, S>(a, st);             \
        else if (dtype == DT_F16) gemv_launch<f16, M, S>(a, st);          \
        else gemv_launch<float, M, S>(a, st);                             \
        return;                                                           \
    }
    SPT_GV_PAIRS(SPT_GV)
#undef SPT_GV
    throw std::runtime_error("gemv: unsupported mode / A source");
}

void dec_embed(int dtype, const int* tok, int R, int Tq, int d, const void* tok_emb, int tok_q, const float* pos_emb,
               const DecState* ds, float* x, hipStream_t st) {
    if (tok_q) {  // a packed resident token embedding (16-bit engines)
        if (dtype == DT_BF16)
            hipLaunchKernelGGL((embed_kernel<bf16, true>), dim3(R), dim3(256), 0, st, tok, Tq, d, (const bf16*)tok_emb, tok_q, pos_emb, ds, x);
        else if (dtype == DT_F16)
            hipLaunchKernelGGL((embed_kernel<f16, true>), dim3(R), dim3(256), 0, st, tok, Tq, d, (const f16*)tok_emb, tok_q, pos_emb, ds, x);
        else throw std::runtime_error("dec_embed: a packed embedding needs a bf16 or f16 engine");
        return;
    }
    if (dtype == DT_BF16)
        hipLaunchKernelGGL(embed_kernel<bf16>, dim3(R), dim3(256), 0, st, tok, Tq, d, (const bf16*)tok_emb, 0, pos_emb, ds, x);
    else if (dtype == DT_F16)
        hipLaunchKernelGGL(embed_kernel<f16>, dim3(R), dim3(256), 0, st, tok, Tq, d, (const f16*)tok_emb, 0, pos_emb, ds, x);
    else
        hipLaunchKernelGGL(embed_kernel<float>, dim3(R), dim3(256), 0, st, tok, Tq, d, (const float*)tok_emb, 0, pos_emb, ds, x);
}

void dec_self_attn(int dtype, const void* q, const void* cache, int B, int H, int ctx, int Tq, const DecState* ds,
                   void* out, hipStream_t st) {
    if (Tq < 1 || Tq > 4) throw std::runtime_error("dec_self_attn: 1..4 queries per sequence");
    const dim3 grid(B * H), blk(64 * AW);
#define SPT_SA(T, NQ) \
    hipLaunchKernelGGL((self_attn_kernel<T, NQ>), grid, blk, 0, st, (const T*)q, H * 64, (const T*)cache, B, H, ctx, Tq, ds, (T*)out)
    if (dtype == DT_BF16) {
        if (Tq == 1) SPT_SA(bf16, 1); else SPT_SA(bf16, 4);
    } else if (dtype == DT_F16) {
        if (Tq == 1) SPT_SA(f16, 1); else SPT_SA(f16, 4);
    } else {
        if (Tq == 1) SPT_SA(float, 1); else SPT_SA(float, 4);
    }
#undef SPT_SA
    SPT_LAUNCH_CHECK();
}

// key blocks in each cross-attention wave's register ring (SPT_XATTN_PF = 2..4; no result changes)
static int xattn_pf() {
    static const int pf = getenv("SPT_XATTN_PF") ? std::max(2, std::min(4, atoi(getenv("SPT_XATTN_PF")))) : 2;
    return pf;
}

void dec_cross_attn(int dtype, const void* q, const void* kv, int B, int B_layout, int H, int T_enc, int Tq, void* out,
                    hipStream_t st, int splits, float* part, const int* kvrow, int share) {
    if (Tq < 1 || Tq > 4) throw std::runtime_error("dec_cross_attn: 1..4 queries per sequence");
    if (splits < 1 || splits > 4 || (splits > 1 && !part)) throw std::runtime_error("dec_cross_attn: 1..4 key chunks");
    if (share < 1 || share > 8 || B % share) throw std::runtime_error("dec_cross_attn: rows per window 1..8, dividing B");
    if (share > 1 && !kvrow) throw std::runtime_error("dec_cross_attn: shared windows need the window map");
    if ((int64_t)cdiv(T_enc, 32) * B_layout * H * 4096 >= (int64_t)INT32_MAX)
        throw std::runtime_error("dec_cross_attn: a layer's cross K/V exceeds 2^31 elements");
    const int nq = share * Tq;
    // queries per workgroup: 1 or 4 as without a window map; a decode step of several rows per
    // window takes 5 (bf16 / f16: beam 5 / best_of 5 in one workgroup; 8 would spill) or 4 (f32) of
    // them.  Every variant gives each lane the
    // same keys as the one-row kernel of the same Tq (NI: keys per lane), so a row's result is
    // bitwise the same whether or not its window is shared.
    const int NQ = nq == 1 ? 1 : Tq > 1 ? 4 : (dtype_size(dtype) == 2 ? 5 : 4);
    if (splits > 1 && nq > NQ) throw std::runtime_error("dec_cross_attn: key chunks need one query chunk per window");
    const dim3 grid((B / share) * H, splits > 1 ? splits : cdiv(nq, NQ)), blk(64 * AW);
#define SPT_XA(T, NQ_, SP, NI, ...)                                                                             \
    hipLaunchKernelGGL((cross_attn_kernel<T, NQ_, SP, AW, NI __VA_ARGS__>), grid, blk, 0, st, (const T*)q,        \
                       (const T*)kv, B_layout, H, T_enc, Tq, (T*)out, part, kvrow, share)
    // NI = 4 for the step kernels of both dtypes (AttnWave's default at NQ = 1)
#define SPT_XA_T(T)                                                                       \
    if (NQ == 1) {                                                                        \
        if (splits > 1) SPT_XA(T, 1, true, 0);                                            \
        else if (xattn_pf() == 4) SPT_XA(T, 1, false, 0, , 4);                            \
        else if (xattn_pf() == 3) SPT_XA(T, 1, false, 0, , 3);                            \
        else SPT_XA(T, 1, false, 0);                                                      \
    }                                                                                     \
    else if (NQ == 4 && Tq > 1) { if (splits > 1) SPT_XA(T, 4, true, 0); else SPT_XA(T, 4, false, 0); } \
    else if (NQ == 4) { if (splits > 1) SPT_XA(T, 4, true, 4); else SPT_XA(T, 4, false, 4); } \
    else { if (splits > 1) SPT_XA(T, 5, true, 4); else SPT_XA(T, 5, false, 4); }
    if (dtype == DT_BF16) { SPT_XA_T(bf16); }
    else if (dtype == DT_F16) { SPT_XA_T(f16); }
    else { SPT_XA_T(float); }
#undef SPT_XA_T
#undef SPT_XA
    SPT_LAUNCH_CHECK();
}

void dec_cross_attn_vw(int dtype, const void* q, const void* kv, int B, int B_layout, int H, int T_enc, int Tq,
                       float* part, hipStream_t st, const int* kvrow, int share, bool per_query) {
    if (Tq < 1 || Tq > 4) throw std::runtime_error("dec_cross_attn_vw: 1..4 queries per sequence");
    if (share < 1 || share > 8 || B % share) throw std::runtime_error("dec_cross_attn_vw: rows per window 1..8, dividing B");
    if (share > 1 && !kvrow) throw std::runtime_error("dec_cross_attn_vw: shared windows need the window map");
    if ((int64_t)cdiv(T_enc, 32) * B_layout * H * 4096 >= (int64_t)INT32_MAX)
        throw std::runtime_error("dec_cross_attn_vw: a layer's cross K/V exceeds 2^31 elements");
    if (!part) throw std::runtime_error("dec_cross_attn_vw: needs the partials buffer");
    const int nq = share * Tq;
    // the same query chunks and keys per lane as dec_cross_attn (bitwise the same partials); per_query
    // (one-token steps): one query per workgroup, the window's K/V re-read per query from L2 -- the
    // same 4 keys per lane as the shared kernels' NIX = 4, so still bitwise the same partials
    const int NQ = (nq == 1 || (per_query && Tq == 1)) ? 1 : Tq > 1 ? 4 : (dtype_size(dtype) == 2 ? 5 : 4);
    const dim3 grid((B / share) * H, AW, cdiv(nq, NQ)), blk(64);
#define SPT_XV(T, NQ_, NI, PF)                                                                               \
    hipLaunchKernelGGL((cross_attn_vw_kernel<T, NQ_, NI, PF>), grid, blk, 0, st, (const T*)q, (const T*)kv,      \
                       B_layout, H, T_enc, Tq, part, kvrow, share)
#define SPT_XV_PF(T, NQ_, NI)                                    \
    if (xattn_pf() == 4) SPT_XV(T, NQ_, NI, 4);                  \
    else if (xattn_pf() == 3) SPT_XV(T, NQ_, NI, 3);             \
    else SPT_XV(T, NQ_, NI, 2);
#define SPT_XV_T(T)                                         \
    if (NQ == 1) { SPT_XV_PF(T, 1, 0) }                     \
    else if (NQ == 4 && Tq > 1) SPT_XV(T, 4, 0, 2);         \
    else if (NQ == 4) SPT_XV(T, 4, 4, 2);                   \
    else { SPT_XV_PF(T, 5, 4) }
    if (dtype == DT_BF16) { SPT_XV_T(bf16); }
    else if (dtype == DT_F16) { SPT_XV_T(f16); }
    else { SPT_XV_T(float); }
#undef SPT_XV_T
#undef SPT_XV_PF
#undef SPT_XV
    SPT_LAUNCH_CHECK();
}

namespace {
// the fused launch's instances by {touched blocks 0 / 2, packed cross-Q weights, staged blocks 0..2}
typedef void (*XqKernel)(GemvArgs, XqFuseArgs);
template <typename T>
XqKernel xq_kernel(int touch, bool qw, int ldsb) {
#define SPT_XQ_L(TO, QW) {xq_fused_kernel<T, TO, QW, 0>, xq_fused_kernel<T, TO, QW, 1>, xq_fused_kernel<T, TO, QW, 2>}
    static const XqKernel tab[2][2][3] = {{SPT_XQ_L(0, false), SPT_XQ_L(0, true)}, {SPT_XQ_L(2, false), SPT_XQ_L(2, true)}};
#undef SPT_XQ_L
    return tab[touch ? 1 : 0][qw ? 1 : 0][ldsb];
}
// dynamic LDS of every workgroup of the launch: the producers' LayerNorm image and reduction, or the
// consumers' scratch and staged blocks (8 waves x ldsb x 8 KiB)
int xq_lds_bytes(int R, int K, int ldsb) {
    const int prod = std::max(4096, gv_img_bytes(R, K, 2) + 10 * 64 * (int)sizeof(f32x4));
    return std::max(prod, ldsb > 0 ? kXqStage + AW * ldsb * 8192 : 0);
}
}  // namespace

// the staged instances take more than 64 KiB of dynamic LDS: enabled per kernel, outside any stream capture
void dec_xq_fused_prepare(int dtype) {
    if (dtype_size(dtype) != 2) return;
    for (int touch = 0; touch <= 2; touch += 2)
        for (int qw = 0; qw < 2; ++qw)
            for (int l = 1; l <= 2; ++l)
                ensure_lds_attr((const void*)(dtype == DT_BF16 ? xq_kernel<bf16>(touch, qw, l) : xq_kernel<f16>(touch, qw, l)),
                                xq_lds_bytes(16, 1280, l));
}

bool dec_xq_fused_ok(int dtype, int B, int d, int H, int T_enc, int n_cu) {
    // the chain's cross-Q must be the exact 10-wave GEMV (GV_EXACT_LN=0 gives it another K order)
    static const bool exact_ln = !getenv("GV_EXACT_LN") || atoi(getenv("GV_EXACT_LN")) != 0;
    return exact_ln && dtype_size(dtype) == 2 && d == 10 * GV<bf16>::KS && H * 64 == d && B >= 1 && B <= 16 &&
           T_enc >= 256 && cdiv(T_enc, 32) <= 48 && d / 16 + B * H <= n_cu;
}

void dec_xq_fused(int dtype, const GemvArgs& cq, const XqFuseArgs& x, int B, hipStream_t st) {
    if (dtype_size(dtype) != 2 || cq.R != B || B < 1 || B > 16 || cq.N != x.H * 64 || cq.K != 10 * GV<bf16>::KS ||
        cq.N % 16 || cq.n_pend != 0 || !cq.ln_w || !cq.ln_b || !cq.C || x.T_enc < 256 || cdiv(x.T_enc, 32) > 48 ||
        x.layer < 0 || x.layer >= 64 || !x.kv || !x.out || !x.gran || !x.ds || !x.err)
        throw std::runtime_error("dec_xq_fused: not the fused launch's shape");
    for (int p = 0; p < 4; ++p)
        if (!cq.pend[p]) throw std::runtime_error("dec_xq_fused: LayerNorm prologue needs 4 pending slabs (zero slab if none)");
    if ((int64_t)cdiv(x.T_enc, 32) * x.B_layout * x.H * 4096 >= (int64_t)INT32_MAX)
        throw std::runtime_error("dec_xq_fused: a layer's cross K/V exceeds 2^31 elements");
    GemvArgs a = cq;
    a.ksplit = 1;
    if (x.lds < 0 || x.lds > 2 || (x.touch != 0 && x.touch != 2))
        throw std::runtime_error("dec_xq_fused: 0..2 staged blocks, 0 or 2 touched blocks");
    const dim3 grid(a.N / 16 + B * x.H), blk(640);
    QPackGeom qg;
    if (a.wq && !qpack_geom(a.wq, &qg)) throw std::runtime_error("dec_xq_fused: no resident layout for this weight type");
    const XqKernel k = dtype == DT_BF16 ? xq_kernel<bf16>(x.touch, a.wq != 0, x.lds) : xq_kernel<f16>(x.touch, a.wq != 0, x.lds);
    hipLaunchKernelGGL(k, grid, blk, xq_lds_bytes(a.R, a.K, x.lds), st, a, x);
    SPT_LAUNCH_CHECK();
}

void dec_attn_part_merge(int dtype, const float* part, int R, int H, void* out, hipStream_t st) {
    if (R < 1 || H < 1 || !part || !out) throw std::runtime_error("dec_attn_part_merge: empty or missing buffers");
    if (dtype == DT_BF16) hipLaunchKernelGGL(attn_part_merge_kernel<bf16>, dim3(R * H), dim3(64), 0, st, part, H, (bf16*)out);
    else if (dtype == DT_F16) hipLaunchKernelGGL(attn_part_merge_kernel<f16>, dim3(R * H), dim3(64), 0, st, part, H, (f16*)out);
    else hipLaunchKernelGGL(attn_part_merge_kernel<float>, dim3(R * H), dim3(64), 0, st, part, H, (float*)out);
    SPT_LAUNCH_CHECK();
}

void dec_finalize(int dtype, const FinalizeArgs& a, int B, hipStream_t st) {
    if (a.emb_q) {  // a packed resident token embedding (16-bit engines)
        if (dtype == DT_BF16) hipLaunchKernelGGL((finalize_kernel<bf16, true>), dim3(B), dim3(FIN_T), 0, st, a);
        else if (dtype == DT_F16) hipLaunchKernelGGL((finalize_kernel<f16, true>), dim3(B), dim3(FIN_T), 0, st, a);
        else throw std::runtime_error("dec_finalize: a packed embedding needs a bf16 or f16 engine");
        return;
    }
    if (dtype == DT_BF16) hipLaunchKernelGGL(finalize_kernel<bf16>, dim3(B), dim3(FIN_T), 0, st, a);
    else if (dtype == DT_F16) hipLaunchKernelGGL(finalize_kernel<f16>, dim3(B), dim3(FIN_T), 0, st, a);
    else hipLaunchKernelGGL(finalize_kernel<float>, dim3(B), dim3(FIN_T), 0, st, a);
}

void dec_advance(DecState* ds, int n, hipStream_t st) {
    hipLaunchKernelGGL(advance_kernel, dim3(1), dim3(1), 0, st, ds, n);
}

void dec_reset(DecState* ds, unsigned* arrive, hipStream_t st) {
    hipLaunchKernelGGL(reset_kernel, dim3(1), dim3(1), 0, st, ds, arrive);
}

}  // namespace spt
