// k_dec_f8.hip -- the fp8 cross K/V cache of SPT_MODEL_CROSS_KV_F8 (format: kv_f8.h): the
// quantiser that turns staged 16-bit layers into records, the dequantiser of the debug reads, and the
// decode-step cross-attention over the records in the two launch shapes of k_dec.hip (8 waves per
// (row run, head), or each of those waves as a workgroup of its own writing partials).
#include <algorithm>
#include <stdexcept>

#include "common.h"
#include "dec_attn.h"
#include "kernels.h"
#include "kv_f8.h"

namespace spt {
namespace {

// four codes of one dword -> f32 (v_cvt_pk_f32_fp8: OCP e4m3fn on gfx950, exact)
__device__ __forceinline__ void f8x4_to_f32(uint32_t w, float* f) {
    const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false);
    const f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
    f[0] = lo[0];
    f[1] = lo[1];
    f[2] = hi[0];
    f[3] = hi[1];
}

// ------------------------------------------------------------------ quantise / dequantise
// One workgroup per record: 64 rows (32 K, 32 V) x 4 lanes, 16 elements per lane.  src: the staged
// layers in the kv_offset layout, [records][2][32][64]; dst: the records, in the same order.  Rows at
// t >= T are not read: code 0, scale 1.
template <typename T>
__global__ __launch_bounds__(256) void kv_quant_f8_kernel(const T* __restrict__ src, char* __restrict__ dst, int nblk,
                                                          int BH, int T_enc) {
#pragma clang fp contract(off)
    const int64_t rec = blockIdx.x;
    const int tid = threadIdx.x, row = tid >> 2, g = tid & 3;  // row 0..63: kvi * 32 + key
    const int kvi = row >> 5, r = row & 31;
    const int tb = (int)((rec / BH) % nblk);
    char* out = dst + rec * f8::kRecBytes;
    uint4 codes = {0u, 0u, 0u, 0u};
    float scale = 1.0f;
    if (tb * 32 + r < T_enc) {  // (uniform over the 4 lanes of a row)
        const T* p = src + rec * 4096 + row * 64 + 16 * g;
        float x[16];
        KVChunk<T> a, b;
        a.load(p);
        b.load(p + 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            x[e] = a.at(e);
            x[8 + e] = b.at(e);
        }
        float amax = 0.f;
#pragma unroll
        for (int e = 0; e < 16; ++e) amax = fmaxf(amax, fabsf(x[e]));
        amax = fmaxf(amax, __shfl_xor(amax, 1, 64));
        amax = fmaxf(amax, __shfl_xor(amax, 2, 64));
        const f8::RowScale rs = f8::row_scale(amax);
        scale = rs.scale;
        if (amax != 0.f) {
            uint32_t w[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                int v = 0;
                v = __builtin_amdgcn_cvt_pk_fp8_f32((x[4 * i] * rs.up) * rs.inv, (x[4 * i + 1] * rs.up) * rs.inv, v, false);
                v = __builtin_amdgcn_cvt_pk_fp8_f32((x[4 * i + 2] * rs.up) * rs.inv, (x[4 * i + 3] * rs.up) * rs.inv, v, true);
                w[i] = (uint32_t)v;
            }
            codes = {w[0], w[1], w[2], w[3]};
        }
    }
    *(uint4*)(out + kvi * f8::kRecV + r * 64 + 16 * g) = codes;
    if (g == 0) *(float*)(out + f8::scale_offset(kvi, r)) = scale;
}

// records of one layer -> f32(code) * scale, [nb][H][T][64] for K and V, and optionally the scales
// [nb][H][T], of windows b0 .. b0 + nb - 1.  One thread per (window, head, key, K-or-V, 4 elements).
__global__ __launch_bounds__(256) void kv_dequant_f8_kernel(const char* __restrict__ recs, int B_layout, int H, int T_enc,
                                                            int b0, int nb, float* __restrict__ k, float* __restrict__ v,
                                                            float* __restrict__ ks, float* __restrict__ vs) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t n = (int64_t)nb * H * T_enc * 32;
    if (i >= n) return;
    const int q = (int)(i & 15), kvi = (int)((i >> 4) & 1);
    const int64_t key = i >> 5;  // (bi * H + h) * T + t
    const int t = (int)(key % T_enc);
    const int64_t bh = key / T_enc;
    const int h = (int)(bh % H), bi = (int)(bh / H);
    const char* rec = recs + f8::rec_offset(b0 + bi, h, t, B_layout, H);
    const float s = *(const float*)(rec + f8::scale_offset(kvi, t & 31));
    const uint32_t w = *(const uint32_t*)(rec + kvi * f8::kRecV + (t & 31) * 64 + 4 * q);
    float f[4];
    f8x4_to_f32(w, f);
    float* o = (kvi ? v : k) + key * 64 + 4 * q;
    *(f32x4*)o = f32x4{f[0] * s, f[1] * s, f[2] * s, f[3] * s};
    if (q == 0) {
        float* so = kvi ? vs : ks;
        if (so) so[key] = s;
    }
}

// ------------------------------------------------------------------ attention over the records
// AttnWave's flash-decoding (dec_attn.h) over fp8 records: a key block is one record (32 keys), 4
// lanes per key with 16 codes each (one 16-byte load of K and of V per 16 keys), key slot s = lane >> 2
// takes keys s and s + 16 of the block, and one 16-byte load brings the slot's four scales.  The score
// is scale_k * sum(q_e * f32(code_e)) and p * scale_v goes into the V accumulation: one rounding each
// per key.  Wave w of NW takes blocks w, w + NW, ... in that order whatever the launch shape, the batch
// or the ring depth, and the arithmetic is spelled out (contraction off, explicit fmaf), so a row's
// bits are its own.  A key at or past n_keys takes scale 1 and score -inf: its stored scale is used nowhere.
struct F8Blk {
    uint4 k[2], v[2];
    f32x4 sc;  // {k[s], k[s + 16], v[s], v[s + 16]}
};

template <int NQ, int NW = AW, int PF = 2>
struct AttnWaveF8 {
    static constexpr int KB = f8::kBlockKeys;
    static_assert(PF >= 2 && PF <= 4, "AttnWaveF8: 2..4 ring slots");
    F8Blk ring_[PF];
    float m[NQ], l[NQ], o[NQ][16];
    const char* base;  // the (window, head)'s record of block 0, at the lane's bytes
    int n_keys, slot, g;
    uint32_t bstride;  // bytes between the records of consecutive blocks

    __device__ __forceinline__ void init(const char* rec0, int nk, int lane, int64_t blk_stride) {
        slot = lane >> 2;
        g = lane & 3;
        base = rec0;
        n_keys = nk;
        bstride = (uint32_t)blk_stride;
#pragma unroll
        for (int t = 0; t < NQ; ++t) {
            m[t] = -INFINITY;
            l[t] = 0.f;
#pragma unroll
            for (int e = 0; e < 16; ++e) o[t][e] = 0.f;
        }
    }
    __device__ __forceinline__ void load_blk(F8Blk& c, int blk) {
        // 32-bit byte offsets (the launchers check that a layer's records span < 2^31 bytes)
        const char* r = base + (uint32_t)blk * bstride;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const uint32_t off = (uint32_t)((16 * i + slot) * 64 + 16 * g);
            c.k[i] = *(const uint4*)(r + off);
            c.v[i] = *(const uint4*)(r + f8::kRecV + off);
        }
        c.sc = *(const f32x4*)(r + f8::kRecScale + slot * 16);
    }
    __device__ __forceinline__ void process(const F8Blk& c, int kbase, const float (&qv)[NQ][16], int Tq) {
#pragma clang fp contract(off)
        bool live[2];
        float sk[2], sv[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            live[i] = kbase + 16 * i + slot < n_keys;
            sk[i] = live[i] ? c.sc[i] : 1.0f;
            sv[i] = live[i] ? c.sc[2 + i] : 1.0f;
        }
        float kf[2][16];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            f8x4_to_f32(c.k[i].x, kf[i]);
            f8x4_to_f32(c.k[i].y, kf[i] + 4);
            f8x4_to_f32(c.k[i].z, kf[i] + 8);
            f8x4_to_f32(c.k[i].w, kf[i] + 12);
        }
#pragma unroll
        for (int t = 0; t < NQ; ++t) {
            if (t >= Tq) break;
            float s[2];
            float mb = -INFINITY;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                float v = 0.f;
#pragma unroll
                for (int e = 0; e < 16; ++e) v = __builtin_fmaf(qv[t][e], kf[i][e], v);
                v += __shfl_xor(v, 1, 64);
                v += __shfl_xor(v, 2, 64);
                v = v * sk[i];
                if (!live[i]) v = -INFINITY;
                s[i] = v;
                mb = fmaxf(mb, v);
            }
            mb = fmaxf(mb, __shfl_xor(mb, 4, 64));
            mb = fmaxf(mb, __shfl_xor(mb, 8, 64));
            mb = fmaxf(mb, __shfl_xor(mb, 16, 64));
            mb = fmaxf(mb, __shfl_xor(mb, 32, 64));
            if (mb == -INFINITY) continue;
            const float mn = fmaxf(m[t], mb);
            const float alpha = exp2f(m[t] - mn);
            float ls = 0.f;
#pragma unroll
            for (int e = 0; e < 16; ++e) o[t][e] *= alpha;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const float p = exp2f(s[i] - mn);
                ls += p;
                const float pw = p * sv[i];
                float vf[16];
                f8x4_to_f32(c.v[i].x, vf);
                f8x4_to_f32(c.v[i].y, vf + 4);
                f8x4_to_f32(c.v[i].z, vf + 8);
                f8x4_to_f32(c.v[i].w, vf + 12);
#pragma unroll
                for (int e = 0; e < 16; ++e) o[t][e] = __builtin_fmaf(pw, vf[e], o[t][e]);
            }
            l[t] = __builtin_fmaf(l[t], alpha, ls);
            m[t] = mn;
        }
    }
    // AttnWave::run's schedule: blocks blk, blk + NW, ... below nblk, PF - 1 of them loading ahead;
    // up to MAXB blocks per wave fully unrolled with unconditional loads (past the wave's last block
    // they repeat it), more in the rolled two-slot loop.  The order of the blocks is the same in both.
    template <int MAXB>
    __device__ __forceinline__ void run(int blk, int nblk, const float (&qv)[NQ][16], int Tq) {
        if (blk >= nblk) return;
        const int cnt = (nblk - 1 - blk) / NW + 1;
        const int mine = blk + (cnt - 1) * NW;
        if (cnt <= MAXB) {
#pragma unroll
            for (int d = 0; d < PF - 1 && d < MAXB; ++d) load_blk(ring_[d], min(blk + d * NW, mine));
#pragma unroll
            for (int i = 0; i < MAXB; ++i) {
                if (i >= cnt) break;
                if (i + PF - 1 < MAXB) load_blk(ring_[(i + PF - 1) % PF], min(blk + (i + PF - 1) * NW, mine));
                process(ring_[i % PF], (blk + i * NW) * KB, qv, Tq);
            }
            return;
        }
        load_blk(ring_[0], blk);
        while (blk < nblk) {
            load_blk(ring_[1], min(blk + NW, mine));
            process(ring_[0], blk * KB, qv, Tq);
            blk += NW;
            if (blk >= nblk) break;
            load_blk(ring_[0], min(blk + NW, mine));
            process(ring_[1], blk * KB, qv, Tq);
            blk += NW;
        }
    }
    // sum l and o over the 16 key slots of the wave (m is wave-uniform) into LDS
    __device__ __forceinline__ void to_lds(float (*s_m)[NQ], float (*s_l)[NQ], float (*s_o)[NQ][64], int wid, int lane) {
#pragma unroll
        for (int t = 0; t < NQ; ++t) {
            float lt = l[t];
            lt += __shfl_xor(lt, 4, 64);
            lt += __shfl_xor(lt, 8, 64);
            lt += __shfl_xor(lt, 16, 64);
            lt += __shfl_xor(lt, 32, 64);
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                float v = o[t][e];
                v += __shfl_xor(v, 4, 64);
                v += __shfl_xor(v, 8, 64);
                v += __shfl_xor(v, 16, 64);
                v += __shfl_xor(v, 32, 64);
                o[t][e] = v;
            }
            if (lane < 4) {
#pragma unroll
                for (int e = 0; e < 16; ++e) s_o[wid][t][16 * g + e] = o[t][e];
            }
            if (lane == 0) {
                s_m[wid][t] = m[t];
                s_l[wid][t] = lt;
            }
        }
    }
};

constexpr int kF8NQ = 3;  // queries per workgroup of the multi-query instances (16 dims of q and of o per lane and query: 4 spill)
constexpr int kF8MaxB = (1500 / f8::kBlockKeys + 1 + AW - 1) / AW;  // blocks per wave of a 1500-key window

// the queries of a workgroup, pre-scaled by log2(e) / 8, at the lane's 16 dims
template <typename T, int NQ>
__device__ __forceinline__ void load_q(const T* q, size_t qrow0, int nq, int H, int h, int g, float (&qv)[NQ][16]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int t = 0; t < NQ; ++t) {
        const int tt = t < nq ? t : nq - 1;
        const T* qr = q + (qrow0 + tt) * (H * 64) + h * 64 + 16 * g;
        KVChunk<T> a, b;
        a.load(qr);
        b.load(qr + 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            qv[t][e] = a.at(e) * kLog2Scale;
            qv[t][8 + e] = b.at(e) * kLog2Scale;
        }
    }
}

// cross_attn_kernel (k_dec.hip) over records: one workgroup of 8 waves per (row run, head), queries
// [blockIdx.y * NQ, + NQ) of the run's share * Tq
template <typename T, int NQ, int PF>
__global__ __launch_bounds__(64 * AW) void cross_attn_f8_kernel(const T* __restrict__ q, const char* __restrict__ kv,
                                                                int B_layout, int H, int T_enc, int Tq,
                                                                T* __restrict__ out, const int* __restrict__ kvrow,
                                                                int share) {
    typedef AttnWaveF8<NQ, AW, PF> W;
    __shared__ float s_m[AW][NQ], s_l[AW][NQ];
    __shared__ float s_o[AW][NQ][64];
    const int bh = blockIdx.x, j = bh / H, h = bh - j * H;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int nq_all = share * Tq;
    const int c0 = (int)blockIdx.y * NQ;
    const int nq = min(NQ, nq_all - c0);
    const int kb = kvrow ? kvrow[j * share] : j;
    W aw;
    aw.init(kv + ((size_t)kb * H + h) * f8::kRecBytes, T_enc, lane, (int64_t)B_layout * H * f8::kRecBytes);
    const size_t qrow0 = (size_t)j * nq_all + c0;
    float qv[NQ][16];
    load_q<T, NQ>(q, qrow0, nq, H, h, lane & 3, qv);
    aw.template run<kF8MaxB>(wid, cdiv(T_enc, W::KB), qv, nq);
    aw.to_lds(s_m, s_l, s_o, wid, lane);
    __syncthreads();
    for (int i = tid; i < 64 * nq; i += 64 * AW) {
        const int t = i >> 6, e = i & 63;
        float M, L, O;
        attn_merge<NQ, AW>(s_m, s_l, s_o, t, e, M, L, O);
        out[(qrow0 + t) * (H * 64) + h * 64 + e] = from_f<T>(O / L);
    }
}

// cross_attn_vw_kernel over records: wave blockIdx.y of the 8-wave kernel as a workgroup of its own,
// its {o[64], m, l} as partial blockIdx.y of [rows][H][8][66]
template <typename T, int NQ, int PF>
__global__ __launch_bounds__(64) void cross_attn_vw_f8_kernel(const T* __restrict__ q, const char* __restrict__ kv,
                                                              int B_layout, int H, int T_enc, int Tq,
                                                              float* __restrict__ part, const int* __restrict__ kvrow,
                                                              int share) {
    typedef AttnWaveF8<NQ, AW, PF> W;
    __shared__ float s_m[1][NQ], s_l[1][NQ];
    __shared__ float s_o[1][NQ][64];
    const int bh = blockIdx.x, j = bh / H, h = bh - j * H;
    const int vw = blockIdx.y;
    const int lane = threadIdx.x;
    const int nq_all = share * Tq;
    const int c0 = (int)blockIdx.z * NQ;
    const int nq = min(NQ, nq_all - c0);
    const int kb = kvrow ? kvrow[j * share] : j;
    W aw;
    aw.init(kv + ((size_t)kb * H + h) * f8::kRecBytes, T_enc, lane, (int64_t)B_layout * H * f8::kRecBytes);
    const size_t qrow0 = (size_t)j * nq_all + c0;
    float qv[NQ][16];
    load_q<T, NQ>(q, qrow0, nq, H, h, lane & 3, qv);
    aw.template run<kF8MaxB>(vw, cdiv(T_enc, W::KB), qv, nq);
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

int64_t cdiv64(int64_t a, int64_t b) { return (a + b - 1) / b; }

void f8_check(const char* who, int dtype, int B, int B_layout, int H, int T_enc, int Tq, const int* kvrow, int share) {
    const std::string w(who);
    if (dtype != DT_BF16 && dtype != DT_F16) throw std::runtime_error(w + ": the fp8 cross K/V is a bf16 or f16 engine's");
    if (B < 1 || H < 1 || B_layout < 1 || T_enc < 1) throw std::runtime_error(w + ": empty shape");
    if (Tq < 1 || Tq > 4) throw std::runtime_error(w + ": 1..4 queries per sequence");
    if (share < 1 || share > 8 || B % share) throw std::runtime_error(w + ": rows per window 1..8, dividing B");
    if (share > 1 && !kvrow) throw std::runtime_error(w + ": shared windows need the window map");
    if (f8::layer_bytes(B_layout, H, T_enc) >= (int64_t)INT32_MAX)
        throw std::runtime_error(w + ": a layer's cross K/V records exceed 2^31 bytes");
}

}  // namespace

void kv_quant_f8(int dtype, const void* staged, void* recs, int layers, int B, int H, int T_enc, hipStream_t st) {
    if (dtype != DT_BF16 && dtype != DT_F16) throw std::runtime_error("kv_quant_f8: the staged layers are bf16 or f16");
    if (layers < 1 || B < 1 || H < 1 || T_enc < 1 || !staged || !recs) throw std::runtime_error("kv_quant_f8: empty or missing buffers");
    const int nblk = cdiv(T_enc, 32);
    const int64_t nrec = (int64_t)layers * nblk * B * H;
    if (nrec >= (int64_t)INT32_MAX) throw std::runtime_error("kv_quant_f8: more than 2^31 records");
    if (dtype == DT_BF16)
        hipLaunchKernelGGL(kv_quant_f8_kernel<bf16>, dim3((unsigned)nrec), dim3(256), 0, st, (const bf16*)staged, (char*)recs,
                           nblk, B * H, T_enc);
    else
        hipLaunchKernelGGL(kv_quant_f8_kernel<f16>, dim3((unsigned)nrec), dim3(256), 0, st, (const f16*)staged, (char*)recs,
                           nblk, B * H, T_enc);
    SPT_LAUNCH_CHECK();
}

void kv_dequant_f8(const void* recs, int B_layout, int H, int T_enc, int b0, int nb, float* k, float* v, float* k_scale,
                   float* v_scale, hipStream_t st) {
    if (B_layout < 1 || H < 1 || T_enc < 1 || nb < 1 || b0 < 0 || b0 + nb > B_layout || !recs || !k || !v)
        throw std::runtime_error("kv_dequant_f8: windows outside the layout or missing buffers");
    const int64_t n = (int64_t)nb * H * T_enc * 32;
    if (cdiv64(n, 256) >= (int64_t)INT32_MAX) throw std::runtime_error("kv_dequant_f8: too many elements");
    hipLaunchKernelGGL(kv_dequant_f8_kernel, dim3((unsigned)cdiv64(n, 256)), dim3(256), 0, st, (const char*)recs, B_layout, H,
                       T_enc, b0, nb, k, v, k_scale, v_scale);
    SPT_LAUNCH_CHECK();
}

void dec_cross_attn_f8(int dtype, const void* q, const void* kv, int B, int B_layout, int H, int T_enc, int Tq, void* out,
                       hipStream_t st, const int* kvrow, int share) {
    f8_check("dec_cross_attn_f8", dtype, B, B_layout, H, T_enc, Tq, kvrow, share);
    if (!q || !kv || !out) throw std::runtime_error("dec_cross_attn_f8: missing buffers");
    const int nq = share * Tq;
    // queries per workgroup: 1, or chunks of kF8NQ.
    // Every variant gives each lane the same keys in the same order, so a row's bits do not depend on it.
    const int NQ = nq == 1 ? 1 : kF8NQ;
    const dim3 grid((B / share) * H, cdiv(nq, NQ)), blk(64 * AW);
#define SPT_XA8(T, NQ_, PF)                                                                                   \
    hipLaunchKernelGGL((cross_attn_f8_kernel<T, NQ_, PF>), grid, blk, 0, st, (const T*)q, (const char*)kv, B_layout, H, \
                       T_enc, Tq, (T*)out, kvrow, share)
#define SPT_XA8_T(T)                   \
    if (NQ == 1) SPT_XA8(T, 1, 2);     \
    else SPT_XA8(T, kF8NQ, 2);
    if (dtype == DT_BF16) { SPT_XA8_T(bf16) }
    else { SPT_XA8_T(f16) }
#undef SPT_XA8_T
#undef SPT_XA8
    SPT_LAUNCH_CHECK();
}

void dec_cross_attn_vw_f8(int dtype, const void* q, const void* kv, int B, int B_layout, int H, int T_enc, int Tq,
                          float* part, hipStream_t st, const int* kvrow, int share, bool per_query) {
    f8_check("dec_cross_attn_vw_f8", dtype, B, B_layout, H, T_enc, Tq, kvrow, share);
    if (!q || !kv || !part) throw std::runtime_error("dec_cross_attn_vw_f8: needs the partials buffer");
    const int nq = share * Tq;
    const int NQ = (nq == 1 || (per_query && Tq == 1)) ? 1 : kF8NQ;
    const dim3 grid((B / share) * H, AW, cdiv(nq, NQ)), blk(64);
#define SPT_XV8(T, NQ_, PF)                                                                                      \
    hipLaunchKernelGGL((cross_attn_vw_f8_kernel<T, NQ_, PF>), grid, blk, 0, st, (const T*)q, (const char*)kv, B_layout, H, \
                       T_enc, Tq, part, kvrow, share)
#define SPT_XV8_T(T)                   \
    if (NQ == 1) SPT_XV8(T, 1, 2);     \
    else SPT_XV8(T, kF8NQ, 2);
    if (dtype == DT_BF16) { SPT_XV8_T(bf16) }
    else { SPT_XV8_T(f16) }
#undef SPT_XV8_T
#undef SPT_XV8
    SPT_LAUNCH_CHECK();
}

}  // namespace spt
