// k_prefill.hip -- attention of the decoder's block prefill: all P positions of a prompt
// prefix ([prev] + prompt tokens, P <= n_text_ctx) in one launch per layer, where the chunked prefill
// runs dec_self_attn / dec_cross_attn once per 4 positions.
//
//   dec_prefill_self_attn   qkv [B*P][3*d] as the QKV GEMM stores it -> the K and V rows into the self
//                           cache at positions 0..P-1 (to_cache: the f16 engine's clamp), and the causal
//                           attention of query t over keys 0..t as stored -> out [B*P][d]
//   dec_prefill_cross_attn  q [B*P][d] over one layer of the blocked cross K/V cache (kv_offset), all
//                           T_enc real keys, through the rows' window map -> out [B*P][d]
//
// One kernel text for both.  Workgroup = 4 waves = 128 queries of one (sequence, head), 32 queries per
// wave; grid (ceil(P / 128), H, B).  Keys go by in tiles of 64, staged global -> registers -> LDS
// (double buffered: tile kt + 1's loads are in flight under tile kt's products; one barrier per tile).
// Register staging, not the encoder's LDS DMA, because the rows are touched on the way: the f16 clamp,
// and rows that are no real key (past T_enc in the last 32-key block, past the workgroup's last query)
// are stored as zeros whatever the memory holds, so nothing they hold can reach a product.
// LDS image as k_attn.hip's attn_bf16_kernel / attn_f32_kernel: rows of 64 elements (128 / 256 B), the
// K tile's 16-byte chunks XOR-swizzled with the row (ds_read_b128 of 32 rows x one chunk column:
// conflict-free), the V tile plain (ds_read_b64_tr_b16 / ds_read_b32 along a row).
// Scores are computed transposed, S^T = K . Q^T, so a lane owns one query column: the online softmax
// is in-lane plus one cross-half shuffle, and the probabilities are the B operand of O^T += V^T . P^T
// with no lane movement (CDNA4 accumulator-as-operand layout).
//   bf16 / f16: v_mfma_f32_32x32x16_{bf16,f16}; scores, maximum and sum in f32; P rounded to the dtype
//               once (v_cvt_pk) before PV; re-based only past a 2^8 growth (P <= 2^8).
//   f32:        v_mfma_f32_32x32x2_f32, f32 throughout.  Roundings on a score: the MFMA's 64
//               accumulations, one for the maximum's scale and one for the score's fused scale and
//               shift: 66 (the chain of the test's f32 bar).
// A key a query may not see gets the score -inf before the maximum and the exponential, so its
// probability is exp2(-inf) = 0 by assignment, not by a product; every query sees key 0, so no
// maximum stays -inf.  A wave whose queries all lie before a tile skips the tile's arithmetic (never
// the barrier).  No workgroup waits on another: each reads K and V of the keys it needs from the
// launch's inputs (self: from qkv, clamped as the store clamps them, not from the cache rows another
// workgroup writes).
#include "common.h"
#include "kernels.h"

#include <type_traits>

namespace spt {

namespace {

constexpr float kScaleLog2 = 0.125f * 1.4426950408889634f;  // (1 / sqrt(64)) * log2(e)
constexpr float kLazy = 8.0f;

typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;  // one 16-byte chunk, storable into LDS

struct PfArgs {
    const void* q; int ldq;     // query rows: row b * P + t at q + row * ldq (+ h * 64)
    const void* kv;             // self: nullptr (K | V follow q in the qkv row); cross: the layer
    void* cache; int cache_B, ctx;  // self: [2][cache_B][H][ctx][64], at the slice's first sequence
    const int* kvrow; int share;    // cross: the window map
    int B_layout, T_enc;
    int P, H;
    void* out;
};

__device__ __forceinline__ int key_of(int kt2, int r, int hf) { return 32 * kt2 + (r & 3) + 8 * (r >> 2) + 4 * hf; }

template <typename ET>
__device__ __forceinline__ f32x16 mfma32(bf16x8 a, bf16x8 b, f32x16 c) {
    if constexpr (std::is_same<ET, f16>::value)
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
template <typename ET>
__device__ __forceinline__ uint32_t pack2(float a, float b) {
    const f32x2 pv = {a, b};
    if constexpr (std::is_same<ET, f16>::value) return __builtin_bit_cast(uint32_t, __builtin_convertvector(pv, f16x2v));
    else return __builtin_bit_cast(uint32_t, __builtin_convertvector(pv, bf16x2v));
}

template <typename T, bool SELF>
__global__ __launch_bounds__(256, sizeof(T) == 2 ? 2 : 1) void prefill_attn_kernel(PfArgs a) {
    constexpr int ES = (int)sizeof(T), ROWB = 64 * ES, CH = ROWB / 16, TILEB = 64 * ROWB;
    constexpr int EPC = 16 / ES;              // elements per 16-byte chunk
    constexpr int NPRE = 2 * 64 * CH / 256;   // chunks of a K + V tile per thread: 4 / 8
    __shared__ __attribute__((aligned(16))) char smem[2 * 2 * TILEB];  // [buf][K|V][64 keys][ROWB]
    const int P = a.P, H = a.H, d = H * 64;
    const int qt = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int l32 = lane & 31, hf = lane >> 5;
    const T* qbase = (const T*)a.q + (size_t)b * P * a.ldq + h * 64;
    const int nk = SELF ? min(P, qt * 128 + 128) : a.T_enc;  // keys this workgroup stages
    const T* kvw = nullptr;
    if constexpr (!SELF) {
        const int w = a.kvrow ? a.kvrow[b / a.share * a.share] : b;
        kvw = (const T*)a.kv + ((size_t)w * H + h) * 4096;
    }
    // the 64 elements of key `key` (< nk): kvi 0 = K, 1 = V
    auto src = [&](int kvi, int key) -> const T* {
        if constexpr (SELF) return qbase + (size_t)key * a.ldq + (1 + kvi) * d;
        else return kvw + (size_t)(key >> 5) * a.B_layout * H * 4096 + kvi * 2048 + (key & 31) * 64;
    };
    auto ld16 = [&](const T* p) -> u32x4 {
        u32x4 v = *(const u32x4*)p;
        if constexpr (SELF && std::is_same<T, f16>::value) {  // as the cache holds them
            union { u32x4 u; f16 e[8]; } x;
            x.u = v;
#pragma unroll
            for (int i = 0; i < 8; ++i) x.e[i] = to_cache<f16>((float)x.e[i]);
            v = x.u;
        }
        return v;
    };
    if constexpr (SELF) {  // this workgroup's 128 positions of the self cache
        T* cache = (T*)a.cache;
#pragma unroll
        for (int i = 0; i < 2 * 128 * CH / 256; ++i) {
            const int c = tid + 256 * i;
            const int kvi = c / (128 * CH), row = (c / CH) & 127, ch = c % CH;
            const int key = qt * 128 + row;
            if (key < P) {
                const u32x4 v = ld16(src(kvi, key) + EPC * ch);
                *(u32x4*)(cache + ((((size_t)kvi * a.cache_B + b) * H + h) * a.ctx + key) * 64 + EPC * ch) = v;
            }
        }
    }
    const int q_abs = qt * 128 + wid * 32 + l32;
    const int qa = min(q_abs, P - 1);  // rows past P repeat the last query (never stored)
    const int q0 = min(qt * 128 + wid * 32, P - 1), q1 = min(qt * 128 + wid * 32 + 31, P - 1);
    const int kmax = SELF ? qa : nk - 1;     // the last key this lane's query sees
    const int wave_kmin = SELF ? q0 : nk - 1, wave_kmax = SELF ? q1 : nk - 1;

    u32x4 pre[NPRE];
    auto fetch = [&](int kt) {
#pragma unroll
        for (int i = 0; i < NPRE; ++i) {
            const int c = tid + 256 * i;
            const int kvi = c / (64 * CH), row = (c / CH) & 63, ch = c % CH;
            const int key = kt * 64 + row;
            pre[i] = key < nk ? ld16(src(kvi, key) + EPC * ch) : u32x4{0u, 0u, 0u, 0u};
        }
    };
    auto stash = [&](int buf) {
#pragma unroll
        for (int i = 0; i < NPRE; ++i) {
            const int c = tid + 256 * i;
            const int kvi = c / (64 * CH), row = (c / CH) & 63, ch = c % CH;
            const int sw = kvi == 0 ? (ch ^ (row & (CH - 1))) : ch;
            *(SPT_LDS u32x4*)((SPT_LDS char*)smem + (buf * 2 + kvi) * TILEB + row * ROWB + (sw << 4)) = pre[i];
        }
    };

    float m_run = -INFINITY, l_run = 0.f;
    f32x16 o[2];
#pragma unroll
    for (int i = 0; i < 16; ++i) { o[0][i] = 0.f; o[1][i] = 0.f; }

    const int nkt = cdiv(nk, 64);
    fetch(0);
    stash(0);
    __syncthreads();

    if constexpr (ES == 2) {
        bf16x8 qf[4];
        {
            const T* qp = qbase + (size_t)qa * a.ldq;
#pragma unroll
            for (int s = 0; s < 4; ++s) qf[s] = *(const bf16x8*)(qp + 16 * s + 8 * hf);
        }
        for (int kt = 0; kt < nkt; ++kt) {
            const int cur = kt & 1;
            if (kt + 1 < nkt) fetch(kt + 1);
            if (kt * 64 <= wave_kmax) {
                const SPT_LDS char* lk = (const SPT_LDS char*)smem + (cur * 2) * TILEB;
                const SPT_LDS char* lv = lk + TILEB;
                f32x16 s[2];
#pragma unroll
                for (int kt2 = 0; kt2 < 2; ++kt2) {
#pragma unroll
                    for (int i = 0; i < 16; ++i) s[kt2][i] = 0.f;
                    const int row = 32 * kt2 + l32;
#pragma unroll
                    for (int st = 0; st < 4; ++st) {
                        const int c = 2 * st + hf;
                        const bf16x8 ka = *(const SPT_LDS bf16x8*)(lk + row * 128 + ((c ^ (row & 7)) << 4));
                        s[kt2] = mfma32<T>(ka, qf[st], s[kt2]);
                    }
                }
                if (kt * 64 + 63 > wave_kmin) {
#pragma unroll
                    for (int kt2 = 0; kt2 < 2; ++kt2)
#pragma unroll
                        for (int r = 0; r < 16; ++r)
                            if (kt * 64 + key_of(kt2, r, hf) > kmax) s[kt2][r] = -INFINITY;
                }
                float mloc = -INFINITY;
#pragma unroll
                for (int r = 0; r < 16; ++r) mloc = fmaxf(mloc, fmaxf(s[0][r], s[1][r]));
                mloc = fmaxf(mloc, __shfl_xor(mloc, 32, 64));
                // lazy re-basing (attn_bf16_kernel): the running maximum moves only past a 2^kLazy growth
                float alpha = 1.0f;
                if (__any((mloc - m_run) * kScaleLog2 > kLazy)) {
                    const float m_new = fmaxf(m_run, mloc);
                    alpha = __builtin_amdgcn_exp2f((m_run - m_new) * kScaleLog2);
                    m_run = m_new;
#pragma unroll
                    for (int i = 0; i < 16; ++i) { o[0][i] *= alpha; o[1][i] *= alpha; }
                }
                const float mc = m_run * kScaleLog2;
                float lsum = 0.f;
                union { bf16x8 v; uint32_t w[4]; } pu[2][2];
#pragma unroll
                for (int kt2 = 0; kt2 < 2; ++kt2)
#pragma unroll
                    for (int r = 0; r < 16; r += 2) {
                        const float p0 = __builtin_amdgcn_exp2f(fmaf(s[kt2][r], kScaleLog2, -mc));
                        const float p1 = __builtin_amdgcn_exp2f(fmaf(s[kt2][r + 1], kScaleLog2, -mc));
                        lsum += p0 + p1;
                        pu[kt2][r >> 3].w[(r & 7) >> 1] = pack2<T>(p0, p1);
                    }
                l_run = l_run * alpha + lsum;
                // O^T += V^T . P^T
                const int g = lane >> 4, i16 = lane & 15;
#pragma unroll
                for (int dt = 0; dt < 2; ++dt) {
                    const int col = 32 * dt + 16 * (g & 1) + 4 * (i16 & 3);
#pragma unroll
                    for (int kt2 = 0; kt2 < 2; ++kt2)
#pragma unroll
                        for (int sp = 0; sp < 2; ++sp) {
                            const int key0 = 32 * kt2 + 16 * sp + 4 * hf + (i16 >> 2);
                            const bf16x4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                                (SPT_LDS bf16x4v*)(lv + key0 * 128 + col * 2));
                            const bf16x4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                                (SPT_LDS bf16x4v*)(lv + (key0 + 8) * 128 + col * 2));
                            const bf16x8 va = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
                            o[dt] = mfma32<T>(va, pu[kt2][sp].v, o[dt]);
                        }
                }
            }
            if (kt + 1 < nkt) stash(cur ^ 1);
            __syncthreads();
        }
    } else {
        float qf[32];
        {
            const float* qp = (const float*)qbase + (size_t)qa * a.ldq + 32 * hf;
#pragma unroll
            for (int s = 0; s < 32; s += 4) {
                const float4 v = *(const float4*)(qp + s);
                qf[s] = v.x; qf[s + 1] = v.y; qf[s + 2] = v.z; qf[s + 3] = v.w;
            }
        }
        for (int kt = 0; kt < nkt; ++kt) {
            const int cur = kt & 1;
            if (kt + 1 < nkt) fetch(kt + 1);
            if (kt * 64 <= wave_kmax) {
                const SPT_LDS char* lk = (const SPT_LDS char*)smem + (cur * 2) * TILEB;
                const SPT_LDS float* lv = (const SPT_LDS float*)(lk + TILEB);
                f32x16 s[2];
#pragma unroll
                for (int kt2 = 0; kt2 < 2; ++kt2) {
#pragma unroll
                    for (int i = 0; i < 16; ++i) s[kt2][i] = 0.f;
                    const int row = 32 * kt2 + l32;
#pragma unroll
                    for (int c8 = 0; c8 < 8; ++c8) {
                        const int c = 8 * hf + c8;
                        const f32x4 kv = *(const SPT_LDS f32x4*)(lk + row * 256 + ((c ^ (row & 15)) << 4));
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            s[kt2] = __builtin_amdgcn_mfma_f32_32x32x2f32(kv[e], qf[4 * c8 + e], s[kt2], 0, 0, 0);
                    }
                }
                if (kt * 64 + 63 > wave_kmin) {
#pragma unroll
                    for (int kt2 = 0; kt2 < 2; ++kt2)
#pragma unroll
                        for (int r = 0; r < 16; ++r)
                            if (kt * 64 + key_of(kt2, r, hf) > kmax) s[kt2][r] = -INFINITY;
                }
                float mloc = -INFINITY;
#pragma unroll
                for (int r = 0; r < 16; ++r) mloc = fmaxf(mloc, fmaxf(s[0][r], s[1][r]));
                mloc = fmaxf(mloc, __shfl_xor(mloc, 32, 64));
                const float m_new = fmaxf(m_run, mloc);
                const float alpha = exp2f((m_run - m_new) * kScaleLog2);
                const float mc = m_new * kScaleLog2;
                float lsum = 0.f;
#pragma unroll
                for (int kt2 = 0; kt2 < 2; ++kt2)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float p = exp2f(fmaf(s[kt2][r], kScaleLog2, -mc));
                        s[kt2][r] = p;
                        lsum += p;
                    }
                l_run = l_run * alpha + lsum;
                m_run = m_new;
#pragma unroll
                for (int i = 0; i < 16; ++i) { o[0][i] *= alpha; o[1][i] *= alpha; }
#pragma unroll
                for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                    for (int kt2 = 0; kt2 < 2; ++kt2)
#pragma unroll
                        for (int st = 0; st < 16; ++st) {
                            const float va = lv[key_of(kt2, st, hf) * 64 + 32 * dt + l32];
                            o[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(va, s[kt2][st], o[dt], 0, 0, 0);
                        }
            }
            if (kt + 1 < nkt) stash(cur ^ 1);
            __syncthreads();
        }
    }
    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    const float inv = 1.0f / l_tot;
    if (q_abs < P) {
        T* orow = (T*)a.out + ((size_t)b * P + q_abs) * d + h * 64;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int gg = 0; gg < 4; ++gg) {
                const int dd = 32 * dt + 8 * gg + 4 * hf;
                const float v0 = o[dt][4 * gg + 0] * inv, v1 = o[dt][4 * gg + 1] * inv;
                const float v2 = o[dt][4 * gg + 2] * inv, v3 = o[dt][4 * gg + 3] * inv;
                if constexpr (ES == 2) *(uint2*)(orow + dd) = make_uint2(pack2<T>(v0, v1), pack2<T>(v2, v3));
                else *(float4*)(orow + dd) = make_float4(v0, v1, v2, v3);
            }
    }
}

template <bool SELF>
void launch(int dtype, const PfArgs& a, int B, hipStream_t st) {
    const dim3 grid(cdiv(a.P, 128), a.H, B), block(256);
    if (dtype == DT_BF16) hipLaunchKernelGGL((prefill_attn_kernel<bf16, SELF>), grid, block, 0, st, a);
    else if (dtype == DT_F16) hipLaunchKernelGGL((prefill_attn_kernel<f16, SELF>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((prefill_attn_kernel<float, SELF>), grid, block, 0, st, a);
    SPT_LAUNCH_CHECK();
}

}  // namespace

void prefill_attn_check(int dtype, int B, int H, int P) {
    if (dtype != DT_F32 && dtype != DT_BF16 && dtype != DT_F16) throw std::runtime_error("prefill attention: dtype is f32, bf16 or f16");
    if (B < 1 || B > 65535 || H < 1 || H > 65535) throw std::runtime_error("prefill attention: need 1..65535 sequences and heads");
    if (P < 1) throw std::runtime_error("prefill attention: need at least one position");
    if ((int64_t)B * P * 3 * H * 64 >= (int64_t)INT32_MAX) throw std::runtime_error("prefill attention: B * P * 3 * H * 64 exceeds 2^31");
}

void dec_prefill_self_attn(int dtype, const void* qkv, void* cache, int B, int cache_B, int H, int ctx, int P, void* out,
                           hipStream_t st) {
    prefill_attn_check(dtype, B, H, P);
    if (P > ctx) throw std::runtime_error("dec_prefill_self_attn: more positions than the cache holds");
    if (cache_B < B) throw std::runtime_error("dec_prefill_self_attn: the cache holds fewer sequences than the launch");
    PfArgs a{};
    a.q = qkv; a.ldq = 3 * H * 64; a.cache = cache; a.cache_B = cache_B; a.ctx = ctx; a.P = P; a.H = H; a.out = out;
    launch<true>(dtype, a, B, st);
}

void dec_prefill_cross_attn(int dtype, const void* q, const void* kv, int B, int B_layout, int H, int T_enc, int P,
                            void* out, hipStream_t st, const int* kvrow, int share) {
    prefill_attn_check(dtype, B, H, P);
    if (T_enc < 1 || B_layout < 1) throw std::runtime_error("dec_prefill_cross_attn: need T_enc, B_layout >= 1");
    if (share < 1 || B % share) throw std::runtime_error("dec_prefill_cross_attn: rows per window must divide B");
    if (share > 1 && !kvrow) throw std::runtime_error("dec_prefill_cross_attn: shared windows need the window map");
    if (kv_layer_elems(B_layout, H, T_enc) >= (int64_t)INT32_MAX)
        throw std::runtime_error("dec_prefill_cross_attn: a layer's cross K/V exceeds 2^31 elements");
    PfArgs a{};
    a.q = q; a.ldq = H * 64; a.kv = kv; a.kvrow = kvrow; a.share = share; a.B_layout = B_layout; a.T_enc = T_enc;
    a.P = P; a.H = H; a.out = out;
    launch<false>(dtype, a, B, st);
}

}  // namespace spt
