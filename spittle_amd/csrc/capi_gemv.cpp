// capi_gemv.cpp -- spt_debug_gemv and spt_debug_dec_step: one gemv() launch of the decoder (k_dec.hip,
// dec_gemv.h) on dense weights with everything the decoder varies exposed -- the A source with its
// pending slabs or attention partials, lda / a_row0, x_out, the six modes, the K/V cache geometry and
// the step state, the suppression mask -- and the small kernels of the step (dec_embed, dec_finalize,
// dec_advance, dec_reset), on caller-supplied arrays (no engine, no model), for tests/test_gpu_gemv.py.
// Each call owns its stream and buffers (capi_debug.h), rounds f32 operands to the engine dtype on
// the host and returns f32.  Everything the launcher would throw on (gemv_plan), and everything that
// would read or write outside a buffer, is refused here before the device is looked for.
#include <hip/hip_runtime.h>
#include <string.h>

#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/spittle_hip.h"
#include "capi_debug.h"
#include "capi_internal.h"
#include "common.h"
#include "ggml_qpack.h"
#include "kernels.h"

namespace {

using namespace spt::dbg;

constexpr int64_t kMaxElems = (int64_t)1 << 26;  // of any one buffer of a call

void need(bool ok, const char* what) {
    if (!ok) throw std::runtime_error(what);
}

bool is_dtype(int32_t dtype) { return dtype == spt::DT_F32 || dtype == spt::DT_BF16 || dtype == spt::DT_F16; }

// a non-null address for gemv_plan, which reads only whether a pointer is null
template <typename T> T* some() { return (T*)(uintptr_t)256; }

struct GemvShape {
    bool ln, attn;
    int esz, csz;           // element sizes of A / W and of C
    int64_t cache_elems;    // GV_QKV_CACHE
    spt::GemvPlan plan;
};

// every refusal of spt_debug_gemv (throws), and what the launch then needs
GemvShape check_gemv(const spt_gemv_debug& g) {
    using namespace spt;
    GemvShape s{};
    need(is_dtype(g.dtype), "debug_gemv: dtype is f32, bf16 or f16");
    need(g.R >= 1 && g.R <= 64, "gemv: rows must be in 1..64");
    need(g.N >= 1 && g.K >= 1, "debug_gemv: need N, K >= 1");
    need((int64_t)g.N * g.K <= kMaxElems, "debug_gemv: N * K above 2^26");
    need(g.mode >= GV_BIAS && g.mode <= GV_BIAS_RESID, "debug_gemv: mode 0..5");
    need(g.a_src >= SPT_GEMV_A_DIRECT && g.a_src <= SPT_GEMV_A_ATTN, "debug_gemv: a_src is A_DIRECT, A_LN or A_ATTN");
    need(g.W && g.C, "debug_gemv: null W or C");
    need(g.ksplit >= 1 && g.ksplit <= 65535, "debug_gemv: ksplit 1..65535 (grid y)");
    s.ln = g.a_src == SPT_GEMV_A_LN;
    s.attn = g.a_src == SPT_GEMV_A_ATTN;
    s.esz = dtype_size(g.dtype);
    const bool f32out = g.mode == GV_PARTIAL || g.mode == GV_LOGITS || g.mode == GV_BIAS_RESID;
    s.csz = f32out ? 4 : s.esz;
    need(!g.merge_first || (s.attn && g.S == 8 && g.out_merged),
         "debug_gemv: merge_first needs A_ATTN with 8 chunks and out_merged");

    // what gemv() itself refuses, on stand-in addresses
    GemvArgs a{};
    a.R = g.R; a.N = g.N; a.K = g.K; a.ksplit = g.ksplit; a.lda = g.lda; a.a_row0 = g.a_row0;
    a.A = s.attn ? nullptr : some<const void>();
    a.W = some<const void>();
    if (s.ln) {
        a.ln_w = g.ln_w ? some<const float>() : nullptr;
        a.ln_b = g.ln_b ? some<const float>() : nullptr;
        for (int p = 0; p < kMaxPend; ++p) a.pend[p] = some<const float>();
        a.n_pend = g.n_pend;
    }
    if (s.attn) {
        a.apart = g.apart; a.a_splits = g.S; a.a_heads = g.H;
    }
    a.p_resid = g.p_resid;
    s.plan = gemv_plan(g.dtype, g.mode, s.ln ? A_LN : s.attn ? A_ATTN : A_DIRECT, a);

    // A: rows i * lda + a_row0 .. + K of a_count elements, on the 16-byte grid of the fragment loads
    if (!s.attn) {
        need(g.A, "debug_gemv: null A");
        need(g.a_count >= 1 && g.a_count <= kMaxElems, "debug_gemv: a_count 1..2^26");
        need(g.lda >= 0 && g.a_row0 >= 0, "debug_gemv: negative lda or a_row0");
        const int grid = s.ln ? 4 : 16 / s.esz;
        need(g.lda % grid == 0 && g.a_row0 % grid == 0, "debug_gemv: lda and a_row0 must keep A's rows 16-byte aligned");
        need((int64_t)(g.R - 1) * g.lda + g.a_row0 + g.K <= g.a_count, "debug_gemv: A read beyond a_count");
        if (s.ln) {
            need(g.n_pend == 0 || g.pend, "debug_gemv: null pending slabs");
            // x_out has A's layout: rows that overlap would be written by several waves
            need(!g.x_out || g.R == 1 || g.lda >= g.K, "debug_gemv: x_out needs lda >= K");
        } else {
            need(!g.x_out && g.n_pend == 0, "debug_gemv: pending slabs and x_out belong to A_LN");
        }
    } else {
        need(g.H >= 1 && (int64_t)g.R * g.H * g.S * 66 <= kMaxElems, "debug_gemv: partials above 2^26 elements");
        need(!g.x_out && g.n_pend == 0, "debug_gemv: pending slabs and x_out belong to A_LN");
    }

    // C
    need(g.c_count >= 1 && g.c_count <= kMaxElems, "debug_gemv: c_count 1..2^26");
    need(g.ldc >= 1 && g.c_split >= 0, "debug_gemv: ldc below 1 or negative c_split");
    int ncol = g.N;
    if (g.mode == GV_QKV_CACHE) {
        need(g.cache, "debug_gemv: GV_QKV_CACHE returns the cache");
        need(g.cache_H >= 1 && g.N == 3 * 64 * g.cache_H, "debug_gemv: GV_QKV_CACHE needs N = 3 d, d = 64 cache_H");
        need(g.B >= 1 && g.Tq >= 1 && (int64_t)g.B * g.Tq == g.R, "debug_gemv: GV_QKV_CACHE needs R = B * Tq");
        need(g.ctx >= 1 && g.pos0 >= 0 && (int64_t)g.pos0 + g.Tq <= g.ctx, "debug_gemv: pos0 + Tq beyond ctx");
        ncol = 64 * g.cache_H;
        s.cache_elems = (int64_t)2 * g.B * g.cache_H * g.ctx * 64;
        need(s.cache_elems <= kMaxElems, "debug_gemv: cache above 2^26 elements");
    }
    need(g.ldc >= ncol, "debug_gemv: ldc below the columns written");
    const int64_t item = (int64_t)(g.R - 1) * g.ldc + ncol;
    if (g.mode == GV_PARTIAL) {
        need(g.ksplit == 1 || g.c_split >= item, "debug_gemv: split-K slabs of C overlap");
        need((int64_t)(g.ksplit - 1) * g.c_split + item <= g.c_count, "debug_gemv: the last split-K slab reaches beyond c_count");
    } else {
        need(item <= g.c_count, "debug_gemv: C written beyond c_count");
    }
    if (g.mode == GV_LOGITS) {
        need(g.suppress && g.part, "debug_gemv: GV_LOGITS needs the suppression mask and returns the partials");
        need(g.suppress_words >= (g.N + 31) / 32 && g.suppress_words <= kMaxElems, "debug_gemv: suppress shorter than ceil(N / 32) words");
        need(g.n_tiles >= 1 && (int64_t)g.R * g.n_tiles * 4 <= kMaxElems, "debug_gemv: n_tiles below 1 or partials above 2^26");
        need(g.step >= 0, "debug_gemv: negative step");
    }
    return s;
}

void fill_plan(int32_t* out, const spt::GemvPlan& p) {
    if (!out) return;
    const int32_t v[8] = {p.nwv, p.ct, p.maxj, p.exact ? 1 : 0, p.rg, p.lds_bytes, p.grid_x, p.grid_y};
    memcpy(out, v, sizeof(v));
}

}  // namespace

extern "C" {

spt_status spt_debug_gemv(int32_t device, const spt_gemv_debug* args, char* err, size_t errlen) {
    using namespace spt;
    if (!args) {
        set_err(err, errlen, "null argument");
        return SPT_ERR_INVALID_ARG;
    }
    const spt_gemv_debug& g = *args;
    GemvShape s{};
    try {
        s = check_gemv(g);
        fill_plan(g.plan, s.plan);
    } catch (const std::exception& e) {
        set_err(err, errlen, e.what());
        return SPT_ERR_INVALID_ARG;
    }
    if (spt_status st = device_ok(device, err, errlen)) return st;
    try {
        const int adt = s.ln ? DT_F32 : g.dtype;           // A's storage
        const int cdt = s.csz == 4 ? DT_F32 : g.dtype;     // C's storage
        std::vector<uint16_t> w16, a16;
        Scope sc(device);
        gemv_prepare(g.dtype);
        GemvArgs a{};
        a.R = g.R; a.N = g.N; a.K = g.K; a.ksplit = g.ksplit; a.lda = g.lda; a.a_row0 = g.a_row0;
        a.W = up_as(sc, g.dtype, g.W, (size_t)g.N * g.K, w16);
        a.bias = g.bias ? sc.up(g.bias, (size_t)g.N) : nullptr;
        float* d_xout = nullptr;
        if (!s.attn) a.A = up_as(sc, adt, g.A, (size_t)g.a_count, a16);
        if (s.ln) {
            a.ln_w = sc.up(g.ln_w, (size_t)g.K);
            a.ln_b = sc.up(g.ln_b, (size_t)g.K);
            float* zero = sc.alloc<float>((size_t)g.a_count);
            HIP_CHECK(hipMemsetAsync(zero, 0, (size_t)g.a_count * sizeof(float), sc.st));
            const float* pend = g.n_pend ? sc.up(g.pend, (size_t)g.n_pend * g.a_count) : nullptr;
            for (int p = 0; p < kMaxPend; ++p) a.pend[p] = p < g.n_pend ? pend + (size_t)p * g.a_count : zero;
            a.n_pend = g.n_pend;
            if (g.x_out) a.x_out = d_xout = sc.out<float>((size_t)g.a_count);
        }
        if (s.attn) {
            a.apart = sc.up(g.apart, (size_t)g.R * g.H * g.S * 66);
            a.a_splits = g.S; a.a_heads = g.H;
            a.lda = g.K; a.a_row0 = 0;
        }
        const DecState ds0{g.pos0, g.step, 0u};
        a.st = sc.up(&ds0, 1);
        // C: the residual rows of GV_BIAS_RESID come from the caller, every other C is 0xFF
        auto new_c = [&]() -> void* {
            if (g.mode == GV_BIAS_RESID) return sc.up((const float*)g.C, (size_t)g.c_count);
            return sc.out<char>((size_t)g.c_count * s.csz);
        };
        void* d_C = new_c();
        void* d_C2 = g.merge_first ? new_c() : nullptr;  // the second projection's C, before g.C is written
        a.C = d_C; a.ldc = g.ldc; a.c_split = g.c_split;
        if (g.mode == GV_PARTIAL && g.p_resid) a.p_resid = sc.up(g.p_resid, (size_t)(g.R - 1) * g.ldc + g.N);
        void* d_cache = nullptr;
        if (g.mode == GV_QKV_CACHE) {
            d_cache = sc.out<char>((size_t)s.cache_elems * s.esz);
            a.cache = d_cache; a.cache_B = g.B; a.cache_H = g.cache_H; a.cache_ctx = g.ctx; a.Tq = g.Tq;
        }
        float* d_part = nullptr;
        if (g.mode == GV_LOGITS) {
            a.suppress = sc.up(g.suppress, (size_t)g.suppress_words);
            a.blank0 = g.blank0; a.blank1 = g.blank1;
            d_part = sc.out<float>((size_t)g.R * g.n_tiles * 4);
            a.part = d_part; a.n_tiles = g.n_tiles;
        }
        gemv(g.dtype, g.mode, s.ln ? A_LN : s.attn ? A_ATTN : A_DIRECT, a, sc.st);
        SPT_LAUNCH_CHECK();
        down_f32(sc, cdt, d_C, g.C, (size_t)g.c_count);
        if (d_xout) sc.down(g.x_out, (const float*)d_xout, (size_t)g.a_count);
        if (d_cache) down_f32(sc, g.dtype, d_cache, g.cache, (size_t)s.cache_elems);
        if (d_part) sc.down(g.part, (const float*)d_part, (size_t)g.R * g.n_tiles * 4);
        if (g.merge_first) {
            // the merge kernel's rows, projected by the A_DIRECT instance on the same W, bias and C
            void* d_m = sc.out<char>((size_t)g.R * g.K * s.esz);
            dec_attn_part_merge(g.dtype, a.apart, g.R, g.H, d_m, sc.st);
            SPT_LAUNCH_CHECK();
            GemvArgs b = a;
            b.apart = nullptr; b.a_splits = 0; b.a_heads = 0;
            b.A = d_m; b.lda = g.K; b.a_row0 = 0;
            b.C = d_C2;
            gemv(g.dtype, g.mode, A_DIRECT, b, sc.st);
            SPT_LAUNCH_CHECK();
            sc.down(g.out_merged, (const float*)d_C2, (size_t)g.c_count);
        }
        sc.sync();
        return SPT_OK;
    } catch (const std::exception& e) {
        set_err(err, errlen, e.what());
        return spt_classify(e);
    }
}

spt_status spt_debug_dec_step(int32_t device, const spt_dec_step_debug* args, char* err, size_t errlen) {
    using namespace spt;
    if (!args) {
        set_err(err, errlen, "null argument");
        return SPT_ERR_INVALID_ARG;
    }
    const spt_dec_step_debug& g = *args;
    std::vector<uint8_t> packed;
    const bool emb_op = g.op == SPT_DEC_STEP_EMBED || g.op == SPT_DEC_STEP_FINALIZE;
    try {
        need(g.op >= SPT_DEC_STEP_EMBED && g.op <= SPT_DEC_STEP_RESET, "debug_dec_step: op 0..3");
        need(g.state, "debug_dec_step: null state");
        need(g.state[0] >= 0 && g.state[1] >= 0 && g.state[3] >= 0, "debug_dec_step: negative pos0, step or arrive");
        if (g.op == SPT_DEC_STEP_ADVANCE) need(g.n_advance >= 0, "debug_dec_step: negative n_advance");
        if (emb_op) {
            need(is_dtype(g.dtype), "debug_dec_step: dtype is f32, bf16 or f16");
            need(g.B >= 1 && g.Tq >= 1 && (int64_t)g.B * g.Tq <= 4096, "debug_dec_step: need B, Tq >= 1, B * Tq <= 4096");
            need(g.d >= 1 && g.ctx >= 1 && g.n_vocab >= 1, "debug_dec_step: need d, ctx, n_vocab >= 1");
            need((int64_t)g.n_vocab * g.d <= kMaxElems && (int64_t)g.ctx * g.d <= kMaxElems,
                 "debug_dec_step: embedding above 2^26 elements");
            need(g.pos && g.x, "debug_dec_step: null pos or x");
            if (g.emb_q) {
                need(g.dtype != DT_F32, "dec_embed: a packed embedding needs a bf16 or f16 engine");
                QPackGeom qg;
                int blck, bb;
                need(qpack_geom(g.emb_q, &qg), "debug_dec_step: no resident layout for this ggml type");
                ggml_block_geom(g.emb_q, &blck, &bb);
                need(g.d % QPACK_KS == 0, "debug_dec_step: a packed embedding needs d a multiple of 128");
                need(g.emb_blocks && g.emb_blocks_bytes == (size_t)g.n_vocab * (size_t)(g.d / 32) * (size_t)bb,
                     "debug_dec_step: emb_blocks_bytes is not the size of [n_vocab][d / 32] blocks");
                packed.resize((size_t)qpack_bytes(g.emb_q, g.n_vocab, g.d));
                need(qpack_rows(g.emb_q, (const uint8_t*)g.emb_blocks, g.emb_blocks_bytes, g.n_vocab, g.d, packed.data()),
                     "debug_dec_step: packing failed");
            } else {
                need(g.emb, "debug_dec_step: null emb");
            }
        }
        if (g.op == SPT_DEC_STEP_EMBED) {
            need(g.tok, "debug_dec_step: null tok");
            need((int64_t)g.state[0] + g.Tq <= g.ctx, "debug_dec_step: pos0 + Tq beyond ctx");
            for (int r = 0; r < g.B * g.Tq; ++r)
                need(g.tok[r] >= 0 && g.tok[r] < g.n_vocab, "debug_dec_step: token outside 0..n_vocab-1");
        }
        if (g.op == SPT_DEC_STEP_FINALIZE) {
            need(g.part && g.done && g.next_tok && g.out_tok && g.out_top1 && g.out_top2, "debug_dec_step: null argument");
            need(g.n_steps >= 1 && g.n_steps <= 64, "debug_dec_step: n_steps 1..64");
            need(g.n_tiles >= 1 && (int64_t)g.n_steps * g.B * g.n_tiles * 4 <= kMaxElems, "debug_dec_step: n_tiles below 1 or partials above 2^26");
            need(g.out_cap >= 1 && (int64_t)g.B * g.out_cap <= kMaxElems, "debug_dec_step: out_cap below 1");
            need(g.forced_len >= 0 && (!g.forced || g.forced_len >= 1), "debug_dec_step: forced needs forced_len >= 1");
            // the next token's row is read from emb: eot is what every out-of-range choice becomes
            need(g.eot >= 0 && g.eot < g.n_vocab, "debug_dec_step: eot outside 0..n_vocab-1");
            need(g.state[3] == 0, "debug_dec_step: dec_finalize starts from arrive == 0");
            need((int64_t)g.state[0] + (int64_t)g.n_steps * g.Tq < ((int64_t)1 << 30), "debug_dec_step: pos0 too large");
        }
    } catch (const std::exception& e) {
        set_err(err, errlen, e.what());
        return SPT_ERR_INVALID_ARG;
    }
    if (spt_status st = device_ok(device, err, errlen)) return st;
    try {
        Scope sc(device);
        const DecState ds0{g.state[0], g.state[1], (unsigned)g.state[2]};
        const unsigned arrive0 = (unsigned)g.state[3];
        DecState* d_ds = sc.up(&ds0, 1);
        unsigned* d_arrive = sc.up(&arrive0, 1);
        std::vector<uint16_t> e16;
        const void* d_emb = nullptr;
        const float* d_pos = nullptr;
        if (emb_op) {
            d_emb = g.emb_q ? (const void*)sc.up(packed.data(), packed.size())
                            : up_as(sc, g.dtype, g.emb, (size_t)g.n_vocab * g.d, e16);
            d_pos = sc.up(g.pos, (size_t)g.ctx * g.d);
        }
        if (g.op == SPT_DEC_STEP_EMBED) {
            const int R = g.B * g.Tq;
            float* d_x = sc.out<float>((size_t)R * g.d);
            dec_embed(g.dtype, sc.up(g.tok, (size_t)R), R, g.Tq, g.d, d_emb, g.emb_q, d_pos, d_ds, d_x, sc.st);
            SPT_LAUNCH_CHECK();
            sc.down(g.x, (const float*)d_x, (size_t)R * g.d);
        } else if (g.op == SPT_DEC_STEP_FINALIZE) {
            const size_t per = (size_t)g.B * g.n_tiles * 4, n_out = (size_t)g.B * g.out_cap;
            const float* d_part = sc.up(g.part, per * g.n_steps);
            int* d_next = sc.out<int>((size_t)g.n_steps * g.B);
            float* d_x = sc.out<float>((size_t)g.n_steps * g.B * g.d);
            int* d_tok = sc.out<int>(n_out);
            float* d_t1 = sc.out<float>(n_out);
            float* d_t2 = sc.out<float>(n_out);
            int* d_done = sc.up((const int*)g.done, (size_t)g.B);
            FinalizeArgs f{};
            f.n_tiles = g.n_tiles; f.eot = g.eot; f.ignore_eot = g.ignore_eot; f.n_vocab = g.n_vocab;
            f.forced = g.forced ? sc.up(g.forced, (size_t)g.B * g.forced_len) : nullptr;
            f.forced_len = g.forced_len;
            f.out_tok = d_tok; f.out_top1 = d_t1; f.out_top2 = d_t2; f.out_cap = g.out_cap;
            f.done = d_done;
            f.emb = d_emb; f.pos = d_pos; f.d = g.d; f.ctx = g.ctx; f.Tq = g.Tq;
            f.ds = d_ds; f.arrive = d_arrive; f.emb_q = g.emb_q;
            for (int s = 0; s < g.n_steps; ++s) {
                f.part = d_part + (size_t)s * per;
                f.next_tok = d_next + (size_t)s * g.B;
                f.x = d_x + (size_t)s * g.B * g.d;
                dec_finalize(g.dtype, f, g.B, sc.st);
                SPT_LAUNCH_CHECK();
            }
            sc.down(g.next_tok, (const int*)d_next, (size_t)g.n_steps * g.B);
            sc.down(g.x, (const float*)d_x, (size_t)g.n_steps * g.B * g.d);
            sc.down(g.out_tok, (const int*)d_tok, n_out);
            sc.down(g.out_top1, (const float*)d_t1, n_out);
            sc.down(g.out_top2, (const float*)d_t2, n_out);
            sc.down(g.done, (const int*)d_done, (size_t)g.B);
        } else if (g.op == SPT_DEC_STEP_ADVANCE) {
            dec_advance(d_ds, g.n_advance, sc.st);
            SPT_LAUNCH_CHECK();
        } else {
            dec_reset(d_ds, d_arrive, sc.st);
            SPT_LAUNCH_CHECK();
        }
        DecState ds1{};
        unsigned arrive1 = 0;
        sc.down(&ds1, (const DecState*)d_ds, 1);
        sc.down(&arrive1, (const unsigned*)d_arrive, 1);
        sc.sync();
        g.state[0] = ds1.pos0; g.state[1] = ds1.step; g.state[2] = (int32_t)ds1.epoch; g.state[3] = (int32_t)arrive1;
        return SPT_OK;
    } catch (const std::exception& e) {
        set_err(err, errlen, e.what());
        return spt_classify(e);
    }
}

}  // extern "C"
