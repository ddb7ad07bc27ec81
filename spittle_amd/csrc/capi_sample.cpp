// capi_sample.cpp -- spt_debug_sample_*: the sampler kernels of k_sample.hip alone, on
// caller-supplied arrays (no engine, no model), for tests/test_gpu_sampler.py.  Each call owns its
// stream and its buffers on the device the caller names; the launches are the engine's
// (Engine::enqueue_head: dec_ts_stats + dec_finalize_ts per step, dec_beam_topk; run_beam:
// dec_kv_gather) through the launchers of kernels.h.
#include <hip/hip_runtime.h>
#include <string.h>

#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/spittle_hip.h"
#include "capi_debug.h"
#include "capi_internal.h"
#include "common.h"
#include "kernels.h"

namespace {

using namespace spt::dbg;

void check_vocab(int32_t B, int32_t n_vocab, int32_t ldl, int32_t eot, int32_t beg, int32_t blank) {
    if (B < 1 || B > 1024) throw std::runtime_error("debug_sample: need 1..1024 rows");
    if (n_vocab < 1) throw std::runtime_error("debug_sample: empty vocabulary");
    if (n_vocab > 53248) throw std::runtime_error("debug_sample: vocabulary above 53248 tokens");
    if (ldl < n_vocab) throw std::runtime_error("debug_sample: ldl below n_vocab");
    if (eot < 0 || eot >= n_vocab || beg < 0 || beg > n_vocab || blank < 0 || blank >= n_vocab)
        throw std::runtime_error("debug_sample: eot / beg / blank outside the vocabulary");
}

spt::TsParams params_of(const spt_sample_params* p) {
    spt::TsParams t{};
    t.temperature = p->temperature;
    t.suppress_blank = p->suppress_blank;
    t.no_ts = p->no_ts;
    t.max_initial = p->max_initial;
    t.n_max = p->n_max;
    t.max_tokens = p->max_tokens;
    t.seed = p->seed;
    return t;
}

}  // namespace

extern "C" {

spt_status spt_debug_sample_tokens(int32_t device, int32_t dtype, const float* logits, int32_t n_steps, int32_t B,
                                   int32_t n_vocab, int32_t ldl, int32_t eot, int32_t beg, int32_t blank,
                                   const uint32_t* suppress, const spt_sample_params* prm, const int32_t* seek,
                                   const int32_t* seek_end, int32_t* state, int32_t* done, const int32_t* forced,
                                   int32_t forced_len, int32_t out_cap, int32_t* dec_state, int32_t Tq, int32_t d,
                                   int32_t ctx, const float* emb, const float* pos, int32_t* out_tok, float* out_plog,
                                   float* out_tid, int32_t* next_tok, float* x, uint32_t* arrive, char* err,
                                   size_t errlen) {
    if (!logits || !suppress || !prm || !seek || !seek_end || !state || !done || !dec_state || !emb || !pos ||
        !out_tok || !out_plog || !out_tid || !next_tok || !x || !arrive) {
        set_err(err, errlen, "null argument");
        return SPT_ERR_INVALID_ARG;
    }
    try {
        check_vocab(B, n_vocab, ldl, eot, beg, blank);
        if (dtype != spt::DT_F32 && dtype != spt::DT_BF16 && dtype != spt::DT_F16)
            throw std::runtime_error("debug_sample: dtype is f32, bf16 or f16");
        if (n_steps < 1 || n_steps > 1024) throw std::runtime_error("debug_sample: need 1..1024 steps");
        if (out_cap < 1 || Tq < 1 || d < 1 || ctx < 1) throw std::runtime_error("debug_sample: out_cap, Tq, d, ctx >= 1");
        if (dec_state[0] < 0 || dec_state[1] < 0) throw std::runtime_error("debug_sample: negative pos0 / step");
        if ((int64_t)dec_state[0] + (int64_t)n_steps * Tq > (1 << 30) || dec_state[1] > (1 << 30))
            throw std::runtime_error("debug_sample: pos0 / step too large");
        if (forced && forced_len < 1) throw std::runtime_error("debug_sample: forced tokens without a length");
    } catch (const std::exception& e) {
        set_err(err, errlen, e.what());
        return SPT_ERR_INVALID_ARG;
    }
    if (spt_status s = device_ok(device, err, errlen)) return s;
    try {
        // host staging first: it outlives the stream's copies (sc is destroyed before it)
        const size_t nb = (size_t)B, row = nb * (size_t)ldl, cap = nb * (size_t)out_cap;
        const spt::TsParams tp = params_of(prm);
        spt::DecState ds0{dec_state[0], dec_state[1], (unsigned)dec_state[2]};
        const unsigned zero = 0;
        std::vector<uint16_t> emb16;
        Scope sc(device);
        spt::TsArgs t{};
        t.logits = nullptr; t.ldl = ldl;
        t.n_vocab = n_vocab; t.eot = eot; t.beg = beg; t.blank = blank;
        const float* d_logits = sc.up(logits, row * (size_t)n_steps);
        t.suppress = sc.up(suppress, ((size_t)n_vocab + 31) / 32);
        t.prm = sc.up(&tp, 1);
        t.seek = sc.up(seek, nb); t.seek_end = sc.up(seek_end, nb);
        t.state = sc.up(state, nb * 4);
        t.forced = forced ? sc.up(forced, nb * (size_t)forced_len) : nullptr;
        t.forced_len = forced ? forced_len : 0;
        t.next_tok = sc.alloc<int>(nb);
        t.out_tok = sc.up(out_tok, cap); t.out_plog = sc.up(out_plog, cap); t.out_tid = sc.up(out_tid, cap);
        t.out_cap = out_cap;
        t.done = sc.up(done, nb);
        if (dtype == spt::DT_F32) {
            t.emb = sc.up(emb, (size_t)n_vocab * d);
        } else {
            emb16 = to_half_storage(dtype, emb, (size_t)n_vocab * d);
            t.emb = sc.up(emb16.data(), emb16.size());
        }
        t.pos = sc.up(pos, (size_t)ctx * d);
        t.d = d; t.ctx = ctx; t.Tq = Tq;
        t.x = sc.alloc<float>(nb * d);
        t.ds = sc.up(&ds0, 1);
        t.arrive = sc.up(&zero, 1);
        t.stat = sc.alloc<float>(nb * spt::TS_CHUNKS * 6);
        HIP_CHECK(hipMemsetAsync(t.next_tok, 0, nb * sizeof(int), sc.st));
        HIP_CHECK(hipMemsetAsync(t.x, 0, nb * d * sizeof(float), sc.st));
        for (int s = 0; s < n_steps; ++s) {
            t.logits = d_logits + (size_t)s * row;
            spt::dec_ts_stats(t, B, sc.st);
            spt::dec_finalize_ts(dtype, t, B, sc.st);
        }
        sc.down(state, t.state, nb * 4);
        sc.down(done, t.done, nb);
        sc.down(out_tok, t.out_tok, cap); sc.down(out_plog, t.out_plog, cap); sc.down(out_tid, t.out_tid, cap);
        sc.down(next_tok, t.next_tok, nb);
        sc.down(x, t.x, nb * d);
        sc.down(&ds0, t.ds, 1);
        sc.down(arrive, t.arrive, 1);
        sc.sync();
        dec_state[0] = ds0.pos0; dec_state[1] = ds0.step; dec_state[2] = (int32_t)ds0.epoch;
        return SPT_OK;
    } catch (const std::exception& e) {
        set_err(err, errlen, e.what());
        return spt_classify(e);
    }
}

spt_status spt_debug_sample_beam(int32_t device, const float* logits, int32_t B, int32_t n_vocab, int32_t ldl,
                                 int32_t eot, int32_t beg, int32_t blank, const uint32_t* suppress,
                                 const spt_sample_params* prm, const int32_t* row, int32_t step, int32_t k,
                                 int32_t chunked, int32_t* cand_id, float* cand_lp, int32_t* tid, char* err,
                                 size_t errlen) {
    if (!logits || !suppress || !prm || !row || !cand_id || !cand_lp || !tid) {
        set_err(err, errlen, "null argument");
        return SPT_ERR_INVALID_ARG;
    }
    try {
        check_vocab(B, n_vocab, ldl, eot, beg, blank);
        if (step < 0) throw std::runtime_error("debug_sample: negative step");
        if (k < 1 || k > 8) throw std::runtime_error("beam_topk: 1..8 candidates");
    } catch (const std::exception& e) {
        set_err(err, errlen, e.what());
        return SPT_ERR_INVALID_ARG;
    }
    if (spt_status s = device_ok(device, err, errlen)) return s;
    try {
        const size_t nb = (size_t)B;
        const spt::TsParams tp = params_of(prm);
        Scope sc(device);
        spt::BeamArgs a{};
        a.logits = sc.up(logits, nb * (size_t)ldl); a.ldl = ldl;
        a.n_vocab = n_vocab; a.eot = eot; a.beg = beg; a.blank = blank;
        a.suppress = sc.up(suppress, ((size_t)n_vocab + 31) / 32);
        a.prm = sc.up(&tp, 1);
        a.row = sc.up(row, nb * 4);
        a.step = sc.up(&step, 1);
        a.k = k;
        a.cand_id = sc.up(cand_id, nb * 8); a.cand_lp = sc.up(cand_lp, nb * 8);
        a.tid = sc.alloc<int>(nb);
        a.stat = chunked ? sc.alloc<float>(nb * spt::TS_CHUNKS * spt::BEAM_STAT) : nullptr;
        HIP_CHECK(hipMemsetAsync(a.tid, 0, nb * sizeof(int), sc.st));
        spt::dec_beam_topk(a, B, sc.st);
        sc.down(cand_id, a.cand_id, nb * 8);
        sc.down(cand_lp, a.cand_lp, nb * 8);
        sc.down(tid, a.tid, nb);
        sc.sync();
        return SPT_OK;
    } catch (const std::exception& e) {
        set_err(err, errlen, e.what());
        return spt_classify(e);
    }
}

spt_status spt_debug_no_speech(int32_t device, const float* logits, int32_t B, int32_t n_vocab, int32_t ldl,
                               int32_t nosp, float* prob, char* err, size_t errlen) {
    if (!logits || !prob) {
        set_err(err, errlen, "null argument");
        return SPT_ERR_INVALID_ARG;
    }
    try {
        if (B < 1 || B > 1024) throw std::runtime_error("debug_no_speech: need 1..1024 rows");
        if (n_vocab < 1) throw std::runtime_error("debug_no_speech: empty vocabulary");
        if (n_vocab > 53248) throw std::runtime_error("debug_no_speech: vocabulary above 53248 tokens");
        if (ldl < n_vocab) throw std::runtime_error("debug_no_speech: ldl below n_vocab");
        if (nosp < 0 || nosp >= n_vocab) throw std::runtime_error("debug_no_speech: nosp outside the vocabulary");
    } catch (const std::exception& e) {
        set_err(err, errlen, e.what());
        return SPT_ERR_INVALID_ARG;
    }
    if (spt_status s = device_ok(device, err, errlen)) return s;
    try {
        const size_t nb = (size_t)B;
        Scope sc(device);
        const float* d_logits = sc.up(logits, nb * (size_t)ldl);
        float* d_prob = sc.alloc<float>(nb);
        float* d_stat = sc.alloc<float>(nb * spt::TS_CHUNKS * 2);
        spt::dec_no_speech(d_logits, ldl, n_vocab, nosp, d_prob, d_stat, B, sc.st);
        sc.down(prob, d_prob, nb);
        sc.sync();
        return SPT_OK;
    } catch (const std::exception& e) {
        set_err(err, errlen, e.what());
        return spt_classify(e);
    }
}

spt_status spt_debug_sample_kv_gather(int32_t device, int32_t dtype, const float* src, float* dst,
                                      const int32_t* rows, int32_t L, int32_t B, int32_t H, int32_t ctx,
                                      int32_t pos0, char* err, size_t errlen) {
    if (!src || !dst || !rows) {
        set_err(err, errlen, "null argument");
        return SPT_ERR_INVALID_ARG;
    }
    try {
        if (dtype != spt::DT_F32 && dtype != spt::DT_BF16 && dtype != spt::DT_F16)
            throw std::runtime_error("debug_sample: dtype is f32, bf16 or f16");
        if (L < 1 || B < 1 || H < 1 || ctx < 1 || (int64_t)L * B * H * ctx > (1 << 22))
            throw std::runtime_error("debug_sample: need L, B, H, ctx >= 1 and L * B * H * ctx <= 4194304");
        if (pos0 < 0 || pos0 > ctx) throw std::runtime_error("debug_sample: pos0 outside 0..ctx");
        for (int b = 0; b < B; ++b)
            if (rows[b] < 0 || rows[b] >= B) throw std::runtime_error("debug_sample: source row outside the batch");
    } catch (const std::exception& e) {
        set_err(err, errlen, e.what());
        return SPT_ERR_INVALID_ARG;
    }
    if (spt_status s = device_ok(device, err, errlen)) return s;
    try {
        const size_t n = (size_t)L * 2 * B * H * ctx * 64;
        const spt::DecState ds0{pos0, 0, 0u};
        std::vector<uint16_t> s16, d16;
        Scope sc(device);
        const spt::DecState* ds = sc.up(&ds0, 1);
        const int* d_rows = sc.up(rows, (size_t)B);
        const void* d_src;
        void* d_dst;
        if (dtype == spt::DT_F32) {
            d_src = sc.up(src, n);
            d_dst = sc.up(dst, n);
        } else {
            s16 = to_half_storage(dtype, src, n);
            d16 = to_half_storage(dtype, dst, n);
            d_src = sc.up(s16.data(), n);
            d_dst = sc.up(d16.data(), n);
        }
        spt::dec_kv_gather(dtype, d_src, d_dst, d_rows, L, B, H, ctx, ds, sc.st);
        float* out = sc.alloc<float>(n);
        spt::to_f32(dtype, d_dst, out, (int64_t)n, sc.st);
        SPT_LAUNCH_CHECK();
        sc.down(dst, out, n);
        sc.sync();
        return SPT_OK;
    } catch (const std::exception& e) {
        set_err(err, errlen, e.what());
        return spt_classify(e);
    }
}

}  // extern "C"
