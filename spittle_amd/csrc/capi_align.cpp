// capi_align.cpp -- spt_debug_align_*: the token-alignment kernels of k_align.hip alone (align_qk,
// align_norm, align_dtw) on caller-supplied arrays (no engine, no model), for tests/test_gpu_align.py,
// and the host-only word grouping.  As in capi_attn.cpp each call owns its stream and its buffers on
// the device the caller names, rounds f32 inputs to the engine dtype on the host, and refuses every
// shape a launcher would throw on, or that would read or write outside a buffer, before any launch.
#include <hip/hip_runtime.h>
#include <string.h>

#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/spittle_hip.h"
#include "align_host.h"
#include "capi_debug.h"
#include "capi_internal.h"
#include "common.h"
#include "kernels.h"

namespace {

using namespace spt::dbg;

constexpr int64_t kMaxElems = (int64_t)1 << 26;  // of any one buffer of a call

// each sequence's rows / keys in use: 0..cap
void check_counts(const char* what, const int32_t* v, int B, int cap) {
    for (int b = 0; b < B; ++b)
        if (v[b] < 0 || v[b] > cap) throw std::runtime_error(std::string("debug_align: ") + what + " outside 0..cap");
}

}  // namespace

extern "C" {

spt_status spt_debug_align_qk(int32_t device, int32_t dtype, const float* q, const float* k, float pad_value, int32_t B,
                              int32_t B_layout, int32_t H, int32_t T_enc, int32_t Tq, int32_t pos0,
                              const int32_t* kvrow, const int32_t* heads, int32_t n_heads, const int32_t* M,
                              int32_t N_cap, int32_t M_cap, float* p, char* err, size_t errlen) {
    if (!q || !k || !heads || !M || !p) {
        set_err(err, errlen, "null argument");
        return SPT_ERR_INVALID_ARG;
    }
    try {
        if (dtype != spt::DT_F32 && dtype != spt::DT_BF16 && dtype != spt::DT_F16)
            throw std::runtime_error("debug_align_qk: dtype is f32, bf16 or f16");
        if (B < 1 || B > 1024 || B_layout < 1 || H < 1) throw std::runtime_error("debug_align_qk: need 1..1024 rows, H, B_layout >= 1");
        if (T_enc < 1 || T_enc > spt::kAlignMaxKeys) throw std::runtime_error("align_qk: 1..3072 keys");
        if (Tq < 1 || Tq > 4) throw std::runtime_error("align_qk: 1..4 queries per sequence");
        if (n_heads < 1 || n_heads > 512) throw std::runtime_error("debug_align_qk: 1..512 alignment heads");
        if (N_cap < 1 || M_cap < 1) throw std::runtime_error("debug_align_qk: need N_cap, M_cap >= 1");
        if (pos0 < 0 || (int64_t)pos0 + Tq > N_cap) throw std::runtime_error("align_qk: rows beyond the workspace");
        if (M_cap > T_enc) throw std::runtime_error("debug_align_qk: M_cap beyond the keys");
        check_counts("M", M, B, M_cap);
        for (int i = 0; i < n_heads; ++i)
            if (heads[i] < 0 || heads[i] >= H) throw std::runtime_error("debug_align_qk: head outside 0..H");
        for (int b = 0; b < B; ++b) {
            const int w = kvrow ? kvrow[b] : b;
            if (w < 0 || w >= B_layout) throw std::runtime_error("debug_align_qk: window outside the layout");
        }
        if (spt::kv_layer_elems(B_layout, H, T_enc) > kMaxElems || (int64_t)B * Tq * H * 64 > kMaxElems ||
            (int64_t)B * n_heads * N_cap * M_cap > kMaxElems)
            throw std::runtime_error("debug_align_qk: buffers above 2^26 elements");
    } catch (const std::exception& e) {
        set_err(err, errlen, e.what());
        return SPT_ERR_INVALID_ARG;
    }
    if (spt_status s = device_ok(device, err, errlen)) return s;
    try {
        // the layer as the K/V GEMM's epilogue writes it (kv_offset): the V halves and the keys of the
        // last 32-key block past T_enc hold pad_value
        const size_t n_kv = (size_t)spt::kv_layer_elems(B_layout, H, T_enc);
        std::vector<float> lay(n_kv, pad_value);
        for (int b = 0; b < B_layout; ++b)
            for (int h = 0; h < H; ++h)
                for (int t = 0; t < T_enc; ++t)
                    memcpy(lay.data() + spt::kv_offset(0, 0, b, h, t, 0, B_layout, H, T_enc),
                           k + (((size_t)b * H + h) * T_enc + t) * 64, 64 * sizeof(float));
        const size_t nq = (size_t)B * Tq * H * 64, np = (size_t)B * n_heads * N_cap * M_cap;
        std::vector<uint16_t> q16, kv16;
        Scope sc(device);
        spt::AlignQkArgs a{};
        if (dtype == spt::DT_F32) {
            a.q = sc.up(q, nq);
            a.kv = sc.up(lay.data(), n_kv);
        } else {
            q16 = to_half_storage(dtype, q, nq);
            kv16 = to_half_storage(dtype, lay.data(), n_kv);
            a.q = sc.up(q16.data(), nq);
            a.kv = sc.up(kv16.data(), n_kv);
        }
        a.Tq = Tq; a.pos0 = pos0; a.B_layout = B_layout; a.H = H; a.T_enc = T_enc;
        a.kvrow = kvrow ? sc.up(kvrow, (size_t)B) : nullptr;
        a.heads = sc.up(heads, (size_t)n_heads);
        a.n_heads = n_heads; a.a0 = 0;
        a.p = sc.out<float>(np); a.A = n_heads; a.N_cap = N_cap; a.M_cap = M_cap;
        a.M = sc.up(M, (size_t)B);
        spt::align_qk(dtype, a, B, sc.st);
        sc.down(p, (const float*)a.p, np);
        sc.sync();
        return SPT_OK;
    } catch (const std::exception& e) {
        set_err(err, errlen, e.what());
        return spt_classify(e);
    }
}

spt_status spt_debug_align_norm(int32_t device, const float* p, int32_t B, int32_t A, int32_t N_cap, int32_t M_cap,
                                const int32_t* N, const int32_t* M, float* stat, float* m, char* err, size_t errlen) {
    if (!p || !N || !M || !m) {
        set_err(err, errlen, "null argument");
        return SPT_ERR_INVALID_ARG;
    }
    try {
        if (B < 1 || B > 1024 || A < 1 || A > 512) throw std::runtime_error("debug_align_norm: 1..1024 sequences, 1..512 heads");
        if (N_cap < 1 || N_cap > 65535 || M_cap < 1) throw std::runtime_error("debug_align_norm: N_cap 1..65535, M_cap >= 1");
        if ((int64_t)B * A * N_cap * M_cap > kMaxElems) throw std::runtime_error("debug_align_norm: p above 2^26 elements");
        check_counts("N", N, B, N_cap);
        check_counts("M", M, B, M_cap);
    } catch (const std::exception& e) {
        set_err(err, errlen, e.what());
        return SPT_ERR_INVALID_ARG;
    }
    if (spt_status s = device_ok(device, err, errlen)) return s;
    try {
        const size_t np = (size_t)B * A * N_cap * M_cap, ns = (size_t)B * A * 2 * M_cap, nm = (size_t)B * N_cap * M_cap;
        Scope sc(device);
        const float* d_p = sc.up(p, np);
        const int* d_N = sc.up(N, (size_t)B);
        const int* d_M = sc.up(M, (size_t)B);
        float* d_stat = sc.out<float>(ns);
        float* d_m = sc.out<float>(nm);
        spt::align_norm(d_p, B, A, N_cap, M_cap, d_N, d_M, d_stat, d_m, sc.st);
        if (stat) sc.down(stat, (const float*)d_stat, ns);
        sc.down(m, (const float*)d_m, nm);
        sc.sync();
        return SPT_OK;
    } catch (const std::exception& e) {
        set_err(err, errlen, e.what());
        return spt_classify(e);
    }
}

spt_status spt_debug_align_dtw(int32_t device, const float* m, int32_t B, int32_t N_cap, int32_t M_cap, const int32_t* N,
                               const int32_t* M, int32_t* jump, int32_t* len, int32_t* path, char* err,
                               size_t errlen) {
    if (!m || !N || !M || !jump || !len) {
        set_err(err, errlen, "null argument");
        return SPT_ERR_INVALID_ARG;
    }
    try {
        if (B < 1 || B > 1024) throw std::runtime_error("debug_align_dtw: 1..1024 sequences");
        if (N_cap < 1 || N_cap > spt::kAlignMaxRows) throw std::runtime_error("align_dtw: N_cap 1..256");
        if (M_cap < 8 || M_cap % 8 || M_cap > 32768) throw std::runtime_error("align_dtw: M_cap a multiple of 8, 8..32768");
        if (((int64_t)2 * 264 + (int64_t)N_cap * ((M_cap + 15) / 16)) * 4 > 160 * 1024)
            throw std::runtime_error("align_dtw: trace beyond 160 KiB of LDS");
        if ((int64_t)B * N_cap * M_cap > kMaxElems) throw std::runtime_error("debug_align_dtw: m above 2^26 elements");
        check_counts("N", N, B, N_cap);
        check_counts("M", M, B, M_cap);
    } catch (const std::exception& e) {
        set_err(err, errlen, e.what());
        return SPT_ERR_INVALID_ARG;
    }
    if (spt_status s = device_ok(device, err, errlen)) return s;
    try {
        const size_t nm = (size_t)B * N_cap * M_cap, nj = (size_t)B * N_cap, npath = (size_t)B * (N_cap + M_cap);
        Scope sc(device);
        const float* d_m = sc.up(m, nm);
        const int* d_N = sc.up(N, (size_t)B);
        const int* d_M = sc.up(M, (size_t)B);
        int* d_jump = sc.out<int>(nj);
        int* d_len = sc.out<int>((size_t)B);
        int* d_path = sc.out<int>(npath);
        spt::align_dtw(d_m, B, N_cap, M_cap, d_N, d_M, d_jump, d_len, d_path, sc.st);
        std::vector<int> hp(npath);
        sc.down(jump, (const int*)d_jump, nj);
        sc.down(len, (const int*)d_len, (size_t)B);
        sc.down(hp.data(), (const int*)d_path, npath);
        sc.sync();
        if (path)  // forwards, as (row, key) pairs
            for (int b = 0; b < B; ++b) {
                int32_t* o = path + (size_t)b * (N_cap + M_cap) * 2;
                const int n = len[b] < 0 ? 0 : len[b] > N_cap + M_cap ? N_cap + M_cap : len[b];
                for (int i = 0; i < n; ++i) {
                    const int v = hp[(size_t)b * (N_cap + M_cap) + (n - 1 - i)];
                    o[2 * i] = (int16_t)(v >> 16);
                    o[2 * i + 1] = (int16_t)(v & 0xFFFF);
                }
                for (int i = n; i < N_cap + M_cap; ++i) o[2 * i] = o[2 * i + 1] = -1;
            }
        return SPT_OK;
    } catch (const std::exception& e) {
        set_err(err, errlen, e.what());
        return spt_classify(e);
    }
}

spt_status spt_debug_align_words(const char* const* pieces, const int32_t* piece_len, const int64_t* t0,
                                 const int64_t* t1, const float* p, int32_t n, int32_t* word_i0, int32_t* word_n,
                                 int64_t* word_t0, int64_t* word_t1, float* word_p, int32_t* n_words, char* err,
                                 size_t errlen) {
    if (!n_words || n < 0 || (n > 0 && (!pieces || !piece_len || !t0 || !t1 || !word_i0 || !word_n || !word_t0 || !word_t1))) {
        set_err(err, errlen, "null argument or negative count");
        return SPT_ERR_INVALID_ARG;
    }
    try {
        std::vector<std::string> pc((size_t)n);
        for (int i = 0; i < n; ++i) {
            if (!pieces[i] || piece_len[i] < 0) throw std::runtime_error("debug_align_words: null piece or negative length");
            pc[(size_t)i].assign(pieces[i], (size_t)piece_len[i]);
        }
        const std::vector<spt::AlignWord> w = spt::align_words(pc, t0, t1, p);
        for (size_t i = 0; i < w.size(); ++i) {  // (at most n words)
            word_i0[i] = w[i].i0;
            word_n[i] = w[i].n;
            word_t0[i] = w[i].t0;
            word_t1[i] = w[i].t1;
            if (word_p) word_p[i] = w[i].p;
        }
        *n_words = (int32_t)w.size();
        return SPT_OK;
    } catch (const std::exception& e) {
        set_err(err, errlen, e.what());
        return SPT_ERR_INVALID_ARG;
    }
}

}  // extern "C"
