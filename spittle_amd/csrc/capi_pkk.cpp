// capi_pkk.cpp -- spt_debug_pk_conv, spt_debug_pk_relpos and spt_debug_pk_rel_attn: one launch of a
// Parakeet encoder kernel (k_pk.hip, through the launchers of pk_kernels.h) on caller-supplied arrays
// (no engine, no model); spt_debug_pk_dec_stage: one pk_decode_stage launch on plain weights the hook
// places; spt_debug_pk_tdt: pk_state_init, then pk_joint_fin step by step on caller-supplied partials;
// spt_debug_pk_tdt_steps: the engine's whole five-launch decode step; for tests/test_gpu_pk_kernels.py.  Each call owns its stream and its buffers
// on the device the caller names, rounds the f32 operands to the engine dtype on the host and returns
// f32; output buffers start as NaN bytes and come back whole.  Everything a launcher would throw on,
// or that would read or write outside a buffer, is refused here first.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/spittle_hip.h"
#include "capi_debug.h"
#include "capi_internal.h"
#include "common.h"
#include "kernels.h"
#include "pk_kernels.h"

namespace {

using namespace spt::dbg;

void check_dtype(int32_t dtype, const char* who) {
    if (dtype != spt::DT_F32 && dtype != spt::DT_BF16 && dtype != spt::DT_F16)
        throw std::runtime_error(std::string(who) + ": dtype is f32, bf16 or f16");
}

constexpr int64_t kMaxElems = (int64_t)1 << 26;  // of any one buffer of a call

int halve(int n) { return (n - 1) / 2 + 1; }  // a stride-2, pad-1, 3-tap stage's output length

// lens [B][4]: no negative count; column `col` at most `cap` where the kernel indexes from it unguarded
void check_lens(const int32_t* lens, int B, int col, int cap, const char* who) {
    for (int i = 0; i < B * 4; ++i)
        if (lens[i] < 0) throw std::runtime_error(std::string(who) + ": negative entry in lens");
    if (col >= 0)
        for (int b = 0; b < B; ++b)
            if (lens[b * 4 + col] > cap) throw std::runtime_error(std::string(who) + ": lens[b][3] above Tp");
}

// an address with the alignment of element `off` of a device allocation (256-byte aligned)
const void* fake_ptr(int64_t off, int esz) { return (const void*)(uintptr_t)((1ull << 32) + (uint64_t)off * esz); }

}  // namespace

extern "C" {

spt_status spt_debug_pk_conv(int32_t device, const spt_pk_conv_debug* a, char* err, size_t errlen) {
    if (!a || !a->x || !a->lens || !a->w || !a->bias || !a->y) {
        set_err(err, errlen, "null argument");
        return SPT_ERR_INVALID_ARG;
    }
    const int B = a->B, Tp = a->Tp, F = a->F, C = a->C, mode = a->mode;
    int64_t n_in = 0, n_out = 0;
    int To = 0, Fo = 0;
    try {
        check_dtype(a->dtype, "debug_pk_conv");
        if (mode < SPT_PK_CONV0 || mode > SPT_PK_CONV_MODULE) throw std::runtime_error("debug_pk_conv: mode 0..3");
        if (B < 1 || B > 65535 || Tp < 1) throw std::runtime_error("debug_pk_conv: need B in 1..65535 (grid y), Tp >= 1");
        if (mode == SPT_PK_CONV_MODULE) {
            spt::pk_conv_module_check(C, 9);
            if (!a->bn_g || !a->bn_b || !a->bn_m || !a->bn_v) throw std::runtime_error("debug_pk_conv: null BatchNorm vector");
            n_in = (int64_t)B * Tp * 2 * C;
            n_out = (int64_t)B * Tp * C;
            check_lens(a->lens, B, 3, Tp, "debug_pk_conv");
        } else {
            if (F < 1) throw std::runtime_error("debug_pk_conv: need F >= 1");
            spt::pk_sub_check(C, mode == SPT_PK_CONV0 ? "pk_conv0" : "pk_dwconv");
            if (mode == SPT_PK_CONV0 && (size_t)3 * F * 4 > 64 * 1024)
                throw std::runtime_error("debug_pk_conv: three mel frames above 64 KiB of LDS");
            To = halve(Tp);
            Fo = halve(F);
            n_in = (int64_t)B * Tp * F * (mode == SPT_PK_CONV0 ? 1 : C);
            n_out = (int64_t)B * To * Fo * C;
            check_lens(a->lens, B, -1, 0, "debug_pk_conv");
        }
        if (n_in > kMaxElems || n_out > kMaxElems || a->y_count > kMaxElems)
            throw std::runtime_error("debug_pk_conv: buffers above 2^26 elements");
        if (a->y_count < n_out) throw std::runtime_error("debug_pk_conv: y_count below what the launch writes");
    } catch (const std::exception& e) {
        set_err(err, errlen, e.what());
        return SPT_ERR_INVALID_ARG;
    }
    if (spt_status s = device_ok(device, err, errlen)) return s;
    try {
        const int dt = a->dtype;
        const size_t esz = (size_t)spt::dtype_size(dt);
        std::vector<uint16_t> x16;
        Scope sc(device);
        const int* dl = sc.up((const int*)a->lens, (size_t)B * 4);
        const float* dw = sc.up(a->w, (size_t)C * 9);
        const float* db = sc.up(a->bias, (size_t)C);
        void* dy = sc.out<char>((size_t)a->y_count * esz);
        if (mode == SPT_PK_CONV0) {
            spt::pk_conv0(dt, sc.up(a->x, (size_t)n_in), dl, B, Tp, F, dw, db, C, dy, To, Fo, sc.st);
        } else if (mode == SPT_PK_CONV_MODULE) {
            spt::pk_conv_module(dt, up_as(sc, dt, a->x, (size_t)n_in, x16), dl, B, Tp, C, 9, dw, db, sc.up(a->bn_g, (size_t)C),
                                sc.up(a->bn_b, (size_t)C), sc.up(a->bn_m, (size_t)C), sc.up(a->bn_v, (size_t)C), dy, sc.st);
        } else {
            spt::pk_dwconv(dt, up_as(sc, dt, a->x, (size_t)n_in, x16), dl, mode == SPT_PK_DWCONV1 ? 1 : 2, B, Tp, F, dw, db, C,
                           dy, To, Fo, sc.st);
        }
        down_f32(sc, dt, dy, a->y, (size_t)a->y_count);
        sc.sync();
        return SPT_OK;
    } catch (const std::exception& e) {
        set_err(err, errlen, e.what());
        return spt_classify(e);
    }
}

spt_status spt_debug_pk_relpos(int32_t device, int32_t dtype, int32_t Tp, int32_t d, float* pe, int64_t pe_count,
                               char* err, size_t errlen) {
    if (!pe) {
        set_err(err, errlen, "null argument");
        return SPT_ERR_INVALID_ARG;
    }
    try {
        check_dtype(dtype, "debug_pk_relpos");
        if (Tp < 1 || d < 2 || d % 2) throw std::runtime_error("debug_pk_relpos: need Tp >= 1 and an even d >= 2");
        if ((int64_t)(2 * (int64_t)Tp - 1) * d > kMaxElems || pe_count > kMaxElems)
            throw std::runtime_error("debug_pk_relpos: buffers above 2^26 elements");
        if (pe_count < (2 * (int64_t)Tp - 1) * d) throw std::runtime_error("debug_pk_relpos: pe_count below (2 Tp - 1) d");
    } catch (const std::exception& e) {
        set_err(err, errlen, e.what());
        return SPT_ERR_INVALID_ARG;
    }
    if (spt_status s = device_ok(device, err, errlen)) return s;
    try {
        Scope sc(device);
        void* dp = sc.out<char>((size_t)pe_count * spt::dtype_size(dtype));
        spt::pk_relpos(dtype, Tp, d, dp, sc.st);
        down_f32(sc, dtype, dp, pe, (size_t)pe_count);
        sc.sync();
        return SPT_OK;
    } catch (const std::exception& e) {
        set_err(err, errlen, e.what());
        return spt_classify(e);
    }
}

spt_status spt_debug_pk_rel_attn(int32_t device, const spt_pk_attn_debug* a, char* err, size_t errlen) {
    if (!a || !a->qkv || !a->p || !a->pu || !a->pv || !a->lens || !a->out) {
        set_err(err, errlen, "null argument");
        return SPT_ERR_INVALID_ARG;
    }
    const int B = a->B, Tp = a->Tp, H = a->H, dk = a->dk, dt = a->dtype;
    int64_t d = 0;
    try {
        check_dtype(dt, "debug_pk_rel_attn");
        if (B < 1 || B > 65535 || H < 1 || H > 65535 || Tp < 1)
            throw std::runtime_error("debug_pk_rel_attn: need B, H in 1..65535 (grid y, z), Tp >= 1");
        if (a->ldp < 1 || a->p_off < 0 || a->p_bstride < 0 || a->p_count < 1)
            throw std::runtime_error("debug_pk_rel_attn: negative offset or stride");
        const int esz = spt::dtype_size(dt);
        // what the launcher refuses, on addresses with the alignment the device buffers will have
        spt::pk_rel_attn_check(dt, fake_ptr(0, esz), fake_ptr(a->p_off, esz), a->ldp, Tp, dk, a->p_bstride, a->variant);
        d = (int64_t)H * dk;
        if ((int64_t)B * Tp * 3 * d > kMaxElems || a->p_count > kMaxElems || a->out_count > kMaxElems)
            throw std::runtime_error("debug_pk_rel_attn: buffers above 2^26 elements");
        if (a->ldp < d) throw std::runtime_error("debug_pk_rel_attn: ldp below d");
        if (a->p_off + (int64_t)(B - 1) * a->p_bstride + (int64_t)(2 * Tp - 2) * a->ldp + d > a->p_count)
            throw std::runtime_error("debug_pk_rel_attn: the last position row reaches beyond p_count");
        if (a->out_count < (int64_t)B * Tp * d) throw std::runtime_error("debug_pk_rel_attn: out_count below B * Tp * d");
        check_lens(a->lens, B, 3, Tp, "debug_pk_rel_attn");
    } catch (const std::exception& e) {
        set_err(err, errlen, e.what());
        return SPT_ERR_INVALID_ARG;
    }
    if (spt_status s = device_ok(device, err, errlen)) return s;
    try {
        const size_t esz = (size_t)spt::dtype_size(dt);
        std::vector<uint16_t> q16, p16;
        Scope sc(device);
        const void* dq = up_as(sc, dt, a->qkv, (size_t)B * Tp * 3 * (size_t)d, q16);
        const char* dp = (const char*)up_as(sc, dt, a->p, (size_t)a->p_count, p16);
        const float* du = sc.up(a->pu, (size_t)d);
        const float* dv = sc.up(a->pv, (size_t)d);
        const int* dl = sc.up((const int*)a->lens, (size_t)B * 4);
        void* dout = sc.out<char>((size_t)a->out_count * esz);
        spt::pk_rel_attn_variant(dt, dq, dp + (size_t)a->p_off * esz, a->ldp, du, dv, dl, B, Tp, H, dk, dout, sc.st,
                                 a->p_bstride, a->variant);
        down_f32(sc, dt, dout, a->out, (size_t)a->out_count);
        sc.sync();
        return SPT_OK;
    } catch (const std::exception& e) {
        set_err(err, errlen, e.what());
        return spt_classify(e);
    }
}

spt_status spt_debug_pk_tdt(int32_t device, const spt_pk_tdt_debug* a, char* err, size_t errlen) {
    if (!a || !a->part || !a->dur || !a->lens || !a->emb || !a->fe || !a->state || !a->xemb || !a->fecur || !a->out_tok ||
        !a->out_frame || !a->out_t1 || !a->out_t2) {
        set_err(err, errlen, "null argument");
        return SPT_ERR_INVALID_ARG;
    }
    const int B = a->B, P = a->P, V = a->V, nd = a->n_dur, nt = a->n_tiles, ns = a->n_steps, cap = a->cap, T3p = a->T3p;
    try {
        if (ns < 1 || ns > 4096) throw std::runtime_error("debug_pk_tdt: n_steps 1..4096");
        if (B > 65535 || T3p < 1 || a->max_symbols < 1) throw std::runtime_error("debug_pk_tdt: need B <= 65535 (grid x), T3p >= 1, max_symbols >= 1");
        spt::PkFinArgs f{};
        f.B = B; f.n_tiles = nt; f.n_dur = nd; f.P = P; f.cap = cap; f.V = V;
        spt::pk_joint_fin_check(f);
        if ((int64_t)ns * B * nt * 4 > kMaxElems || (int64_t)ns * B * nd > kMaxElems || (int64_t)(V + 1) * P > kMaxElems ||
            (int64_t)B * T3p * P > kMaxElems || (int64_t)(ns + 1) * B * P > kMaxElems || (int64_t)ns * ((int64_t)B * cap + 1) > kMaxElems)
            throw std::runtime_error("debug_pk_tdt: buffers above 2^26 elements");
        check_lens(a->lens, B, 3, T3p, "debug_pk_tdt");
        // the kernel reads emb[tok] of the index it finds: every (step, row) must find one in 0 .. V
        for (int64_t r = 0; r < (int64_t)ns * B; ++r) {
            bool any = false;
            for (int i = 0; i < nt; ++i) {
                const float* p = a->part + (r * nt + i) * 4;
                int32_t idx;
                memcpy(&idx, p + 1, 4);
                if (p[0] != p[0]) throw std::runtime_error("debug_pk_tdt: a partial's best is NaN");
                if (p[0] > -INFINITY) {
                    if (idx < 0 || idx > V) throw std::runtime_error("debug_pk_tdt: a partial's index outside 0 .. V");
                    any = true;
                }
            }
            if (!any) throw std::runtime_error("debug_pk_tdt: a (step, row) with no best above -inf");
        }
    } catch (const std::exception& e) {
        set_err(err, errlen, e.what());
        return SPT_ERR_INVALID_ARG;
    }
    if (spt_status s = device_ok(device, err, errlen)) return s;
    try {
        Scope sc(device);
        const size_t bp = (size_t)B * P, no = (size_t)B * cap + 1;
        const float* dpart = sc.up(a->part, (size_t)ns * B * nt * 4);
        const float* ddur = sc.up(a->dur, (size_t)ns * B * nd);
        const int* dl = sc.up((const int*)a->lens, (size_t)B * 4);
        const float* demb = sc.up(a->emb, (size_t)(V + 1) * P);
        const float* dfe = sc.up(a->fe, (size_t)B * T3p * P);
        spt::PkState* st = sc.out<spt::PkState>((size_t)B);
        float* hc = sc.out<float>(2);  // pk_state_init also zeroes n floats of two LSTM buffers: n = 1 here
        float* xemb = sc.out<float>(bp);
        float* fecur = sc.out<float>(bp);
        int* otok = sc.out<int>(no);
        int* ofr = sc.out<int>(no);
        float* o1 = sc.out<float>(no);
        float* o2 = sc.out<float>(no);
        static_assert(sizeof(spt::PkState) == 7 * sizeof(int32_t), "spt_debug_pk_tdt returns PkState as 7 int32");
        auto snap = [&](int slot) {
            sc.down(a->state + (size_t)slot * B * 7, (const int32_t*)st, (size_t)B * 7);
            sc.down(a->xemb + (size_t)slot * bp, (const float*)xemb, bp);
            sc.down(a->fecur + (size_t)slot * bp, (const float*)fecur, bp);
        };
        spt::pk_state_init(st, B, V, hc, hc + 1, 1, xemb, fecur, dfe, dl, T3p, P, sc.st);
        snap(0);
        for (int s = 0; s < ns; ++s) {
            spt::PkFinArgs f{};
            f.part = (const float4*)(dpart + (size_t)s * B * nt * 4); f.n_tiles = nt;
            f.dur = ddur + (size_t)s * B * nd;
            f.V = V; f.n_dur = nd; f.max_symbols = a->max_symbols; f.B = B; f.cap = cap;
            f.lens = dl; f.st = st; f.P = P; f.emb = demb; f.fe = dfe; f.xemb = xemb; f.fecur = fecur;
            f.out_tok = otok; f.out_frame = ofr; f.out_t1 = o1; f.out_t2 = o2;
            spt::pk_joint_fin(f, sc.st);
            snap(s + 1);
            sc.down(a->out_tok + (size_t)s * no, (const int32_t*)otok, no);
            sc.down(a->out_frame + (size_t)s * no, (const int32_t*)ofr, no);
            sc.down(a->out_t1 + (size_t)s * no, (const float*)o1, no);
            sc.down(a->out_t2 + (size_t)s * no, (const float*)o2, no);
        }
        sc.sync();
        return SPT_OK;
    } catch (const std::exception& e) {
        set_err(err, errlen, e.what());
        return spt_classify(e);
    }
}

spt_status spt_debug_pk_dec_stage(int32_t device, const spt_pk_dec_debug* a, char* err, size_t errlen) {
    if (!a || !a->W || !a->b0 || !a->state) {
        set_err(err, errlen, "null argument");
        return SPT_ERR_INVALID_ARG;
    }
    const int mode = a->mode, B = a->B, P = a->P, V = a->V, nd = a->n_dur;
    spt::PkDecArgs g{};
    int n_tiles = 0;
    try {
        if (mode < SPT_PK_DEC_LSTM || mode > SPT_PK_DEC_JOINT) throw std::runtime_error("debug_pk_dec_stage: mode 0..2");
        if (P < 1 || P > 4096) throw std::runtime_error("pk_decode_stage: bad shape");
        g.B = B; g.P = P; g.V = V; g.n_dur = nd;
        if (mode == SPT_PK_DEC_LSTM) {
            if (!a->W2 || !a->b1 || !a->xin || !a->h_in || !a->c_in || !a->h_out || !a->c_out)
                throw std::runtime_error("debug_pk_dec_stage: the LSTM stage needs W2, b1, xin, h_in, c_in, h_out, c_out");
            g.ld = 4 * P; g.K = 2 * P; g.N = 4 * P;
        } else if (mode == SPT_PK_DEC_PRED) {
            if (!a->xin || !a->gp) throw std::runtime_error("debug_pk_dec_stage: the prediction stage needs xin and gp");
            g.ld = (P + 63) / 64 * 64; g.K = P; g.N = P;
        } else {
            if (!a->fe || !a->gp || !a->part || !a->dur) throw std::runtime_error("debug_pk_dec_stage: the joint stage needs fe, gp, part and dur");
            if (V < 0 || nd < 1 || V > (1 << 20) || nd > 64) throw std::runtime_error("debug_pk_dec_stage: need 0 <= V <= 2^20, 1 <= n_dur <= 64");
            g.N = V + 1 + nd;
            g.ld = (g.N + 63) / 64 * 64; g.K = P;
            n_tiles = g.ld / spt::pk_joint_tile();
        }
        spt::pk_decode_stage_check(mode, g);
        if ((int64_t)g.ld * g.K > kMaxElems) throw std::runtime_error("debug_pk_dec_stage: buffers above 2^26 elements");
    } catch (const std::exception& e) {
        set_err(err, errlen, e.what());
        return SPT_ERR_INVALID_ARG;
    }
    if (spt_status s = device_ok(device, err, errlen)) return s;
    try {
        Scope sc(device);
        const size_t bp = (size_t)B * P;
        static_assert(sizeof(spt::PkState) == 7 * sizeof(int32_t), "spt_debug_pk_dec_stage takes PkState as 7 int32");
        g.st = (const spt::PkState*)sc.up(a->state, (size_t)B * 7);
        float* wt = sc.out<float>((size_t)g.ld * g.K);   // NaN bytes: what the placement leaves stays NaN
        g.WT = wt;
        if (mode == SPT_PK_DEC_LSTM) {
            spt::pk_place_lstm(sc.up(a->W, (size_t)4 * P * P), P, wt, 0, sc.st);
            spt::pk_place_lstm(sc.up(a->W2, (size_t)4 * P * P), P, wt, P, sc.st);
            g.b0 = sc.up(a->b0, (size_t)4 * P);
            g.b1 = sc.up(a->b1, (size_t)4 * P);
            g.xin = sc.up(a->xin, bp); g.h_in = sc.up(a->h_in, bp); g.c_in = sc.up(a->c_in, bp);
            g.h_out = sc.out<float>(bp); g.c_out = sc.out<float>(bp);
            spt::pk_decode_stage(mode, g, sc.st);
            sc.down(a->h_out, (const float*)g.h_out, bp);
            sc.down(a->c_out, (const float*)g.c_out, bp);
        } else if (mode == SPT_PK_DEC_PRED) {
            spt::pk_place_blocked(sc.up(a->W, (size_t)P * P), P, P, spt::PKD_PRED, wt, sc.st);
            g.b0 = sc.up(a->b0, (size_t)P);
            g.xin = sc.up(a->xin, bp);
            g.gp = sc.up((const float*)a->gp, bp);
            spt::pk_decode_stage(mode, g, sc.st);
            sc.down(a->gp, (const float*)g.gp, bp);
        } else {
            spt::pk_place_blocked(sc.up(a->W, (size_t)g.N * P), g.N, P, spt::PKD_JOINT, wt, sc.st);
            g.b0 = sc.up(a->b0, (size_t)g.N);
            g.fe = sc.up(a->fe, bp);
            g.gp = sc.up((const float*)a->gp, bp);
            float* part = sc.out<float>((size_t)B * n_tiles * 4);
            g.part = (float4*)part; g.n_tiles = n_tiles;
            g.dur = sc.out<float>((size_t)B * nd);
            spt::pk_decode_stage(mode, g, sc.st);
            sc.down(a->part, (const float*)part, (size_t)B * n_tiles * 4);
            sc.down(a->dur, (const float*)g.dur, (size_t)B * nd);
        }
        sc.sync();
        return SPT_OK;
    } catch (const std::exception& e) {
        set_err(err, errlen, e.what());
        return spt_classify(e);
    }
}

spt_status spt_debug_pk_tdt_steps(int32_t device, const spt_pk_steps_debug* a, char* err, size_t errlen) {
    bool null = !a;
    if (a) {
        for (int l = 0; l < 2; ++l)
            for (int i = 0; i < 4; ++i) null = null || !a->lstm[l][i];
        null = null || !a->pred_w || !a->pred_b || !a->joint_w || !a->joint_b || !a->emb || !a->fe || !a->lens || !a->state ||
               !a->out_tok || !a->out_frame || !a->out_t1 || !a->out_t2;
    }
    if (null) {
        set_err(err, errlen, "null argument");
        return SPT_ERR_INVALID_ARG;
    }
    const int B = a->B, P = a->P, V = a->V, nd = a->n_dur, ns = a->n_steps, cap = a->cap, T3p = a->T3p;
    spt::PkDecArgs gl{}, gp{}, gj{};
    try {
        if (ns < 1 || ns > 4096) throw std::runtime_error("debug_pk_tdt_steps: n_steps 1..4096");
        if (T3p < 1 || a->max_symbols < 1 || cap < 0 || cap > (1 << 16)) throw std::runtime_error("debug_pk_tdt_steps: need T3p >= 1, max_symbols >= 1, 0 <= cap <= 65536");
        if (P < 1 || P > 4096 || V < 0 || V > (1 << 20) || nd < 1 || nd > 64) throw std::runtime_error("pk_decode_stage: bad shape");
        gl.B = gp.B = gj.B = B; gl.P = gp.P = gj.P = P; gl.V = gp.V = gj.V = V; gl.n_dur = gp.n_dur = gj.n_dur = nd;
        gl.ld = 4 * P; gl.K = 2 * P; gl.N = 4 * P;
        gp.ld = (P + 63) / 64 * 64; gp.K = P; gp.N = P;
        gj.N = V + 1 + nd; gj.ld = (gj.N + 63) / 64 * 64; gj.K = P;
        spt::pk_decode_stage_check(spt::PKD_LSTM, gl);
        spt::pk_decode_stage_check(spt::PKD_PRED, gp);
        spt::pk_decode_stage_check(spt::PKD_JOINT, gj);
        if ((int64_t)gj.ld * P > kMaxElems || (int64_t)B * T3p * P > kMaxElems || (int64_t)(ns + 1) * B * 7 > kMaxElems)
            throw std::runtime_error("debug_pk_tdt_steps: buffers above 2^26 elements");
        check_lens(a->lens, B, 3, T3p, "debug_pk_tdt_steps");
    } catch (const std::exception& e) {
        set_err(err, errlen, e.what());
        return SPT_ERR_INVALID_ARG;
    }
    if (spt_status s = device_ok(device, err, errlen)) return s;
    try {
        Scope sc(device);
        const size_t bp = (size_t)B * P, no = (size_t)B * cap + 1;
        const int n_tiles = gj.ld / spt::pk_joint_tile();
        float* wl[2];
        const float* bih[2];
        const float* bhh[2];
        for (int l = 0; l < 2; ++l) {
            wl[l] = sc.out<float>((size_t)gl.ld * gl.K);
            spt::pk_place_lstm(sc.up(a->lstm[l][0], (size_t)4 * P * P), P, wl[l], 0, sc.st);
            spt::pk_place_lstm(sc.up(a->lstm[l][1], (size_t)4 * P * P), P, wl[l], P, sc.st);
            bih[l] = sc.up(a->lstm[l][2], (size_t)4 * P);
            bhh[l] = sc.up(a->lstm[l][3], (size_t)4 * P);
        }
        float* wp = sc.out<float>((size_t)gp.ld * P);
        spt::pk_place_blocked(sc.up(a->pred_w, (size_t)P * P), P, P, spt::PKD_PRED, wp, sc.st);
        float* wj = sc.out<float>((size_t)gj.ld * P);
        spt::pk_place_blocked(sc.up(a->joint_w, (size_t)gj.N * P), gj.N, P, spt::PKD_JOINT, wj, sc.st);
        const float* pb = sc.up(a->pred_b, (size_t)P);
        const float* jb = sc.up(a->joint_b, (size_t)gj.N);
        const float* demb = sc.up(a->emb, (size_t)(V + 1) * P);
        const float* dfe = sc.up(a->fe, (size_t)B * T3p * P);
        const int* dl = sc.up((const int*)a->lens, (size_t)B * 4);
        spt::PkState* st = sc.out<spt::PkState>((size_t)B);
        float* h = sc.out<float>(4 * bp);    // [layer][parity][B][P], as the engine's
        float* c = sc.out<float>(4 * bp);
        float* xemb = sc.out<float>(bp);
        float* fecur = sc.out<float>(bp);
        float* gpb = sc.out<float>(bp);
        float* part = sc.out<float>((size_t)B * n_tiles * 4);
        float* dur = sc.out<float>((size_t)B * nd);
        int* otok = sc.out<int>(no);
        int* ofr = sc.out<int>(no);
        float* o1 = sc.out<float>(no);
        float* o2 = sc.out<float>(no);
        auto hbuf = [&](float* base, int layer, int par) { return base + ((size_t)layer * 2 + par) * bp; };
        spt::pk_state_init(st, B, V, h, c, (int)(4 * bp), xemb, fecur, dfe, dl, T3p, P, sc.st);
        sc.down(a->state, (const int32_t*)st, (size_t)B * 7);
        for (int s = 0; s < ns; ++s) {
            const int p = s & 1, q = p ^ 1;
            spt::PkDecArgs g = gl;
            g.st = st;
            g.WT = wl[0]; g.b0 = bih[0]; g.b1 = bhh[0];
            g.xin = xemb; g.h_in = hbuf(h, 0, p); g.c_in = hbuf(c, 0, p); g.h_out = hbuf(h, 0, q); g.c_out = hbuf(c, 0, q);
            spt::pk_decode_stage(spt::PKD_LSTM, g, sc.st);
            g.WT = wl[1]; g.b0 = bih[1]; g.b1 = bhh[1]; g.xin = hbuf(h, 0, q);
            g.h_in = hbuf(h, 1, p); g.c_in = hbuf(c, 1, p); g.h_out = hbuf(h, 1, q); g.c_out = hbuf(c, 1, q);
            spt::pk_decode_stage(spt::PKD_LSTM, g, sc.st);
            g.WT = wp; g.ld = gp.ld; g.K = P; g.N = P; g.b0 = pb; g.b1 = nullptr; g.xin = hbuf(h, 1, q); g.gp = gpb;
            spt::pk_decode_stage(spt::PKD_PRED, g, sc.st);
            g.WT = wj; g.ld = gj.ld; g.K = P; g.N = gj.N; g.b0 = jb;
            g.fe = fecur; g.part = (float4*)part; g.n_tiles = n_tiles; g.dur = dur;
            spt::pk_decode_stage(spt::PKD_JOINT, g, sc.st);
            spt::PkFinArgs f{};
            f.part = (const float4*)part; f.n_tiles = n_tiles; f.dur = dur;
            f.V = V; f.n_dur = nd; f.max_symbols = a->max_symbols; f.B = B; f.cap = cap; f.lens = dl;
            f.st = st; f.out_tok = otok; f.out_frame = ofr; f.out_t1 = o1; f.out_t2 = o2;
            f.P = P; f.emb = demb; f.fe = dfe; f.xemb = xemb; f.fecur = fecur;
            spt::pk_joint_fin(f, sc.st);
            sc.down(a->state + (size_t)(s + 1) * B * 7, (const int32_t*)st, (size_t)B * 7);
        }
        sc.down(a->out_tok, (const int32_t*)otok, no);
        sc.down(a->out_frame, (const int32_t*)ofr, no);
        sc.down(a->out_t1, (const float*)o1, no);
        sc.down(a->out_t2, (const float*)o2, no);
        sc.sync();
        return SPT_OK;
    } catch (const std::exception& e) {
        set_err(err, errlen, e.what());
        return spt_classify(e);
    }
}

}  // extern "C"
