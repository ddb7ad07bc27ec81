// ms_kernels.h -- host launchers of the Moonshine kernels (k_ms.hip), gfx950.
//
// Batch layout as in pk_kernels.h: B utterances padded to the longest one, row (b, t) of a
// [B * Tp][...] tensor is b * Tp + t.  lens[b][4] = {samples, T1, T2, T3} lives on the device; every
// kernel that mixes frames masks t >= len (loads clamped to zero, never multiplied away), so a
// padded batch row computes exactly what it computes alone.  Widths: d is the model width, dp the
// same padded to a multiple of 64 (the GEMM tiles' N and K granule); pad columns are kept zero.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace spt {

constexpr int MS_K1 = 127, MS_K1P = 128, MS_S1 = 64, MS_K2 = 7, MS_S2 = 3, MS_K3 = 3, MS_S3 = 2;
constexpr int MS_MIN_SAMPLES = 895;  // the shortest input with one encoder frame
// the longest: 7811 encoder frames and 1227 decode steps, inside the decode attention's 8192-key score buffer
constexpr int MS_MAX_SAMPLES = 3000000;

struct MsState {       // device-resident decode-step state (read by the captured step graph)
    int step;          // index of the token being produced = position of the token fed
    int t3p;           // this call's padded encoder frames (row stride of the cross K/V)
    int forced_len;    // > 0: teacher forcing, step s feeds forced[b * forced_len + s]
    int log_all;       // 1: the logits of step s go to logits + s * R * V (debug), else to logits
    float* logits;     // [R][V] (or [steps][R][V])
    int eos;
    int cap;           // row stride of out_tok / out_top1 / out_top2
    int reserved;
};

// frames[(b * T1p + t)][i] = pcm_b[t * 64 + i] for i < 127 and t < T1_b, else 0   (f32 [B*T1p][128])
void ms_frames(const float* pcm, int64_t stride, const int* lens, int B, int T1p, float* frames, hipStream_t st);
// h [B*T1p][dp] (conv1 output): tanh in place, then per utterance the mean and rstd (eps) of its
// [T1_b][d] valid values -> stats[b][2]; two passes, one workgroup per utterance
void ms_tanh_gn_stats(float* h, const int* lens, int B, int T1p, int d, int dp, float eps, float* stats, hipStream_t st);
// conv2's gathered input: A [(b * T2p + t2)][k * dp + c] = f16(GroupNorm(h)[b][3 t2 + k][c]) (t2 < T2_b, c < d; else 0)
void ms_gather2(const float* h, const float* stats, const float* gw, const float* gb, const int* lens, int B, int T1p,
                int T2p, int d, int dp, void* A, hipStream_t st);
// conv3's gathered input: A [(b * T3p + t3)][k * n2p + c] = f16(gelu(c2[b][2 t3 + k][c])) (t3 < T3_b; else 0)
void ms_gather3(const float* c2, const int* lens, int B, int T2p, int T3p, int n2p, void* A, hipStream_t st);
// x [B*Tp][ld] f32: erf GELU in place for t < lens[b][li], zero for the other rows
void ms_gelu_rows(float* x, const int* lens, int li, int B, int Tp, int ld, hipStream_t st);
// y16 [M][ld] = f16(gelu(x [M][ld]))
void ms_gelu_f16(const float* x, int64_t n, void* y, hipStream_t st);
// bias-free LayerNorm (eps 1e-5) of x [M][ldx] over its first d columns -> y [M][ldy] (f16, or f32
// when out_f32), columns d .. ldy - 1 zeroed
void ms_layernorm(const float* x, int M, int d, int ldx, const float* w, void* y, int ldy, bool out_f32, hipStream_t st);
// encoder rotary: qkv32 [B*Tp][3 dp] (q | k | v, head h at h * dh) -> qkv16 (f16), q and k rotated at
// position t (interleaved pairs, the first `rot` dims of each head), v copied; tab [P][rot] = cos | sin halves
void ms_rope_enc(const float* qkv32, int B, int Tp, int H, int dh, int rot, int dp, const float* tab, void* qkv16,
                 hipStream_t st);
// decode rotary + cache append: qkv32 [R][3 d] -> q16 [R][d], K/V cache [2][R][ctx][d] row st->step
void ms_rope_dec(const float* qkv32, int R, int H, int dh, int rot, int d, const float* tab, const MsState* s, void* q16,
                 void* cache, int ctx, hipStream_t st);
// attention, f32 softmax over f16 q / k / v, head dim dh <= 64, scale dh^-0.5; out f16.
// MS_ATT_ENC: queries and keys t < T3_b of utterance b (rows >= T3_b of out zeroed); MS_ATT_SELF: one
// query per row, keys 0 .. st->step of the cache; MS_ATT_CROSS: one query per row, keys t < T3_b.
enum { MS_ATT_ENC = 0, MS_ATT_SELF = 1, MS_ATT_CROSS = 2 };
struct MsAttnArgs {
    const void* q; int ldq; int64_t q_bstride;   // query rows of batch b at q + b * q_bstride
    const void* k; const void* v; int ldk; int64_t k_bstride;  // k_bstride == 0 (cross): b * st->t3p * ldk
    void* out; int ldo; int64_t o_bstride;
    const int* lens; const MsState* s;
    int B, H, dh, Tq;                            // Tq: padded query rows per batch item (grid)
};
void ms_attention(int mode, const MsAttnArgs& a, hipStream_t st);
// decode-step GEMV: y[r][n] = x16[r] . W[n] (+ bias[n]); W f16 [N][K], x16 f16 [R][K], K % 8 == 0, R <= 64
// F32: out f32 [R][N]; RESID: out f32 [R][N] += ; F16: out f16; SILU: W has 2N rows, out f16 [R][N] =
// silu(y[n + N]) * y[n]; LOGITS: F32 written at the MsState's logits (+ step * R * N when log_all)
enum { MS_GV_F32 = 0, MS_GV_RESID = 1, MS_GV_F16 = 2, MS_GV_SILU = 3, MS_GV_LOGITS = 4 };
void ms_gemv(int mode, const void* x16, int R, int K, const void* W, const float* bias, int N, void* out,
             const MsState* s, hipStream_t st);
// x [R][d] = emb[token fed at this step] (forced or the previous argmax)
void ms_embed(const void* emb, int d, int R, const int* cur_tok, const int* forced, const MsState* s, float* x,
              hipStream_t st);
struct MsFinArgs {
    int R, V;
    const MsState* s;
    int* cur_tok; int* done; int* n_out; int* hit_eos; const int* limit;  // [R]
    int* out_tok; float* out_top1; float* out_top2;                       // [R][cap]
};
// argmax (lowest index on ties) + runner-up of each row's logits, recorded while the row is live;
// a live row ends at eos (not recorded) or at its limit
void ms_finalize(const MsFinArgs& a, hipStream_t st);
void ms_advance(MsState* s, hipStream_t st);

}  // namespace spt
