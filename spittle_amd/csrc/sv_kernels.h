// sv_kernels.h -- host launchers of the SenseVoice kernels (k_sv.hip), gfx950.
//
// Batch layout as in ms_kernels.h: B utterances padded to the longest one, row (b, t) of a
// [B * Tp][...] tensor is b * Tp + t.  lens[b][4] = {samples, T fbank frames, T_lfr, R = T_lfr + 4}
// lives on the device; every kernel that mixes rows masks t >= len (loads clamped, never multiplied
// away), so a padded batch row computes exactly what it computes alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace spt {

// Kaldi framing: frames[(b * Tp + t)][i] = window[i] * preemph(x - mean(x))[i] for the 400 samples
// x = 32768 * pcm_b[160 t ..], i < 400 and t < T_b; columns 400..511 and rows t >= T_b are zero
void sv_frames(const float* pcm, int64_t stride, const int* lens, int B, int Tp, const float* window, float* frames,
               hipStream_t st);
// spec [M][640] (re 0..256 | im 257..513) -> mel [M][80] = log(max(fbT^T |spec|^2, 2^-23)); fbT [257][80]
void sv_melpow(const float* spec, int M, const float* fbT, float* mel, hipStream_t st);

struct SvRowsArgs {
    const float* mel;        // [B * Tp][80]
    const int* lens;
    const float* neg_mean;   // [in]
    const float* inv_std;    // [in]
    const float* embed;      // [16][in]
    const float* inv_freq;   // [in / 2]
    int Tp, Rp, in, ld, lfr_m, lfr_n;
    int q[4];                // embed row of each query row
    float scale;             // sqrt(d)
    int feat_only;           // 1: CMVN rows only (no scale, no positions), query rows zero
    float* out;              // [B * Rp][ld], columns >= in and rows >= R_b zero
};
// the encoder's input rows: 4 query rows, then the LFR rows after CMVN; all scaled, plus the sinusoid
// of position row + 1
void sv_lfr_rows(const SvRowsArgs& a, int B, hipStream_t st);
// LayerNorm with weight and bias over the first d columns of x [M][ldx] -> y [M][ldy] (f16, or f32 when
// out_f32), columns d .. ldy - 1 zeroed.  y may be x when out_f32 and ldy == ldx.
void sv_layernorm(const float* x, int M, int d, int ldx, const float* w, const float* b, float eps, void* y, int ldy,
                  bool out_f32, hipStream_t st);
// FSMN memory: mem[t][c] = sum_j w[c][j] * v[t + j - (5 + shift)][c] + v[t][c], v f16 [B * Rp][ldv] rows
// outside [0, R_b) read as zero; x [B * Rp][d] f32 += mem (add) or = mem; rows t >= R_b of x are zeroed
void sv_fsmn(const void* v, int ldv, const float* w, const int* lens, int B, int Rp, int d, int shift, bool add, float* x,
             hipStream_t st);
// attention with head dim 128 over the fused f16 qkv [B * Rp][3 d] (q | k | v, head h at h * 128):
// softmax((q . k) * 128^-0.5 over keys < R_b) v -> out f16 [B * Rp][d]; query rows >= R_b write zeros
void sv_attention(const void* qkv, const int* lens, int B, int Rp, int H, void* out, hipStream_t st);
// per row of logits [M][ld]: argmax (lowest index on ties) and runner-up over columns < V only
void sv_ctc_top2(const float* logits, int M, int V, int ld, int* ids, float* top1, float* top2, hipStream_t st);

// per utterance: out[b][0] = token count, out[b][1..4] = prefix labels (-1 beyond n_prefix), then at
// out[b] + 8: tokens [cap], frames [cap], top1 bits [cap], top2 bits [cap]; row stride 8 + 4 cap
struct SvCollapseArgs {
    const int* ids; const float* top1; const float* top2;  // [B * Rp]
    const int* lens;
    int Rp, n_prefix, blank, cap;
    int* out;
};
void sv_ctc_collapse(const SvCollapseArgs& a, int B, hipStream_t st);

}  // namespace spt
