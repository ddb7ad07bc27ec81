// sv_host.h -- the host-only parts of the SenseVoice engine: dimensions, the model-spec grammar, the
// tensor-name table, the frame / LFR / row arithmetic, the CTC collapse rule and the detokeniser.
// No HIP here (SV_HD is empty outside hipcc), so the sanitizer harness (tests/native/sv_fuzz.cpp)
// builds it alone.
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "ms_host.h"

#if defined(__HIPCC__)
#define SV_HD __host__ __device__
#else
#define SV_HD
#endif

namespace spt {

constexpr int SV_FRAME = 400, SV_HOP = 160, SV_NFFT = 512, SV_NBIN = 257, SV_DFT_N = 640, SV_MELS = 80;
constexpr int SV_NQ = 4;          // query rows in front of the LFR rows: language, event, emotion, text norm
constexpr int SV_EMBED_ROWS = 16;
constexpr int SV_FSMN_K = 11;
constexpr int SV_N_LANG = 6;      // auto, zh, en, yue, ja, ko
constexpr int SV_MAX_SAMPLES = 4800000;  // 300 s

struct SvDims {
    int d = 512, H = 4, dh = 128, ff = 2048, n0 = 1, n1 = 49, n2 = 20, vocab = 25055;
    // [upstream, unverifiable offline]: recalled defaults, all settable through the model parameters
    int lfr_m = 7, lfr_n = 6, sanm_shift = 0, blank = 0, n_prefix = 4;
    float ln_eps = 1e-5f;
    int lang_rows[SV_N_LANG] = {0, 3, 4, 7, 11, 12};
    int event_row = 1, emo_row = 2, itn_row = 14, no_itn_row = 15;
    int in() const { return SV_MELS * lfr_m; }
    int layers() const { return n0 + n1 + n2; }
};

struct SvSpec {
    bool synthetic = true;   // false: "empty:", weights through set_tensor
    SvDims dims;
    bool has_seed = false;
    uint64_t seed = 0;
};

inline int sv_pad64(int v) { return (v + 63) / 64 * 64; }
// Kaldi snip_edges frames of n samples
inline int sv_frames_of(int64_t n) {
    if (n > INT32_MAX) n = INT32_MAX;  // the count stays an int whatever the caller passes
    return n < SV_FRAME ? 0 : (int)((n - SV_FRAME) / SV_HOP + 1);
}
// low-frame-rate rows of T frames
inline int sv_lfr_rows_of(int T, int lfr_n) { return T <= 0 || lfr_n <= 0 ? 0 : (T + lfr_n - 1) / lfr_n; }
// encoder rows of n samples (0: nothing to transcribe)
inline int sv_rows_of(int64_t n, int lfr_n) {
    const int t = sv_lfr_rows_of(sv_frames_of(n), lfr_n);
    return t ? t + SV_NQ : 0;
}
// the fbank frame that column block k of LFR row i reads: (lfr_m - 1) / 2 copies of frame 0 in front,
// copies of the last frame behind
SV_HD inline int sv_lfr_frame(int i, int k, int T, int lfr_m, int lfr_n) {
    int64_t f = (int64_t)i * lfr_n + k - (lfr_m - 1) / 2;
    if (f < 0) f = 0;
    if (f > T - 1) f = T - 1;
    return (int)f;
}

inline bool sv_dims_ok(const SvDims& d, std::string* err) {
    if (d.dh != 128 || d.H < 1 || d.d != d.H * d.dh || d.d > 1280) { *err = "sensevoice: head dim must be 128 and d = H * 128 <= 1280"; return false; }
    if (d.ff < 64 || d.ff % 64 || d.ff > 16384) { *err = "sensevoice: ff must be a multiple of 64"; return false; }
    if (d.n0 != 1 || d.n1 < 0 || d.n2 < 0 || d.layers() > 256) { *err = "sensevoice: bad layer counts"; return false; }
    if (d.vocab < 4 || d.vocab > (1 << 20)) { *err = "sensevoice: vocabulary outside 4..2^20"; return false; }
    if (d.lfr_m < 1 || d.lfr_m > 16 || d.lfr_n < 1 || d.lfr_n > 16) { *err = "sensevoice: lfr_m and lfr_n must be in 1..16"; return false; }
    if (d.sanm_shift < -5 || d.sanm_shift > 5) { *err = "sensevoice: sanm_shift must be in -5..5"; return false; }
    if (d.blank < 0 || d.blank >= d.vocab) { *err = "sensevoice: blank id outside the vocabulary"; return false; }
    if (d.n_prefix < 0 || d.n_prefix > SV_NQ) { *err = "sensevoice: n_prefix must be in 0..4"; return false; }
    if (!(d.ln_eps > 0.0f && d.ln_eps < 1.0f)) { *err = "sensevoice: ln_eps must be in (0, 1)"; return false; }
    const int rows[4] = {d.event_row, d.emo_row, d.itn_row, d.no_itn_row};
    for (int r : rows)
        if (r < 0 || r >= SV_EMBED_ROWS) { *err = "sensevoice: query row outside 0..15"; return false; }
    for (int r : d.lang_rows)
        if (r < 0 || r >= SV_EMBED_ROWS) { *err = "sensevoice: language row outside 0..15"; return false; }
    return true;
}

// "synthetic:sensevoice-small|sensevoice-test-small[:layers=a,b][:vocab=V][:seed=S]" or "empty:..." with
// the same grammar; layers=a,b sets encoders / tp_encoders (encoders0 is always one layer).
inline bool sv_parse_spec(const char* spec, SvSpec* out, std::string* err) {
    if (!spec) { *err = "null model spec"; return false; }
    std::string s(spec);
    std::vector<std::string> parts;
    size_t at = 0;
    while (true) {
        const size_t c = s.find(':', at);
        parts.push_back(s.substr(at, c == std::string::npos ? std::string::npos : c - at));
        if (c == std::string::npos) break;
        at = c + 1;
    }
    SvSpec r;
    if (parts[0] == "synthetic") r.synthetic = true;
    else if (parts[0] == "empty") r.synthetic = false;
    else { *err = "model spec must start with synthetic: or empty: (got '" + s.substr(0, 64) + "')"; return false; }
    if (parts.size() < 2) { *err = "model spec names no model"; return false; }
    SvDims& d = r.dims;
    if (parts[1] == "sensevoice-small") {
    } else if (parts[1] == "sensevoice-test-small") {
        d.d = 256; d.H = 2; d.ff = 512; d.n1 = 2; d.n2 = 1; d.vocab = 500;
    } else { *err = "unknown sensevoice model '" + parts[1].substr(0, 64) + "'"; return false; }
    for (size_t i = 2; i < parts.size(); i++) {
        const size_t eq = parts[i].find('=');
        if (eq == std::string::npos) { *err = "bad model spec option '" + parts[i].substr(0, 64) + "'"; return false; }
        const std::string key = parts[i].substr(0, eq), val = parts[i].substr(eq + 1);
        uint64_t v = 0, w = 0;
        const size_t comma = val.find(',');
        if (key == "layers" && comma != std::string::npos && ms_parse_uint(val.substr(0, comma), 128, &v) &&
            ms_parse_uint(val.substr(comma + 1), 128, &w)) { d.n1 = (int)v; d.n2 = (int)w; }
        else if (key == "vocab" && ms_parse_uint(val, 1u << 20, &v) && v >= 4) d.vocab = (int)v;
        else if (key == "seed" && ms_parse_uint(val, UINT64_MAX, &v)) { r.seed = v; r.has_seed = true; }
        else { *err = "bad model spec option '" + parts[i].substr(0, 64) + "'"; return false; }
    }
    *out = r;
    return true;
}

// FunASR state-dict prefix of layer l of the n0 + n1 + n2 stack
inline std::string sv_layer_prefix(const SvDims& d, int l) {
    if (l < d.n0) return "encoder.encoders0." + std::to_string(l) + ".";
    if (l < d.n0 + d.n1) return "encoder.encoders." + std::to_string(l - d.n0) + ".";
    return "encoder.tp_encoders." + std::to_string(l - d.n0 - d.n1) + ".";
}

struct SvTensorName {
    std::string name;
    int64_t numel;
};
// every tensor the engine takes, in load order, with its element count
inline std::vector<SvTensorName> sv_tensor_names(const SvDims& D) {
    std::vector<SvTensorName> v;
    const int64_t d = D.d, ff = D.ff;
    v.push_back({"embed.weight", (int64_t)SV_EMBED_ROWS * D.in()});
    for (int l = 0; l < D.layers(); l++) {
        const std::string P = sv_layer_prefix(D, l);
        const int64_t din = l < D.n0 ? D.in() : d;
        v.push_back({P + "norm1.weight", din});
        v.push_back({P + "norm1.bias", din});
        v.push_back({P + "self_attn.linear_q_k_v.weight", 3 * d * din});
        v.push_back({P + "self_attn.linear_q_k_v.bias", 3 * d});
        v.push_back({P + "self_attn.fsmn_block.weight", d * SV_FSMN_K});
        v.push_back({P + "self_attn.linear_out.weight", d * d});
        v.push_back({P + "self_attn.linear_out.bias", d});
        v.push_back({P + "norm2.weight", d});
        v.push_back({P + "norm2.bias", d});
        v.push_back({P + "feed_forward.w_1.weight", ff * d});
        v.push_back({P + "feed_forward.w_1.bias", ff});
        v.push_back({P + "feed_forward.w_2.weight", d * ff});
        v.push_back({P + "feed_forward.w_2.bias", d});
    }
    v.push_back({"encoder.after_norm.weight", d});
    v.push_back({"encoder.after_norm.bias", d});
    v.push_back({"encoder.tp_norm.weight", d});
    v.push_back({"encoder.tp_norm.bias", d});
    v.push_back({"ctc.ctc_lo.weight", (int64_t)D.vocab * d});
    v.push_back({"ctc.ctc_lo.bias", D.vocab});
    return v;
}

// CTC greedy rule over ids[0 .. R): rows < n_prefix are labels; over the rest a run of equal ids
// counts once, at its first row, and blank runs are dropped.  frames are rows counted from n_prefix.
inline void sv_ctc_collapse_host(const int32_t* ids, int R, int n_prefix, int blank, std::vector<int32_t>* tok,
                                 std::vector<int32_t>* frame) {
    tok->clear();
    frame->clear();
    if (!ids) return;
    const int p = n_prefix < 0 ? 0 : n_prefix;
    for (int r = p; r < R; r++) {
        if (r > p && ids[r] == ids[r - 1]) continue;
        if (ids[r] == blank) continue;
        tok->push_back(ids[r]);
        frame->push_back(r - p);
    }
}

// SentencePiece decoding as the Moonshine engine's, plus the "<|...|>" tags of this vocabulary dropped
inline std::string sv_detokenize(const std::vector<std::string>& pieces, const int32_t* ids, int n) {
    if (pieces.empty() || !ids || n <= 0) return ms_detokenize(pieces, ids, n);
    std::vector<int32_t> keep;
    for (int i = 0; i < n; i++) {
        if (ids[i] < 0 || (size_t)ids[i] >= pieces.size()) continue;
        const std::string& p = pieces[(size_t)ids[i]];
        if (p.size() >= 4 && p.compare(0, 2, "<|") == 0 && p.compare(p.size() - 2, 2, "|>") == 0) continue;
        keep.push_back(ids[i]);
    }
    return ms_detokenize(pieces, keep.data(), (int)keep.size());
}

}  // namespace spt
