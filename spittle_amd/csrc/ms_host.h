// ms_host.h -- the host-only parts of the Moonshine engine: dimensions, the model-spec grammar and
// the detokeniser.  No HIP here, so the sanitizer harness (tests/native/ms_fuzz.cpp) builds it alone.
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

namespace spt {

struct MsDims {
    int d = 416, H = 8, dh = 52, rot = 46, ff = 1664, n_enc = 8, n_dec = 8, vocab = 32768;
    int bos = 1, eos = 2;
    float theta = 10000.0f;
};

struct MsSpec {
    bool synthetic = true;   // false: "empty:", weights through set_tensor
    MsDims dims;
    bool has_seed = false;
    uint64_t seed = 0;
};

// rotary dim of a head: int(dh * 0.9) as HF computes it (double product truncated)
inline int ms_rotary_dim(int dh) { return (int)((double)dh * 0.9); }

inline bool ms_parse_uint(const std::string& s, uint64_t max, uint64_t* out) {
    if (s.empty() || s.size() > 20) return false;
    uint64_t v = 0;
    for (char c : s) {
        if (c < '0' || c > '9') return false;
        const uint64_t dgt = (uint64_t)(c - '0');
        if (v > (UINT64_MAX - dgt) / 10) return false;  // would overflow
        v = v * 10 + dgt;
    }
    if (v > max) return false;
    *out = v;
    return true;
}

// "synthetic:moonshine-base|moonshine-tiny|moonshine-test-small[:layers=N][:vocab=V][:eos=E][:seed=S]"
// or "empty:..." with the same grammar.  false + a message for anything else.
inline bool ms_parse_spec(const char* spec, MsSpec* out, std::string* err) {
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
    MsSpec r;
    if (parts[0] == "synthetic") r.synthetic = true;
    else if (parts[0] == "empty") r.synthetic = false;
    else { *err = "model spec must start with synthetic: or empty: (got '" + s.substr(0, 64) + "')"; return false; }
    if (parts.size() < 2) { *err = "model spec names no model"; return false; }
    MsDims& d = r.dims;
    if (parts[1] == "moonshine-base") {
    } else if (parts[1] == "moonshine-tiny") {
        d.d = 288; d.dh = 36; d.ff = 1152; d.n_enc = d.n_dec = 6;
    } else if (parts[1] == "moonshine-test-small") {
        d.n_enc = d.n_dec = 2; d.vocab = 1024;
    } else { *err = "unknown moonshine model '" + parts[1].substr(0, 64) + "'"; return false; }
    d.rot = ms_rotary_dim(d.dh);
    for (size_t i = 2; i < parts.size(); i++) {
        const size_t eq = parts[i].find('=');
        if (eq == std::string::npos) { *err = "bad model spec option '" + parts[i].substr(0, 64) + "'"; return false; }
        const std::string key = parts[i].substr(0, eq), val = parts[i].substr(eq + 1);
        uint64_t v = 0;
        if (key == "layers" && ms_parse_uint(val, 64, &v) && v >= 1) d.n_enc = d.n_dec = (int)v;
        else if (key == "vocab" && ms_parse_uint(val, 1u << 20, &v) && v >= 4) d.vocab = (int)v;
        else if (key == "eos" && ms_parse_uint(val, 1u << 20, &v)) d.eos = (int)v;
        else if (key == "seed" && ms_parse_uint(val, UINT64_MAX, &v)) { r.seed = v; r.has_seed = true; }
        else { *err = "bad model spec option '" + parts[i].substr(0, 64) + "'"; return false; }
    }
    if (d.eos >= d.vocab) { *err = "eos outside the vocabulary"; return false; }
    *out = r;
    return true;
}

// a piece the tokenizer never prints: <unk>, <s>, </s> and the "<<...>>" added tokens
inline bool ms_is_special_piece(const std::string& p) {
    if (p == "<unk>" || p == "<s>" || p == "</s>") return true;
    return p.size() >= 4 && p.compare(0, 2, "<<") == 0 && p.compare(p.size() - 2, 2, ">>") == 0;
}

// "<0xNN>" byte-fallback piece -> its byte, or -1
inline int ms_byte_piece(const std::string& p) {
    if (p.size() != 6 || p.compare(0, 3, "<0x") != 0 || p[5] != '>') return -1;
    int v = 0;
    for (int i = 3; i < 5; i++) {
        const char c = p[i];
        int h;
        if (c >= '0' && c <= '9') h = c - '0';
        else if (c >= 'A' && c <= 'F') h = c - 'A' + 10;
        else if (c >= 'a' && c <= 'f') h = c - 'a' + 10;
        else return -1;
        v = v * 16 + h;
    }
    return v;
}

// SentencePiece decoding of token ids: specials dropped, byte pieces to bytes, U+2581 to a space, the
// leading space stripped.  Ids outside the vocabulary are skipped; without a vocabulary "[id]".
inline std::string ms_detokenize(const std::vector<std::string>& pieces, const int32_t* ids, int n) {
    std::string out;
    if (!ids || n <= 0) return out;
    if (pieces.empty()) {
        for (int i = 0; i < n; i++) out += "[" + std::to_string(ids[i]) + "]";
        return out;
    }
    for (int i = 0; i < n; i++) {
        if (ids[i] < 0 || (size_t)ids[i] >= pieces.size()) continue;
        const std::string& p = pieces[(size_t)ids[i]];
        if (ms_is_special_piece(p)) continue;
        const int b = ms_byte_piece(p);
        if (b >= 0) { out.push_back((char)b); continue; }
        for (size_t j = 0; j < p.size();) {
            if (j + 2 < p.size() && (unsigned char)p[j] == 0xE2 && (unsigned char)p[j + 1] == 0x96 &&
                (unsigned char)p[j + 2] == 0x81) {
                out.push_back(' ');
                j += 3;
            } else
                out.push_back(p[j++]);
        }
    }
    if (!out.empty() && out[0] == ' ') out.erase(0, 1);
    return out;
}

}  // namespace spt
