// align_host.h -- the host side of the token alignment: grouping aligned tokens into words.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

namespace spt {

// whether the bytes end on a whole UTF-8 sequence (a byte-level BPE piece may stop inside one)
inline bool utf8_ends_whole(const std::string& s) {
    int i = (int)s.size() - 1, cont = 0;
    while (i >= 0 && cont < 3 && ((unsigned char)s[i] & 0xC0) == 0x80) {
        --i;
        ++cont;
    }
    if (i < 0) return cont == 0;
    const unsigned char c = (unsigned char)s[i];
    const int need = c < 0x80 ? 0 : (c & 0xE0) == 0xC0 ? 1 : (c & 0xF0) == 0xE0 ? 2 : (c & 0xF8) == 0xF0 ? 3 : -1;
    return need < 0 ? true : cont >= need;  // (a stray continuation or invalid lead byte splits nothing)
}

struct AlignWord {
    int i0, n;          // first token and token count
    int64_t t0, t1;     // first token's start, last token's end
    float p;            // mean of the token probabilities
    std::string text;   // the tokens' bytes
};

// A word starts at the first token and at every token whose piece begins with a space, except that a
// token whose bytes stop inside a UTF-8 sequence joins the token after it.
inline std::vector<AlignWord> align_words(const std::vector<std::string>& pieces, const int64_t* t0, const int64_t* t1,
                                          const float* p) {
    std::vector<AlignWord> w;
    double psum = 0.0;
    for (int i = 0; i < (int)pieces.size(); ++i) {
        const bool starts = i == 0 || (!pieces[i].empty() && pieces[i][0] == ' ' && utf8_ends_whole(w.back().text));
        if (starts) {
            w.push_back(AlignWord{i, 0, t0[i], t1[i], 0.0f, std::string()});
            psum = 0.0;
        }
        AlignWord& c = w.back();
        c.n += 1;
        c.t1 = t1[i];
        c.text += pieces[i];
        psum += p ? (double)p[i] : 0.0;
        c.p = (float)(psum / c.n);
    }
    return w;
}

}  // namespace spt
