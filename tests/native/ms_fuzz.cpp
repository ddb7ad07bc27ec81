// ms_fuzz.cpp -- the Moonshine engine's host-only input handling (spittle_amd/csrc/ms_host.h: the
// model-spec grammar and the detokeniser) under AddressSanitizer + UndefinedBehaviorSanitizer.
// A plain executable: `ms_fuzz spec <model spec>` prints "parsed ..." or "rejected: ...";
// `ms_fuzz detok <file>` reads pieces (one per line, the first line a list of ids) and prints the text;
// `ms_fuzz selftest` drives both with malformed input built here.  Exit 0 unless a check fails.
#include <stdio.h>
#include <string.h>

#include <fstream>
#include <string>
#include <vector>

#include "../../spittle_amd/csrc/ms_host.h"

static int do_spec(const char* s) {
    spt::MsSpec spec;
    std::string err;
    if (spt::ms_parse_spec(s, &spec, &err)) {
        const spt::MsDims& d = spec.dims;
        printf("parsed: %s d %d heads %d dh %d rot %d ff %d layers %d+%d vocab %d eos %d seed %s%llu\n",
               spec.synthetic ? "synthetic" : "empty", d.d, d.H, d.dh, d.rot, d.ff, d.n_enc, d.n_dec, d.vocab, d.eos,
               spec.has_seed ? "" : "default ", (unsigned long long)spec.seed);
    } else
        printf("rejected: %s\n", err.c_str());
    return 0;
}

static int selftest() {
    int bad = 0;
    const char* specs[] = {"", ":", "::::", "synthetic", "synthetic:", "empty:moonshine-base:", "synthetic:moonshine-base:layers=",
                           "synthetic:moonshine-base:layers=0", "synthetic:moonshine-base:layers=99999999999999999999999",
                           "synthetic:moonshine-base:vocab=-3", "synthetic:moonshine-base:eos=40000", "synthetic:moonshine-base:seed=1x",
                           "synthetic:moonshine-base:=5", "synthetic:moonshine-base:layers", "whisper:tiny",
                           "synthetic:moonshine-base:seed=18446744073709551616"};
    for (const char* s : specs) {
        spt::MsSpec spec;
        std::string err;
        if (spt::ms_parse_spec(s, &spec, &err) || err.empty()) {
            printf("accepted a bad spec: '%s'\n", s);
            bad++;
        }
    }
    std::string longspec = "synthetic:" + std::string(100000, 'm') + ":layers=" + std::string(5000, '9');
    spt::MsSpec spec;
    std::string err;
    if (spt::ms_parse_spec(longspec.c_str(), &spec, &err)) bad++;
    if (spt::ms_parse_spec(nullptr, &spec, &err)) bad++;
    if (!spt::ms_parse_spec("empty:moonshine-tiny:layers=2:vocab=1024:eos=7:seed=18446744073709551615", &spec, &err) ||
        spec.synthetic || spec.dims.d != 288 || spec.dims.rot != 32 || spec.dims.n_dec != 2 || spec.dims.eos != 7 ||
        spec.seed != 18446744073709551615ull)
        bad++;

    std::vector<std::string> pieces = {"<unk>", "<s>", "</s>", "\xE2\x96\x81hi", "<0xC3>", "<0xA9>", "<<ST_3>>", "<0xZZ>",
                                       "<0x4", "\xE2\x96", "", "\xE2\x96\x81", "<0xFF>", "<<", ">>", "<<>>"};
    std::vector<int32_t> ids;
    for (int i = -3; i < (int)pieces.size() + 3; i++) ids.push_back(i);
    ids.push_back(INT32_MAX);
    ids.push_back(INT32_MIN);
    const std::string all = spt::ms_detokenize(pieces, ids.data(), (int)ids.size());
    const int32_t cafe[] = {1, 3, 4, 5, 6, 2};
    if (spt::ms_detokenize(pieces, cafe, 6) != "hi\xC3\xA9") bad++;
    if (spt::ms_detokenize(pieces, nullptr, 5) != "" || spt::ms_detokenize(pieces, cafe, 0) != "" ||
        spt::ms_detokenize(pieces, cafe, -4) != "")
        bad++;
    if (spt::ms_detokenize(std::vector<std::string>(), cafe, 2) != "[1][3]") bad++;
    printf("selftest: %d failures, %zu bytes of text\n", bad, all.size());
    return bad ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc >= 2 && !strcmp(argv[1], "selftest")) return selftest();
    if (argc >= 3 && !strcmp(argv[1], "spec")) return do_spec(argv[2]);
    if (argc >= 3 && !strcmp(argv[1], "detok")) {
        std::ifstream f(argv[2], std::ios::binary);
        std::string line;
        std::vector<int32_t> ids;
        std::vector<std::string> pieces;
        if (std::getline(f, line)) {
            size_t at = 0;
            while (at < line.size()) {
                size_t e = line.find(' ', at);
                if (e == std::string::npos) e = line.size();
                uint64_t v = 0;
                const std::string tok = line.substr(at, e - at);
                if (!tok.empty() && tok[0] == '-') ids.push_back(-1);
                else if (spt::ms_parse_uint(tok, INT32_MAX, &v)) ids.push_back((int32_t)v);
                at = e + 1;
            }
        }
        while (std::getline(f, line)) pieces.push_back(line);
        const std::string text = spt::ms_detokenize(pieces, ids.data(), (int)ids.size());
        printf("text: ");
        fwrite(text.data(), 1, text.size(), stdout);
        printf("\n");
        return 0;
    }
    fprintf(stderr, "usage: ms_fuzz selftest | spec <model spec> | detok <file>\n");
    return 2;
}
