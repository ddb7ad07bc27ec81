// sv_fuzz.cpp -- the SenseVoice engine's host-only input handling (spittle_amd/csrc/sv_host.h: the
// model-spec grammar, the tensor-name table, the frame / LFR / row arithmetic, the CTC collapse rule
// and the detokeniser) under AddressSanitizer + UndefinedBehaviorSanitizer.
// A plain executable: `sv_fuzz spec <model spec>` prints "parsed ..." or "rejected: ...";
// `sv_fuzz lfr <samples> <lfr_m> <lfr_n>` prints the counts and the frame index of every LFR column block;
// `sv_fuzz names <model spec>` prints the tensor table; `sv_fuzz collapse <n_prefix> <blank> <ids...>`;
// `sv_fuzz detok <file>` reads pieces (one per line, the first line a list of ids) and prints the text;
// `sv_fuzz selftest` drives all of them with malformed input built here.  Exit 0 unless a check fails.
#include <stdio.h>
#include <string.h>

#include <fstream>
#include <string>
#include <vector>

#include "../../spittle_amd/csrc/sv_host.h"

static int do_spec(const char* s) {
    spt::SvSpec spec;
    std::string err;
    if (spt::sv_parse_spec(s, &spec, &err)) {
        const spt::SvDims& d = spec.dims;
        printf("parsed: %s d %d heads %d dh %d ff %d layers %d+%d+%d vocab %d in %d seed %s%llu\n",
               spec.synthetic ? "synthetic" : "empty", d.d, d.H, d.dh, d.ff, d.n0, d.n1, d.n2, d.vocab, d.in(),
               spec.has_seed ? "" : "default ", (unsigned long long)spec.seed);
    } else
        printf("rejected: %s\n", err.c_str());
    return 0;
}

static int do_lfr(int64_t n, int m, int k) {
    const int T = spt::sv_frames_of(n), Tl = spt::sv_lfr_rows_of(T, k), R = spt::sv_rows_of(n, k);
    printf("frames %d lfr %d rows %d\n", T, Tl, R);
    if (m < 1 || m > 16 || k < 1 || k > 16) return 0;
    for (int i = 0; i < Tl; i++) {
        printf("row %d:", i);
        for (int j = 0; j < m; j++) {
            const int f = spt::sv_lfr_frame(i, j, T, m, k);
            if (f < 0 || f >= T) {
                printf(" OUT-OF-RANGE\n");
                return 1;
            }
            printf(" %d", f);
        }
        printf("\n");
    }
    return 0;
}

static int selftest() {
    int bad = 0;
    const char* specs[] = {"", ":", "::::", "synthetic", "synthetic:", "empty:sensevoice-small:", "synthetic:sensevoice-small:layers=",
                           "synthetic:sensevoice-small:layers=3", "synthetic:sensevoice-small:layers=3,", "synthetic:sensevoice-small:layers=,3",
                           "synthetic:sensevoice-small:layers=999,1", "synthetic:sensevoice-small:layers=1,99999999999999999999999",
                           "synthetic:sensevoice-small:vocab=-3", "synthetic:sensevoice-small:vocab=3", "synthetic:sensevoice-small:seed=1x",
                           "synthetic:sensevoice-small:=5", "synthetic:sensevoice-small:layers", "synthetic:moonshine-base",
                           "synthetic:sensevoice-small:seed=18446744073709551616", "synthetic:sensevoice-small:layers=1,2,3"};
    for (const char* s : specs) {
        spt::SvSpec spec;
        std::string err;
        if (spt::sv_parse_spec(s, &spec, &err) || err.empty()) {
            printf("accepted a bad spec: '%s'\n", s);
            bad++;
        }
    }
    std::string longspec = "synthetic:" + std::string(100000, 's') + ":layers=" + std::string(5000, '9');
    spt::SvSpec spec;
    std::string err;
    if (spt::sv_parse_spec(longspec.c_str(), &spec, &err)) bad++;
    if (spt::sv_parse_spec(nullptr, &spec, &err)) bad++;
    if (!spt::sv_parse_spec("empty:sensevoice-test-small:layers=0,3:vocab=777:seed=18446744073709551615", &spec, &err) ||
        spec.synthetic || spec.dims.d != 256 || spec.dims.H != 2 || spec.dims.n1 != 0 || spec.dims.n2 != 3 ||
        spec.dims.vocab != 777 || spec.seed != 18446744073709551615ull || !spt::sv_dims_ok(spec.dims, &err))
        bad++;

    // dimension checks: each recalled parameter out of range is refused
    {
        spt::SvDims d;
        if (!spt::sv_dims_ok(d, &err)) bad++;
        spt::SvDims e = d; e.lfr_m = 0; if (spt::sv_dims_ok(e, &err)) bad++;
        e = d; e.lfr_n = 17; if (spt::sv_dims_ok(e, &err)) bad++;
        e = d; e.sanm_shift = 6; if (spt::sv_dims_ok(e, &err)) bad++;
        e = d; e.blank = d.vocab; if (spt::sv_dims_ok(e, &err)) bad++;
        e = d; e.n_prefix = 5; if (spt::sv_dims_ok(e, &err)) bad++;
        e = d; e.ln_eps = 0.0f; if (spt::sv_dims_ok(e, &err)) bad++;
        e = d; e.lang_rows[5] = 16; if (spt::sv_dims_ok(e, &err)) bad++;
        e = d; e.itn_row = -1; if (spt::sv_dims_ok(e, &err)) bad++;
        e = d; e.dh = 64; if (spt::sv_dims_ok(e, &err)) bad++;
    }

    // tensor table: names are unique, layer prefixes walk the three blocks, counts add up
    {
        spt::SvDims d;
        const std::vector<spt::SvTensorName> names = spt::sv_tensor_names(d);
        if (names.size() != 1u + 13u * 70u + 6u) bad++;
        int64_t params = 0;
        for (size_t i = 0; i < names.size(); i++) {
            params += names[i].numel;
            if (names[i].numel <= 0) bad++;
            for (size_t j = 0; j < i; j++)
                if (names[i].name == names[j].name) bad++;
        }
        if (params < 230000000 || params > 240000000) bad++;  // about 234 M
        if (spt::sv_layer_prefix(d, 0) != "encoder.encoders0.0." || spt::sv_layer_prefix(d, 1) != "encoder.encoders.0." ||
            spt::sv_layer_prefix(d, 49) != "encoder.encoders.48." || spt::sv_layer_prefix(d, 50) != "encoder.tp_encoders.0." ||
            spt::sv_layer_prefix(d, 69) != "encoder.tp_encoders.19.")
            bad++;
    }

    // frame / LFR / row arithmetic at the edges, and every index inside [0, T)
    {
        const int64_t ns[] = {-5, 0, 399, 400, 559, 560, 1360, 57999, 58000, 160000, 480000, 4800000, (int64_t)1 << 40};
        const int want_T[] = {0, 0, 0, 1, 1, 2, 7, 360, 361, 998, 2998, 29998, 13421771};
        for (size_t i = 0; i < sizeof(ns) / sizeof(ns[0]); i++) {
            if (spt::sv_frames_of(ns[i]) != want_T[i]) bad++;
            for (int m = 1; m <= 16; m += 3)
                for (int k = 1; k <= 16; k += 5) {
                    const int T = spt::sv_frames_of(ns[i]), Tl = spt::sv_lfr_rows_of(T, k);
                    if (T > 0 && (Tl < 1 || (int64_t)(Tl - 1) * k >= T || (int64_t)Tl * k < T)) bad++;
                    if (spt::sv_rows_of(ns[i], k) != (Tl ? Tl + 4 : 0)) bad++;
                    const int rows[] = {0, Tl / 2, Tl - 1};
                    for (int r : rows)
                        for (int j = 0; j < m && T > 0; j++) {
                            const int f = spt::sv_lfr_frame(r, j, T, m, k);
                            if (f < 0 || f >= T) bad++;
                        }
                }
        }
        if (spt::sv_rows_of(400, 6) != 5 || spt::sv_rows_of(1360, 6) != 6 || spt::sv_rows_of(57999, 6) != 64 ||
            spt::sv_rows_of(58000, 6) != 65 || spt::sv_rows_of(160000, 6) != 171 || spt::sv_rows_of(480000, 6) != 504)
            bad++;
        if (spt::sv_lfr_rows_of(5, 0) != 0 || spt::sv_lfr_rows_of(-3, 6) != 0) bad++;
        // T = 7, m = 7, n = 6: rows 0 and 1
        const int want0[] = {0, 0, 0, 0, 1, 2, 3}, want1[] = {3, 4, 5, 6, 6, 6, 6};
        for (int j = 0; j < 7; j++)
            if (spt::sv_lfr_frame(0, j, 7, 7, 6) != want0[j] || spt::sv_lfr_frame(1, j, 7, 7, 6) != want1[j]) bad++;
        if (spt::sv_lfr_frame(INT32_MAX, 15, 1, 16, 16) != 0) bad++;  // no overflow in the row product
    }

    // CTC collapse
    {
        std::vector<int32_t> tok, fr;
        const int32_t ids[] = {7, 0, 0, 9, 5, 5, 0, 0, 5, 6, 6, 6, 0};
        spt::sv_ctc_collapse_host(ids, 13, 4, 0, &tok, &fr);
        if (tok != std::vector<int32_t>({5, 5, 6}) || fr != std::vector<int32_t>({0, 4, 5})) bad++;
        spt::sv_ctc_collapse_host(ids, 13, 0, 5, &tok, &fr);
        if (tok != std::vector<int32_t>({7, 0, 9, 0, 6, 0}) || fr != std::vector<int32_t>({0, 1, 3, 6, 9, 12})) bad++;
        spt::sv_ctc_collapse_host(ids, 3, 4, 0, &tok, &fr);
        if (!tok.empty() || !fr.empty()) bad++;
        spt::sv_ctc_collapse_host(nullptr, 9, 4, 0, &tok, &fr);
        if (!tok.empty()) bad++;
        spt::sv_ctc_collapse_host(ids, 13, -2, 0, &tok, &fr);
        if (tok.empty()) bad++;
        spt::sv_ctc_collapse_host(ids, -1, 4, 0, &tok, &fr);
        if (!tok.empty()) bad++;
    }

    std::vector<std::string> pieces = {"<unk>", "<s>", "</s>", "\xE2\x96\x81hi", "<0xC3>", "<0xA9>", "<|en|>", "<0xZZ>",
                                       "<0x4", "\xE2\x96", "", "\xE2\x96\x81", "<0xFF>", "<|", "|>", "<||>", "<|NEUTRAL|>"};
    std::vector<int32_t> ids;
    for (int i = -3; i < (int)pieces.size() + 3; i++) ids.push_back(i);
    ids.push_back(INT32_MAX);
    ids.push_back(INT32_MIN);
    const std::string all = spt::sv_detokenize(pieces, ids.data(), (int)ids.size());
    const int32_t cafe[] = {6, 16, 3, 4, 5, 15, 2};
    if (spt::sv_detokenize(pieces, cafe, 7) != "hi\xC3\xA9") bad++;
    const int32_t tags[] = {6, 16, 15};
    if (spt::sv_detokenize(pieces, tags, 3) != "") bad++;
    if (spt::sv_detokenize(pieces, nullptr, 5) != "" || spt::sv_detokenize(pieces, cafe, 0) != "" ||
        spt::sv_detokenize(pieces, cafe, -4) != "")
        bad++;
    if (spt::sv_detokenize(std::vector<std::string>(), cafe, 2) != "[6][16]") bad++;
    printf("selftest: %d failures, %zu bytes of text\n", bad, all.size());
    return bad ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc >= 2 && !strcmp(argv[1], "selftest")) return selftest();
    if (argc >= 3 && !strcmp(argv[1], "spec")) return do_spec(argv[2]);
    if (argc >= 5 && !strcmp(argv[1], "lfr")) return do_lfr(atoll(argv[2]), atoi(argv[3]), atoi(argv[4]));
    if (argc >= 3 && !strcmp(argv[1], "names")) {
        spt::SvSpec spec;
        std::string err;
        if (!spt::sv_parse_spec(argv[2], &spec, &err)) {
            printf("rejected: %s\n", err.c_str());
            return 0;
        }
        for (const spt::SvTensorName& t : spt::sv_tensor_names(spec.dims)) printf("%s %lld\n", t.name.c_str(), (long long)t.numel);
        return 0;
    }
    if (argc >= 4 && !strcmp(argv[1], "collapse")) {
        std::vector<int32_t> ids, tok, fr;
        for (int i = 4; i < argc; i++) ids.push_back(atoi(argv[i]));
        spt::sv_ctc_collapse_host(ids.data(), (int)ids.size(), atoi(argv[2]), atoi(argv[3]), &tok, &fr);
        printf("tokens:");
        for (size_t i = 0; i < tok.size(); i++) printf(" %d@%d", tok[i], fr[i]);
        printf("\n");
        return 0;
    }
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
        const std::string text = spt::sv_detokenize(pieces, ids.data(), (int)ids.size());
        printf("text: ");
        fwrite(text.data(), 1, text.size(), stdout);
        printf("\n");
        return 0;
    }
    fprintf(stderr, "usage: sv_fuzz selftest | spec <s> | lfr <n> <m> <k> | names <s> | collapse <p> <b> <ids..> | detok <file>\n");
    return 2;
}
