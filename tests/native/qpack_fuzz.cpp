// qpack_fuzz.cpp -- the host packer of SPT_MODEL_QUANT_RESIDENT (spittle_amd/csrc/ggml_qpack.h) alone, for a
// build with AddressSanitizer + UndefinedBehaviorSanitizer (g++, no device code; tests/test_qresident_sanitizers.py).
//   qpack_fuzz <ggml type> <N> <K> <file of blocks>
// The file's bytes are read into a heap buffer of exactly their size, so a packer that reads past a
// truncated tensor is caught.  Prints "rejected" (unsupported type, K not a multiple of 128, or a source
// shorter than [N][K / 32] blocks) or "packed: <N> x <K> lossless" once every element unpacked from the
// records equals ggml_dequant_block's value of the file's block bit for bit; exit 1 on a mismatch.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../spittle_amd/csrc/ggml_qpack.h"

int main(int argc, char** argv) {
    if (argc != 5) {
        fprintf(stderr, "usage: qpack_fuzz <ggml type> <N> <K> <file>\n");
        return 2;
    }
    const int type = atoi(argv[1]);
    const long long N = atoll(argv[2]), K = atoll(argv[3]);
    FILE* f = fopen(argv[4], "rb");
    if (!f) return 2;
    fseek(f, 0, SEEK_END);
    const long sz = ftell(f);
    fseek(f, 0, SEEK_SET);
    uint8_t* src = (uint8_t*)malloc(sz > 0 ? (size_t)sz : 1);  // exactly the file: no slack behind it
    if (sz > 0 && fread(src, 1, (size_t)sz, f) != (size_t)sz) return 2;
    fclose(f);
    const int64_t pb = spt::qpack_bytes(type, N, K);
    if (pb <= 0 || pb > ((int64_t)1 << 30)) {
        printf("rejected\n");
        free(src);
        return 0;
    }
    uint8_t* dst = (uint8_t*)malloc((size_t)pb);  // exactly the records
    if (!spt::qpack_rows(type, src, (size_t)sz, N, K, dst)) {
        printf("rejected\n");
        free(src);
        free(dst);
        return 0;
    }
    std::vector<float> back((size_t)(N * K));
    if (!spt::qpack_unpack_f32(type, dst, N, K, back.data())) return 1;
    int blck, bb;
    spt::ggml_block_geom(type, &blck, &bb);
    long long bad = 0;
    for (long long b = 0; b < N * K / 32; ++b) {
        float want[32];
        spt::ggml_dequant_block(type, src + b * bb, [&](int i, float v) { want[i] = v; });
        bad += memcmp(want, back.data() + b * 32, sizeof(want)) != 0;
    }
    free(src);
    free(dst);
    if (bad) {
        printf("mismatch in %lld blocks\n", bad);
        return 1;
    }
    printf("packed: %lld x %lld lossless\n", N, K);
    return 0;
}
