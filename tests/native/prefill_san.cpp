// prefill_san.cpp -- the host-only arithmetic of the block prefill (spittle_amd/csrc/prefill_host.h) under
// AddressSanitizer + UndefinedBehaviorSanitizer, stand-alone (tests/test_prefill_api.py builds and runs
// it): the workspace rows and bytes, the slices over a decode group's sequences, whether a prefix takes
// the block pass, and every refusal of the two spt_debug_attn_prefill_* hooks.  Exit 0 and "ok" when
// every property holds; a message and exit 1 otherwise.
#include <limits.h>
#include <stdio.h>

#include <vector>

#include "../../spittle_amd/csrc/prefill_host.h"

using namespace spt;

static int fails = 0;
#define CHECK(c)                                               \
    do {                                                       \
        if (!(c)) {                                            \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++fails;                                           \
        }                                                      \
    } while (0)

int main() {
    // workspace rows: the cap, never below one whole prefix
    CHECK(prefill_ws_rows(kPrefillRowCap, 448) == 2048);
    CHECK(prefill_ws_rows(1, 448) == 225 && prefill_ws_rows(0, 448) == 225 && prefill_ws_rows(-7, 448) == 225);
    CHECK(prefill_ws_rows(INT_MAX, 448) == INT_MAX);
    // bytes: large-v3 bf16 at the default cap; every array a multiple of 256 bytes; monotone in the rows
    CHECK(prefill_ws_bytes(2048, 1280, 2) == (int64_t)2048 * (4 + 1280 * 4 + 10 * 1280 * 2));
    CHECK(prefill_ws_bytes(225, 384, 4) % 256 == 0 && prefill_ws_bytes(1, 384, 2) % 256 == 0);
    CHECK(prefill_ws_bytes(INT_MAX, 1280, 4) > prefill_ws_bytes(INT_MAX - 1, 1280, 4));
    for (int rows = 1; rows < 600; rows += 7) CHECK(prefill_ws_bytes(rows + 1, 384, 2) >= prefill_ws_bytes(rows, 384, 2));
    // slices: whole sequences, every sequence in exactly one slice, no slice above the workspace
    for (int ws : {225, 226, 449, 450, 2048, INT_MAX})
        for (int P = 1; P <= 225; P += (P < 10 ? 1 : 13))
            for (int B = 1; B <= 64; B += (B < 6 ? 1 : 7)) {
                const int per = prefill_slice_seqs(B, P, ws), n = per ? (B + per - 1) / per : 0;
                CHECK(per >= 1 && per <= B && (int64_t)per * P <= ws);
                CHECK(n >= 1 && (int64_t)(n - 1) * per < B && (int64_t)n * per >= B);
                int covered = 0;
                for (int s0 = 0; s0 < B; s0 += per) covered += (B - s0 < per ? B - s0 : per);
                CHECK(covered == B);
            }
    CHECK(prefill_slice_seqs(4, 65, 225) == 3 && prefill_slice_seqs(4, 65, 2048) == 4);
    CHECK(prefill_slice_seqs(0, 65, 225) == 0 && prefill_slice_seqs(4, 0, 225) == 0 && prefill_slice_seqs(4, 226, 225) == 0);
    // the decision
    CHECK(kPrefillMinDefault == 17 && prefill_takes_block(true, false, 17, kPrefillMinDefault) && !prefill_takes_block(true, false, 16, kPrefillMinDefault));
    CHECK(prefill_takes_block(true, false, 8, 8) && !prefill_takes_block(true, false, 7, 8));
    CHECK(!prefill_takes_block(false, false, 225, 8) && !prefill_takes_block(true, true, 225, 8));
    CHECK(!prefill_takes_block(true, false, 0, 0) && prefill_takes_block(true, false, 1, -3));

    // the hooks' refusals (the pointers are only compared with null)
    float x = 0.f;
    const void* p = &x;
    CHECK(prefill_self_refusal(0, p, p, p, 2, 2, 448, 225).empty());
    CHECK(prefill_self_refusal(2, p, p, p, 1, 1, 1, 1).empty());
    CHECK(!prefill_self_refusal(0, nullptr, p, p, 2, 2, 448, 5).empty());
    CHECK(!prefill_self_refusal(0, p, nullptr, p, 2, 2, 448, 5).empty());
    CHECK(!prefill_self_refusal(0, p, p, nullptr, 2, 2, 448, 5).empty());
    for (int dt : {-1, 3, 4, INT_MAX, INT_MIN}) CHECK(!prefill_self_refusal(dt, p, p, p, 2, 2, 448, 5).empty());
    for (int P : {0, -1, 449, INT_MAX, INT_MIN}) CHECK(!prefill_self_refusal(0, p, p, p, 2, 2, 448, P).empty());
    for (int H : {0, -1, 1025, INT_MAX}) CHECK(!prefill_self_refusal(0, p, p, p, 2, H, 448, 5).empty());
    for (int B : {0, -1, 1025, INT_MAX}) CHECK(!prefill_self_refusal(0, p, p, p, B, 2, 448, 5).empty());
    CHECK(!prefill_self_refusal(0, p, p, p, 2, 2, 0, 1).empty());
    CHECK(!prefill_self_refusal(0, p, p, p, 1024, 1024, INT_MAX, INT_MAX).empty());  // no overflow on the way to "too large"

    std::vector<int32_t> map = {2, 2, 2, 2, 2, 0, 0, 0, 0, 0};
    CHECK(prefill_cross_refusal(1, p, p, p, p, 2, 3, 1, 2, 1500, 225, 448, nullptr, 1).empty());
    CHECK(prefill_cross_refusal(1, p, p, p, p, 10, 3, 0, 2, 257, 5, 448, map.data(), 5).empty());
    CHECK(!prefill_cross_refusal(1, nullptr, p, p, p, 2, 3, 1, 2, 33, 5, 448, nullptr, 1).empty());
    CHECK(!prefill_cross_refusal(1, p, nullptr, p, p, 2, 3, 1, 2, 33, 5, 448, nullptr, 1).empty());
    CHECK(!prefill_cross_refusal(1, p, p, nullptr, p, 2, 3, 1, 2, 33, 5, 448, nullptr, 1).empty());
    CHECK(!prefill_cross_refusal(1, p, p, p, nullptr, 2, 3, 1, 2, 33, 5, 448, nullptr, 1).empty());
    CHECK(!prefill_cross_refusal(5, p, p, p, p, 2, 3, 1, 2, 33, 5, 448, nullptr, 1).empty());
    for (int T : {0, -1, INT_MIN}) CHECK(!prefill_cross_refusal(1, p, p, p, p, 2, 3, 1, 2, T, 5, 448, nullptr, 1).empty());
    CHECK(!prefill_cross_refusal(1, p, p, p, p, 2, 3, 1, 2, INT_MAX, 5, 448, nullptr, 1).empty());
    for (int P : {0, -1, 449, INT_MAX}) CHECK(!prefill_cross_refusal(1, p, p, p, p, 2, 3, 1, 2, 33, P, 448, nullptr, 1).empty());
    for (int H : {0, -1, 1025}) CHECK(!prefill_cross_refusal(1, p, p, p, p, 2, 3, 1, H, 33, 5, 448, nullptr, 1).empty());
    CHECK(!prefill_cross_refusal(1, p, p, p, p, 2, 3, 2, 2, 33, 5, 448, nullptr, 1).empty());        // b0 + B > B_layout
    CHECK(!prefill_cross_refusal(1, p, p, p, p, 2, 3, -1, 2, 33, 5, 448, nullptr, 1).empty());
    CHECK(!prefill_cross_refusal(1, p, p, p, p, 2, 3, INT_MAX, 2, 33, 5, 448, nullptr, 1).empty());
    CHECK(!prefill_cross_refusal(1, p, p, p, p, 10, 3, 0, 2, 257, 5, 448, nullptr, 5).empty());       // share without a map
    CHECK(!prefill_cross_refusal(1, p, p, p, p, 10, 3, 0, 2, 257, 5, 448, map.data(), 3).empty());    // 3 does not divide 10
    CHECK(!prefill_cross_refusal(1, p, p, p, p, 10, 3, 0, 2, 257, 5, 448, map.data(), 0).empty());
    CHECK(!prefill_cross_refusal(1, p, p, p, p, 10, 3, 1, 2, 257, 5, 448, map.data(), 5).empty());    // b0 + 2 = the layout's end
    map[7] = 3;
    CHECK(!prefill_cross_refusal(1, p, p, p, p, 10, 3, 0, 2, 257, 5, 448, map.data(), 5).empty());    // a window outside the layout
    map[7] = -1;
    CHECK(!prefill_cross_refusal(1, p, p, p, p, 10, 3, 0, 2, 257, 5, 448, map.data(), 5).empty());
    map[7] = INT_MAX;
    CHECK(!prefill_cross_refusal(1, p, p, p, p, 10, 3, 0, 2, 257, 5, 448, map.data(), 5).empty());
    if (fails) return 1;
    printf("ok\n");
    return 0;
}
