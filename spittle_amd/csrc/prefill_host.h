// prefill_host.h -- the host-only arithmetic of the block prefill: the workspace's row cap
// and bytes, the slices a decode group's sequences run in, and what the spt_debug_attn_prefill_* hooks
// refuse before they look for a device.  No HIP: tests/native/prefill_san.cpp compiles it alone under the
// sanitizers.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <string>

namespace spt {

// P_min, in prefix positions: the smallest measured prefix from which the block pass wins at B = 1 and B = 8
// (16 prompt tokens + [prev]; 9 positions lose by 0.9 ms at B = 1: DESIGN 4.7); SPT_BLOCK_PREFILL_MIN overrides it
constexpr int kPrefillMinDefault = 17;
constexpr int kPrefillRowCap = 2048;       // workspace rows of a decode group (SPT_BLOCK_PREFILL_ROWS: tests)
constexpr int64_t kPrefillMaxElems = (int64_t)1 << 26;  // of any one buffer of a hook call

// rows the workspace is allocated for: the cap, but never fewer than one whole prefix (P <= ctx / 2 + 1)
inline int prefill_ws_rows(int cap, int n_text_ctx) { return std::max(std::max(cap, 1), n_text_ctx / 2 + 1); }

// bytes of one decode group's workspace: per row the token (int32), the f32 residual (d) and, in the
// engine dtype, the normalised row (d), qkv (3 d), the cross q (d), the attention output (d) and fc1's
// output (4 d); each array rounded up to 256 bytes
inline int64_t prefill_ws_bytes(int rows, int d, int esz) {
    auto up = [](int64_t n) { return (n + 255) / 256 * 256; };
    const int64_t r = rows;
    return up(r * 4) + up(r * d * 4) + up(r * d * esz) + up(r * 3 * d * esz) + 2 * up(r * d * esz) + up(r * 4 * d * esz);
}

// whole sequences per slice: B sequences of P rows each through a workspace of ws_rows rows (>= P)
inline int prefill_slice_seqs(int B, int P, int ws_rows) {
    if (B < 1 || P < 1 || ws_rows < P) return 0;
    return std::min(B, ws_rows / P);
}

// whether a prefix of P positions takes the block pass (flag set, dense weights, P >= P_min)
inline bool prefill_takes_block(bool flag, bool quant_resident, int P, int p_min) {
    return flag && !quant_resident && P >= std::max(1, p_min);
}

inline bool prefill_dtype_ok(int dtype) { return dtype == 0 || dtype == 1 || dtype == 2; }

// the hooks' refusals: "" when the call is valid
inline std::string prefill_self_refusal(int dtype, const void* qkv, const void* cache, const void* out, int B, int H,
                                        int ctx, int P) {
    if (!qkv || !cache || !out) return "null argument";
    if (!prefill_dtype_ok(dtype)) return "debug_attn_prefill: dtype is f32, bf16 or f16";
    if (H < 1) return "debug_attn_prefill_self: need at least one head";
    if (B < 1 || B > 1024 || H > 1024) return "debug_attn_prefill_self: need 1..1024 sequences and heads";
    if (ctx < 1) return "debug_attn_prefill_self: need ctx >= 1";
    if (P < 1) return "debug_attn_prefill_self: need at least one position";
    if (P > ctx) return "debug_attn_prefill_self: more positions than the cache holds";
    if ((int64_t)2 * B * H * ctx * 64 > kPrefillMaxElems) return "debug_attn_prefill_self: cache above 2^26 elements";
    if ((int64_t)B * P * 3 * H * 64 > kPrefillMaxElems) return "debug_attn_prefill_self: qkv above 2^26 elements";
    return "";
}

inline std::string prefill_cross_refusal(int dtype, const void* q, const void* k, const void* v, const void* out, int B,
                                         int B_layout, int b0, int H, int T_enc, int P, int ctx, const int32_t* kvrow,
                                         int share) {
    if (!q || !k || !v || !out) return "null argument";
    if (!prefill_dtype_ok(dtype)) return "debug_attn_prefill: dtype is f32, bf16 or f16";
    if (H < 1) return "debug_attn_prefill_cross: need at least one head";
    if (B < 1 || B > 1024 || H > 1024 || B_layout < 1 || B_layout > 1024)
        return "debug_attn_prefill_cross: need 1..1024 rows, heads and windows";
    if (T_enc < 1) return "debug_attn_prefill_cross: T_enc below 1";
    if (T_enc > kPrefillMaxElems / 64) return "debug_attn_prefill_cross: buffers above 2^26 elements";
    if (P < 1) return "debug_attn_prefill_cross: need at least one position";
    if (ctx < 1 || P > ctx) return "debug_attn_prefill_cross: more positions than ctx";
    if (share < 1 || share > 8 || B % share) return "debug_attn_prefill_cross: rows per window 1..8, dividing B";
    if (share > 1 && !kvrow) return "debug_attn_prefill_cross: shared windows need the window map";
    const int64_t layer = (int64_t)((T_enc + 31) / 32) * B_layout * H * 4096;
    if (layer > kPrefillMaxElems || (int64_t)B * P * H * 64 > kPrefillMaxElems)
        return "debug_attn_prefill_cross: buffers above 2^26 elements";
    if (b0 < 0 || (int64_t)b0 + B / share > B_layout) return "debug_attn_prefill_cross: b0 + B / share beyond B_layout";
    if (kvrow)
        for (int i = 0; i < B; ++i)
            if (kvrow[i] < 0 || (int64_t)b0 + kvrow[i] >= B_layout)
                return "debug_attn_prefill_cross: window map entry outside the layout";
    return "";
}

}  // namespace spt
