// ggml_qpack.h -- the device layout of a decoder matrix that stays quantised in HBM
// (SPT_MODEL_QUANT_RESIDENT), its host packer, and the one element read every
// consumer outside the GEMV shares (embedding rows, the checksum, the test hook's unpack).
//
// A ggml file stores a [N][K] matrix as rows of 32-element blocks of 18..24 unaligned bytes.  The
// decoder GEMV (dec_gemv.h) walks K in super-steps of 128 elements = 4 blocks; in MFMA step i the
// lane group fq of a weight row takes elements [32 i + 8 fq, + 8): block i, positions 8 fq .. 8 fq + 7.
// Position j < 16 of a block is the low nibble of qs[j], j + 16 the high nibble of the same byte, so
// lane groups fq and fq + 2 want the same 8 bytes qs[8 (fq & 1) ..] and byte fq of qh.
//
// The packed matrix is [N][K / 128] records; one record holds the 4 blocks of a row's super-step as
// planes, every plane at a 16-byte-aligned record and an aligned offset:
//   [ 0, 64)  nibbles [h][i][8]: qs[8 h .. 8 h + 8) of block i   (a lane: 32 contiguous bytes at 32 h)
//   q4_1 (80 B):  [64, 72) d[i] f16   [72, 80) m[i] f16
//   q5_0 (96 B):  [64, 80) qh bytes [fq][i] (a lane: one dword at 64 + 4 fq)   [80, 88) d[i]   [88, 96) zero
//   q5_1 (96 B):  [64, 80) qh bytes [fq][i]                                  [80, 88) d[i]   [88, 96) m[i]
// Every bit of the file's blocks is kept (lossless), nothing is recomputed.  Bytes per weight: q4_1
// 0.625 (the file's), q5_0 0.75 (1.09 x the file's 0.6875: the pad keeps records 16-byte aligned),
// q5_1 0.75 (the file's).
#pragma once
#include "ggml_quant.h"

namespace spt {

struct QPackGeom {
    int rec;       // bytes per record
    int off_qh;    // fifth-bit plane (q4_1: the d plane, read and ignored)
    int off_d;     // scales
    int off_m;     // minima (q5_0: the zero pad)
    int q5;        // 0x10 if the type has a fifth bit, else 0
    int sub;       // the offset taken from the code: 16 (q5_0) or 0
    int has_m;
};

// false for a type with no resident layout
__host__ __device__ inline bool qpack_geom(int type, QPackGeom* g) {
    switch (type) {
        case GQ_Q4_1: *g = QPackGeom{80, 64, 64, 72, 0, 0, 1}; return true;
        case GQ_Q5_0: *g = QPackGeom{96, 64, 80, 88, 0x10, 16, 0}; return true;
        case GQ_Q5_1: *g = QPackGeom{96, 64, 80, 88, 0x10, 0, 1}; return true;
        default: *g = QPackGeom{0, 0, 0, 0, 0, 0, 0}; return false;
    }
}

constexpr int QPACK_KS = 128;  // elements per record: the 16-bit GEMV's super-step

// bytes of a packed [N][K] matrix; 0 for an unsupported type or K not a multiple of 128
inline int64_t qpack_bytes(int type, int64_t N, int64_t K) {
    QPackGeom g;
    if (!qpack_geom(type, &g) || N < 0 || K < 0 || K % QPACK_KS) return 0;
    return N * (K / QPACK_KS) * g.rec;
}

// element e (0..127) of a record, as ggml_dequant_block gives it (f32)
__host__ __device__ inline float qpack_elem(const QPackGeom& g, const uint8_t* rec, int e) {
    const int i = e >> 5, j = e & 31, fq = j >> 3, b = j & 7;
    const uint8_t byte = rec[32 * (fq & 1) + 8 * i + b];
    int x = fq < 2 ? byte & 0xf : byte >> 4;
    if (g.q5) x |= ((rec[g.off_qh + 4 * fq + i] >> b) & 1) << 4;
    const float d = gq_half(rec + g.off_d + 2 * i);
    const float m = g.has_m ? gq_half(rec + g.off_m + 2 * i) : 0.0f;
    return gq_dequant_elem(x, g.sub, d, g.has_m != 0, m);
}

// element k of row n of a packed [N][K] matrix
__host__ __device__ inline float qpack_at(const QPackGeom& g, const uint8_t* w, int64_t K, int64_t n, int64_t k) {
    return qpack_elem(g, w + (n * (K / QPACK_KS) + k / QPACK_KS) * g.rec, (int)(k % QPACK_KS));
}

// ggml blocks [N][K / 32] of `type` (src_bytes of them) -> records at dst (qpack_bytes of them).
// false: unsupported type, K not a multiple of 128, or a source shorter than the tensor.
inline bool qpack_rows(int type, const uint8_t* src, size_t src_bytes, int64_t N, int64_t K, uint8_t* dst) {
    QPackGeom g;
    int blck, bb;
    ggml_block_geom(type, &blck, &bb);
    if (!qpack_geom(type, &g) || N < 0 || K < 0 || K % QPACK_KS || !src || !dst) return false;
    const int64_t nrec = N * (K / QPACK_KS);
    if (nrec && (uint64_t)nrec > src_bytes / (size_t)(4 * bb)) return false;
    const int hdr = g.has_m ? 4 : 2;  // d (, m) ahead of qh / qs in the file's block
    for (int64_t r = 0; r < nrec; ++r) {
        uint8_t* o = dst + r * g.rec;
        memset(o, 0, (size_t)g.rec);
        for (int i = 0; i < 4; ++i) {
            const uint8_t* p = src + (r * 4 + i) * bb;
            const uint8_t* qs = p + hdr + (g.q5 ? 4 : 0);
            for (int h = 0; h < 2; ++h) memcpy(o + 32 * h + 8 * i, qs + 8 * h, 8);
            if (g.q5)
                for (int fq = 0; fq < 4; ++fq) o[g.off_qh + 4 * fq + i] = p[hdr + fq];
            memcpy(o + g.off_d + 2 * i, p, 2);
            if (g.has_m) memcpy(o + g.off_m + 2 * i, p + 2, 2);
        }
    }
    return true;
}

// a packed [N][K] matrix dequantised to f32 [N][K] (host: the test hook, the checksum's reference)
inline bool qpack_unpack_f32(int type, const uint8_t* w, int64_t N, int64_t K, float* out) {
    QPackGeom g;
    if (!qpack_geom(type, &g) || K % QPACK_KS) return false;
    for (int64_t n = 0; n < N; ++n)
        for (int64_t k = 0; k < K; ++k) out[n * K + k] = qpack_at(g, w, K, n, k);
    return true;
}

#if defined(__HIPCC__)
}  // namespace spt
#include "common.h"
namespace spt {
// Element i of row `tok` of the token embedding [V][d], as the decoder reads it when it embeds a token:
// the one row read of embed_kernel, finalize_kernel and finalize_ts_kernel.  QE = false: the engine
// dtype's rows (the instructions those kernels had before the format existed); QE = true: a packed
// matrix of ggml type q, the value rounded to T as the loader's dequantisation would have stored it.
template <typename T, bool QE>
__device__ __forceinline__ float emb_row_read(const void* emb, int q, int d, int tok, int i) {
    if constexpr (QE) {
        QPackGeom g;
        qpack_geom(q, &g);
        return to_f<T>(from_f<T>(qpack_at(g, (const uint8_t*)emb, d, tok, i)));
    } else {
        return to_f<T>(((const T*)emb)[(size_t)tok * d + i]);
    }
}
#endif

}  // namespace spt
