// k_dec_q.hip -- the decoder GEMV kernels of k_dec.hip over a weight matrix that stays in its packed
// ggml blocks (SPT_MODEL_QUANT_RESIDENT; layout: ggml_qpack.h) and is dequantised in registers.  One
// kernel per (dtype, mode, A source, geometry) of the plain set -- the block type is a run-time field
// of GemvArgs -- for the two 16-bit engine dtypes, in a translation unit of its own so that it compiles
// beside k_dec.o.  Everything but the weight fetch is dec_gemv.h's one text (bitwise the plain result).
#define SPT_GEMV_QW 1
#include "dec_gemv.h"

namespace spt {

void gemv_q_prepare(int dtype) {
    if (dtype == DT_BF16) gemv_attr_modes<bf16>();
    else if (dtype == DT_F16) gemv_attr_modes<f16>();
    else throw std::runtime_error("gemv: resident quantised weights need a bf16 or f16 engine");
}

void gemv_q(int dtype, int mode, int code, const GemvArgs& a, hipStream_t st) {
    if (dtype != DT_BF16 && dtype != DT_F16)
        throw std::runtime_error("gemv: resident quantised weights need a bf16 or f16 engine");
#define SPT_GV(M, S)                                                      \
    if (mode == M && code == S) {                                         \
        if (dtype == DT_BF16) gemv_launch<bf16, M, S>(a, st);             \
        else gemv_launch<f16, M, S>(a, st);                               \
        return;                                                           \
    }
    SPT_GV_PAIRS(SPT_GV)
#undef SPT_GV
    throw std::runtime_error("gemv: unsupported mode / A source");
}

}  // namespace spt
