"""The decoder GEMV alone over one quantised matrix (spt_debug_qgemv, csrc/capi_qgemv.cpp): one launch on
the weights expanded by the loader's dequantisation and one on the matrix packed in its ggml blocks
(SPT_MODEL_QUANT_RESIDENT's layout), on numpy arrays, without an engine or a model.  Test
infrastructure: tests/test_gpu_qgemv.py and tests/test_qresident_ref.py."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _lib as L
from .engine import TranscriptionError

DTYPES = {"f32": L.SPT_DTYPE_F32, "bf16": L.SPT_DTYPE_BF16, "f16": L.SPT_DTYPE_F16}
MODES = {"bias": L.SPT_GV_BIAS, "bias_gelu": L.SPT_GV_BIAS_GELU, "partial": L.SPT_GV_PARTIAL,
         "qkv_cache": L.SPT_GV_QKV_CACHE, "logits": L.SPT_GV_LOGITS, "bias_resid": L.SPT_GV_BIAS_RESID}
A_SRC = {"direct": L.SPT_QGEMV_A_DIRECT, "ln": L.SPT_QGEMV_A_LN}


@dataclass
class QGemvResult:
    status: int                  # SPT_OK, or SPT_ERR_DEVICE when no device ran the launches
    plain: np.ndarray            # f32 [R][N] ([ksplit][R][N] for "partial"): the expanded weights' launch
    packed: np.ndarray           # the same from the packed matrix
    top_plain: Optional[np.ndarray]   # "logits": uint32 [R][ceil(N / 16)][4] top-2 partials as stored
    top_packed: Optional[np.ndarray]
    unpacked: Optional[np.ndarray]    # f32 [N][K]: the packed matrix dequantised back on the host


def _ptr(x):
    return None if x is None else x.ctypes.data_as(C.POINTER(C.c_float))


def _f32(x):
    return None if x is None else np.ascontiguousarray(x, np.float32)


def qgemv(blocks: bytes, ggml_type: int, N: int, K: int, act, *, mode="bias", a_src="ln", ln_w=None, ln_b=None,
          bias=None, resid=None, ksplit: int = 1, dtype="bf16", device: int = 0, need_device: bool = True,
          R: Optional[int] = None, want_unpacked: bool = True) -> QGemvResult:
    """blocks: the ggml blocks of W [N][K / 32] as the file holds them; act f32 [R][K].  With
    need_device=False a valid call that finds no device returns status SPT_ERR_DEVICE and the host
    side's `unpacked` instead of raising."""
    lib = L.load()
    a = _f32(act)
    if R is None:
        R = 0 if a is None else a.shape[0]
    m = MODES[mode] if isinstance(mode, str) else int(mode)
    s = A_SRC[a_src] if isinstance(a_src, str) else int(a_src)
    ks = max(int(ksplit), 1)
    rows, cols = max(R, 1), max(N, 1)
    shape = (ks, rows, cols) if m == L.SPT_GV_PARTIAL else (rows, cols)
    plain = np.full(shape, np.nan, np.float32)
    packed = np.full(shape, np.nan, np.float32)
    logits = m == L.SPT_GV_LOGITS
    tp = np.zeros((rows, (cols + 15) // 16, 4), np.float32) if logits else None
    tq = np.zeros((rows, (cols + 15) // 16, 4), np.float32) if logits else None
    unp = np.full((cols, max(K, 1)), np.nan, np.float32) if want_unpacked else None
    lw, lb, bi, rs = _f32(ln_w), _f32(ln_b), _f32(bias), _f32(resid)
    buf = None if blocks is None else (C.c_char * max(len(blocks), 1)).from_buffer_copy(bytes(blocks) or b"\0")
    err = C.create_string_buffer(512)
    st = lib.spt_debug_qgemv(device, DTYPES[dtype] if isinstance(dtype, str) else int(dtype), int(ggml_type),
                             None if buf is None else C.cast(buf, C.c_void_p), 0 if blocks is None else len(blocks),
                             N, K, _ptr(a), R, _ptr(lw), _ptr(lb), _ptr(bi), _ptr(rs), m, s, int(ksplit),
                             _ptr(plain), _ptr(packed), _ptr(tp), _ptr(tq), _ptr(unp), err, 512)
    if st != L.SPT_OK and not (st == L.SPT_ERR_DEVICE and not need_device):
        raise TranscriptionError(st, err.value.decode())
    return QGemvResult(st, plain, packed, None if tp is None else tp.view(np.uint32),
                       None if tq is None else tq.view(np.uint32), unp)
