"""The fp8 cross K/V kernels alone (spt_debug_attn_cross_quant, csrc/capi_f8kv.cpp) and the cache read of a
context (spt_debug_cross_kv), on numpy arrays.  Test infrastructure: tests/test_f8kv_ref.py and
tests/test_gpu_f8kv_attn.py compare these with tests/f8kv_ref.py."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _lib as L
from .attn_debug import DTYPES, MODES, _ptr
from .engine import TranscriptionError


@dataclass
class CrossF8:
    status: int                 # SPT_OK, or SPT_ERR_DEVICE with the host quantiser's arrays below
    message: str
    kq: np.ndarray              # [B_layout][H][T_enc][64] dequantised K rows (f32(code) * scale)
    vq: np.ndarray
    k_scale: np.ndarray         # [B_layout][H][T_enc]
    v_scale: np.ndarray
    out: Optional[np.ndarray]   # [B*Tq][H*64], or None
    part: Optional[np.ndarray]  # [B*Tq][H][8][66] = {o[64], m, l}, or None


def cross_f8(q, k, v, *, Tq=1, mode="8wave", b0=0, B=None, kvrow=None, share=1, pad_value=0.0, dtype="bf16",
             device: int = 0, allow_no_device: bool = False) -> CrossF8:
    """Quantise plain k, v [B_layout][H][T_enc][64] (rounded to dtype first) per key row and run one
    cross-attention launch over the records (mode: attn_debug.MODES).  Without a device and with
    allow_no_device the host quantiser's arrays come back with status SPT_ERR_DEVICE; every other
    failure raises TranscriptionError."""
    lib = L.load()
    kk = np.ascontiguousarray(k, np.float32)
    vv = np.ascontiguousarray(v, np.float32)
    B_layout, H, T_enc, hd = kk.shape
    if hd != 64 or vv.shape != kk.shape:
        raise ValueError("cross_f8: k and v are [B_layout][H][T_enc][64]")
    x = np.ascontiguousarray(q, np.float32)
    if B is None:
        B = x.size // (max(Tq, 1) * H * 64)
    if 1 <= Tq <= 4 and x.size != B * Tq * H * 64:
        raise ValueError("cross_f8: q is [B*Tq][H*64]")
    km = None if kvrow is None else np.ascontiguousarray(kvrow, np.int32)
    if km is not None and km.shape != (B,):
        raise ValueError("cross_f8: one window per row")
    m = MODES[mode] if isinstance(mode, str) else int(mode)
    R = max(B * max(Tq, 1), 1)
    want_part = m in (L.SPT_ATTN_CROSS_VW, L.SPT_ATTN_CROSS_VW_PQ)
    kq = np.zeros(kk.shape, np.float32)
    vq = np.zeros(kk.shape, np.float32)
    ks = np.zeros(kk.shape[:3], np.float32)
    vs = np.zeros(kk.shape[:3], np.float32)
    out = np.zeros((R, H * 64), np.float32)
    part = np.zeros((R, H, 8, 66), np.float32)
    err = C.create_string_buffer(512)
    st = lib.spt_debug_attn_cross_quant(device, DTYPES[dtype], m, _ptr(x), _ptr(kk), _ptr(vv), float(pad_value), B, B_layout,
                                     b0, H, T_enc, Tq, _ptr(km, C.c_int32), share, _ptr(kq), _ptr(vq), _ptr(ks), _ptr(vs),
                                     _ptr(out), _ptr(part), err, 512)
    if st == L.SPT_ERR_DEVICE and allow_no_device:
        return CrossF8(st, err.value.decode(), kq, vq, ks, vs, None, None)
    if st != L.SPT_OK:
        raise TranscriptionError(st, err.value.decode())
    return CrossF8(st, "", kq, vq, ks, vs, None if want_part else out, part if want_part else None)


def cross_kv(engine, layer: int, window: int):
    """(k, v), each [n_head][n_audio_ctx][64] f32: one layer and window of the cross K/V cache the
    engine's last call left, an fp8 cache dequantised on the device (spt_debug_cross_kv)."""
    info = engine.info()
    shape = (info["n_head"], info["n_audio_ctx"], 64)
    k = np.zeros(shape, np.float32)
    v = np.zeros(shape, np.float32)
    engine._check(engine._lib.spt_debug_cross_kv(engine._ctx, layer, window, _ptr(k), _ptr(v)))
    return k, v
