"""The Whisper attention kernels alone (spt_debug_attn_*, csrc/capi_attn.cpp): the encoder attention,
the decoder self-attention and the cross-attention variants on numpy arrays, without an engine or a
model.  Test infrastructure: tests/test_gpu_attn.py compares these with tests/attn_ref.py."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .engine import TranscriptionError

DTYPES = {"f32": L.SPT_DTYPE_F32, "bf16": L.SPT_DTYPE_BF16, "f16": L.SPT_DTYPE_F16}
MODES = {"8wave": L.SPT_ATTN_CROSS_8WAVE, "vw": L.SPT_ATTN_CROSS_VW, "vw_pq": L.SPT_ATTN_CROSS_VW_PQ,
         "vw_merge": L.SPT_ATTN_CROSS_VW_MERGE, "vw_pq_merge": L.SPT_ATTN_CROSS_VW_PQ_MERGE}


def _ptr(x, t=C.c_float):
    return None if x is None else x.ctypes.data_as(C.POINTER(t))


def _check(st, err):
    if st != L.SPT_OK:
        raise TranscriptionError(st, err.value.decode())


def enc(qkv, B, T, H, dtype="f32", device: int = 0) -> np.ndarray:
    """One enc_attention launch: qkv [B*T][3*H*64] -> out [B*T][H*64] (f32; NaN where nothing wrote)."""
    lib = L.load()
    x = None if qkv is None else np.ascontiguousarray(qkv, np.float32)
    if x is not None and x.size != B * T * 3 * H * 64:
        raise ValueError("enc: qkv is [B*T][3*H*64]")
    out = np.zeros((max(B * T, 1), max(H, 1) * 64), np.float32)
    err = C.create_string_buffer(512)
    _check(lib.spt_debug_attn_enc(device, DTYPES[dtype], _ptr(x), B, T, H, _ptr(out), err, 512), err)
    return out


def self_attn(q, cache, pos0, Tq, dtype="f32", device: int = 0) -> np.ndarray:
    """One dec_self_attn launch: q [B*Tq][H*64], cache [2][B][H][ctx][64] (used whole, as given)
    -> out [B*Tq][H*64]."""
    lib = L.load()
    c = np.ascontiguousarray(cache, np.float32)
    two, B, H, ctx, hd = c.shape
    if two != 2 or hd != 64:
        raise ValueError("self_attn: cache is [2][B][H][ctx][64]")
    x = np.ascontiguousarray(q, np.float32)
    if x.size != B * max(Tq, 0) * H * 64 and 1 <= Tq <= 4:
        raise ValueError("self_attn: q is [B*Tq][H*64]")
    out = np.zeros((B * max(Tq, 1), H * 64), np.float32)
    err = C.create_string_buffer(512)
    _check(lib.spt_debug_attn_self(device, DTYPES[dtype], _ptr(x), _ptr(c), B, H, ctx, Tq, pos0, _ptr(out), err, 512),
           err)
    return out


def cross(q, k, v, *, Tq=1, mode="8wave", splits=1, b0=0, B=None, kvrow=None, share=1, pad_value=0.0, dtype="f32",
          device: int = 0) -> np.ndarray:
    """One cross-attention launch (mode: MODES) on q [B*Tq][H*64] and plain k, v [B_layout][H][T_enc][64].
    -> out [B*Tq][H*64], or the partials [B*Tq][H][S][66] = {o[64], m, l} (S = splits for the 8-wave
    kernel with splits > 1, 8 for the vw modes without the merge launch)."""
    lib = L.load()
    kk = np.ascontiguousarray(k, np.float32)
    vv = np.ascontiguousarray(v, np.float32)
    B_layout, H, T_enc, hd = kk.shape
    if hd != 64 or vv.shape != kk.shape:
        raise ValueError("cross: k and v are [B_layout][H][T_enc][64]")
    x = np.ascontiguousarray(q, np.float32)
    if B is None:
        B = x.size // (max(Tq, 1) * H * 64)
    if 1 <= Tq <= 4 and x.size != B * Tq * H * 64:
        raise ValueError("cross: q is [B*Tq][H*64]")
    km = None if kvrow is None else np.ascontiguousarray(kvrow, np.int32)
    if km is not None and km.shape != (B,):
        raise ValueError("cross: one window per row")
    m = MODES[mode] if isinstance(mode, str) else int(mode)
    R = max(B * max(Tq, 1), 1)
    vw = m >= L.SPT_ATTN_CROSS_VW
    want_part = (vw and m not in (L.SPT_ATTN_CROSS_VW_MERGE, L.SPT_ATTN_CROSS_VW_PQ_MERGE)) or (not vw and splits > 1)
    out = np.zeros((R, H * 64), np.float32)
    part = np.zeros((R, H, 8 if vw else max(min(splits, 4), 1), 66), np.float32)
    err = C.create_string_buffer(512)
    st = lib.spt_debug_attn_cross(device, DTYPES[dtype], m, _ptr(x), _ptr(kk), _ptr(vv), float(pad_value), B, B_layout,
                                  b0, H, T_enc, Tq, splits, _ptr(km, C.c_int32), share, _ptr(out), _ptr(part), err, 512)
    _check(st, err)
    return part if want_part else out


def xq_fused(x, ln_w, ln_b, wq, bias, k, v, *, lds=0, touch=2, pad_value=0.0, dtype="bf16", H=None, device: int = 0):
    """One fused cross-Q + cross-attention launch (dec_xq_fused): f32 residual rows x [B][1280], LN2
    (ln_w, ln_b [1280]), the cross-Q projection (wq [1280][1280], bias [1280]) and plain k, v
    [B][20][T_enc][64], row b on window b.  lds / touch: key blocks per attention wave staged in LDS /
    touched before q arrives.  -> (q [B][1280], out [B][1280]) as f32."""
    lib = L.load()
    f = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)
    xx, kk, vv = f(x), f(k), f(v)
    B = xx.shape[0] if xx is not None else kk.shape[0]
    if H is None:
        H = kk.shape[1]
    T_enc = kk.shape[2]
    if kk.shape != (B, H, T_enc, 64) or (vv is not None and vv.shape != kk.shape):
        raise ValueError("xq_fused: k and v are [B][H][T_enc][64]")
    q = np.zeros((max(B, 1), 1280), np.float32)
    out = np.zeros((max(B, 1), 1280), np.float32)
    err = C.create_string_buffer(512)
    st = lib.spt_debug_xq_fused(device, DTYPES[dtype], _ptr(xx), _ptr(f(ln_w)), _ptr(f(ln_b)), _ptr(f(wq)), _ptr(f(bias)),
                                _ptr(kk), _ptr(vv), float(pad_value), B, H, T_enc, int(lds), int(touch), _ptr(q), _ptr(out),
                                err, 512)
    _check(st, err)
    return q, out
