"""The block prefill's attention kernels alone (spt_debug_attn_prefill_self / _cross, csrc/capi_attn.cpp;
DESIGN 2g / 4.7) on numpy arrays, without an engine or a model.  Test infrastructure:
tests/test_gpu_prefill_attn.py compares these with tests/attn_ref.py."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .engine import TranscriptionError

DTYPES = {"f32": L.SPT_DTYPE_F32, "bf16": L.SPT_DTYPE_BF16, "f16": L.SPT_DTYPE_F16}


def _ptr(x, t=C.c_float):
    return None if x is None else x.ctypes.data_as(C.POINTER(t))


def _check(st, err):
    if st != L.SPT_OK:
        raise TranscriptionError(st, err.value.decode())


def _f32(a):
    return None if a is None else np.ascontiguousarray(a, np.float32)


def self_attn(qkv, cache, P, *, B=None, H=None, ctx=None, dtype="f32", device: int = 0):
    """One dec_prefill_self_attn launch: qkv [B*P][3*H*64] (q | k | v), cache [2][B][H][ctx][64] as given
    -> (out [B*P][H*64], the cache after the launch), both f32.  B, H and ctx default to the cache's; a
    dtype that is no key of DTYPES is passed through as a number (the refusal tests)."""
    lib = L.load()
    c = _f32(cache)
    if c is not None:
        c = c.copy()
        if B is None:
            B = c.shape[1]
        if H is None:
            H = c.shape[2]
        if ctx is None:
            ctx = c.shape[3]
    x = _f32(qkv)
    out = np.zeros((max(int(B) * max(int(P), 1), 1), max(int(H), 1) * 64), np.float32)
    err = C.create_string_buffer(512)
    st = lib.spt_debug_attn_prefill_self(device, DTYPES.get(dtype, dtype), _ptr(x), _ptr(c), int(B), int(H), int(ctx), int(P),
                                         _ptr(out), err, 512)
    _check(st, err)
    return out, c


def cross(q, k, v, P, *, ctx=448, b0=0, B=None, B_layout=None, H=None, T_enc=None, kvrow=None, share=1, pad_value=0.0,
          dtype="f32", device: int = 0, out=True):
    """One dec_prefill_cross_attn launch on q [B*P][H*64] and plain k, v [B_layout][H][T_enc][64] (laid out
    as one layer of the cross K/V cache, the padded keys holding pad_value) -> out [B*P][H*64] (f32).
    out=False passes a null output (the refusal tests)."""
    lib = L.load()
    kk, vv, x = _f32(k), _f32(v), _f32(q)
    if kk is not None:
        if B_layout is None:
            B_layout = kk.shape[0]
        if H is None:
            H = kk.shape[1]
        if T_enc is None:
            T_enc = kk.shape[2]
    if B is None:
        B = x.size // (max(int(P), 1) * int(H) * 64)
    km = None if kvrow is None else np.ascontiguousarray(kvrow, np.int32)
    o = np.zeros((max(int(B) * max(int(P), 1), 1), max(int(H), 1) * 64), np.float32) if out else None
    err = C.create_string_buffer(512)
    st = lib.spt_debug_attn_prefill_cross(device, DTYPES.get(dtype, dtype), _ptr(x), _ptr(kk), _ptr(vv), float(pad_value),
                                          int(B), int(B_layout), int(b0), int(H), int(T_enc), int(P), int(ctx),
                                          _ptr(km, C.c_int32), int(share), _ptr(o), err, 512)
    _check(st, err)
    return o
