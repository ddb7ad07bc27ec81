"""The GEMM tiles and the LayerNorm kernels alone (spt_debug_gemm, spt_debug_layernorm;
csrc/capi_gemm.cpp): one gemm_nt_variant launch, or one layernorm / layernorm_pend / layernorm_pend2
launch, on numpy arrays, without an engine or a model.  Test infrastructure: tests/test_gpu_gemm.py
compares these with tests/gemm_ref.py."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .engine import TranscriptionError

DTYPES = {"f32": L.SPT_DTYPE_F32, "bf16": L.SPT_DTYPE_BF16, "f16": L.SPT_DTYPE_F16}
EPI = {"bias": 0, "gelu": 1, "gelu_pos": 2, "resid": 3, "kvsplit": 4, "swish": 5, "relu": 6, "bias_f32": 7, "partial": 8}
VARIANTS = {"auto": 0, "128x128": 1, "256x256": 2, "skinny": 3, "64x128": 4, "64x64": 5}


def _ptr(x, t=C.c_float):
    return None if x is None else x.ctypes.data_as(C.POINTER(t))


def _check(st, err):
    if st != L.SPT_OK:
        raise TranscriptionError(st, err.value.decode())


def _f32(a):
    return None if a is None else np.ascontiguousarray(a, np.float32)


def gemm(A, W, C_in, *, M, N, K, dtype="bf16", epi="bias", variant=0, batch=1, a_off=0, lda=None, sA=0, ldw=None,
         bias=None, pos=None, c_off=0, ldc=None, sC=0, alpha=1.0, ksplit=1, c_split=0, kv=(0, 0, 0),
         device: int = 0) -> np.ndarray:
    """One gemm_nt_variant launch.  A and C_in are flat f32 arrays (any shape; used flat): batch item z's
    row m starts at a_off + z * sA + m * lda and c_off + z * sC + m * ldc.  W is [N][ldw].  Returns the
    whole C buffer after the launch as a new flat f32 array (C_in is not changed)."""
    lib = L.load()
    a, w, c = _f32(A), _f32(W), _f32(C_in)
    c = None if c is None else c.ravel().copy()
    lda = K if lda is None else lda
    ldw = K if ldw is None else ldw
    ldc = N if ldc is None else ldc
    if w is not None and N >= 1 and ldw >= 1 and w.size != N * ldw:
        raise ValueError("gemm: W is [N][ldw]")
    b, p = _f32(bias), _f32(pos)
    if b is not None and b.size != N:
        raise ValueError("gemm: bias is [N]")
    if p is not None and p.size != M * N:
        raise ValueError("gemm: pos is [M][N]")
    e = EPI[epi] if isinstance(epi, str) else int(epi)
    v = VARIANTS[variant] if isinstance(variant, str) else int(variant)
    err = C.create_string_buffer(512)
    st = lib.spt_debug_gemm(device, DTYPES[dtype] if isinstance(dtype, str) else int(dtype), e, v, batch, M, N, K,
                            _ptr(a), 0 if a is None else a.size, a_off, lda, sA, _ptr(w), ldw, _ptr(b), _ptr(p), _ptr(c),
                            0 if c is None else c.size, c_off, ldc, sC, float(alpha), ksplit, c_split, int(kv[0]),
                            int(kv[1]), int(kv[2]), err, 512)
    _check(st, err)
    return c


def _ln(mode, x, w, b, dtype, *, slab=None, ks=1, slab_stride=0, pbias=None, alpha=1.0, w2=None, b2=None, write_x=True,
        M=None, d=None, device=0):
    lib = L.load()
    xx = np.array(x, np.float32, order="C")  # in and out: a copy
    if M is None:
        M, d = xx.shape
    s = _f32(slab)
    y = np.zeros((max(M, 1), max(d, 1)), np.float32)
    y2 = np.zeros_like(y)
    err = C.create_string_buffer(512)
    st = lib.spt_debug_layernorm(device, DTYPES[dtype] if isinstance(dtype, str) else int(dtype), mode, _ptr(xx), M, d,
                                 _ptr(s), 0 if s is None else s.size, ks, slab_stride, _ptr(_f32(pbias)), float(alpha),
                                 _ptr(_f32(w)), _ptr(_f32(b)), _ptr(_f32(w2)), _ptr(_f32(b2)), int(bool(write_x)), _ptr(y),
                                 _ptr(y2), err, 512)
    _check(st, err)
    return xx, y, y2


def layernorm(x, w, b, dtype="f32", **kw) -> np.ndarray:
    """One layernorm launch: x [M][d] -> y [M][d] (stored as dtype, returned as f32)."""
    return _ln(L.SPT_LN_PLAIN, x, w, b, dtype, **kw)[1]


def layernorm_pend(x, slab, ks, slab_stride, pbias, alpha, w, b, dtype="f32", write_x=True, **kw):
    """One layernorm_pend launch; the slabs are a flat array, slab q's row m at q * slab_stride + m * d.
    -> (x after the launch, y)."""
    return _ln(L.SPT_LN_PEND, x, w, b, dtype, slab=slab, ks=ks, slab_stride=slab_stride, pbias=pbias, alpha=alpha,
               write_x=write_x, **kw)[:2]


def layernorm_pend2(x, slab, ks, slab_stride, pbias, alpha, w, b, w2, b2, dtype="f32", **kw):
    """One layernorm_pend2 launch -> (y f32, y2 stored as dtype)."""
    return _ln(L.SPT_LN_PEND2, x, w, b, dtype, slab=slab, ks=ks, slab_stride=slab_stride, pbias=pbias, alpha=alpha,
               w2=w2, b2=b2, **kw)[1:]
