"""The token-alignment kernels alone (spt_debug_align_*, csrc/capi_align.cpp): the alignment heads'
attention probabilities, the normalise + median + head mean, and the dynamic time warping on numpy
arrays, without an engine or a model, plus the host-only word grouping.  Test infrastructure:
tests/test_gpu_align.py compares these with tests/align_ref.py."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .attn_debug import DTYPES, _check, _ptr


def _i32(x, n=None):
    a = np.ascontiguousarray(x, np.int32).reshape(-1)
    if n is not None and a.size == 1 and n > 1:
        a = np.repeat(a, n)
    return a


def qk(q, k, heads, M, *, Tq=1, pos0=0, kvrow=None, N_cap=None, M_cap=None, pad_value=0.0, dtype="f32",
       device: int = 0) -> np.ndarray:
    """One align_qk launch: q [B*Tq][H*64], plain k [B_layout][H][T_enc][64], heads a list of heads, M
    the keys kept (an int or one per sequence) -> p [B][len(heads)][N_cap][M_cap] (NaN where nothing
    wrote); rows pos0 .. pos0 + Tq - 1 are the launch's."""
    lib = L.load()
    kk = np.ascontiguousarray(k, np.float32)
    B_layout, H, T_enc, hd = kk.shape
    if hd != 64:
        raise ValueError("qk: k is [B_layout][H][T_enc][64]")
    x = np.ascontiguousarray(q, np.float32)
    B = x.size // (max(Tq, 1) * H * 64)
    if 1 <= Tq <= 4 and x.size != B * Tq * H * 64:
        raise ValueError("qk: q is [B*Tq][H*64]")
    hs = _i32(heads)
    Ms = _i32(M, B)
    km = None if kvrow is None else _i32(kvrow)
    if Ms.shape != (B,) or (km is not None and km.shape != (B,)):
        raise ValueError("qk: one M and one window per sequence")
    N_cap = pos0 + Tq if N_cap is None else N_cap
    M_cap = int(Ms.max()) if M_cap is None else M_cap
    p = np.zeros((B, hs.size, max(N_cap, 1), max(M_cap, 1)), np.float32)
    err = C.create_string_buffer(512)
    st = lib.spt_debug_align_qk(device, DTYPES[dtype], _ptr(x), _ptr(kk), float(pad_value), B, B_layout, H, T_enc, Tq,
                                pos0, _ptr(km, C.c_int32), _ptr(hs, C.c_int32), hs.size, _ptr(Ms, C.c_int32), N_cap,
                                M_cap, _ptr(p), err, 512)
    _check(st, err)
    return p


def norm(p, N=None, M=None, device: int = 0):
    """One align_norm: p [B][A][N_cap][M_cap], N / M the rows / keys in use (default: all)
    -> (stat [B][A][2][M_cap] = mean, std; m [B][N_cap][M_cap])."""
    lib = L.load()
    x = np.ascontiguousarray(p, np.float32)
    B, A, N_cap, M_cap = x.shape
    Ns = _i32(N_cap if N is None else N, B)
    Ms = _i32(M_cap if M is None else M, B)
    stat = np.zeros((B, A, 2, M_cap), np.float32)
    m = np.zeros((B, N_cap, M_cap), np.float32)
    err = C.create_string_buffer(512)
    st = lib.spt_debug_align_norm(device, _ptr(x), B, A, N_cap, M_cap, _ptr(Ns, C.c_int32), _ptr(Ms, C.c_int32),
                                  _ptr(stat), _ptr(m), err, 512)
    _check(st, err)
    return stat, m


def dtw(m, N=None, M=None, device: int = 0):
    """One align_dtw on -m: m [B][N_cap][M_cap] (the keys are padded here to a multiple of 8), N / M
    the rows / keys in use (default: all) -> per sequence (path [len][2] of (row, key), jump [N], len)."""
    lib = L.load()
    x = np.ascontiguousarray(m, np.float32)
    B, N_cap, M0 = x.shape
    M_cap = max((M0 + 7) // 8 * 8, 8)
    if M_cap != M0:
        x = np.concatenate([x, np.full((B, N_cap, M_cap - M0), np.nan, np.float32)], -1)
    Ns = _i32(N_cap if N is None else N, B)
    Ms = _i32(M0 if M is None else M, B)
    jump = np.zeros((B, N_cap), np.int32)
    ln = np.zeros(B, np.int32)
    path = np.zeros((B, N_cap + M_cap, 2), np.int32)
    err = C.create_string_buffer(512)
    st = lib.spt_debug_align_dtw(device, _ptr(np.ascontiguousarray(x)), B, N_cap, M_cap, _ptr(Ns, C.c_int32),
                                 _ptr(Ms, C.c_int32), _ptr(jump, C.c_int32), _ptr(ln, C.c_int32),
                                 _ptr(path, C.c_int32), err, 512)
    _check(st, err)
    return [(path[b, :ln[b]].copy(), jump[b, :Ns[b]].copy(), int(ln[b])) for b in range(B)]


def words(pieces, t0, t1, p=None):
    """Host only: aligned tokens (piece bytes, start, end, probability) grouped into words
    -> [(i0, n_tokens, t0, t1, p)]."""
    lib = L.load()
    n = len(pieces)
    raw = [bytes(x) for x in pieces]
    arr = (C.c_char_p * max(n, 1))(*raw)
    lens = np.array([len(x) for x in raw] or [0], np.int32)
    a0 = np.ascontiguousarray(list(t0) or [0], np.int64)
    a1 = np.ascontiguousarray(list(t1) or [0], np.int64)
    pp = None if p is None else np.ascontiguousarray(list(p) or [0], np.float32)
    wi, wn = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
    w0, w1 = np.zeros(max(n, 1), np.int64), np.zeros(max(n, 1), np.int64)
    wp = np.zeros(max(n, 1), np.float32)
    nw = C.c_int32(0)
    err = C.create_string_buffer(512)
    st = lib.spt_debug_align_words(arr, _ptr(lens, C.c_int32), _ptr(a0, C.c_int64), _ptr(a1, C.c_int64), _ptr(pp), n,
                                   _ptr(wi, C.c_int32), _ptr(wn, C.c_int32), _ptr(w0, C.c_int64), _ptr(w1, C.c_int64),
                                   _ptr(wp), C.byref(nw), err, 512)
    _check(st, err)
    return [(int(wi[i]), int(wn[i]), int(w0[i]), int(w1[i]), float(wp[i])) for i in range(nw.value)]
