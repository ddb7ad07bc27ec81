"""The decoder GEMV and the small kernels of the decode step alone (spt_debug_gemv, spt_debug_dec_step of
csrc/capi_gemv.cpp) on numpy arrays, without an engine or a model.  Test infrastructure:
tests/test_gpu_gemv.py and tests/test_gemv_ref.py.

Every array a kernel writes starts with each byte 0xFF on the device and comes back whole: what the launch
did not write reads as NaN (f32), as the 16-bit NaN 0xFFFF converted to f32, or as -1 (int32)."""
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
A_SRC = {"direct": L.SPT_GEMV_A_DIRECT, "ln": L.SPT_GEMV_A_LN, "attn": L.SPT_GEMV_A_ATTN}
OPS = {"embed": L.SPT_DEC_STEP_EMBED, "finalize": L.SPT_DEC_STEP_FINALIZE, "advance": L.SPT_DEC_STEP_ADVANCE,
       "reset": L.SPT_DEC_STEP_RESET}
PLAN_FIELDS = ("nwv", "ct", "maxj", "exact", "rg", "lds_bytes", "grid_x", "grid_y")


def _f32(x):
    return None if x is None else np.ascontiguousarray(x, np.float32)


def _i32(x):
    return None if x is None else np.ascontiguousarray(x, np.int32)


def _fp(x):
    return None if x is None else x.ctypes.data_as(C.POINTER(C.c_float))


def _ip(x):
    return None if x is None else x.ctypes.data_as(C.POINTER(C.c_int32))


def _code(table, v):
    return table[v] if isinstance(v, str) else int(v)


@dataclass
class GemvResult:
    status: int                       # SPT_OK, or SPT_ERR_DEVICE when no device ran the launch
    plan: dict                        # what gemv_plan() chose (PLAN_FIELDS)
    C: np.ndarray                     # f32 [c_count], whole
    x_out: Optional[np.ndarray]       # f32 [a_count], whole (A_LN with x_out)
    cache: Optional[np.ndarray]       # f32 [2][B][H][ctx][64], whole (qkv_cache)
    part: Optional[np.ndarray]        # uint32 [R][n_tiles][4] as stored (logits)
    merged: Optional[np.ndarray]      # f32 [c_count]: merge_first's second projection


def gemv(W, *, mode, a_src, dtype, R, N, K, A=None, lda=None, a_row0=0, ln_w=None, ln_b=None, pend=None, n_pend=None,
         x_out=False, apart=None, S=0, H=0, merge_first=False, bias=None, C_in=None, c_count=None, ldc=None, ksplit=1,
         c_split=0, p_resid=None, B=0, Tq=0, cache_H=0, ctx=0, pos0=0, suppress=None, blank0=-1, blank1=-1, step=0,
         n_tiles=None, device: int = 0, need_device: bool = True) -> GemvResult:
    """One gemv() launch.  A: f32, any shape (flattened: a_count elements); pend [n_pend][a_count]; C_in: the
    rows of bias_resid (flattened: c_count elements; other modes take c_count alone)."""
    lib = L.load()
    g = L.GemvDebug()
    keep = []

    def fp(x):
        x = _f32(x)
        keep.append(x)
        return _fp(x)

    m, s = _code(MODES, mode), _code(A_SRC, a_src)
    g.dtype, g.mode, g.a_src, g.R, g.N, g.K = _code(DTYPES, dtype), m, s, R, N, K
    g.W = fp(W)
    a = _f32(A)
    g.A = fp(a)
    g.a_count = 0 if a is None else a.size
    g.lda, g.a_row0 = K if lda is None else lda, a_row0
    g.ln_w, g.ln_b = fp(ln_w), fp(ln_b)
    pd = _f32(pend)
    g.pend = fp(pd)
    g.n_pend = (0 if pd is None else pd.shape[0]) if n_pend is None else n_pend
    xo = np.full(max(int(g.a_count), 1), np.nan, np.float32) if x_out else None
    g.x_out = _fp(xo)
    g.apart, g.S, g.H, g.merge_first = fp(apart), S, H, int(merge_first)
    g.bias = fp(bias)
    if C_in is not None:
        c = np.array(C_in, np.float32).reshape(-1)
    else:
        c = np.full(max(int(c_count if c_count is not None else R * N), 1), np.nan, np.float32)
    g.C, g.c_count = _fp(c), (c.size if c_count is None else c_count)
    g.ldc, g.ksplit, g.c_split = N if ldc is None else ldc, ksplit, c_split
    g.p_resid = fp(p_resid)
    merged = np.full(c.size, np.nan, np.float32) if merge_first else None
    g.out_merged = _fp(merged)
    g.B, g.Tq, g.cache_H, g.ctx, g.pos0 = B, Tq, cache_H, ctx, pos0
    cache = None
    if m == L.SPT_GV_QKV_CACHE:
        cache = np.full((2, max(B, 1), max(cache_H, 1), max(ctx, 1), 64), np.nan, np.float32)
        g.cache = _fp(cache)
    part = None
    sup = None
    if m == L.SPT_GV_LOGITS:
        nt = (N + 15) // 16 if n_tiles is None else n_tiles
        g.n_tiles = nt
        part = np.zeros((max(R, 1), max(nt, 1), 4), np.float32)
        g.part = _fp(part)
        sup = np.zeros((N + 31) // 32, np.uint32) if suppress is None else np.ascontiguousarray(suppress, np.uint32)
        g.suppress = sup.ctypes.data_as(C.POINTER(C.c_uint32))
        g.suppress_words = sup.size
        g.blank0, g.blank1, g.step = blank0, blank1, step
    plan = np.full(8, -1, np.int32)
    g.plan = _ip(plan)
    err = C.create_string_buffer(512)
    st = lib.spt_debug_gemv(device, C.byref(g), err, 512)
    if st != L.SPT_OK and not (st == L.SPT_ERR_DEVICE and not need_device):
        raise TranscriptionError(st, err.value.decode())
    return GemvResult(st, dict(zip(PLAN_FIELDS, (int(v) for v in plan))), c, xo, cache,
                      None if part is None else part.view(np.uint32), merged)


@dataclass
class StepResult:
    status: int
    state: np.ndarray                 # int32 [4]: pos0, step, epoch, arrive after the call
    x: Optional[np.ndarray]           # embed: f32 [B * Tq][d]; finalize: f32 [n_steps][B][d]
    next_tok: Optional[np.ndarray]    # finalize: int32 [n_steps][B]
    out_tok: Optional[np.ndarray]     # finalize: int32 [B][out_cap], whole
    out_top1: Optional[np.ndarray]    # f32 [B][out_cap], whole
    out_top2: Optional[np.ndarray]
    done: Optional[np.ndarray]        # finalize: int32 [B]


def dec_step(op, *, state, dtype="f32", B=0, Tq=1, d=0, ctx=0, n_vocab=0, emb=None, emb_blocks: Optional[bytes] = None,
             emb_q=0, pos=None, tok=None, part=None, n_tiles=0, n_steps=1, forced=None, forced_len=None, done=None,
             ignore_eot=False, out_cap=0, eot=0, n_advance=0, device: int = 0, need_device: bool = True) -> StepResult:
    """op: "embed", "finalize", "advance" or "reset"; state = (pos0, step, epoch, arrive); part: the partials
    [n_steps][B][n_tiles][4] as spt_debug_gemv stores them (uint32 or float32 words)."""
    lib = L.load()
    g = L.DecStepDebug()
    o = _code(OPS, op)
    g.op, g.dtype = o, _code(DTYPES, dtype)
    g.B, g.Tq, g.d, g.ctx, g.n_vocab, g.n_tiles, g.n_steps = B, Tq, d, ctx, n_vocab, n_tiles, n_steps
    g.ignore_eot, g.out_cap, g.eot, g.emb_q, g.n_advance = int(ignore_eot), out_cap, eot, emb_q, n_advance
    st_arr = None if state is None else np.array(state, np.int64).astype(np.uint32).view(np.int32).copy()
    g.state = _ip(st_arr)
    e, p, t = _f32(emb), _f32(pos), _i32(tok)
    g.emb, g.pos, g.tok = _fp(e), _fp(p), _ip(t)
    buf = None
    if emb_blocks is not None:
        buf = (C.c_char * max(len(emb_blocks), 1)).from_buffer_copy(bytes(emb_blocks) or b"\0")
        g.emb_blocks = C.cast(buf, C.c_void_p)
        g.emb_blocks_bytes = len(emb_blocks)
    pt = None
    if part is not None:
        pt = np.ascontiguousarray(part)
        pt = pt.view(np.float32) if pt.dtype == np.uint32 else np.ascontiguousarray(pt, np.float32)
        g.part = _fp(pt)
    f = _i32(forced)
    g.forced = _ip(f)
    g.forced_len = (0 if f is None else f.shape[-1]) if forced_len is None else forced_len
    x = nxt = ot = o1 = o2 = dn = None
    rows, dd = max(B, 1), max(d, 1)
    if o == L.SPT_DEC_STEP_EMBED:
        x = np.full((rows * max(Tq, 1), dd), np.nan, np.float32)
    elif o == L.SPT_DEC_STEP_FINALIZE:
        ns, cap = max(n_steps, 1), max(out_cap, 1)
        x = np.full((ns, rows, dd), np.nan, np.float32)
        nxt = np.full((ns, rows), -3, np.int32)
        ot = np.full((rows, cap), -3, np.int32)
        o1 = np.zeros((rows, cap), np.float32)
        o2 = np.zeros((rows, cap), np.float32)
        dn = np.zeros(rows, np.int32) if done is None else np.array(done, np.int32)
        g.next_tok, g.out_tok, g.out_top1, g.out_top2, g.done = _ip(nxt), _ip(ot), _fp(o1), _fp(o2), _ip(dn)
    g.x = _fp(x)
    err = C.create_string_buffer(512)
    st = lib.spt_debug_dec_step(device, C.byref(g), err, 512)
    if st != L.SPT_OK and not (st == L.SPT_ERR_DEVICE and not need_device):
        raise TranscriptionError(st, err.value.decode())
    return StepResult(st, st_arr, x, nxt, ot, o1, o2, dn)
