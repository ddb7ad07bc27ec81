"""The Parakeet kernels alone (spt_debug_pk_conv, spt_debug_pk_relpos, spt_debug_pk_rel_attn, spt_debug_pk_dec_stage,
spt_debug_pk_tdt, spt_debug_pk_tdt_steps of csrc/capi_pkk.cpp) on numpy arrays, without an engine or a model.  Test infrastructure:
tests/test_gpu_pk_kernels.py and tests/test_pk_ref.py.

Every array a kernel writes starts with each byte 0xFF on the device and comes back whole: what the launch
did not write reads as NaN (f32) or as the 16-bit NaN 0xFFFF converted to f32.  `guard` appends that many
elements past what the launch owns; they must come back NaN."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .engine import TranscriptionError

DTYPES = {"f32": L.SPT_DTYPE_F32, "bf16": L.SPT_DTYPE_BF16, "f16": L.SPT_DTYPE_F16}
CONV_MODES = {"conv0": L.SPT_PK_CONV0, "dwconv1": L.SPT_PK_DWCONV1, "dwconv2": L.SPT_PK_DWCONV2,
              "conv_module": L.SPT_PK_CONV_MODULE}
VARIANTS = {"auto": L.SPT_PK_ATTN_AUTO, "valu": L.SPT_PK_ATTN_VALU, "mfma": L.SPT_PK_ATTN_MFMA}


def _f32(x):
    return None if x is None else np.ascontiguousarray(x, np.float32)


def _fp(x):
    return None if x is None else x.ctypes.data_as(C.POINTER(C.c_float))


def _code(table, v):
    return table[v] if isinstance(v, str) else int(v)


def halve(n: int) -> int:
    return (n - 1) // 2 + 1


def _finish(st, err, need_device):
    if st != L.SPT_OK and not (st == L.SPT_ERR_DEVICE and not need_device):
        raise TranscriptionError(st, err.value.decode())
    return st


def conv(mode, x, lens, w, bias, *, dtype, B, Tp, C_, F=0, bn=None, guard=0, y_count=None, device: int = 0,
         need_device: bool = True):
    """One pk_conv0 / pk_dwconv / pk_conv_module launch -> (status, y f32 [y_count], n_owned).  bn = (g, b, m, v)."""
    lib = L.load()
    a = L.PkConvDebug()
    m = _code(CONV_MODES, mode)
    keep = [_f32(x), np.ascontiguousarray(lens, np.int32), _f32(w), _f32(bias)] + [_f32(v) for v in (bn or (None,) * 4)]
    a.x, a.w, a.bias = _fp(keep[0]), _fp(keep[2]), _fp(keep[3])
    a.lens = keep[1].ctypes.data_as(C.POINTER(C.c_int32))
    a.bn_g, a.bn_b, a.bn_m, a.bn_v = (_fp(v) for v in keep[4:8])
    a.dtype, a.mode, a.B, a.Tp, a.F, a.C = _code(DTYPES, dtype), m, B, Tp, F, C_
    owned = B * Tp * C_ if m == L.SPT_PK_CONV_MODULE else B * halve(max(Tp, 1)) * halve(max(F, 1)) * C_
    n = max(owned, 0) + guard if y_count is None else y_count
    y = np.full(max(n, 1), np.nan, np.float32)
    a.y, a.y_count = _fp(y), n
    err = C.create_string_buffer(512)
    st = _finish(lib.spt_debug_pk_conv(device, C.byref(a), err, 512), err, need_device)
    return st, y, owned


def relpos(Tp, d, *, dtype, guard=0, pe_count=None, device: int = 0, need_device: bool = True):
    """One pk_relpos launch -> (status, pe f32 [pe_count])."""
    lib = L.load()
    n = (2 * Tp - 1) * d + guard if pe_count is None else pe_count
    pe = np.full(max(n, 1), np.nan, np.float32)
    err = C.create_string_buffer(512)
    st = _finish(lib.spt_debug_pk_relpos(device, _code(DTYPES, dtype), Tp, d, _fp(pe), n, err, 512), err, need_device)
    return st, pe


def rel_attn(qkv, p, pu, pv, lens, *, dtype, B, Tp, H, dk, ldp, p_off=0, p_bstride=0, variant="auto", guard=0,
             out_count=None, p_count=None, device: int = 0, need_device: bool = True):
    """One pk_rel_attn_variant launch -> (status, out f32 [out_count]); the first B * Tp * H * dk are the launch's."""
    lib = L.load()
    a = L.PkAttnDebug()
    keep = [_f32(qkv), _f32(p), _f32(pu), _f32(pv), np.ascontiguousarray(lens, np.int32)]
    a.qkv, a.p, a.pu, a.pv = (_fp(v) for v in keep[:4])
    a.lens = keep[4].ctypes.data_as(C.POINTER(C.c_int32))
    a.p_count = keep[1].size if p_count is None else p_count
    a.p_off, a.p_bstride = p_off, p_bstride
    a.dtype, a.variant, a.B, a.Tp, a.H, a.dk, a.ldp = _code(DTYPES, dtype), _code(VARIANTS, variant), B, Tp, H, dk, ldp
    n = B * Tp * H * dk + guard if out_count is None else out_count
    out = np.full(max(n, 1), np.nan, np.float32)
    a.out, a.out_count = _fp(out), n
    err = C.create_string_buffer(512)
    st = _finish(lib.spt_debug_pk_rel_attn(device, C.byref(a), err, 512), err, need_device)
    return st, out


STATE_FIELDS = ("t", "at_t", "n_out", "done", "upd", "tok", "t3p")


def pack_part(v1, i1, v2):
    """The joint stage's partials {f32 best, i32 index, f32 runner-up, 0} [..][4] as f32 words."""
    v1 = np.asarray(v1, np.float32)
    out = np.zeros(v1.shape + (4,), np.float32)
    out[..., 0], out[..., 2] = v1, np.asarray(v2, np.float32)
    out[..., 1] = np.broadcast_to(np.asarray(i1, np.int32), v1.shape).copy().view(np.float32)
    return out


def tdt(part, dur, lens, emb, fe, *, V, max_symbols, cap, T3p, n_steps=None, n_tiles=None, n_dur=None, B=None, P=None,
        device: int = 0, need_device: bool = True):
    """pk_state_init, then pk_joint_fin per step on part [n_steps][B][n_tiles][4] (pack_part) and dur
    [n_steps][B][n_dur] -> dict(status, state int32 [n_steps + 1][B][7] (STATE_FIELDS; slot 0: after the init),
    xemb, fecur f32 [n_steps + 1][B][P], out_tok, out_frame int32 and out_t1, out_t2 f32 [n_steps][B * cap + 1]:
    the arrays whole after every step, the last element a guard).  What no kernel wrote is -1 / NaN."""
    lib = L.load()
    a = L.PkTdtDebug()
    pt, du, em, fe_ = _f32(part), _f32(dur), _f32(emb), _f32(fe)
    ln = np.ascontiguousarray(lens, np.int32)
    a.B = ln.shape[0] if B is None else B
    a.n_steps = pt.shape[0] if n_steps is None else n_steps
    a.n_tiles = pt.shape[2] if n_tiles is None else n_tiles
    a.n_dur = du.shape[-1] if n_dur is None else n_dur
    a.P = em.shape[-1] if P is None else P
    a.V, a.max_symbols, a.cap, a.T3p = V, max_symbols, cap, T3p
    ns, Bn, Pn, no = max(a.n_steps, 1), max(a.B, 1), max(a.P, 1), max(a.B, 1) * max(cap, 0) + 1
    state = np.full((ns + 1, Bn, 7), -3, np.int32)
    xemb, fecur = (np.full((ns + 1, Bn, Pn), np.nan, np.float32) for _ in range(2))
    otok, ofr = (np.full((ns, no), -3, np.int32) for _ in range(2))
    o1, o2 = (np.zeros((ns, no), np.float32) for _ in range(2))
    ip = lambda x: x.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
    a.part, a.dur, a.emb, a.fe, a.lens = _fp(pt), _fp(du), _fp(em), _fp(fe_), ip(ln)
    a.state, a.xemb, a.fecur = ip(state), _fp(xemb), _fp(fecur)
    a.out_tok, a.out_frame, a.out_t1, a.out_t2 = ip(otok), ip(ofr), _fp(o1), _fp(o2)
    err = C.create_string_buffer(512)
    st = _finish(lib.spt_debug_pk_tdt(device, C.byref(a), err, 512), err, need_device)
    return dict(status=st, state=state, xemb=xemb, fecur=fecur, out_tok=otok, out_frame=ofr, out_t1=o1, out_t2=o2)


DEC_MODES = {"lstm": L.SPT_PK_DEC_LSTM, "pred": L.SPT_PK_DEC_PRED, "joint": L.SPT_PK_DEC_JOINT}


def state_rows(upd):
    """PkState rows [B][7] for a stage that reads upd alone: every other field holds 77."""
    upd = np.asarray(upd, np.int32)
    st = np.full((upd.size, 7), 77, np.int32)
    st[:, 4] = upd
    return st


def dec_stage(mode, W, b0, state, *, B, P, W2=None, b1=None, xin=None, h_in=None, c_in=None, fe=None, gp=None, V=0, n_dur=0,
              device: int = 0, need_device: bool = True):
    """One pk_decode_stage launch on plain weights -> dict(status, h_out, c_out [B][P] (lstm), gp [B][P] (pred: the
    caller's rows, overwritten where upd), part uint32 [B][n_tiles][4] and dur [B][n_dur] (joint))."""
    lib = L.load()
    a = L.PkDecDebug()
    m = _code(DEC_MODES, mode)
    keep = [_f32(v) for v in (W, W2, b0, b1, xin, h_in, c_in, fe)]
    a.W, a.W2, a.b0, a.b1, a.xin, a.h_in, a.c_in, a.fe = (_fp(v) for v in keep)
    st = None if state is None else np.ascontiguousarray(state, np.int32)
    a.state = None if st is None else st.ctypes.data_as(C.POINTER(C.c_int32))
    a.mode, a.B, a.P, a.V, a.n_dur = m, B, P, V, n_dur
    bp = (max(B, 1), max(P, 1))
    g = None if gp is None else np.array(gp, np.float32).reshape(bp)
    a.gp = _fp(g)
    h = c = part = dur = None
    if m == L.SPT_PK_DEC_LSTM:
        h, c = np.full(bp, np.nan, np.float32), np.full(bp, np.nan, np.float32)
        a.h_out, a.c_out = _fp(h), _fp(c)
    elif m == L.SPT_PK_DEC_JOINT:
        nt = (max(V, 0) + 1 + max(n_dur, 0) + 63) // 64
        part = np.full((bp[0], nt, 4), np.nan, np.float32)
        dur = np.full((bp[0], max(n_dur, 1)), np.nan, np.float32)
        a.part, a.dur = _fp(part), _fp(dur)
    err = C.create_string_buffer(512)
    s = _finish(lib.spt_debug_pk_dec_stage(device, C.byref(a), err, 512), err, need_device)
    return dict(status=s, h_out=h, c_out=c, gp=g, part=None if part is None else part.view(np.uint32), dur=dur)


def tdt_steps(lstm, pred_w, pred_b, joint_w, joint_b, emb, fe, lens, *, V, n_dur, max_symbols, cap, T3p, n_steps, B=None,
              P=None, device: int = 0, need_device: bool = True):
    """pk_state_init, then n_steps whole decode steps (LSTM 0, LSTM 1, prediction, joint, fin) on plain weights;
    lstm [2] = (W_ih, W_hh, b_ih, b_hh) -> dict(status, state int32 [n_steps + 1][B][7], out_tok, out_frame int32 and
    out_t1, out_t2 f32 [B * cap + 1] after the last step)."""
    lib = L.load()
    a = L.PkStepsDebug()
    keep = [[_f32(w) for w in layer] for layer in lstm]
    for l in range(2):
        for i in range(4):
            a.lstm[l][i] = _fp(keep[l][i])
    rest = [_f32(v) for v in (pred_w, pred_b, joint_w, joint_b, emb, fe)]
    a.pred_w, a.pred_b, a.joint_w, a.joint_b, a.emb, a.fe = (_fp(v) for v in rest)
    ln = np.ascontiguousarray(lens, np.int32)
    ip = lambda x: x.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
    a.lens = ip(ln)
    a.B = ln.shape[0] if B is None else B
    a.P = rest[4].shape[-1] if P is None else P
    a.V, a.n_dur, a.n_steps, a.max_symbols, a.cap, a.T3p = V, n_dur, n_steps, max_symbols, cap, T3p
    ns, Bn, no = max(n_steps, 1), max(a.B, 1), max(a.B, 1) * max(cap, 0) + 1
    state = np.full((ns + 1, Bn, 7), -3, np.int32)
    otok, ofr = np.full(no, -3, np.int32), np.full(no, -3, np.int32)
    o1, o2 = np.zeros(no, np.float32), np.zeros(no, np.float32)
    a.state, a.out_tok, a.out_frame, a.out_t1, a.out_t2 = ip(state), ip(otok), ip(ofr), _fp(o1), _fp(o2)
    err = C.create_string_buffer(512)
    st = _finish(lib.spt_debug_pk_tdt_steps(device, C.byref(a), err, 512), err, need_device)
    return dict(status=st, state=state, out_tok=otok, out_frame=ofr, out_t1=o1, out_t2=o2)
