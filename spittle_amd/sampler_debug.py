"""The sampler kernels alone (spt_debug_sample_*, csrc/capi_sample.cpp): whisper_full's token
rules, the beam candidates and the beam K/V gather on numpy arrays, without an engine or a model.
Test infrastructure: tests/test_gpu_sampler.py compares these with tests/sampler_ref.py."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib as L
from .engine import TranscriptionError

DTYPES = {"f32": L.SPT_DTYPE_F32, "bf16": L.SPT_DTYPE_BF16, "f16": L.SPT_DTYPE_F16}


@dataclass
class SampleParams:
    """TsParams of kernels.h: one call's decoding parameters as the kernels read them."""
    temperature: float = 0.0
    suppress_blank: bool = True
    no_ts: bool = False
    max_initial: int = 50
    n_max: int = 220
    max_tokens: int = 0
    seed: int = 0

    def c(self) -> L.SampleParams:
        return L.SampleParams(self.temperature, int(self.suppress_blank), int(self.no_ts), self.max_initial,
                              self.n_max, self.max_tokens, self.seed & (2 ** 64 - 1))


def suppress_words(mask) -> np.ndarray:
    """bool [n_vocab] -> the kernels' bit words (token n: bit n & 31 of word n >> 5)."""
    m = np.asarray(mask, bool)
    bits = np.zeros((m.size + 31) // 32 * 32, np.uint8)
    bits[:m.size] = m
    return np.packbits(bits.reshape(-1, 32), axis=1, bitorder="little").view("<u4").reshape(-1).copy()


def _ptr(x, t):
    return None if x is None else x.ctypes.data_as(C.POINTER(t))


def _check(st, err):
    if st != L.SPT_OK:
        raise TranscriptionError(st, err.value.decode())


def sample_tokens(logits, suppress, prm: SampleParams, *, eot, beg, blank, seek, seek_end, emb, pos, n_vocab=None,
                  state=None, done=None, forced=None, out_cap=None, pos0=0, step=0, epoch=0, Tq=1, dtype="f32",
                  history=None, device: int = 0) -> dict:
    """S steps of dec_ts_stats + dec_finalize_ts on logits [S][B][ldl] (suppress: the bit words).
    -> dict(out_tok, out_plog, out_tid [B][out_cap] (rows pre-filled with -9 / 0 / -9), state [B][4],
    done, next_tok [B], x [B][d], pos0, step, epoch, arrive).  history: the initial out_tok (the tokens before
    `step`) when the run starts at step > 0."""
    lib = L.load()
    lg = None if logits is None else np.ascontiguousarray(logits, np.float32)
    S, B, ldl = (1, 1, 1) if lg is None else lg.shape
    V = ldl if n_vocab is None else n_vocab
    cap = S + step if out_cap is None else out_cap
    sup = np.ascontiguousarray(suppress, np.uint32)
    emb = np.ascontiguousarray(emb, np.float32)
    pos = np.ascontiguousarray(pos, np.float32)
    ctx, d = pos.shape
    sk = np.ascontiguousarray(np.broadcast_to(seek, (max(B, 1),)), np.int32)
    se = np.ascontiguousarray(np.broadcast_to(seek_end, (max(B, 1),)), np.int32)
    st8 = np.zeros((max(B, 1), 4), np.int32) if state is None else np.array(state, np.int32).reshape(B, 4)
    dn = np.zeros(max(B, 1), np.int32) if done is None else np.array(done, np.int32).reshape(B)
    fc = None if forced is None else np.ascontiguousarray(forced, np.int32).reshape(B, -1)
    out = dict(out_tok=np.full((max(B, 1), max(cap, 1)), -9, np.int32), out_plog=np.zeros((max(B, 1), max(cap, 1)), np.float32),
               out_tid=np.full((max(B, 1), max(cap, 1)), -9.0, np.float32), state=st8, done=dn,
               next_tok=np.full(max(B, 1), -9, np.int32), x=np.zeros((max(B, 1), d), np.float32))
    if history is not None:
        out["out_tok"][...] = np.asarray(history, np.int32).reshape(B, cap)
    ds = np.array([pos0, step, epoch], np.int32)
    arrive = np.full(1, 0xFFFFFFFF, np.uint32)
    p = prm.c()
    err = C.create_string_buffer(512)
    i32, f32 = C.c_int32, C.c_float
    st = lib.spt_debug_sample_tokens(device, DTYPES[dtype], _ptr(lg, f32), S, B, V, ldl, eot, beg, blank,
                                     _ptr(sup, C.c_uint32), C.byref(p), _ptr(sk, i32), _ptr(se, i32), _ptr(st8, i32),
                                     _ptr(dn, i32), _ptr(fc, i32), 0 if fc is None else fc.shape[1], cap, _ptr(ds, i32), Tq,
                                     d, ctx, _ptr(emb, f32), _ptr(pos, f32), _ptr(out["out_tok"], i32),
                                     _ptr(out["out_plog"], f32), _ptr(out["out_tid"], f32), _ptr(out["next_tok"], i32),
                                     _ptr(out["x"], f32), _ptr(arrive, C.c_uint32), err, 512)
    _check(st, err)
    out.update(pos0=int(ds[0]), step=int(ds[1]), epoch=int(ds[2]) & 0xFFFFFFFF, arrive=int(arrive[0]))
    return out


def sample_beam(logits, suppress, prm: SampleParams, *, eot, beg, blank, row, step, k, chunked, n_vocab=None,
                device: int = 0) -> dict:
    """One dec_beam_topk launch on logits [B][ldl]; row [B][4] = last, previous token, has_ts,
    seek_delta.  chunked: the chunk + merge kernels, else the one-workgroup kernel.
    -> dict(cand_id, cand_lp [B][8] (pre-filled with -9 / 0), tid [B])."""
    lib = L.load()
    lg = np.ascontiguousarray(logits, np.float32)
    B, ldl = lg.shape
    V = ldl if n_vocab is None else n_vocab
    sup = np.ascontiguousarray(suppress, np.uint32)
    rw = np.ascontiguousarray(row, np.int32).reshape(B, 4)
    out = dict(cand_id=np.full((B, 8), -9, np.int32), cand_lp=np.zeros((B, 8), np.float32), tid=np.full(B, -9, np.int32))
    p = prm.c()
    err = C.create_string_buffer(512)
    st = lib.spt_debug_sample_beam(device, _ptr(lg, C.c_float), B, V, ldl, eot, beg, blank, _ptr(sup, C.c_uint32),
                                   C.byref(p), _ptr(rw, C.c_int32), step, k, int(bool(chunked)),
                                   _ptr(out["cand_id"], C.c_int32), _ptr(out["cand_lp"], C.c_float),
                                   _ptr(out["tid"], C.c_int32), err, 512)
    _check(st, err)
    return out


def kv_gather(src, dst, rows, pos0, dtype="f32", device: int = 0) -> np.ndarray:
    """One dec_kv_gather launch: src, dst [L][2][B][H][ctx][64] f32 (stored as dtype for the launch);
    -> dst after it, as f32."""
    lib = L.load()
    src = np.ascontiguousarray(src, np.float32)
    out = np.array(dst, np.float32, order="C")
    Ln, two, B, H, ctx, hd = src.shape
    if two != 2 or hd != 64 or out.shape != src.shape:
        raise ValueError("kv_gather: src and dst are [L][2][B][H][ctx][64]")
    rw = np.ascontiguousarray(rows, np.int32)
    if rw.shape != (B,):
        raise ValueError("kv_gather: one source row per batch row")
    err = C.create_string_buffer(512)
    st = lib.spt_debug_sample_kv_gather(device, DTYPES[dtype], _ptr(src, C.c_float), _ptr(out, C.c_float),
                                        _ptr(rw, C.c_int32), Ln, B, H, ctx, pos0, err, 512)
    _check(st, err)
    return out
