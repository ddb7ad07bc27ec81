"""Float64 reference of one decoder GEMV launch (spt_debug_gemv) and of the small kernels of the decode step
(spt_debug_dec_step), with their error bars.  Shared by tests/test_gpu_gemv.py and tests/test_gemv_ref.py
(CPU: the reference against torch, the cases' preconditions, and the same references recomputed with named
faults).  Nothing here knows of a wave, a tile of K, a slab order other than the documented one, or LDS.

Reference.  W and an A_DIRECT operand are rounded once to the engine dtype T; a LayerNorm source is the
float32 sum x + p0 + p1 + .. in that order (asserted bit for bit through x_out, so it adds no bar term),
normalised in float64, its image rounded to T; an attention-merge source is O / L of the chunks' {o, m, l}
in float64, rounded to T.  Everything after that is float64.

Bars (none is taken from what a kernel returns).  u = 2^-24, u_T = 2^-8 (bf16), 2^-11 (f16).
  linear      2 (K + 4) u S, S = sum_k |a_k w_k| + |bias| + |residual|            (qgemv_ref's A_DIRECT bar)
  LN image    16-bit: 2 u_T sum_k |ln_k w_k| (an element within f32 error of a rounding boundary of T rounds
              the other way: one ulp_T).  f32: sum_k |w_k| |dy_k| with |dy_k| the two-pass LayerNorm bound of
              DESIGN.md 2e (gemm_ref.ln_bar, which carries its factor 4).
  ATTN image  16-bit: the same boundary argument, 2 u_T sum_k |a_k w_k|.  f32: sum_k |w_k| |da_k| with
              |da| = 2 (dO / L + |O| dL / L^2 + u |O / L|), dO = sum_c |o_c| f_c (e_c + S u), dL = sum_c l_c f_c
              (e_c + S u), e_c = (ln 2 |m_c - M| + 2) u: the subtraction's rounding carried through 2^x, one ulp
              (2 u) of v_exp_f32 (assumed, as in 2e), S fused multiply-adds, the division.
  stored T    + half an ulp of T at the reference value.
  GELU        1.13 x linear + 2^-17 |g| (+ the store's half ulp).
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from tests import gemm_ref as G
from tests.qgemv_ref import U32, half_ulp_t
from tests.qgemv_ref import U_T as _U16
from tests.qgemv_ref import round_t as _round16

DTYPES = ("f32", "bf16", "f16")
U_T = dict(_U16, f32=U32)
KS = {"f32": 64, "bf16": 128, "f16": 128}
INVALID = 0x7FFFFFFF
F16_MAX = 65504.0
FAULTS = ("slab_dropped", "a_row0_ignored", "cache_pos_off_by_one", "kv_exchanged", "b_t_exchanged",
          "merge_unweighted", "empty_chunk_not_skipped", "blank_at_step_1", "mask_bit_shifted", "v2_second_distinct",
          "tie_to_higher_index", "pos_clamp_at_ctx")


def round_t(x, dtype: str) -> np.ndarray:
    """f32 -> T -> f32 (qgemv_ref's rounding; f32 is itself)."""
    x = np.asarray(x, np.float32)
    return x if dtype == "f32" else _round16(x, dtype)


def store_half_ulp(v, dtype: str):
    return 0.0 if dtype == "f32" else half_ulp_t(v, dtype)


# ------------------------------------------------------------------------------------------ A sources
def rows_of(flat, R: int, lda: int, a_row0: int, K: int) -> np.ndarray:
    flat = np.asarray(flat).reshape(-1)
    return flat[(np.arange(R)[:, None] * lda + a_row0) + np.arange(K)[None, :]]


def sum_f32(x, pend) -> np.ndarray:
    """x + p0 + p1 + ..., each add rounded to float32, in that order (flat arrays of A's layout)."""
    v = np.asarray(x, np.float32).copy()
    for p in ([] if pend is None else pend):
        v = (v + np.asarray(p, np.float32)).astype(np.float32)
    return v


def layernorm(v, w, b) -> np.ndarray:
    return G.layernorm(v, w, b)


def attn_merge(apart, fault: Optional[str] = None) -> np.ndarray:
    """[R][H][S][66] = {o[64], m, l} -> [R][H * 64] float64: sum_c o_c 2^(m_c - M) / sum_c l_c 2^(m_c - M), the
    chunks with m = -inf left out."""
    p = np.asarray(apart, np.float64)
    R, H, S, _ = p.shape
    o, m, l = p[..., :64], p[..., 64], p[..., 65]
    M = m.max(axis=2, keepdims=True)
    with np.errstate(invalid="ignore", over="ignore"):
        f = np.exp2(m - M)
        if fault == "merge_unweighted":
            f = np.ones_like(f)
        live = np.isfinite(m)
        f = np.where(live, f, 0.0)
        if fault != "empty_chunk_not_skipped":   # a kernel without the skip multiplies the chunk's o by 0
            o = np.where(live[..., None], o, 0.0)
            l = np.where(live, l, 0.0)
        L = (l * f).sum(axis=2)
        O = (o * f[..., None]).sum(axis=2)
        return (O / L[..., None]).reshape(R, H * 64)


def attn_err_f32(apart) -> np.ndarray:
    """|da| of the f32 merge, [R][H * 64] (module docstring)."""
    p = np.asarray(apart, np.float64)
    R, H, S, _ = p.shape
    o, m, l = p[..., :64], p[..., 64], p[..., 65]
    M = m.max(axis=2, keepdims=True)
    live = np.isfinite(m)
    with np.errstate(invalid="ignore"):
        f = np.where(live, np.exp2(m - M), 0.0)
        e = np.where(live, (np.log(2.0) * np.abs(m - M) + 2.0) * U32, 0.0) + S * U32
    o = np.where(live[..., None], o, 0.0)
    l = np.where(live, l, 0.0)
    L = (l * f).sum(axis=2)
    O = (o * f[..., None]).sum(axis=2)
    dL = (l * f * e).sum(axis=2)
    dO = (np.abs(o) * (f * e)[..., None]).sum(axis=2)
    Lx = L[..., None]
    return (2.0 * (dO / Lx + np.abs(O) * dL[..., None] / Lx ** 2 + U32 * np.abs(O / Lx))).reshape(R, H * 64)


def image(a_src: str, dtype: str, *, A=None, R=0, K=0, lda=0, a_row0=0, pend=None, ln_w=None, ln_b=None, apart=None,
          fault: Optional[str] = None):
    """(a [R][K] float64 as the MFMA sees it, da [R][K]: the image's own error bound per element, x: the
    float32-summed flat rows of an A_LN source or None)."""
    if a_src == "direct":
        if fault == "a_row0_ignored":
            a_row0 = 0
        a = round_t(rows_of(A, R, lda, a_row0, K), dtype).astype(np.float64)
        return a, np.zeros_like(a), None
    if a_src == "ln":
        if fault == "slab_dropped" and pend is not None and len(pend):
            pend = pend[:-1]
        if fault == "a_row0_ignored":
            a_row0 = 0
        x = sum_f32(A, pend)
        v = rows_of(x, R, lda, a_row0, K).astype(np.float64)
        ln = layernorm(v, ln_w, ln_b)
        a = round_t(ln.astype(np.float32), dtype).astype(np.float64)
        da = G.ln_bar(v, ln_w, ln_b, "f32") if dtype == "f32" else 2.0 * U_T[dtype] * np.abs(a)
        return a, da, x
    m = attn_merge(apart, fault)
    with np.errstate(invalid="ignore"):
        a = round_t(m.astype(np.float32), dtype).astype(np.float64)
    da = attn_err_f32(apart) if dtype == "f32" else 2.0 * U_T[dtype] * np.abs(a)
    return a, da, None


# ------------------------------------------------------------------------------------------ the launch
def gelu(x):
    return G.gelu(x)


def linear(a, da, W, dtype, bias=None, resid=None, k0=0, k1=None):
    """(y, bar) of a[:, k0:k1] W[:, k0:k1]^T + bias + resid, the linear bar with the image term."""
    w = round_t(W, dtype).astype(np.float64)
    K = a.shape[1]
    k1 = K if k1 is None else k1
    aa, ww = a[:, k0:k1], w[:, k0:k1]
    with np.errstate(invalid="ignore"):
        y = aa @ ww.T
        S = np.abs(aa) @ np.abs(ww).T
        img = da[:, k0:k1] @ np.abs(ww).T
    if bias is not None:
        y = y + np.asarray(bias, np.float64)
        S = S + np.abs(np.asarray(bias, np.float64))
    if resid is not None:
        y = y + np.asarray(resid, np.float64)
        S = S + np.abs(np.asarray(resid, np.float64))
    return y, 2.0 * (K + 4) * U32 * S + img


def stored(y, lin, dtype):
    """A value stored in T: (y, bar)."""
    return y, lin + store_half_ulp(np.abs(y) + lin, dtype)


def gelu_out(y, lin, dtype):
    g = gelu(y)
    soft = 1.13 * lin + 2.0 ** -17 * np.abs(g)
    return g, soft + store_half_ulp(np.abs(g) + soft, dtype)


def partial_slabs(a, da, W, dtype, ksplit, bias=None, resid=None):
    """GV_PARTIAL: [ksplit][R][N] (ref, bar); split kz owns super-steps [kz * per, (kz + 1) * per) of K, slab 0
    takes the bias and the residual rows."""
    K = a.shape[1]
    ks = KS[dtype]
    nss = K // ks
    per = -(-nss // ksplit)
    ref, bar = [], []
    for kz in range(ksplit):
        k0, k1 = min(kz * per, nss) * ks, min((kz + 1) * per, nss) * ks
        y, b = linear(a, da, W, dtype, bias if kz == 0 else None, resid if kz == 0 else None, k0, k1)
        ref.append(y)
        bar.append(b)
    return np.stack(ref), np.stack(bar)


def cache_index(B, Tq, H, ctx, pos0, fault: Optional[str] = None):
    """For row r = b * Tq + t, head h: (part, b, h, pos) of the k / v rows it appends -> arrays b [R], pos [R]."""
    r = np.arange(B * Tq)
    b, t = r // Tq, r % Tq
    if fault == "b_t_exchanged":
        b, t = r % B, r // B
    pos = pos0 + t + (1 if fault == "cache_pos_off_by_one" else 0)
    return b, pos


def cache_ref(y, bar, B, Tq, H, ctx, pos0, dtype, fault: Optional[str] = None):
    """y, bar [R][3 d] -> (cache [2][B][H][ctx][64] float64 with NaN where nothing is written, its bar, the
    mask of written elements).  f16 clamps to +-65504 before the store."""
    d = 64 * H
    ref = np.full((2, B, H, ctx, 64), np.nan)
    cb = np.zeros_like(ref)
    b, pos = cache_index(B, Tq, H, ctx, pos0, fault)
    for part in range(2):
        src = 1 - part if fault == "kv_exchanged" else part
        v = y[:, (src + 1) * d:(src + 2) * d].reshape(B * Tq, H, 64)
        e = bar[:, (src + 1) * d:(src + 2) * d].reshape(B * Tq, H, 64)
        if dtype == "f16":
            v = np.clip(v, -F16_MAX, F16_MAX)
        ok = pos < ctx
        ref[part, b[ok], :, pos[ok], :] = v[ok]
        cb[part, b[ok], :, pos[ok], :] = e[ok]
    return ref, cb, ~np.isnan(ref)


# ------------------------------------------------------------------------------------------ logits
def suppressed(N, mask_words, blank0, blank1, step, fault: Optional[str] = None) -> np.ndarray:
    n = np.arange(N)
    bit = (n + 1) & 31 if fault == "mask_bit_shifted" else n & 31
    sup = ((np.asarray(mask_words, np.uint32)[n >> 5] >> bit.astype(np.uint32)) & 1).astype(bool)
    if step == 0 or (fault == "blank_at_step_1" and step == 1):
        sup |= (n == blank0) | (n == blank1)
    return sup


def tile_top2(logits_row, sup, n_tiles: Optional[int] = None, fault: Optional[str] = None):
    """The partials of one row as a pure function of the returned f32 logits: per tile of 16 columns
    (v1, i1, v2) = the largest unsuppressed value at its lowest index and the second of the multiset (a
    suppressed or missing column counts as -inf; a fully suppressed tile gives -inf at its lowest valid column)."""
    row = np.asarray(logits_row, np.float32)
    N = row.size
    nt = -(-N // 16) if n_tiles is None else n_tiles
    v1 = np.full(nt, -np.inf, np.float32)
    i1 = np.full(nt, INVALID, np.int64)
    v2 = np.full(nt, -np.inf, np.float32)
    for t in range(min(nt, -(-N // 16))):
        n0, n1 = 16 * t, min(16 * t + 16, N)
        v = np.where(sup[n0:n1], np.float32(-np.inf), row[n0:n1])
        best = v.max()
        at = np.flatnonzero(v == best)
        k = at[-1] if fault == "tie_to_higher_index" else at[0]
        rest = np.delete(v, k)
        if fault == "v2_second_distinct":
            rest = rest[rest != best]
        v1[t], i1[t] = best, n0 + k
        v2[t] = rest.max() if rest.size else -np.inf
    return v1, i1, v2


def parts_words(v1, i1, v2) -> np.ndarray:
    """(v1, i1, v2) -> uint32 [..][4] as the kernel stores a partial."""
    out = np.zeros(np.shape(v1) + (4,), np.uint32)
    out[..., 0] = np.asarray(v1, np.float32).view(np.uint32)
    out[..., 1] = np.asarray(i1, np.int64).astype(np.uint32)
    out[..., 2] = np.asarray(v2, np.float32).view(np.uint32)
    return out


# ------------------------------------------------------------------------------------------ the step
def merge_parts(part_words, fault: Optional[str] = None):
    """All tiles of one sequence -> (v1, i1, v2): the largest v1 at the lowest index, v2 the second of the
    multiset of every tile's v1 and v2."""
    p = np.asarray(part_words, np.uint32).reshape(-1, 4)
    v1, i1, v2 = p[:, 0].copy().view(np.float32), p[:, 1].astype(np.int64), p[:, 2].copy().view(np.float32)
    i1 = np.where(i1 >= 2 ** 31, i1 - 2 ** 32, i1)
    # the kernel starts from (-inf, INVALID, -inf)
    v1 = np.concatenate([v1, np.float32([-np.inf])])
    i1 = np.concatenate([i1, [INVALID]])
    v2 = np.concatenate([v2, np.float32([-np.inf])])
    best = v1.max()
    cand = np.flatnonzero(v1 == best)
    w = cand[np.argmax(i1[cand])] if fault == "tie_to_higher_index" else cand[np.argmin(i1[cand])]
    rest = np.concatenate([np.delete(v1, w), v2])
    if fault == "v2_second_distinct":
        rest = rest[rest != best]
    return np.float32(best), int(i1[w]), np.float32(rest.max() if rest.size else -np.inf)


def emb_rows(emb, dtype):
    return round_t(emb, dtype)


def embed_ref(tok, Tq, pos0, emb_t, pos) -> np.ndarray:
    """x[r] = float32(emb_t[tok[r]] + pos[pos0 + r % Tq]) (emb_t already rounded to T)."""
    r = np.arange(len(tok))
    return (np.asarray(emb_t, np.float32)[np.asarray(tok)] + np.asarray(pos, np.float32)[pos0 + r % Tq]).astype(np.float32)


def finalize_ref(parts, state, *, B, n_tiles, n_vocab, eot, ignore_eot, forced, forced_len, done, out_cap, Tq, ctx, emb_t,
                 pos, fault: Optional[str] = None):
    """dec_finalize n_steps times on parts [n_steps][B][n_tiles][4] -> dict of everything the hook returns.
    Untouched outputs keep the hook's fill: -1 (int) and NaN (float; compared as 'still 0xFF')."""
    parts = np.asarray(parts, np.uint32)
    n_steps = parts.shape[0]
    pos0, step, epoch, arrive = (int(v) for v in state)
    d = emb_t.shape[1]
    done = np.array(done, np.int32).copy()
    out_tok = np.full((B, out_cap), -1, np.int32)
    top1 = np.full((B, out_cap), np.nan, np.float32)
    top2 = np.full((B, out_cap), np.nan, np.float32)
    nxt_all = np.zeros((n_steps, B), np.int32)
    x = np.zeros((n_steps, B, d), np.float32)
    for s in range(n_steps):
        for b in range(B):
            v1, i1, v2 = merge_parts(parts[s, b], fault)
            if i1 < 0 or i1 >= n_vocab:
                i1, v1, v2 = -2, np.float32(np.nan), np.float32(np.nan)
            nxt = eot
            if step < out_cap:
                if done[b]:
                    out_tok[b, step], top1[b, step], top2[b, step] = -1, -np.inf, -np.inf
                else:
                    out_tok[b, step], top1[b, step], top2[b, step] = i1, v1, v2
                    nxt = i1
                    if forced is not None and step < forced_len:
                        nxt = int(forced[b][step])
                    if not ignore_eot and i1 == eot:
                        done[b] = 1
                    if nxt < 0 or nxt >= n_vocab:
                        nxt = eot
            nxt_all[s, b] = nxt
            pn = min(pos0 + Tq, ctx if fault == "pos_clamp_at_ctx" else ctx - 1)
            x[s, b] = (np.asarray(emb_t, np.float32)[nxt] + np.asarray(pos, np.float32)[min(pn, ctx - 1)]
                       if pn < ctx else np.full(d, np.inf, np.float32))
        pos0, step, epoch = pos0 + Tq, step + 1, (epoch + 1) & 0xFFFFFFFF
    return dict(next_tok=nxt_all, x=x, out_tok=out_tok, out_top1=top1, out_top2=top2, done=done,
                state=np.array([pos0, step, epoch, 0], np.int64))
