"""Float64 reference of the decoder GEMV over a quantised matrix (spt_debug_qgemv), the crafted ggml
blocks it runs on, the cases of tests/test_gpu_qgemv.py and their error bars.  Shared by the GPU test
and by tests/test_qresident_ref.py (CPU: the same references recomputed with named faults).

Reference.  The weights are the file's blocks dequantised as ggml does (f32, each product and sum rounded
once) and rounded once to the engine dtype T; A_DIRECT activations are rounded to T; everything after
that is float64.  A LayerNorm source is normalised in float64 and its image rounded to T.

Bars (none is taken from what a kernel returns).  u32 = 2^-24, u_T = 2^-8 (bf16) or 2^-11 (f16).
  A_DIRECT   2 (K + 4) u32 S, S = sum_k |a_k w_k| (+ |bias| + |residual|: the two further f32 additions
             of the epilogue are two more terms of the same sum): K products exact in f32, at most K + 4
             roundings of partial sums in whatever order the MFMA, the wave split and the epilogue add them,
             each below u32 times the running magnitude <= S, doubled for the second-order terms and the
             reference's own rounding.
  A_LN       + 2 u_T sum_k |ln_k w_k|: the device normalises in f32, so an image element that lies within
             f32 error of a rounding boundary of T may round the other way than the float64 image does: one
             ulp_T = 2 u_T |ln_k| on that element.
  stored T   + half an ulp of T at the reference value (the one rounding of the store).
  GELU       the linear bar times 1.13 (the largest slope of GELU) + 2^-17 |g| (v_exp_f32 and v_rcp_f32 are
             good to an ulp; the exponent's argument, up to ~20 in size, carries 3 f32 roundings: 2.5e-6
             relative) + the store's half ulp.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np

Q4_1, Q5_0, Q5_1 = 3, 6, 7
BLOCK_BYTES = {Q4_1: 20, Q5_0: 22, Q5_1: 24}
HAS_M = {Q4_1: True, Q5_0: False, Q5_1: True}
Q5 = {Q4_1: False, Q5_0: True, Q5_1: True}
OFFSET = {Q4_1: 0, Q5_0: 16, Q5_1: 0}
FAULTS = ("nibbles_swapped", "qh_bit_j_for_j_plus_16", "offset_dropped", "m_dropped", "neighbour_scale")
U32 = 2.0 ** -24
U_T = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}


# ------------------------------------------------------------------------------------------ blocks
def make_blocks(t: int, codes: np.ndarray, d: np.ndarray, m: Optional[np.ndarray] = None) -> bytes:
    """ggml blocks from codes [nb][32] (0..31 for the 5-bit types, 0..15 for q4_1), scales d [nb] and
    minima m [nb] (f16 values)."""
    nb = codes.shape[0]
    codes = codes.astype(np.uint32)
    out = np.zeros((nb, BLOCK_BYTES[t]), np.uint8)
    off = 0
    out[:, 0:2] = np.asarray(d, np.float16).reshape(nb, 1).view(np.uint8)
    off = 2
    if HAS_M[t]:
        out[:, 2:4] = np.asarray(m, np.float16).reshape(nb, 1).view(np.uint8)
        off = 4
    if Q5[t]:
        qh = np.zeros(nb, np.uint32)
        for j in range(32):
            qh |= ((codes[:, j] >> 4) & 1) << j
        out[:, off:off + 4] = qh.astype("<u4").reshape(nb, 1).view(np.uint8)
        off += 4
    out[:, off:off + 16] = ((codes[:, :16] & 15) | ((codes[:, 16:] & 15) << 4)).astype(np.uint8)
    return out.tobytes()


def dequant(raw: bytes, t: int, fault: Optional[str] = None) -> np.ndarray:
    """ggml's dequantize_row of 32-element blocks in f32 (each product and sum rounded once), flat;
    fault: one of FAULTS, the mistakes an in-register dequantisation can make."""
    a = np.frombuffer(raw, np.uint8).reshape(-1, BLOCK_BYTES[t])
    nb = a.shape[0]
    d = a[:, 0:2].copy().view(np.float16).astype(np.float32).reshape(nb)
    off = 2
    m = np.zeros(nb, np.float32)
    if HAS_M[t]:
        m = a[:, 2:4].copy().view(np.float16).astype(np.float32).reshape(nb)
        off = 4
    qh = np.zeros(nb, np.uint32)
    if Q5[t]:
        qh = a[:, off:off + 4].copy().view("<u4").reshape(nb).astype(np.uint32)
        off += 4
    qs = a[:, off:off + 16]
    lo, hi = (qs & 15).astype(np.int32), (qs >> 4).astype(np.int32)
    if fault == "nibbles_swapped":
        lo, hi = hi, lo
    j = np.arange(16, dtype=np.uint32)
    if Q5[t]:
        lo = lo | ((((qh[:, None] >> j) & 1) << 4).astype(np.int32))
        hj = j if fault == "qh_bit_j_for_j_plus_16" else j + 16
        hi = hi | ((((qh[:, None] >> hj) & 1) << 4).astype(np.int32))
    x = np.concatenate([lo, hi], axis=1)
    sub = 0 if fault == "offset_dropped" else OFFSET[t]
    if fault == "neighbour_scale":
        d = np.roll(d, 1)
    v = ((x - sub).astype(np.float32) * d[:, None]).astype(np.float32)
    if HAS_M[t] and fault != "m_dropped":
        v = (v + m[:, None]).astype(np.float32)
    return v.reshape(-1)


def fault_applies(t: int, fault: str) -> bool:
    return {"offset_dropped": OFFSET[t] != 0, "m_dropped": HAS_M[t], "qh_bit_j_for_j_plus_16": Q5[t]}.get(fault, True)


# ------------------------------------------------------------------------------------------ rounding
def round_t(x: np.ndarray, dtype: str) -> np.ndarray:
    """f32 -> T -> f32, round to nearest even (finite values)."""
    x = np.asarray(x, np.float32)
    if dtype == "f16":
        return x.astype(np.float16).astype(np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def half_ulp_t(v: np.ndarray, dtype: str) -> np.ndarray:
    """half the spacing of T at |v| (float64)."""
    mant, emin = (7, -126) if dtype == "bf16" else (10, -14)
    e = np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** emin)))
    return 0.5 * 2.0 ** (e - mant)


# ------------------------------------------------------------------------------------------ cases
@dataclass(frozen=True)
class Case:
    mode: str
    a_src: str
    K: int
    N: int
    R: int
    ksplit: int = 1
    resid: bool = False

    @property
    def id(self):
        return f"{self.mode}-{self.a_src}-K{self.K}-N{self.N}-R{self.R}-ks{self.ksplit}{'-res' if self.resid else ''}"


# The smallest shapes at which each launch configuration exists (dec_gemv.h gemv_launch_rg): K = 128 one
# super-step; 384 tiny.en; 1024 the 8-wave shape (and 8 waves x 2 tiles at N >= 4096); 1280 the exact 10-wave
# shapes below and above N = 4096; 1536 the exact 12-wave shape; 5120 sixteen waves (ksplit 1) and the
# GV_PARTIAL slabs (ksplit 4).  N = 40 has a ragged last tile, 4112 = 4096 + 16; R = 1 / 5 / 17 / 33 take row
# groups 1 / 1 / 2 / 4 with masked rows.  The LayerNorm image bounds the rows at K = 1536 (31).  GV_QKV_CACHE
# needs N = 3 d with d a multiple of 64; GV_LOGITS runs N = 1000 (a ragged last tile of 8 columns).
CASES = (
    Case("bias", "ln", 128, 16, 1), Case("bias", "ln", 384, 40, 5), Case("bias", "ln", 1024, 40, 17),
    Case("bias", "ln", 1280, 40, 33), Case("bias", "ln", 1280, 4112, 5), Case("bias", "ln", 1536, 16, 17),
    Case("bias", "ln", 1024, 4112, 1),
    Case("bias_gelu", "ln", 1280, 4112, 5), Case("bias_gelu", "ln", 384, 40, 33),
    Case("qkv_cache", "ln", 128, 192, 1), Case("qkv_cache", "ln", 1280, 384, 17), Case("qkv_cache", "ln", 1536, 192, 5),
    Case("logits", "ln", 384, 1000, 5), Case("logits", "ln", 1280, 1000, 33), Case("logits", "ln", 1024, 1000, 1),
    Case("partial", "direct", 128, 16, 1), Case("partial", "direct", 1280, 40, 5),
    Case("partial", "direct", 1536, 40, 17), Case("partial", "direct", 5120, 40, 33),
    Case("partial", "direct", 5120, 16, 5, ksplit=4), Case("partial", "direct", 5120, 40, 1, ksplit=4),
    Case("partial", "direct", 1024, 40, 17, ksplit=2, resid=True),
    Case("bias_resid", "direct", 384, 40, 5, resid=True), Case("bias_resid", "direct", 1280, 4112, 17, resid=True),
    Case("bias_resid", "direct", 5120, 16, 33, resid=True), Case("bias_resid", "direct", 1536, 40, 1, resid=True),
)
TYPES = {"q5_0": Q5_0, "q4_1": Q4_1}   # the required types; q5_1 rides on one case of each pair
DTYPES = ("bf16", "f16")


@dataclass
class Inputs:
    blocks: bytes
    act: np.ndarray
    ln_w: Optional[np.ndarray]
    ln_b: Optional[np.ndarray]
    bias: np.ndarray
    resid: Optional[np.ndarray]


def make_inputs(c: Case, t: int, seed: int = 0) -> Inputs:
    """Random codes over the type's whole range; scales of both signs around 2^-6 with, in one block in
    eight, an f16 subnormal, 2^-14, 1 or 2 (|d| <= 2); minima of both signs.  Activations of order 1."""
    rng = np.random.default_rng([seed, c.K, c.N, c.R, t])
    nb = c.N * c.K // 32
    codes = rng.integers(0, 32 if Q5[t] else 16, (nb, 32), dtype=np.uint8)
    d = (rng.uniform(0.5, 1.5, nb) * 2.0 ** -6 * rng.choice([-1.0, 1.0], nb)).astype(np.float32)
    special = np.array([2.0 ** -24, -3 * 2.0 ** -24, 2.0 ** -14, -(2.0 ** -14), 1.0, -1.0, 2.0, -2.0], np.float32)
    pick = rng.integers(0, 8, nb) == 0
    d[pick] = special[rng.integers(0, 8, int(pick.sum()))]
    m = (rng.uniform(-1, 1, nb) * 2.0 ** -3).astype(np.float32)
    act = rng.standard_normal((c.R, c.K)).astype(np.float32)
    if c.a_src == "ln":
        act = (act * rng.uniform(0.5, 3.0, (c.R, 1)) + rng.uniform(-1, 1, (c.R, 1))).astype(np.float32)
    ln_w = ln_b = None
    if c.a_src == "ln":
        ln_w = rng.uniform(0.5, 1.5, c.K).astype(np.float32)
        ln_b = rng.uniform(-0.25, 0.25, c.K).astype(np.float32)
    _probes(c, t, rng, act, ln_w, ln_b, codes, d, m)
    blocks = make_blocks(t, codes, d, m)
    bias = rng.uniform(-0.5, 0.5, c.N).astype(np.float32)
    resid = rng.standard_normal((c.R, c.N)).astype(np.float32) if c.resid else None
    return Inputs(blocks, act, ln_w, ln_b, bias, resid)


def _probes(c, t, rng, act, ln_w, ln_b, codes, d, m):
    """Activation row 0 and weight rows 0..4, crafted so that each of FAULTS shows on output (0, n) far above
    any bar, whatever the signs of the random rest: a worst-case bar is a fraction of sum |a_k w_k|, which
    a fault that merely scrambles random weights does not exceed a hundredfold.

    Row 0 of the activations is one spike of +-4 per 32-element block over noise of 0.004 (signs alternate,
    so a LayerNorm keeps them): at position 3 (a low nibble) in even blocks, 21 (a high nibble) in odd ones.
    A probe row's weights are zero wherever the fault does not reach (code 16 of q5_0, code 0 with m = 0
    else); where it does, the true weight is zero or tiny at the spike and the faulted one is large there,
    with the scale's sign chosen so that the faulted products add up:
      row 0  nibbles swapped      the spike's partner (j +- 16) holds nibble 15, the spike nibble 0
      row 1  qh bit j for j + 16  odd blocks: the spike's own fifth bit and bit j of the low half differ
      row 2  offset dropped       q5_0: every code 16 (true weight 0, faulted 16 d)
      row 3  m dropped            8 d + m = 0 exactly with code 8 everywhere (faulted: 8 d = -m)
      row 4  neighbour's scale    odd blocks: code 15 at the spike under d = 2^-14, the block before it d = 1
    """
    nbr = c.K // 32
    b = np.arange(nbr)
    sp = np.where(b % 2 == 0, 3, 21)
    x0 = rng.standard_normal(c.K) * 0.004
    x0[32 * b + sp] = np.where((b // 2) % 2 == 0, 4.0, -4.0) * np.where(b % 2 == 0, 1.0, -1.0)
    act[0] = x0.astype(np.float32)
    a0 = act[0].astype(np.float64)
    if c.a_src == "ln":
        a0 = (a0 - a0.mean()) / np.sqrt(a0.var() + 1e-5) * ln_w + ln_b
    sgn = np.sign(a0[32 * b + sp]).astype(np.float32)
    tot = np.sign(a0.reshape(nbr, 32).sum(axis=1)).astype(np.float32)
    zero = 16 if t == Q5_0 else 0
    odd = b % 2 == 1

    def row(n):
        sl = slice(n * nbr, (n + 1) * nbr)
        codes[sl] = zero
        d[sl] = 0.125
        m[sl] = 0.0
        return codes[sl], d[sl], m[sl]

    cw, dw, _ = row(0)   # nibbles swapped
    cw[b, sp ^ 16] = zero | 15
    dw[:] = 0.125 * sgn
    cw, dw, _ = row(1)   # qh: only the 5-bit types (q4_1: a row of zeros)
    if t == Q5_0:        # spike: nibble 0 with its bit set (0); low partner: bit clear, nibble 15 (-d)
        cw[b[odd], sp[odd] ^ 16] = 15
        dw[:] = -0.125 * sgn
    elif t == Q5_1:      # spike: code 0; low partner: code 16
        cw[b[odd], sp[odd] ^ 16] = 16
        dw[:] = 0.125 * sgn
    cw, dw, _ = row(2)   # offset dropped (q5_0; the other types have none: zeros)
    dw[:] = 0.125 * tot
    cw, dw, mw = row(3)  # m dropped
    if HAS_M[t]:
        cw[:] = 8
        dw[:] = 0.125 * tot
        mw[:] = -1.0 * tot
    cw, dw, _ = row(4)   # neighbour's scale
    cw[b[odd], sp[odd]] = zero | 15
    dw[odd] = 2.0 ** -14 * sgn[odd]
    dw[~odd] = np.roll(sgn, -1)[~odd]


# ------------------------------------------------------------------------------------------ reference
def _gelu(x):
    return 0.5 * x * (1.0 + np.tanh(0.7978845608028654 * (x + 0.044715 * x ** 3)))


def reference(c: Case, inp: Inputs, t: int, dtype: str, fault: Optional[str] = None):
    """(ref, bar): float64 arrays of the hook's output shape."""
    w = round_t(dequant(inp.blocks, t, fault), dtype).astype(np.float64).reshape(c.N, c.K)
    if c.a_src == "direct":
        a = round_t(inp.act, dtype).astype(np.float64)
        img_bar = 0.0
    else:
        x = inp.act.astype(np.float64)
        mean = x.mean(axis=1, keepdims=True)
        var = ((x - mean) ** 2).mean(axis=1, keepdims=True)
        ln = (x - mean) / np.sqrt(var + 1e-5) * inp.ln_w.astype(np.float64) + inp.ln_b.astype(np.float64)
        a = round_t(ln.astype(np.float32), dtype).astype(np.float64)
        img_bar = 2.0 * U_T[dtype] * (np.abs(a) @ np.abs(w).T)
    bias = inp.bias.astype(np.float64)
    if c.mode == "partial":
        nss = c.K // 128
        per = -(-nss // c.ksplit)
        ref = np.zeros((c.ksplit, c.R, c.N))
        S = np.zeros((c.ksplit, c.R, c.N))
        for kz in range(c.ksplit):
            k0, k1 = min(kz * per, nss) * 128, min((kz + 1) * per, nss) * 128
            ref[kz] = a[:, k0:k1] @ w[:, k0:k1].T
            S[kz] = np.abs(a[:, k0:k1]) @ np.abs(w[:, k0:k1]).T
        ref[0] += bias
        S[0] += np.abs(bias)
        if inp.resid is not None:
            ref[0] += inp.resid
            S[0] += np.abs(inp.resid)
        return ref, 2.0 * (c.K + 4) * U32 * S
    y = a @ w.T
    S = np.abs(a) @ np.abs(w).T
    if c.mode != "logits":
        y = y + bias
        S = S + np.abs(bias)
    if c.mode == "bias_resid":
        y = y + inp.resid
        S = S + np.abs(inp.resid)
    lin = 2.0 * (c.K + 4) * U32 * S + img_bar
    if c.mode in ("logits", "bias_resid"):
        return y, lin
    if c.mode == "bias_gelu":
        g = _gelu(y)
        soft = 1.13 * lin + 2.0 ** -17 * np.abs(g)
        return g, soft + half_ulp_t(np.abs(g) + soft, dtype)
    return y, lin + half_ulp_t(np.abs(y) + lin, dtype)   # bias, qkv_cache: stored in T
