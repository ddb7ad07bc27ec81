"""Crafted inputs of the block prefill's attention kernels for tests/test_prefill_ref.py (CPU:
the float64 reference and each case's sensitivity) and tests/test_gpu_prefill_attn.py (the kernels
against it), built with the helpers of tests/attn_cases.py as DESIGN 2c builds its scores: a code in
dimensions 1..nbits selects each query's peak key (4 log2 units per bit), seeded noise of about +-0.5 log2
units, |score| <= 64 log2 units on every key a query may see, V = +-(0.5 .. 1) with a sign pattern per key.

Self-attention, the keys a query must not see.  Key u > t has to score +100 for query t.  That step
pattern has one independent row per query, so 64 dimensions cannot hold it for every query of a prefix:
each head (b, h) carries it for the 32 queries of one 32-position block (a wave's queries, half a key
tile): the block `self_target` names, a different one per head, the last blocks of the prefix first; the
`-s4` / `-s8` / `-s12` cases repeat P = 225 and 448 with the targets moved down, so every block is one.  A
query t of that block holds A0 in dimension 27 + t % 32; a key u of the block holds 100 A0 in dimensions
27 .. 27 + u % 32 - 1, every later key in all 32, every earlier key in none.  So for those queries EVERY
key u > t scores +100 (and no key u <= t is touched); the other queries of the head see plain scores.

Bars (none taken from what a kernel gives): f32 4 x attn_ref.rel_bound_f32(chain = 66: the MFMA's 64
accumulations, the maximum's scale, the score's fused scale and shift) x max |v| over the visible keys;
bf16 / f16 that plus 3 u max |v|, u = 2^-9 / 2^-11 (P rounded before PV, the output's own rounding)."""
from __future__ import annotations

import functools

import numpy as np

from tests import attn_cases as K
from tests import attn_ref as R

H = K.H
CTX = 448
CHAIN = 66          # roundings on an f32 score in k_prefill.hip
PZ0, PZN = 27, 32   # the poison dimensions: one per query of a 32-position block
DT = K.DT

# every P the issue names, both sides of the wave (32 queries), key tile (64) and workgroup (128) edges up
# to two workgroups and a tile into the third, and the whole cache
SELF_P = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 159, 160, 161, 191, 192, 193, 224, 225,
          255, 256, 257, 321, 448)
CROSS_T = (1, 31, 32, 33, 255, 256, 257, 1500)
CROSS_P = (1, 5, 64, 65, 225)


def _self_cases():
    out = [dict(id=f"P{P}", P=P, B=2, big=False, shift=0) for P in SELF_P]
    # the four heads of a case carry the poison in its last four blocks: the same prefixes again with the
    # targets moved down by four, so that every 32-position block of P = 225 (8) and 448 (14) is one
    out += [dict(id=f"P{P}-s{s}", P=P, B=2, big=False, shift=s) for P, s in ((225, 4), (448, 4), (448, 8), (448, 12))]
    out.append(dict(id="P33-7e4", P=33, B=2, big=True, shift=0))  # f16 only: |k| and |v| entries of 7e4
    out.append(dict(id="P161-B3", P=161, B=3, big=False, shift=0))  # the batch invariance
    return out


SELF_CASES = _self_cases()
SELF_BY_ID = {c["id"]: c for c in SELF_CASES}


def self_target(P, b, h, shift=0):
    """The 32-position block whose queries carry the poison in head (b, h)."""
    nblk = -(-P // 32)
    return (nblk - 1 - (b * H + h) - shift) % nblk


@functools.lru_cache(maxsize=None)
def self_inputs(cid):
    """-> q, k, v [B][H][P][64] float32 (not yet rounded), peak [B][H][P]."""
    c = SELF_BY_ID[cid]
    P, B = c["P"], c["B"]
    nbits = int(CTX - 1).bit_length()
    q, k, v = (np.zeros((B, H, P, 64), np.float32) for _ in range(3))
    peak = np.zeros((B, H, P), np.int64)
    t = np.arange(P)
    for b in range(B):
        for h in range(H):
            edge = t // 32 * 32 - 1  # the key just below the query's 32-position block (every other one: its 64-key tile)
            kind = (b * H + h + t) % 3
            pk = np.where(kind == 0, t, np.where(kind == 1, 0, np.where(edge >= 0, edge, t)))
            qq, kk = K.qk(41000 + 100 * SELF_CASES.index(c) + 10 * b + h, pk, np.arange(P), nbits, 4.0)
            qq[:, PZ0:PZ0 + PZN] = 0.0
            kk[:, PZ0:PZ0 + PZN] = 0.0
            tb = self_target(P, b, h, c["shift"])
            for i in range(P):
                if i // 32 == tb:
                    qq[i, PZ0 + i % 32] = K.A0
                    kk[i, PZ0:PZ0 + i % 32] = K.POISON * K.A0
                elif i // 32 > tb:
                    kk[i, PZ0:PZ0 + PZN] = K.POISON * K.A0
            vv = K.values(b, h, P).astype(np.float64)
            if c["big"]:  # dimension 11 is zero in every query: the score does not see the entry, a product with Inf would
                kk[0, 11], kk[P - 1, 11] = 7e4, -7e4
                vv[0, 3], vv[0, 40] = 7e4, -7e4
            q[b, h], k[b, h], v[b, h], peak[b, h] = qq, kk, vv, pk
    return q, k, v, peak


def self_pack(q, k, v):
    """[B][H][P][64] x 3 -> qkv [B*P][3*H*64]."""
    return K.enc_pack(q, k, v)


def stored(x, dtype, clamp=True):
    """x rounded to dtype as the cache holds it: the f16 engine clamps to +-65504 (to_cache)."""
    r = R.round_dtype(x, dtype)
    if dtype == "f16" and clamp:
        r = np.clip(r, -65504.0, 65504.0)
    return r


def tol_of(qr, kr, vr, vis, dtype):
    """[.., nq, 1]: the f32 bar, plus the 16-bit terms."""
    vmax = R.vmax_visible(vr, vis)
    tol = 4.0 * R.rel_bound_f32(qr, kr, vis, chain=CHAIN) * vmax
    if dtype != "f32":
        tol = tol + 3.0 * R.U[dtype] * vmax
    return tol[..., None]


def _tiles_unweighted(qr, kr, vr, vis, tile=64):
    s = R.scores(qr, kr)
    n = kr.shape[-2]
    parts = []
    for t0 in range(0, n, tile):
        vv = None if vis is None else vis[..., t0:t0 + tile]
        parts.append(R.partial(s[..., t0:t0 + tile], vr[..., t0:t0 + tile, :], vv))
    return R.merge(parts, weighted=False)


SELF_FAULTS = ("admit_next", "drop_last", "unweighted", "unclamped")


def self_ref(cid, dtype, fault=None):
    """-> (out [B][H][P][64] float64, tol, rows [B][H][P] the fault targets)."""
    c = SELF_BY_ID[cid]
    q, k, v, peak = self_inputs(cid)
    P, B = c["P"], c["B"]
    with np.errstate(over="ignore"):
        qr = R.round_dtype(q, dtype)
        kr, vr = stored(k, dtype), stored(v, dtype)
    vis = R.causal(0, P, P)
    tol = tol_of(qr, kr, vr, vis, dtype)
    t = np.arange(P)
    rows = np.ones((B, H, P), bool)
    if fault is None:
        ref = R.attend(qr, kr, vr, vis)
    elif fault == "admit_next":  # the key one past the causal limit: the queries that carry the poison
        ref = R.attend(qr, kr, vr, R.causal(1, P, P))
        rows = np.zeros((B, H, P), bool)
        for b in range(B):
            for h in range(H):
                rows[b, h] = (t // 32 == self_target(P, b, h, c["shift"])) & (t + 1 < P)
    elif fault == "drop_last":  # the newest key dropped
        ref = R.attend(qr, kr, vr, R.causal(-1, P, P))
        rows = peak == t[None, None, :]
    elif fault == "unweighted":  # the 64-key tiles merged without their weights
        ref = _tiles_unweighted(qr, kr, vr, vis)
        rows = np.broadcast_to(t >= 64, (B, H, P)) & (peak < t // 64 * 64)  # the peak in an earlier tile than the newest
    elif fault == "unclamped":  # the f16 store without its clamp: Inf in the cache
        with np.errstate(over="ignore", invalid="ignore"):
            ref = R.attend(qr, stored(k, dtype, False), stored(v, dtype, False), vis)
        rows = np.broadcast_to(bool(c["big"]) and dtype == "f16", (B, H, P))
    else:
        raise ValueError(fault)
    return ref, np.broadcast_to(tol, ref.shape), rows


def self_faults(c, dtype):
    if c["big"]:  # max |v| = 65504 sets this case's bar: it is built for the clamp alone
        return ["unclamped"] if dtype == "f16" else []
    f = ["drop_last"]
    if c["P"] > 1:
        f.append("admit_next")
    if c["P"] > 64:
        f.append("unweighted")
    if c["big"] and dtype == "f16":
        f.append("unclamped")
    return f


# ------------------------------------------------------------------------------------------- cross
def cross_peaks(T):
    """Keys 0 and T - 1, then both sides of every 32-key block edge, the last edges first."""
    want = [0, T - 1]
    for e in range((T - 1) // 32 * 32, 0, -32):
        want += [e - 1, e]
    seen = []
    for p in want:
        if 0 <= p < T and p not in seen:
            seen.append(p)
    return seen


def _cross_cases():
    out = []
    for T in CROSS_T:
        for P in CROSS_P:
            out.append(dict(id=f"T{T}-P{P}", T=T, P=P, B=2, B_layout=3, b0=1, share=1, kvrow=None))
    for T in (257, 1500):
        out.append(dict(id=f"T{T}-P5-share5", T=T, P=5, B=10, B_layout=3, b0=0, share=5, kvrow=[2] * 5 + [0] * 5))
    out.append(dict(id="T257-P65-B3", T=257, P=65, B=3, B_layout=4, b0=1, share=1, kvrow=None))  # the batch invariance
    return out


CROSS_CASES = _cross_cases()
CROSS_BY_ID = {c["id"]: c for c in CROSS_CASES}


def cross_window(c, b):
    return c["b0"] + (b if c["kvrow"] is None else c["kvrow"][b // c["share"] * c["share"]])


@functools.lru_cache(maxsize=None)
def cross_inputs(cid):
    """-> q [B][H][P][64], k, v [B_layout][H][T][64] float32, peak [B][H][P]."""
    c = CROSS_BY_ID[cid]
    T, B, P, BL = c["T"], c["B"], c["P"], c["B_layout"]
    nbits = max(1, int(T - 1).bit_length())
    pk = cross_peaks(T)
    q = np.zeros((B, H, P, 64), np.float32)
    k, v = (np.zeros((BL, H, T, 64), np.float32) for _ in range(2))
    peak = np.zeros((B, H, P), np.int64)
    base = 60000 + 1000 * CROSS_CASES.index(c)
    for w in range(BL):
        for h in range(H):
            _, kk = K.qk(base + 10 * w + h, [0], np.arange(T), nbits, 4.0)
            k[w, h], v[w, h] = kk, K.values(w, h, T)
    n = 0
    for b in range(B):
        for t in range(P):
            for h in range(H):
                peak[b, h, t] = pk[n % len(pk)]
                n += 1
    for b in range(B):
        for h in range(H):
            qq, _ = K.qk(base + 500 + 10 * b + h, peak[b, h], [0], nbits, 4.0)
            qq[:, 63] = K.GUARD
            q[b, h] = qq
    return q, k, v, peak


def cross_ref(cid, dtype, fault=None):
    """-> (out [B][H][P][64] float64, tol, rows [B][H][P])."""
    c = CROSS_BY_ID[cid]
    q, k, v, peak = cross_inputs(cid)
    T, B = c["T"], c["B"]
    qr, kr, vr = (R.round_dtype(x, dtype) for x in (q, k, v))
    win = [cross_window(c, b) for b in range(B)]
    if fault == "wrong_window":  # kvrow[j * share] -> j
        win = [c["b0"] + b // c["share"] for b in range(B)]
    kw, vw = kr[win], vr[win]
    rows = np.ones(peak.shape, bool)
    tol = tol_of(qr, kr[[cross_window(c, b) for b in range(B)]], vr[[cross_window(c, b) for b in range(B)]], None, dtype)
    if fault is None:
        ref = R.attend(qr, kw, vw)
    elif fault == "wrong_window":
        ref = R.attend(qr, kw, vw)
        rows = np.broadcast_to((np.array(win) != [cross_window(c, b) for b in range(B)])[:, None, None], peak.shape)
    elif fault == "drop_last":
        ref = R.attend(qr, kw, vw, (np.arange(T) < T - 1)[None, :])
        rows = peak == T - 1
    elif fault == "admit_pad":
        n = -T % 32
        pad = np.full(kw.shape[:2] + (n, 64), K.PAD, np.float64)
        ref = R.attend(qr, np.concatenate([kw, pad], 2), np.concatenate([vw, pad], 2))
    elif fault == "unweighted":
        ref = _tiles_unweighted(qr, kw, vw, None)
        rows = np.broadcast_to(T > 64, peak.shape)
    else:
        raise ValueError(fault)
    return ref, np.broadcast_to(tol, ref.shape), rows


def cross_faults(c):
    f = ["drop_last"]
    if c["T"] % 32:
        f.append("admit_pad")
    if c["kvrow"] is not None:
        f.append("wrong_window")
    if c["T"] > 64:
        f.append("unweighted")
    return f
