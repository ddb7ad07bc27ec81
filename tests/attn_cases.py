"""Crafted attention inputs for tests/test_attn_ref.py (CPU: the reference and each case's
sensitivity) and tests/test_gpu_attn.py (the kernels against the reference).

Scores are built, not drawn: of the 64 head dimensions, dimension 0 carries a per-key ladder (log2
units), dimensions 1..nbits a +-1 code of the key index whose match with the query's code selects that
query's peak key (w log2 units per bit: a key one bit away lies 2 w below the peak), dimensions 59..62
mark poisoned self-attention keys per query, dimension 63 makes the sum of every cross query's
elements positive (so a padded key holding pad_value in every element wins), and the rest is seeded
noise of about +-0.5 log2 units.  V is +-(0.5..1) with a sign pattern of its own per key (or per
64-key tile), so a wrong key shows in half of the 64 outputs.

Every case names the faults it is built for; fault=... recomputes the reference with that fault."""
from __future__ import annotations

import functools

import numpy as np

from tests import attn_ref as R

H = 2
A0 = (1.0 / R.C64) ** 0.5  # an element pair (A0 x, A0 y) adds x * y log2 units to a score
POISON = 100.0              # log2 units a poisoned key adds for the queries that must not see it
NOISE0 = 12                 # first noise dimension is max(NOISE0, nbits + 1)
DT = ("f32", "bf16", "f16")


def _u01(*idx) -> np.ndarray:
    """A deterministic hash of integer index arrays (broadcast) to [0, 1)."""
    x = np.zeros(np.broadcast(*idx).shape, np.uint64) + np.uint64(0x9E3779B97F4A7C15)
    for a in idx:
        x = (x ^ np.asarray(a).astype(np.uint64)) * np.uint64(0xBF58476D1CE4E5B9) & np.uint64(0xFFFFFFFFFFFFFFFF)
        x ^= x >> np.uint64(29)
    return ((x >> np.uint64(11)) % np.uint64(1 << 20)).astype(np.float64) / float(1 << 20)


def values(b, h, n, style="key", scale=1.0) -> np.ndarray:
    """V [n][64] of head (b, h): +-(0.5 .. 1), the pattern per key, per 64-key tile, or one pattern
    with the last key negated (`lastneg`, magnitude 1)."""
    j, e = np.arange(n)[:, None], np.arange(64)[None, :]
    g = j // 64 if style == "tile" else j * (style == "key")
    sign = np.where(_u01(g, e, b, h, 1) < 0.5, -1.0, 1.0)
    if style == "lastneg":
        sign = sign * np.where(j == n - 1, -1.0, 1.0)
        return (scale * sign).astype(np.float32)
    return (scale * sign * (0.5 + 0.5 * _u01(g, e, b, h, 2))).astype(np.float32)


def code_rows(code, nbits, w) -> np.ndarray:
    """[n][nbits]: +-sqrt(w / c) by the bits of code."""
    bits = (np.asarray(code)[:, None] >> np.arange(nbits)[None, :]) & 1
    return (2.0 * bits - 1.0) * (w ** 0.5) * A0


def qk(seed, peak_code, key_code, nbits, w, ladder=None, qmul=None, noise=0.45):
    """q [nq][64], k [nk][64] (float64) with score(i, j) = qmul[i] ladder[j] + w (matching - differing
    bits of peak_code[i], key_code[j]) + noise, in log2 units."""
    nq, nk = len(peak_code), len(key_code)
    rng = np.random.default_rng(seed)
    q, k = np.zeros((nq, 64)), np.zeros((nk, 64))
    n0 = max(NOISE0, nbits + 1)
    q[:, n0:59] = rng.normal(0, noise, (nq, 59 - n0))
    k[:, n0:59] = rng.normal(0, noise, (nk, 59 - n0))
    q[:, 0] = A0 * (1.0 if qmul is None else np.asarray(qmul, np.float64))
    k[:, 0] = A0 * (0.0 if ladder is None else np.asarray(ladder, np.float64))
    q[:, 1:1 + nbits] = code_rows(peak_code, nbits, w)
    k[:, 1:1 + nbits] = code_rows(key_code, nbits, w)
    return q, k


def diff(a, b) -> np.ndarray:
    """|a - b| per element; a NaN (no key left) differs by inf."""
    d = np.abs(a - b)
    return np.where(np.isnan(d), np.inf, d)


# ---------------------------------------------------------------------------------------- encoder
ENC_T = (1, 28, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1500)


def _enc_cases():
    out = []
    for T in ENC_T:
        out.append(dict(id=f"peaks-T{T}", T=T, B=2 if T < 1500 else 3, kind="peaks", faults=("drop_last",)))
    # ladders over 64-key tiles, centred so that |score| stays within 64 log2 units
    out += [
        dict(id="ladder+11.5", T=257, B=2, kind="ladder", step=11.5, faults=("unweighted",)),
        dict(id="ladder+12.5", T=257, B=2, kind="ladder", step=12.5, faults=("unweighted",)),
        dict(id="stairs5.9", T=700, B=2, kind="ladder", step=5.9, faults=("unweighted",)),
        dict(id="tile+6.5", T=300, B=2, kind="tile", lift=6.5, faults=("unweighted",)),
        dict(id="tile+7.5", T=300, B=2, kind="tile", lift=7.5, faults=("unweighted",)),
        dict(id="descend20", T=255, B=2, kind="ladder", step=-20.0, faults=("unweighted",)),
        dict(id="equal", T=28, B=2, kind="equal", faults=("admit_pad",)),
        dict(id="-60+60", T=128, B=2, kind="jump", faults=("unweighted",)),
        # rising for even queries, falling for odd ones: a wave re-bases for its rising lanes while
        # the tile maximum of its falling lanes lies below their running maximum (delta = max(0, .))
        dict(id="mixed+-12.5", T=257, B=2, kind="ladder", step=12.5, mixed=True, faults=("unweighted",)),
    ]
    return out


ENC_CASES = _enc_cases()


@functools.lru_cache(maxsize=None)
def enc_inputs(cid):
    """-> q, k, v [B][H][T][64] float32 (not yet rounded), peak [B][H][T] (or None)."""
    c = next(x for x in ENC_CASES if x["id"] == cid)
    T, B, kind = c["T"], c["B"], c["kind"]
    q, k, v = (np.zeros((B, H, T, 64), np.float32) for _ in range(3))
    peak = np.zeros((B, H, T), np.int64)
    tile = np.arange(T) // 64
    ntile = int(tile[-1]) + 1
    for b in range(B):
        for h in range(H):
            seed = 1000 * ENC_CASES.index(c) + 10 * b + h
            i = np.arange(T)
            if kind == "peaks":
                # (7 i + 3) mod T: every position of a 64-key tile, both lane halves; then the edges
                pk = (7 * i + 3 + 5 * (b * H + h)) % T
                for n, key in enumerate((0, T - 1, 63, 64)):
                    if key < T and n < T and b * H + h > 0:  # head (0, 0) keeps the plain sequence
                        pk[(n + b * H + h) % T] = key
                nbits = max(1, int(T - 1).bit_length())
                qq, kk = qk(seed, pk, np.arange(T), nbits, 4.0)
                vv = values(b, h, T)
            elif kind == "ladder":
                # one peak per tile (the code is the key's position in its tile) at the ladder's height
                pk = (7 * i + 3 + 5 * (b * H + h)) % 64
                lad = c["step"] * (tile - (ntile - 1) / 2.0)
                qmul = np.where(i % 2 == 1, -1.0, 1.0) if c.get("mixed") else None
                qq, kk = qk(seed, pk, np.arange(T) % 64, 6, 4.0, lad, qmul, 0.1)
                pk = None
                vv = values(b, h, T)
            elif kind == "tile":  # every key of tile 2 lifted, no code: 32 keys per lane at 2^lift
                pk = None
                qq, kk = qk(seed, np.zeros(T, int), np.zeros(T, int), 0, 0.0, c["lift"] * (tile == 2), None, 0.0)
                vv = values(b, h, T, "tile")
            elif kind == "jump":
                pk = None
                qq, kk = qk(seed, np.zeros(T, int), np.zeros(T, int), 0, 0.0, np.where(tile == 0, -60.0, 60.0), None, 0.0)
                vv = values(b, h, T, "tile")
            else:  # equal: q . k = 0 everywhere, the output is the mean of V
                pk = None
                qq, kk = qk(seed, np.zeros(T, int), np.zeros(T, int), 0, 0.0, None, np.zeros(T), 0.0)
                vv = values(b, h, T, "lastneg")
            q[b, h], k[b, h], v[b, h] = qq, kk, vv
            if pk is not None:
                peak[b, h] = pk
    return q, k, v, (peak if kind == "peaks" else None)


def enc_pack(q, k, v) -> np.ndarray:
    """[B][H][T][64] x 3 -> qkv [B*T][3*H*64] (q | k | v, head h at h*64)."""
    B, Hh, T, _ = q.shape
    rows = [np.transpose(x, (0, 2, 1, 3)).reshape(B * T, Hh * 64) for x in (q, k, v)]
    return np.ascontiguousarray(np.concatenate(rows, 1), np.float32)


def enc_unpack(out, B, T) -> np.ndarray:
    """out [B*T][H*64] -> [B][H][T][64]."""
    return np.transpose(np.asarray(out).reshape(B, T, H, 64), (0, 2, 1, 3))


def enc_ref(cid, dtype, sum4=True, fault=None):
    """-> (out [B][H][T][64] float64, tol broadcastable to it, rows: bool [B][H][T] the fault targets)."""
    q, k, v, peak = enc_inputs(cid)
    B, _, T, _ = q.shape
    qr, kr, vr = (R.round_dtype(x, dtype) for x in (q, k, v))
    pre = dtype != "f32" and sum4
    if pre:
        qr = R.scale_q(qr, dtype)
    rows = np.ones((B, H, T), bool)
    if fault is None:
        out = R.attend(qr, kr, vr, None, pre)
    elif fault == "drop_last":
        out = R.attend(qr, kr, vr, (np.arange(T) < T - 1)[None, :], pre)
        rows = peak == T - 1
    elif fault == "admit_pad":  # the tail tile's padded keys: the staging clamps them to key T - 1
        n = -T % 64
        kp = np.concatenate([kr, np.repeat(kr[:, :, -1:], n, 2)], 2)
        vp = np.concatenate([vr, np.repeat(vr[:, :, -1:], n, 2)], 2)
        out = R.attend(qr, kp, vp, None, pre)
    elif fault == "unweighted":  # the 64-key tiles merged without their weights
        s = R.scores(qr, kr, pre)
        parts = [R.partial(s[..., t0:t0 + 64], vr[..., t0:t0 + 64, :]) for t0 in range(0, T, 64)]
        out = R.merge(parts, weighted=False)
    else:
        raise ValueError(fault)
    vmax = np.abs(vr).max((2, 3))[:, :, None, None]
    if dtype == "f32":
        tol = 4.0 * R.rel_bound_f32(qr, kr, None, chain=66)[..., None] * vmax
    else:
        tol = 3.0 * R.U[dtype] * vmax
    return out, np.broadcast_to(tol, out.shape), rows


# ---------------------------------------------------------------------------- decoder self-attention
def _self_cases():
    out = []
    for pos0 in (0, 1, 30, 31, 32, 33, 254, 255, 256, 257, 446, 447):
        out.append(dict(ctx=448, Tq=1, pos0=pos0))
    for Tq in (2, 3, 4):
        # limits straddling a 32-key block edge and the 8-wave stride (256 keys); 13..16: the f32
        # prompt kernel's 16-key blocks
        for pos0 in (0, 29, 30, 253, 444, 13, 14, 15, 16):
            out.append(dict(ctx=448, Tq=Tq, pos0=pos0))
    out.append(dict(ctx=1024, Tq=1, pos0=1000))  # more than MAXB blocks per wave: the rolled loop
    out.append(dict(ctx=1024, Tq=3, pos0=1000))
    for c in out:
        c["B"] = 3 if c["Tq"] == 1 else 2
        c["id"] = f"ctx{c['ctx']}-Tq{c['Tq']}-pos{c['pos0']}"
    return out


SELF_CASES = _self_cases()


@functools.lru_cache(maxsize=None)
def self_inputs(cid):
    """-> q [B][H][Tq][64], cache k, v [B][H][ctx][64] float32, peak [B][H][Tq].
    Key pos0 + u (u >= 1) carries POISON for the queries t < u of the pass; the rows from pos0 + Tq up
    carry it for all of them, with V = +-1e4."""
    c = next(x for x in SELF_CASES if x["id"] == cid)
    B, ctx, Tq, pos0 = c["B"], c["ctx"], c["Tq"], c["pos0"]
    nbits = int(ctx - 1).bit_length()
    q = np.zeros((B, H, Tq, 64), np.float32)
    k, v = (np.zeros((B, H, ctx, 64), np.float32) for _ in range(2))
    peak = np.zeros((B, H, Tq), np.int64)
    for b in range(B):
        for h in range(H):
            for t in range(Tq):
                newest = pos0 + t
                edge = newest // 32 * 32 - 1  # the key just below the newest key's block
                peak[b, h, t] = (newest, 0, edge if edge >= 0 else newest)[(b * H + h + t) % 3]
            qq, kk = qk(7000 + 100 * SELF_CASES.index(c) + 10 * b + h, peak[b, h], np.arange(ctx), nbits, 4.0)
            vv = values(b, h, ctx).astype(np.float64)
            for t in range(Tq):
                qq[t, 59 + t] = A0
            for key in range(pos0 + 1, ctx):
                kk[key, 59:59 + min(key - pos0, 4)] = POISON * A0
            kk[pos0 + Tq:, 1:1 + nbits] = 0.0
            vv[pos0 + Tq:] = values(b, h, ctx - pos0 - Tq, "key", 1e4)
            q[b, h], k[b, h], v[b, h] = qq, kk, vv
    return q, k, v, peak


def rows_pack(q) -> np.ndarray:
    """q [B][H][Tq][64] -> [B*Tq][H*64]."""
    B, Hh, Tq, _ = q.shape
    return np.ascontiguousarray(np.transpose(q, (0, 2, 1, 3)).reshape(B * Tq, Hh * 64), np.float32)


def rows_unpack(out, B, Tq) -> np.ndarray:
    return np.transpose(np.asarray(out).reshape(B, Tq, H, 64), (0, 2, 1, 3))


def dec_tol(qr, kr, vr, vis, ref, dtype) -> np.ndarray:
    """4 x the f32 linear bound x max |v| over the visible keys (+ half an ulp of a 16-bit output)."""
    tol = 4.0 * R.rel_bound_f32(qr, kr, vis)[..., None] * R.vmax_visible(vr, vis)[..., None]
    return tol + R.half_ulp(ref, dtype)


def self_ref(cid, dtype, fault=None):
    """-> (out [B][H][Tq][64], tol, rows [B][H][Tq])."""
    c = next(x for x in SELF_CASES if x["id"] == cid)
    q, k, v, peak = self_inputs(cid)
    qr, kr, vr = (R.round_dtype(x, dtype) for x in (q, k, v))
    ctx, Tq, pos0 = c["ctx"], c["Tq"], c["pos0"]
    vis = R.causal(pos0, Tq, ctx)
    ref = R.attend(qr, kr, vr, vis)
    tol = dec_tol(qr, kr, vr, vis, ref, dtype)
    rows = np.ones(peak.shape, bool)
    if fault == "admit_next":  # one key past the limit (the last position of the cache has none)
        lim = pos0 + np.arange(Tq) + 1
        rows = np.broadcast_to(lim < ctx, peak.shape)
        ref = R.attend(qr, kr, vr, np.arange(ctx)[None, :] < np.minimum(lim + 1, ctx)[:, None])
    elif fault == "drop_last":
        ref = R.attend(qr, kr, vr, R.causal(pos0 - 1, Tq, ctx))
        rows = peak == (pos0 + np.arange(Tq))[None, None, :]
    elif fault == "poison":  # every row of the cache read
        ref = R.attend(qr, kr, vr, None)
        rows = np.broadcast_to((pos0 + np.arange(Tq) + 1) < ctx, peak.shape)
    elif fault is not None:
        raise ValueError(fault)
    return ref, tol, rows


SELF_FAULTS = ("admit_next", "drop_last", "poison")


# --------------------------------------------------------------------------- decoder cross-attention
CROSS_T = (1, 31, 32, 33, 255, 256, 257, 1500, 1536, 1600)
PAD = 32.0    # pad_value: K and V of the padded keys; with sum(q) >= 16 the padded score is >= 92
GUARD = 80.0  # dimension 63 of every cross query (the keys hold 0 there)


def cross_peaks(T):
    """Peak keys for T_enc: the ends, 31 / 32, 255 / 256 and both sides of every chunk edge
    cdiv(nblk, S) * kb for S = 2, 3, 4, with the step kernels' 32-key blocks and the f32 prompt
    kernels' 16-key blocks (key_block)."""
    want = [0, T - 1, 31, 32, 255, 256]
    for kb in (32, 16):
        nblk = -(-T // kb)
        for S in (2, 3, 4):
            per = -(-nblk // S)
            for s in range(1, S):
                want += [s * per * kb - 1, s * per * kb]
    seen = []
    for p in want:
        if 0 <= p < T and p not in seen:
            seen.append(p)
    return seen


def _cross_cases():
    out = []
    for T in CROSS_T:
        # one token per row, and four tokens per row (the prompt kernels), with at least as many
        # (row, head, token) slots as cross_peaks(T) has keys; windows 1.. of a layout with one more,
        # so the b index and b0 matter
        n = len(cross_peaks(T))
        B1, B4 = max(8, -(-n // H)), max(2, -(-n // (4 * H)))
        out.append(dict(id=f"T{T}-Tq1", T=T, B=B1, Tq=1, B_layout=B1 + 1, b0=1, share=1, kvrow=None))
        out.append(dict(id=f"T{T}-Tq4", T=T, B=B4, Tq=4, B_layout=B4 + 1, b0=1, share=1, kvrow=None))
    for T in (257, 1500):
        out.append(dict(id=f"T{T}-share5", T=T, B=10, Tq=1, B_layout=3, b0=0, share=5, kvrow=[2] * 5 + [0] * 5))
        out.append(dict(id=f"T{T}-share8", T=T, B=16, Tq=1, B_layout=3, b0=0, share=8, kvrow=[1] * 8 + [2] * 8))
        out.append(dict(id=f"T{T}-share2-Tq3", T=T, B=4, Tq=3, B_layout=3, b0=0, share=2, kvrow=[1, 1, 0, 0]))
    return out


CROSS_CASES = _cross_cases()
CROSS_BY_ID = {c["id"]: c for c in CROSS_CASES}


def cross_window(c, b) -> int:
    return c["b0"] + (b if c["kvrow"] is None else c["kvrow"][b // c["share"] * c["share"]])


@functools.lru_cache(maxsize=None)
def cross_inputs(cid):
    """-> q [B][H][Tq][64], k, v [B_layout][H][T][64] float32, peak [B][H][Tq]."""
    c = CROSS_BY_ID[cid]
    T, B, Tq, BL = c["T"], c["B"], c["Tq"], c["B_layout"]
    nbits = max(1, int(T - 1).bit_length())
    pk = cross_peaks(T)
    q = np.zeros((B, H, Tq, 64), np.float32)
    k, v = (np.zeros((BL, H, T, 64), np.float32) for _ in range(2))
    peak = np.zeros((B, H, Tq), np.int64)
    base = 20000 + 1000 * CROSS_CASES.index(c)
    for w in range(BL):
        for h in range(H):
            _, kk = qk(base + 10 * w + h, [0], np.arange(T), nbits, 4.0)
            k[w, h], v[w, h] = kk, values(w, h, T)
    n = 0
    for b in range(B):
        for t in range(Tq):
            for h in range(H):  # each row (and head) peaks at a different key
                peak[b, h, t] = pk[n % len(pk)]
                n += 1
    for b in range(B):
        for h in range(H):
            qq, _ = qk(base + 500 + 10 * b + h, peak[b, h], [0], nbits, 4.0)
            qq[:, 63] = GUARD
            q[b, h] = qq
    return q, k, v, peak


def key_block(dtype, Tq) -> int:
    """Keys per block of the cross kernels: 32, or 16 for the f32 prompt kernels (Tq > 1)."""
    return 16 if dtype == "f32" and Tq > 1 else 32


def chunk_edges(T, S, kb=32):
    """Key ranges of the S chunks of dec_cross_attn's splits (whole kb-key blocks, cdiv(nblk, S) each)."""
    nblk = -(-T // kb)
    per = -(-nblk // S)
    return [(min(s * per * kb, T), min((s + 1) * per * kb, T)) for s in range(S)]


def wave_keys(T, w, kb=32):
    """The keys wave w of 8 takes: blocks w, w + 8, .. of kb keys."""
    j = np.arange(T)
    return (j // kb) % 8 == w


def cross_ref(cid, dtype, fault=None, splits=1):
    """-> (out [B][H][Tq][64], tol, rows [B][H][Tq], parts): parts is the reference's partials
    [(o, m, l)] per chunk (splits > 1), else None."""
    c = CROSS_BY_ID[cid]
    q, k, v, peak = cross_inputs(cid)
    T, B = c["T"], c["B"]
    qr, kr, vr = (R.round_dtype(x, dtype) for x in (q, k, v))
    win = [cross_window(c, b) for b in range(B)]
    if fault == "wrong_window":  # kvrow[j * share] -> j
        win = [c["b0"] + b // c["share"] for b in range(B)]
    kw, vw = kr[win], vr[win]  # [B][H][T][64]
    rows = np.ones(peak.shape, bool)
    ref = R.attend(qr, kw, vw)
    tol = dec_tol(qr, kw, vw, None, ref, dtype)
    if fault is None or fault == "wrong_window":
        if fault:
            rows = np.broadcast_to((np.array(win) != [cross_window(c, b) for b in range(B)])[:, None, None], peak.shape)
    elif fault == "drop_last":
        ref = R.attend(qr, kw, vw, (np.arange(T) < T - 1)[None, :])
        rows = peak == T - 1
    elif fault == "admit_pad":
        n = -T % 32
        pad = np.full(kw.shape[:2] + (n, 64), PAD, np.float64)
        ref = R.attend(qr, np.concatenate([kw, pad], 2), np.concatenate([vw, pad], 2))
    elif fault == "neighbour_block":  # the peak's 32-key block read from the next block (or the previous)
        ref = np.array(ref)
        nblk = -(-T // 32)
        for idx in np.ndindex(peak.shape if nblk > 1 else (0, 0, 0)):
            b, h, t = idx
            blk = peak[idx] // 32
            other = blk + 1 if blk + 1 < nblk else blk - 1
            j = np.arange(T)
            src = np.where(j // 32 == blk, np.minimum(j + 32 * (other - blk), T - 1), j)
            ref[b, h, t] = R.attend(qr[b, h, t:t + 1], kw[b, h][src], vw[b, h][src])[0]
        rows = np.broadcast_to(nblk > 1, peak.shape)
    elif fault == "unweighted":
        s = R.scores(qr, kw)
        ref = R.merge([R.partial(s[..., a:e], vw[..., a:e, :]) for a, e in chunk_edges(T, splits)], weighted=False)
        # rows whose peak chunk is not alone in holding keys
        rows = np.broadcast_to(sum(e > a for a, e in chunk_edges(T, splits)) > 1, peak.shape)
    else:
        raise ValueError(fault)
    parts = None
    if splits > 1 and fault is None:
        s = R.scores(qr, kw)
        parts = [R.partial(s[..., a:e], vw[..., a:e, :]) for a, e in chunk_edges(T, splits, key_block(dtype, c["Tq"]))]
    return ref, tol, rows, parts


def cross_faults(c):
    f = ["drop_last", "neighbour_block"]
    if c["T"] % 32:
        f.append("admit_pad")
    if c["kvrow"] is not None:
        f.append("wrong_window")
    return f


def part_merge(part) -> np.ndarray:
    """The float64 merge of a partial buffer [R][H][S][66] -> [R][H][64]."""
    p = np.asarray(part, np.float64)
    return R.merge([(p[:, :, s, :64], p[:, :, s, 64], p[:, :, s, 65]) for s in range(p.shape[2])])
