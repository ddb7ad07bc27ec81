"""Crafted inputs of the Parakeet encoder kernels and of the TDT decode step for tests/test_pk_ref.py (CPU: the
reference, each case's preconditions and sensitivity) and tests/test_gpu_pk_kernels.py (the kernels against
the reference).  Every case names the faults it is built for.

Attention scores are built, not drawn (as tests/attn_cases.py does for Whisper).  Of a head's dk dimensions,
the first nA carry a +-a code of the key index in k and of the query's peak key in (q + u); the next nB a code
of the relative index r in the position rows and of the query's target r = Tp - 1 - i + peak in (q + v); k is
zero in the position dimensions and p in the key dimensions, so the two terms do not mix.  a^2 / sqrt(dk) =
4 ln 2: a key one bit away lies 8 log2 units below the peak.  Dimension dk - 1 makes every key row j >= T3
score +100 for every query (its V is +-1e4), dimension dk - 2 does the same for the position rows no live
(i, j) pair uses; these decoys are finite, not NaN: the MFMA kernel multiplies a masked key's V by a zero
probability and reads clamped position rows into lanes it masks afterwards, and the engine's padded rows are
finite too.  The rest is noise of +-0.3.  V is +-(0.5 .. 1) with a sign pattern per key."""
from __future__ import annotations

import functools
import math

import numpy as np

from tests.attn_cases import _u01

H = 2
W_BIT = 4.0 * math.log(2.0)    # natural units per matching code bit
DECOY = 100.0                  # natural units a decoy row adds to a score
QC = 4.0                       # (q + u)[dk - 1] and (q + v)[dk - 2]
DT = ("f32", "bf16", "f16")
# (kernel, dtype, head dim): the VALU kernel in every dtype, the two MFMA instantiations, and head dims
# neither MFMA kernel takes
ATTN_KERNELS = (("valu", "f32", 64), ("valu", "bf16", 64), ("valu", "f16", 64), ("mfma", "f16", 64),
                ("mfma", "f16", 128), ("valu", "f32", 40), ("valu", "f16", 72), ("valu", "bf16", 40))
EDGES = (0, 31, 32, 63, 64, 95, 96)


def _attn_cases():
    shapes = [dict(sid=f"tight-T{t}", Tp=t, lens=(t, t)) for t in (1, 32, 33, 64, 97)]
    shapes += [dict(sid=f"pad-T{t}", Tp=t + 40, lens=(t, t)) for t in (0, 1, 31, 32, 33, 63, 64, 65, 97)]
    shapes += [dict(sid="ragged-Tp97", Tp=97, lens=(97, 33, 1, 0)), dict(sid="ragged-Tp137", Tp=137, lens=(97, 33, 1, 0))]
    geometry = ("skew+1", "skew-1", "drop_last", "admit_one", "read_pad", "lens_col")
    out = []
    for s in shapes:
        wide = s["Tp"] > max(s["lens"])
        f = geometry + (("p_col0",) if wide else ("clamp_early",)) + ("swap_uv",)
        out.append(dict(s, id=s["sid"] + "-bd", family="bd", wide=wide, faults=f))
        if s["sid"] in ("tight-T64", "tight-T97", "pad-T31", "pad-T65", "pad-T97", "ragged-Tp97", "ragged-Tp137"):
            out.append(dict(s, id=s["sid"] + "-ac", family="ac", wide=wide,
                            faults=("drop_last", "admit_one", "read_pad", "swap_uv", "lens_col")))
            out.append(dict(s, id=s["sid"] + "-mix", family="mix", wide=wide, faults=geometry + ("swap_uv",)))
        if s["sid"] in ("tight-T97", "pad-T65", "ragged-Tp137"):
            out.append(dict(s, id=s["sid"] + "-soft", family="soft", wide=wide, faults=("no_scale", "swap_uv", "skew+1")))
    out.append(dict(sid="pad-T33", id="pad-T33-equal", Tp=73, lens=(33, 33), family="equal", wide=True,
                    faults=("admit_one", "read_pad")))
    # per-utterance position tables (the int8 mode's), f32 only
    for s in (dict(sid="pad-T33", Tp=73, lens=(33, 33)), dict(sid="ragged-Tp137", Tp=137, lens=(97, 33, 1, 0))):
        out.append(dict(s, id=s["sid"] + "-bstride", family="bd", wide=True, bstride=True, f32_only=True,
                        faults=("p_shared", "p_col0", "skew+1", "skew-1")))
    return out


ATTN_CASES = _attn_cases()


def attn_case(cid):
    return next(c for c in ATTN_CASES if c["id"] == cid)


def attn_kernels(c):
    return tuple(k for k in ATTN_KERNELS if not c.get("f32_only") or k[:2] == ("valu", "f32"))


def peaks(g, T3):
    """The peak key of each query of head g = b H + h: (7 i + 3 + 5 g) mod T3, and at the ends of every
    32-query tile (l32 = 0 and 31: the skew rows 31 +- 31) the keys on both sides of every 32-key tile edge,
    key 0 and key T3 - 1; head 0 holds the extreme relative positions (i, j) = (0, T3 - 1) and (T3 - 1, 0)."""
    i = np.arange(T3)
    pk = (7 * i + 3 + 5 * g) % max(T3, 1)
    eq = [e for e in EDGES + (T3 - 1,) if 0 <= e < T3]
    ek = [e for e in (0, T3 - 1) + EDGES[1:] if 0 <= e < T3]
    ek = list(dict.fromkeys(ek))
    for m, qi in enumerate(dict.fromkeys(eq)):
        pk[qi] = ek[(m + g) % len(ek)]
    if T3 and g % 2 == 0:
        pk[0], pk[T3 - 1] = T3 - 1, 0
    return pk


def _bits(code, n):
    return 2.0 * ((np.asarray(code)[:, None] >> np.arange(n)[None, :]) & 1) - 1.0


def _noise(shape, *key, amp=0.1):
    idx = np.indices(shape)
    return amp * (2.0 * _u01(*idx, *key) - 1.0)


@functools.lru_cache(maxsize=None)
def attn_inputs(cid, dk):
    """-> dict(qkv f32 [B * Tp][3 d], p f32 flat, pu, pv f32 [H][dk], lens int32 [B][4], B, Tp, H, dk, ldp, p_off,
    p_bstride, peak [B][H][Tp] (-1: none)), not yet rounded to a dtype."""
    c = attn_case(cid)
    Tp, lens3, fam = c["Tp"], c["lens"], c["family"]
    B, d, nr = len(lens3), H * dk, 2 * Tp - 1
    a = math.sqrt(W_BIT * math.sqrt(dk))
    if fam == "soft":
        a *= 0.25
    nbr = max(1, (nr - 1).bit_length())
    nbk = max(1, (Tp - 1).bit_length())
    nA, nB = {"bd": (0, nbr), "ac": (nbk, 0), "mix": (max(1, nbk - 3), 3), "soft": (max(1, nbk - 3), 3),
              "equal": (0, 0)}[fam]
    DK_, DP_ = dk - 1, dk - 2
    assert nA + nB <= dk - 2
    wide, bstride = c["wide"], bool(c.get("bstride"))
    ldp, p_off = (3 * d, d) if wide else (d, 0)
    nt = B if bstride else 1
    p_bstride = nr * ldp if bstride else 0
    seed = ATTN_CASES.index(c)

    def kcode(j):
        return j if fam == "ac" else j // 8

    def rcode(r, b):
        r = (r + 3 * b) % nr if bstride else r
        return r if fam == "bd" else r % 8

    e = np.arange(dk)
    pu = np.where(_u01(e[None, :], np.arange(H)[:, None], 11) < 0.5, -1.0, 1.0) * (1.0 + _u01(e[None, :], np.arange(H)[:, None], 12))
    pv = np.where(_u01(e[None, :], np.arange(H)[:, None], 13) < 0.5, -1.0, 1.0) * (1.0 + _u01(e[None, :], np.arange(H)[:, None], 14))
    qkv = np.zeros((B, Tp, 3, H, dk))
    P = np.zeros((nt, nr, ldp))
    peak = np.full((B, H, Tp), -1, np.int64)
    Tmax = max(lens3)
    for t in range(nt):
        live_r = np.zeros(nr, bool)
        Tt = lens3[t] if bstride else Tmax
        if Tt:
            live_r[Tp - Tt:Tp - 1 + Tt] = True
        for h in range(H):
            row = np.zeros((nr, dk))
            if fam != "equal":
                row[:, nA + nB:DP_] = _noise((nr, DP_ - nA - nB), seed, t, h, 3)
                if nB:
                    row[:, nA:nA + nB] = a * _bits(rcode(np.arange(nr), t), nB)
            row[~live_r] = 0.0 if fam == "equal" else row[~live_r]
            row[:, DP_] = np.where(live_r, 0.0, DECOY * math.sqrt(dk) / QC)
            row[:, DK_] = 0.0
            P[t, :, p_off + h * dk:p_off + (h + 1) * dk] = row
            if wide:  # the columns beside the slice: the code of the next relative index, twice as strong
                dec = np.zeros((nr, dk))
                if nB:
                    dec[:, nA:nA + nB] = 2 * a * _bits(rcode((np.arange(nr) + 1) % nr, t), nB)
                dec[:, DP_] = 25.0
                P[t, :, h * dk:(h + 1) * dk] = dec
                P[t, :, 2 * d + h * dk:2 * d + (h + 1) * dk] = -dec
    for b in range(B):
        T3 = lens3[b]
        for h in range(H):
            g = b * H + h
            pk = peaks(g, T3)
            peak[b, h, :T3] = pk
            q = _noise((Tp, dk), seed, g, 4, amp=0.3)
            k = np.zeros((Tp, dk))
            if fam != "equal":
                k[:, nA + nB:DP_] = _noise((Tp, DP_ - nA - nB), seed, g, 5)
            i = np.arange(T3)
            if nA:
                k[:, :nA] = a * _bits(kcode(np.arange(Tp)), nA)
                q[:T3, :nA] = a * _bits(kcode(pk), nA) - pu[h, :nA]
            if nB:
                q[:T3, nA:nA + nB] = a * _bits(rcode(Tp - 1 - i + pk, b), nB) - pv[h, nA:nA + nB]
            q[:, DK_] = QC - pu[h, DK_]
            q[:, DP_] = QC - pv[h, DP_]
            k[:, DK_] = 0.0
            k[T3:, DK_] = DECOY * math.sqrt(dk) / QC
            j = np.arange(Tp)[:, None]
            sign = np.where(_u01(j, e[None, :], g, 1) < 0.5, -1.0, 1.0)
            v = sign * (0.5 + 0.5 * _u01(j, e[None, :], g, 2))
            v[T3:] = 1e4 * sign[T3:]
            qkv[b, :, 0, h], qkv[b, :, 1, h], qkv[b, :, 2, h] = q, k, v
    l4 = np.array([[4 * t + 3, 2 * t + 1, t - 1 if t > 0 else 1, t] for t in lens3], np.int32)
    return dict(qkv=qkv.reshape(B * Tp, 3 * d).astype(np.float32), p=P.reshape(-1).astype(np.float32),
                pu=pu.astype(np.float32), pv=pv.astype(np.float32), lens=l4, B=B, Tp=Tp, H=H, dk=dk, ldp=ldp,
                p_off=p_off, p_bstride=p_bstride, peak=peak)


# ------------------------------------------------------------------------------------- conv module
# (d, Tp, T3 per utterance): d = 1028 has a second blockIdx.z with one live thread; Tp = T3 and Tp no
# multiple of 8; T3 on both sides of the 8-frame tile and of the 4 frames a tap reaches back
CM_CASES = [dict(id=f"d{d}-Tp{Tp}-" + "_".join(map(str, lens)), d=d, Tp=Tp, lens=lens) for d, Tp, lens in (
    (256, 1, (1, 1)), (256, 4, (4, 3)), (256, 5, (5, 1)), (256, 8, (8, 8)), (1024, 9, (9, 4)), (1024, 12, (12, 5)),
    (1028, 13, (13, 8)), (1028, 17, (17, 9, 0)), (256, 11, (1, 4, 5)), (1024, 19, (8, 9, 12)), (1028, 21, (13, 17, 0)),
    (1028, 10, (4, 9)))]
CM_FAMILIES = ("rounded", "integer")
CM_FAULTS = ("shift", "tp_valid", "lens_col")
CM_DECOY = 1000.0


@functools.lru_cache(maxsize=None)
def cm_inputs(cid, family):
    """-> dict(a f32 [B * Tp][2 d], lens, dw_w [d][9], dw_b, bn = (g, b, m, v)).  Rows t >= T3 hold +-1000 behind
    an open gate (+30); |taps| >= 0.25, so a tap that reads one moves the output by hundreds."""
    c = next(x for x in CM_CASES if x["id"] == cid)
    d, Tp, lens3 = c["d"], c["Tp"], c["lens"]
    B = len(lens3)
    rng = np.random.default_rng(100 + CM_CASES.index(c))
    if family == "integer":
        x = rng.integers(-3, 4, (B, Tp, d)).astype(np.float64)
        gate = np.full((B, Tp, d), 30.0)
        w = rng.integers(1, 3, (d, 9)) * rng.choice([-1.0, 1.0], (d, 9))
        bias = rng.integers(-2, 3, d).astype(np.float64)
        bn = (np.ones(d), np.zeros(d), np.zeros(d), np.ones(d))
    else:
        x = rng.normal(0, 1, (B, Tp, d))
        gate = rng.normal(0, 2, (B, Tp, d))
        w = rng.uniform(0.25, 1.0, (d, 9)) * rng.choice([-1.0, 1.0], (d, 9))
        bias = rng.normal(0, 0.5, d)
        bn = (rng.uniform(0.5, 1.5, d) * rng.choice([-1.0, 1.0], d), rng.normal(0, 0.5, d), rng.normal(0, 0.5, d),
              rng.uniform(0.5, 2.0, d))
    for b, T3 in enumerate(lens3):
        x[b, T3:] = CM_DECOY * rng.choice([-1.0, 1.0], (Tp - T3, d))
        gate[b, T3:] = 30.0
    a = np.concatenate([x, gate], 2).reshape(B * Tp, 2 * d)
    l4 = np.array([[8 * t + 1, 4 * t + 1, t - 1 if t > 0 else 1, t] for t in lens3], np.int32)
    f = lambda v: np.asarray(v, np.float32)  # noqa: E731
    return dict(a=f(a), lens=l4, dw_w=f(w), dw_b=f(bias), bn=tuple(f(v) for v in bn), B=B, Tp=Tp, d=d)


# ------------------------------------------------------------------------------------- subsampling
# (C, F, Tp, valid frames per utterance): F odd and even (the last ff in and out of range), lens at, below
# and once above Tp
SUB_CASES = [dict(id=f"C{C}-F{F}-Tp{Tp}-" + "_".join(map(str, lens)), C=C, F=F, Tp=Tp, lens=lens) for C, F, Tp, lens in (
    (64, 9, 1, (1, 1)), (64, 16, 2, (2, 1)), (64, 9, 3, (3, 2, 0)), (1024, 16, 4, (4, 3)), (1024, 9, 5, (5, 9)),
    (64, 16, 9, (9, 4, 7)), (1024, 9, 9, (5, 12)))]
SUB_MODES = ("conv0", "dwconv1", "dwconv2")
SUB_COL = {"conv0": 0, "dwconv1": 1, "dwconv2": 2}
SUB_FAULTS = ("lens_col", "shift")


@functools.lru_cache(maxsize=None)
def sub_inputs(cid, mode):
    """Small integers throughout (|x| <= 3, |w| <= 2, |bias| <= 2: every sum is an integer below 64, exact in
    f32, bf16 and f16); frames >= the valid count hold 100.  The lens columns the mode does not read hold
    other counts."""
    c = next(x for x in SUB_CASES if x["id"] == cid)
    C, F, Tp, lens3 = c["C"], c["F"], c["Tp"], c["lens"]
    B = len(lens3)
    rng = np.random.default_rng(200 + 10 * SUB_CASES.index(c) + SUB_MODES.index(mode))
    shape = (B, Tp, F) if mode == "conv0" else (B, Tp, F, C)
    x = rng.integers(-3, 4, shape).astype(np.float32)
    for b, n in enumerate(lens3):
        x[b, n:] = 100.0
    w = rng.integers(-2, 3, (C, 9)).astype(np.float32)
    w[w == 0] = 1.0
    bias = rng.integers(-2, 3, C).astype(np.float32)
    col = SUB_COL[mode]
    l4 = np.zeros((B, 4), np.int32)
    for b, n in enumerate(lens3):
        l4[b] = [n + 1 if n < Tp else n - 1] * 4   # what a wrong column reads: one frame more, or one less
        l4[b, col] = n
    return dict(x=x, lens=l4, w=w, bias=bias, B=B, Tp=Tp, F=F, C=C, col=col)


RELPOS_CASES = [(Tp, d) for Tp in (1, 2, 37) for d in (64, 256)]


# ---------------------------------------------------------------------------------- TDT bookkeeping
# crafted partials for joint_fin_kernel: n_tiles 1, 2, 17 (fewer than its 256 threads), 129 and 300 (some threads
# take two partials), max_symbols 1, 2 and 10; B = 10 rows with T3 = 0 (done from the init), 1, 5, 9 and 12 = T3p
TDT_CASES = [dict(id=f"tiles{nt}-ms{ms}", n_tiles=nt, max_symbols=ms, P=260 if nt == 17 else 8)
             for nt in (1, 2, 17, 129, 300) for ms in (1, 2, 10)]
TDT_FAULTS = ("tie_high", "second_win_tile", "dur_ge")
TDT_STEPS, TDT_T3P, TDT_CAP, TDT_NDUR = 24, 12, 3, 5
TDT_LENS = (12, 0, 1, 5, 12, 12, 12, 12, 9, 12)


@functools.lru_cache(maxsize=None)
def tdt_inputs(cid):
    """Bests, runners-up and duration logits are small integers, so ties are frequent and every comparison is
    exact; about a quarter of the tiles hold no token at all (best -inf, index 0x7fffffff: a tile of duration
    logits only); the blank (index V, in the last tile) wins about a third of the steps.  V = 64 n_tiles - 8."""
    from spittle_amd.pk_debug import pack_part
    c = next(x for x in TDT_CASES if x["id"] == cid)
    nt, P = c["n_tiles"], c["P"]
    V, B, ns = 64 * nt - 8, len(TDT_LENS), TDT_STEPS
    rng = np.random.default_rng(300 + TDT_CASES.index(c))
    lo = 64 * np.arange(nt)
    hi = np.minimum(lo + 63, V)
    v1 = rng.integers(-3, 4, (ns, B, nt)).astype(np.float32)
    i1 = rng.integers(lo, hi + 1, (ns, B, nt)).astype(np.int32)
    blank = rng.random((ns, B)) < 0.33                      # the blank leads, or ties with a token of a lower index
    i1[..., -1] = np.where(blank, V, i1[..., -1])
    v1[..., -1] = np.where(blank, np.where(rng.random((ns, B)) < 0.5, 4.0, 3.0), v1[..., -1])   # 4: above every token
    v2 = np.minimum(v1, rng.integers(-4, 4, (ns, B, nt)).astype(np.float32))
    v2[rng.random((ns, B, nt)) < 0.3] = -np.inf
    dead = rng.random((ns, B, nt)) < 0.25
    dead[..., -1] = False                                   # one tile always holds a token or the blank
    v1[dead], v2[dead], i1[dead] = -np.inf, -np.inf, 0x7FFFFFFF
    dur = rng.integers(0, 3, (ns, B, TDT_NDUR)).astype(np.float32)
    # two events placed by hand, on rows that are still live: the blank alone at the top with duration 0
    # (step 1, row 0), and a token with duration 0 (step 0, row 4: no blank in its last tile)
    dur[1, 0], dur[0, 4] = (2, 0, 0, 0, 0), (2, 0, 0, 0, 0)
    v1[1, 0, -1], i1[1, 0, -1], v2[1, 0, -1] = 4.0, V, -np.inf
    if i1[0, 4, -1] == V:
        v1[0, 4, -1], i1[0, 4, -1], v2[0, 4, -1] = 3.0, V - 1, -np.inf
    # row 5: ten tokens in a row with duration 0, so at_t reaches max_symbols = 10 too (a forced skip of 1)
    for s in range(10):
        dur[s, 5] = (2, 0, 0, 0, 0)
        if i1[s, 5, -1] == V:
            v1[s, 5, -1], i1[s, 5, -1], v2[s, 5, -1] = 3.0, V - 1, -np.inf
    emb = rng.normal(0, 1, (V + 1, P)).astype(np.float32)
    emb[V] = 0.0
    fe = rng.normal(0, 1, (B * TDT_T3P, P)).astype(np.float32)
    lens = np.array([[8 * t, 4 * t, 2 * t, t] for t in TDT_LENS], np.int32)
    return dict(part=pack_part(v1, i1, v2), dur=dur, lens=lens, emb=emb, fe=fe, V=V, max_symbols=c["max_symbols"],
                cap=TDT_CAP, T3p=TDT_T3P)


# -------------------------------------------------------------------------------- the decode stages
# P: the smallest pk_decode_stage admits, one with NW < NWM in every stage, and the full model's (every register
# slot live); B: R < DR, a full row group, a one-row tail, two row groups in one workgroup with a tail, and both
# grid.y workgroups four times over
DEC_P, DEC_B = (128, 384, 640), (1, 7, 8, 9, 17, 64)
DEC_SHAPES = [(P, B) for P in DEC_P for B in DEC_B]
JOINT_V = (61, 63, 64, 1024)   # durations astride two tiles; a tile of durations only; the blank alone with them; the test model's
N_DUR = 5
DEC_FAULTS = {"lstm": ("gate_order", "neighbour", "upd_ignored"), "pred": ("upd_ignored",), "joint": ("blank_out",)}


def _upd(B, rng):
    u = (rng.random(B) < 0.6).astype(np.int32)
    u[0] = 1
    if B > 1:
        u[-1] = 0
    return u * rng.integers(1, 4, B).astype(np.int32)    # any non-zero value is a set flag


@functools.lru_cache(maxsize=None)
def lstm_inputs(P, B):
    """Seeded weights of a trained LSTM's size (|w| about 1 / sqrt(P)); the biases of a few units push each gate
    to both saturations (+-12); upd mixed per row."""
    rng = np.random.default_rng(400 + P + B)
    f = lambda *s: rng.normal(0, 1, s).astype(np.float32)  # noqa: E731
    sc = np.float32(1.0 / math.sqrt(P))
    b_ih, b_hh = 0.1 * f(4 * P), 0.1 * f(4 * P)
    for q in range(4):
        b_ih[q * P + 3 * q + 1], b_ih[q * P + 3 * q + 2] = 12.0, -12.0
    return dict(W_ih=sc * f(4 * P, P), W_hh=sc * f(4 * P, P), b_ih=b_ih, b_hh=b_hh, x=f(B, P), h=0.5 * f(B, P), c=f(B, P),
                upd=_upd(B, rng))


@functools.lru_cache(maxsize=None)
def pred_inputs(P, B, exact):
    """exact: small integers (|w| <= 2, |x| <= 3, sums below 2^24: zero tolerance); gp pre-filled."""
    rng = np.random.default_rng(500 + P + B + exact)
    if exact:
        W, b, x = (rng.integers(-k, k + 1, s).astype(np.float32) for k, s in ((2, (P, P)), (5, (P,)), (3, (B, P))))
    else:
        W, b, x = (rng.normal(0, 1, s).astype(np.float32) for s in ((P, P), (P,), (B, P)))
    return dict(W=W, b=b, x=x, gp=(1000.0 + rng.integers(0, 9, (B, P))).astype(np.float32), upd=_upd(B, rng))


@functools.lru_cache(maxsize=None)
def joint_inputs(P, B, V, kind):
    """kind `exact`: small integers (ties within and across tiles abound; zero tolerance on the partials and the
    durations); `rounded`: seeded normals.  joint_bias_case sets the logits through the bias with W = 0."""
    N = V + 1 + N_DUR
    rng = np.random.default_rng(600 + P + B + V)
    fe, gp = (rng.integers(-3, 4, (B, P)).astype(np.float32) for _ in range(2))
    if kind == "rounded":
        return dict(W=(rng.normal(0, 1, (N, P)) / math.sqrt(P)).astype(np.float32), b=rng.normal(0, 1, N).astype(np.float32),
                    fe=rng.normal(0, 1, (B, P)).astype(np.float32), gp=rng.normal(0, 1, (B, P)).astype(np.float32))
    if kind == "exact":
        return dict(W=rng.integers(-1, 2, (N, P)).astype(np.float32), b=rng.integers(-4, 5, N).astype(np.float32), fe=fe, gp=gp)
    raise ValueError(kind)


def joint_bias_case(V, pat):
    """-> (bias [N], expected (token, v1, v2)) for W = 0: every logit is its bias."""
    N = V + 1 + N_DUR
    b = -np.abs(np.random.default_rng(700 + V + pat).integers(1, 9, N)).astype(np.float32)   # everything else below 0
    b[V + 1:] = 50.0                                        # durations above every token: they must not enter the top-2
    last = (V // 64) * 64                                    # first index of the blank's tile
    far = 3 if V >= 64 else None                             # an index in another tile than the blank's
    if pat == 0:       # top-1 and top-2 in one tile
        b[5], b[9] = 7.0, 6.0
        want = (5, 7.0, 6.0)
    elif pat == 1:     # in two tiles (the blank's tile holds the runner-up when there is a second tile)
        i2 = V - 1 if far is not None and V - 1 >= last else 11
        b[5], b[i2] = 7.0, 6.0
        want = (5, 7.0, 6.0)
    elif pat == 2:     # equal maxima at two indices of one tile
        b[9], b[5] = 7.0, 7.0
        want = (5, 7.0, 7.0)
    elif pat == 3:     # equal maxima in two tiles
        i2 = V - 1 if V - 1 >= 64 else 40
        b[5], b[i2] = 7.0, 7.0
        want = (5, 7.0, 7.0)
    elif pat == 4:     # the blank wins; the runner-up comes from another tile where there is one
        b[V], b[5] = 7.0, 6.0
        want = (V, 7.0, 6.0)
    else:              # the blank ties a token: the token's lower index wins and v2 = v1
        b[V], b[5] = 7.0, 7.0
        want = (5, 7.0, 7.0)
    return b, want


# ------------------------------------------------------------------------------------ the whole step
STEPS = dict(P=128, B=9, V=61, n_steps=14, max_symbols=3, cap=4, T3p=6, lens=(6, 0, 1, 3, 6, 6, 5, 6, 2))


@functools.lru_cache(maxsize=None)
def steps_inputs():
    """Seeded weights of the step at P = 128, B = 9, V = 61.  The joint's bias is a permutation of multiples of 0.75
    over the tokens (and of 1.5 over the durations) and its weights are small, so the state moves the winner
    among the few leading tokens while every decision keeps a wide lead (asserted on the CPU)."""
    P, B, V, T3p = STEPS["P"], STEPS["B"], STEPS["V"], STEPS["T3p"]
    N = V + 1 + N_DUR
    rng = np.random.default_rng(811)
    f = lambda sc, *s: (sc * rng.normal(0, 1, s)).astype(np.float32)  # noqa: E731
    w = 1.0 / math.sqrt(P)
    lstm = tuple((f(w, 4 * P, P), f(w, 4 * P, P), f(0.1, 4 * P), f(0.1, 4 * P)) for _ in range(2))
    jb = np.concatenate([0.75 * rng.permutation(V + 1), 1.5 * rng.permutation(N_DUR)]).astype(np.float32)
    emb = f(1.0, V + 1, P)
    emb[V] = 0.0
    lens = np.array([[8 * t, 4 * t, 2 * t, t] for t in STEPS["lens"]], np.int32)
    jb[V] = 0.75 * (V - 1) + 0.4                            # the blank among the leaders: some steps emit nothing
    jw = (0.5 * np.random.default_rng(814).normal(0, 1, (N, P))).astype(np.float32)
    return dict(lstm=lstm, pred_w=f(w, P, P), pred_b=f(0.1, P), joint_w=jw, joint_b=jb, emb=emb,
                fe=f(1.0, B * T3p, P), lens=lens)
