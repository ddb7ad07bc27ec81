"""Crafted inputs of the token-alignment kernels for tests/test_align_ref.py (CPU: the
reference against HF transformers, and what each case is built to catch) and tests/test_gpu_align.py
(the kernels against the reference).

align_qk: peaked scores within 64 log2 units built as tests/attn_cases.py builds them (a +-1 code of
the key index selects each query's peak key; dimension 63 of every query makes a padded key holding
pad_value in every element the winner, were it admitted).  align_norm: positive columns of widely
different magnitude whose rows are spread by construction.  align_dtw: matrices of multiples of 1/8 in
[-8, 8], so every f32 sum is exact and ties are real."""
from __future__ import annotations

import functools
import itertools

import numpy as np

from tests import align_ref as A
from tests import attn_cases as K
from tests import attn_ref as R

DT = K.DT
PAD = K.PAD
H = 6

# ---------------------------------------------------------------------------------------- align_qk
QK_SHAPES = ((1, 0), (4, 0), (3, 221))   # (Tq, pos0)
QK_M = (4, 50, 750)
QK_T = (1500, 1024)                      # 1504 stored keys with 4 padded ones; a multiple of 32
# a head list that skips heads and is unordered; two sequences on a row -> window map
QK_SETS = {"heads": dict(B=1, B_layout=1, heads=(4, 1, 3), kvrow=None),
           "map": dict(B=2, B_layout=3, heads=(0, 5), kvrow=(2, 0))}
QK_CASES = [dict(id=f"T{T}-{s}-Tq{Tq}at{pos0}-M{M}", T=T, set=s, Tq=Tq, pos0=pos0, M=M)
            for T, s, (Tq, pos0), M in itertools.product(QK_T, QK_SETS, QK_SHAPES, QK_M)]
QK_BY_ID = {c["id"]: c for c in QK_CASES}
W_BIT = 2.75  # log2 units per code bit: 11 bits put the peak 30 above the mean, a key one bit away 5.5 below it


def qk_M(c):
    """Keys kept per sequence: M, and about half of it for the second sequence."""
    return [c["M"], c["M"] // 2 + 1][:QK_SETS[c["set"]]["B"]]


@functools.lru_cache(maxsize=None)
def qk_keys(T, BL):
    nbits = int(T - 1).bit_length()
    k = np.zeros((BL, H, T, 64), np.float32)
    for w in range(BL):
        for h in range(H):
            _, k[w, h] = K.qk(31000 + 10 * w + h + T, [0], np.arange(T), nbits, W_BIT)
    return k


@functools.lru_cache(maxsize=None)
def qk_inputs(cid):
    """-> q [B][H][Tq][64], k [B_layout][H][T][64] float32, peak [B][H][Tq]."""
    c = QK_BY_ID[cid]
    s = QK_SETS[c["set"]]
    T, B, Tq, M = c["T"], s["B"], c["Tq"], c["M"]
    nbits = int(T - 1).bit_length()
    pk = [0, T - 1, 31, 32, M - 1, M, M // 2, 749, 750, T - 5, 1, T // 2]
    pk = [p for p in pk if 0 <= p < T]
    q = np.zeros((B, H, Tq, 64), np.float32)
    peak = np.zeros((B, H, Tq), np.int64)
    n = QK_CASES.index(c)
    for b in range(B):
        for h in range(H):
            for t in range(Tq):
                peak[b, h, t] = pk[n % len(pk)]
                n += 1
            qq, _ = K.qk(32000 + 100 * QK_CASES.index(c) + 10 * b + h, peak[b, h], [0], nbits, W_BIT)
            qq[:, 63] = K.GUARD
            q[b, h] = qq
    return q, qk_keys(T, s["B_layout"]), peak


def qk_ref(cid, dtype, fault=None, full=False):
    """-> per sequence (p [A][Tq][M_b] float64, tol of the same shape): the reference on the rounded
    inputs and 4 x attn_ref.rel_bound_f32 x p.  full: every key kept (the rows then sum to 1).
    fault="admit_pad": the padded keys of the last 32-key block take part."""
    c = QK_BY_ID[cid]
    s = QK_SETS[c["set"]]
    q, k, _ = qk_inputs(cid)
    qr, kr = R.round_dtype(q, dtype), R.round_dtype(k, dtype)
    heads = list(s["heads"])
    out = []
    for b in range(s["B"]):
        w = b if s["kvrow"] is None else s["kvrow"][b]
        M = c["T"] if full else qk_M(c)[b]
        pad = (-c["T"] % 32, PAD) if fault == "admit_pad" else None
        p = A.probs(qr[b, heads], kr[w, heads], M, pad=pad)
        tol = 4.0 * R.rel_bound_f32(qr[b, heads], kr[w, heads])[..., None] * A.probs(qr[b, heads], kr[w, heads], M)
        out.append((p, tol))
    return out


def rows_pack(q) -> np.ndarray:
    """[B][H][Tq][64] -> the hook's [B*Tq][H*64]."""
    B, H_, Tq, _ = q.shape
    return np.ascontiguousarray(q.transpose(0, 2, 1, 3)).reshape(B * Tq, H_ * 64)


# -------------------------------------------------------------------------------------- align_norm
NORM_CASES = [dict(id=f"N{N}-M{M}-A{A_}", N=N, M=M, A=A_) for N, M, A_ in
              itertools.product((2, 5, 226), (3, 4, 7, 750), (1, 6))]
NORM_BY_ID = {c["id"]: c for c in NORM_CASES}
NORM_FLAT = "N5-M7-A6"       # the case with a std = 0 column: head 2, key 1
NORM_RAGGED = dict(A=3, N_cap=6, M_cap=56, N=(5, 3), M=(50, 20))  # two sequences in one workspace


def _norm_block(seed, A_, N, M) -> np.ndarray:
    """p [A][N][M] float32: column magnitudes 1e-1 .. 1e-4, the N rows of a column spread over
    (0.5 .. 1.5) x that magnitude by a random permutation of N evenly spaced levels plus jitter."""
    rng = np.random.default_rng(seed)
    base = 10.0 ** (-1.0 - 3.0 * rng.random((A_, 1, M)))
    level = np.argsort(rng.random((A_, N, M)), 1) + 0.5 * rng.random((A_, N, M))
    return (base * (0.5 + level / N)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def norm_inputs(cid) -> np.ndarray:
    c = NORM_BY_ID[cid]
    p = _norm_block(41000 + NORM_CASES.index(c), c["A"], c["N"], c["M"])
    if cid == NORM_FLAT:
        p[2, :, 1] = p[2, 0, 1]
    return p


@functools.lru_cache(maxsize=None)
def norm_ragged_inputs() -> np.ndarray:
    """p [2][A][N_cap][M_cap]: NaN outside each sequence's N x M."""
    g = NORM_RAGGED
    p = np.full((2, g["A"], g["N_cap"], g["M_cap"]), np.nan, np.float32)
    for b in range(2):
        p[b, :, :g["N"][b], :g["M"][b]] = _norm_block(42000 + b, g["A"], g["N"][b], g["M"][b])
    return p


# --------------------------------------------------------------------------------------- align_dtw
DTW_SHAPES = ((1, 1), (1, 50), (2, 4), (226, 4), (5, 1500), (226, 1500))
# fine: every multiple of 1/8 in [-8, 8]; coarse: {-1/8, 0, 1/8}, where most cells see a tie
DTW_CASES = [dict(id=f"{N}x{M}-{kind}", N=N, M=M, kind=kind) for (N, M) in DTW_SHAPES for kind in ("fine", "coarse")]
DTW_CASES.append(dict(id="2x2-c0==c1<c2", N=2, M=2, kind="tie"))
DTW_BY_ID = {c["id"]: c for c in DTW_CASES}
DTW_RAGGED = dict(N_cap=6, M_cap=56, N=(5, 3), M=(50, 20))


@functools.lru_cache(maxsize=None)
def dtw_inputs(cid) -> np.ndarray:
    """m [N][M] float32 (the kernels warp -m)."""
    c = DTW_BY_ID[cid]
    if c["kind"] == "tie":
        # cost = -m: cell (2, 2) sees c0 == c1 (= 1) < c2 (= 2): the rule takes step 2, a plain minimum step 0
        return -np.array([[1.0, 0.0], [1.0, -0.5]], np.float32)
    rng = np.random.default_rng(51000 + DTW_CASES.index(c))
    lim = 64 if c["kind"] == "fine" else 1
    return (rng.integers(-lim, lim + 1, (c["N"], c["M"])) / 8.0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def dtw_float_inputs() -> np.ndarray:
    """m [50][300] of unrounded normal floats: sums round, so only the f32 reference matches."""
    return np.random.default_rng(52000).normal(0, 1, (50, 300)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def dtw_ragged_inputs() -> np.ndarray:
    g = DTW_RAGGED
    m = np.full((2, g["N_cap"], g["M_cap"]), np.nan, np.float32)
    rng = np.random.default_rng(53000)
    for b in range(2):
        m[b, :g["N"][b], :g["M"][b]] = rng.integers(-16, 17, (g["N"][b], g["M"][b])) / 8.0
    return m


@functools.lru_cache(maxsize=None)
def dtw_ref(cid):
    """-> (text_indices, time_indices) of the f32 reference on -m."""
    return A.dtw(-dtw_inputs(cid), np.float32)


# ------------------------------------------------------------------------ the three kernels in a row
SHARP = dict(T=1500, n_rows=6, M=60, heads=(1, 4), chunks=((0, 4), (4, 2)))  # (pos0, Tq) of the two passes


@functools.lru_cache(maxsize=None)
def sharp_inputs():
    """q [1][H][n_rows][64], k [1][H][T][64]: row r attends the frames [10 r, 10 r + 10) alike (the key
    code is the frame's decade), so the jumps are 10 r exactly."""
    g = SHARP
    T, n = g["T"], g["n_rows"]
    q = np.zeros((1, H, n, 64), np.float32)
    k = np.zeros((1, H, T, 64), np.float32)
    for h in range(H):
        qq, kk = K.qk(61000 + h, np.arange(n), np.arange(T) // 10, 8, 4.0, noise=0.0)
        q[0, h], k[0, h] = qq, kk
    return q, k
