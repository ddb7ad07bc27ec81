"""float64 restatement of the token alignment, for tests/test_align_ref.py
and tests/test_gpu_align.py, on the inputs the spt_debug_align_* hooks take: the alignment heads'
probabilities, their normalisation, median filter and head mean, the dynamic time warping with HF
transformers' recurrence and tie rule (also in float32, adding in np.float32), and the jump times.

It states the arithmetic contract and nothing about the kernels' schedules."""
from __future__ import annotations

import numpy as np

from tests import attn_ref as R

U32 = 2.0 ** -24


def probs(q, k, M=None, pad=None) -> np.ndarray:
    """softmax over ALL keys of q . k / 8 (q [.., nq, 64], k [.., nk, 64], float64), then the first M.
    pad = (n, value): the fault `the padded keys of the last block take part` (n keys of value)."""
    k = np.asarray(k, np.float64)
    if pad is not None:
        k = np.concatenate([k, np.full(k.shape[:-2] + (pad[0], 64), pad[1], np.float64)], -2)
    s = R.scores(q, k)
    p = np.exp2(s - s.max(-1, keepdims=True))
    p = p / p.sum(-1, keepdims=True)
    return p if M is None else p[..., :M]


def stats(p):
    """p [.., A, N, M] -> (mean, population std) over the N rows, [.., A, 1, M]."""
    p = np.asarray(p, np.float64)
    return p.mean(-2, keepdims=True), p.std(-2, keepdims=True)


def normalise(p) -> np.ndarray:
    """z = (p - mean) / std per column over the rows; 0 where std == 0 (HF: NaN)."""
    p = np.asarray(p, np.float64)
    mean, std = stats(p)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(std > 0, (p - mean) / std, 0.0)


def _windows(x, width=7) -> np.ndarray:
    """[.., M] -> [.., M, width]: the reflect-padded windows along the last axis (M > width // 2)."""
    h = width // 2
    xp = np.pad(x, [(0, 0)] * (x.ndim - 1) + [(h, h)], mode="reflect")
    return np.lib.stride_tricks.sliding_window_view(xp, width, axis=-1)


def median_filter(z, width=7) -> np.ndarray:
    """Width-7 median along the last axis with reflect padding; unchanged when M <= width // 2."""
    z = np.asarray(z, np.float64)
    if z.shape[-1] <= width // 2:
        return z
    return np.sort(_windows(z, width), -1)[..., width // 2]


def matrix(p) -> np.ndarray:
    """p [A][N][M] -> m [N][M]: normalise, median, mean over the heads."""
    return median_filter(normalise(p)).mean(-3)


def norm_bars(p):
    """The propagated f32 bars of align_norm on p [A][N][M]: (bar_z, bar_med, bar_m).  Per element
    4 u32 (|p| + |mean|) (2 + |z|) / std on z (0 where std == 0: both sides give 0 exactly), the
    largest such bar in the 7-wide window on the median, the mean over the heads on m."""
    p = np.asarray(p, np.float64)
    mean, std = stats(p)
    z = normalise(p)
    with np.errstate(invalid="ignore", divide="ignore"):
        bz = np.where(std > 0, 4 * U32 * (np.abs(p) + np.abs(mean)) * (2 + np.abs(z)) / std, 0.0)
    bmed = bz if p.shape[-1] <= 3 else _windows(bz).max(-1)
    return bz, bmed, bmed.mean(-3)


def dtw(x, dtype=np.float64, rule="hf"):
    """HF _dynamic_time_warping on the cost matrix x [N][M] (pass -m), restated along anti-diagonals:
    the same recurrence, tie rule (step 0 only if c0 < c1 and c0 < c2, step 1 only if c1 < c0 and
    c1 < c2, else step 2 at cost c2) and backtrace; costs held and added in dtype.
    rule="min": the other function, a DTW that takes the smallest of the three.
    -> (text_indices, time_indices)."""
    cost, trace = sweep(x, dtype, rule)
    N, M = np.asarray(x).shape
    trace[0, :] = 2
    trace[:, 0] = 1
    i, j = N, M
    ti, tj = [], []
    while i > 0 or j > 0:
        ti.append(i - 1)
        tj.append(j - 1)
        t = trace[i, j]
        if t == 0:
            i, j = i - 1, j - 1
        elif t == 1:
            i -= 1
        else:
            j -= 1
    return np.array(ti[::-1]), np.array(tj[::-1])


def tie_kinds(x, dtype=np.float32) -> dict:
    """How many cells of the sweep see each kind of tie among finite costs: c0 == c1 < c2, c0 == c2 < c1,
    c1 == c2 < c0, and all three equal."""
    cost, _ = sweep(x, dtype)
    c0, c1, c2 = cost[:-1, :-1], cost[:-1, 1:], cost[1:, :-1]
    fin = np.isfinite(c0) & np.isfinite(c1) & np.isfinite(c2)
    return {"c0==c1<c2": int((fin & (c0 == c1) & (c0 < c2)).sum()), "c0==c2<c1": int((fin & (c0 == c2) & (c0 < c1)).sum()),
            "c1==c2<c0": int((fin & (c1 == c2) & (c1 < c0)).sum()), "all": int((fin & (c0 == c1) & (c1 == c2)).sum())}


def sweep(x, dtype=np.float64, rule="hf"):
    """The cost and trace grids [N + 1][M + 1] of dtw()."""
    x = np.asarray(x, dtype)
    N, M = x.shape
    cost = np.full((N + 1, M + 1), np.inf, dtype)
    trace = np.full((N + 1, M + 1), -1, np.int8)
    cost[0, 0] = 0
    for d in range(2, N + M + 1):
        i = np.arange(max(1, d - M), min(N, d - 1) + 1)
        j = d - i
        c0, c1, c2 = cost[i - 1, j - 1], cost[i - 1, j], cost[i, j - 1]
        if rule == "hf":
            t = np.where((c0 < c1) & (c0 < c2), 0, np.where((c1 < c0) & (c1 < c2), 1, 2))
        else:
            t = np.argmin(np.stack([c0, c1, c2]), 0)
        c = np.where(t == 0, c0, np.where(t == 1, c1, c2)).astype(dtype)
        cost[i, j] = x[i - 1, j - 1] + c
        trace[i, j] = t
    return cost, trace


def path_cost(x, ti, tj) -> float:
    return float(np.asarray(x, np.float64)[ti, tj].sum())


def jumps(ti, tj) -> np.ndarray:
    """The first frame of each row on the path (HF: time_indices where text_indices steps)."""
    ti, tj = np.asarray(ti), np.asarray(tj)
    return tj[np.pad(np.diff(ti), (1, 0), constant_values=1).astype(bool)]


def token_times(jump, seek):
    """jump [n + 1] (n text tokens and the end row) -> (t0 [n], t1 [n]) in 10 ms units."""
    jump = np.asarray(jump, np.int64)
    return seek + 2 * jump[:-1], seek + 2 * jump[1:]
