"""float64 reference of the Whisper attention kernels, for tests/test_attn_ref.py and
tests/test_gpu_attn.py, on the inputs the spt_debug_attn_* hooks take.

It states the arithmetic contract -- softmax(q . k / 8) v over the keys a query may see, from the
dtype-rounded inputs -- and nothing about the kernels' schedules (tiles, waves, re-basing).  The one
intermediate rounding the contract has is the 16-bit encoder's pre-scaled Q at SPT_ATTN_SUM = 4
(scale_q).  Partials {o, m, l} are merged here in float64 (merge)."""
from __future__ import annotations

import numpy as np

LOG2E = 1.4426950408889634
# the kernels' constant (1 / sqrt(64)) * log2(e), as f32 arithmetic holds it (kScaleLog2 / kLog2Scale)
C32 = np.float32(0.125) * np.float32(LOG2E)
C64 = LOG2E / 8.0
U = {"bf16": 2.0 ** -9, "f16": 2.0 ** -11}  # the 16-bit encoder bar's unit


def round_dtype(x, dtype) -> np.ndarray:
    """f32 values rounded to nearest even into the engine dtype's storage, back as f32."""
    x = np.ascontiguousarray(x, np.float32)
    if dtype == "f32":
        return x.copy()
    if dtype == "f16":
        return x.astype(np.float16).astype(np.float32)
    if dtype != "bf16":
        raise ValueError(dtype)
    b = x.view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) >> 16 << 16
    return b.astype(np.uint32).view(np.float32).reshape(x.shape)


def half_ulp(x, dtype) -> np.ndarray:
    """Half a unit in the last place of dtype at |x| (0 for f32: f32 outputs are not rounded again)."""
    x = np.abs(np.asarray(x, np.float64))
    if dtype == "f32":
        return np.zeros_like(x)
    bits, emin = (8, -126) if dtype == "bf16" else (11, -14)
    e = np.floor(np.log2(np.maximum(x, 2.0 ** emin)))
    return 0.5 * 2.0 ** (e - (bits - 1))


def scale_q(q, dtype) -> np.ndarray:
    """The 16-bit encoder's Q at SUM = 4: round_ET(f32(q) * f32(log2(e) / 8)), in np.float32."""
    return round_dtype(np.asarray(q, np.float32) * C32, dtype)


def scores(q, k, prescaled=False) -> np.ndarray:
    """q [.., nq, 64], k [.., nk, 64] -> scores [.., nq, nk] in log2 units (float64)."""
    s = np.asarray(q, np.float64) @ np.swapaxes(np.asarray(k, np.float64), -1, -2)
    return s if prescaled else s * C64


def partial(s, v, vis=None):
    """Online-softmax partial of scores s [.., nq, nk] (log2 units) over the keys vis marks:
    (o [.., nq, 64] = sum 2^(s - m) v, m, l).  A query with no visible key has m = -inf, l = 0, o = 0."""
    s = np.array(s, np.float64)
    if vis is not None:
        s = np.where(vis, s, -np.inf)
    m = s.max(-1) if s.shape[-1] else np.full(s.shape[:-1], -np.inf)
    with np.errstate(invalid="ignore"):
        p = np.exp2(s - np.where(np.isfinite(m), m, 0.0)[..., None])
    p = np.where(np.isfinite(s), p, 0.0)
    return p @ np.asarray(v, np.float64), m, p.sum(-1)


def merge(parts, weighted=True):
    """sum o_s 2^(m_s - M) / sum l_s 2^(m_s - M) over partials [(o, m, l), ..]; a chunk with
    m = -inf takes no part.  weighted=False is the fault `a chunk merged without its weight`."""
    M = np.max(np.stack([m for _, m, _ in parts]), 0)
    O = 0.0
    Lsum = 0.0
    for o, m, l in parts:
        live = np.isfinite(m)
        with np.errstate(invalid="ignore"):
            f = np.where(live, np.exp2(np.where(live, m, 0.0) - M) if weighted else 1.0, 0.0)
        O = O + np.where(live[..., None], o, 0.0) * f[..., None]
        Lsum = Lsum + np.where(live, l, 0.0) * f
    return O / Lsum[..., None]


def attend(q, k, v, vis=None, prescaled=False) -> np.ndarray:
    """softmax over the visible keys of q . k / 8 (or of q . k, log2 units, for a pre-scaled q), times v."""
    o, _, l = partial(scores(q, k, prescaled), v, vis)
    with np.errstate(invalid="ignore"):  # a query with no visible key: NaN
        return o / l[..., None]


def causal(pos0, Tq, n_keys) -> np.ndarray:
    """vis [Tq][n_keys]: query t at position pos0 + t sees keys 0 .. pos0 + t."""
    return np.arange(n_keys)[None, :] < (pos0 + np.arange(Tq) + 1)[:, None]


def rel_bound_f32(q, k, vis=None, chain=12) -> np.ndarray:
    """The linear error model of an f32 attention kernel, per query [.., nq]: `chain` roundings on a
    score (decoder: one of q * kLog2Scale, 8 fmaf, 3 shuffle adds; f32 encoder: the MFMA's 64
    accumulations and two for the scale and the shift), |ds| <= chain 2^-24 sum|q_e k_e| log2(e) / 8; a
    relative error ln2 * 2 |ds| on a probability; exp2f within 4 ulp; one accumulation per key."""
    a = (np.abs(np.asarray(q, np.float64)) @ np.swapaxes(np.abs(np.asarray(k, np.float64)), -1, -2)) * C64
    n = a.shape[-1]
    if vis is not None:
        a = np.where(vis, a, 0.0)
        n = np.broadcast_to(vis, a.shape).sum(-1)
    ds = chain * 2.0 ** -24 * a.max(-1)
    return np.log(2.0) * 2.0 * ds + 4 * 2.0 ** -24 + n * 2.0 ** -24


def vmax_visible(v, vis=None) -> np.ndarray:
    """max |v| over the keys each query sees: v [.., nk, 64] -> [.., nq] (vis [.., nq, nk]) or [.., 1]."""
    a = np.abs(np.asarray(v, np.float64)).max(-1)
    if vis is None:
        return a.max(-1, keepdims=True)
    return np.where(vis, a[..., None, :], 0.0).max(-1)
