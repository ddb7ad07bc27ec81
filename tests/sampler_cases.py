"""Crafted inputs shared by tests/test_sampler_ref.py (CPU: the reference alone) and
tests/test_gpu_sampler.py (the kernels against it): vocabularies, the one rule for base logits (a
seeded normal x 2 with chosen entries overwritten), the bookkeeping scripts, the temperature rows
and the f32 emulation of the sampling kernel's sums that the CDF tolerance rests on."""
from __future__ import annotations

import functools

import numpy as np

from oracle import oracle as O
from oracle import whisper_full as W
from tests import sampler_ref as R

BLANK = 220
D, CTX = 48, 16
TEXT = 600       # a plain text token (of the small vocabulary too)
TOP, LADDER_TOP = 26.0, 24.0   # the crafted maximum; the runners-up below it, one apart
CHUNKS, TS_T, TW = 16, 256, 1024   # k_sample.hip's layout: chunks per row, threads per chunk / per row


@functools.lru_cache(None)
def vocab(V: int):
    """(sp, smask) of a real vocabulary size, or of the small hand-placed one (V = 1000)."""
    if V == 1000:
        sp = dict(eot=900, sot=901, translate=904, transcribe=905, solm=906, prev=907, nosp=908, beg=910, n_langs=2)
        sp["not"] = 909
    else:
        sp = O.special_tokens(V)
    return sp, W.static_mask(V, sp)


@functools.lru_cache(None)
def tables(V: int):
    """emb [V][D], pos [CTX][D] (f32)."""
    g = np.random.default_rng(V)
    return g.standard_normal((V, D)).astype(np.float32), g.standard_normal((CTX, D)).astype(np.float32)


def base(seed: int, V: int, n: int = 1) -> np.ndarray:
    """n rows of base logits: a seeded normal x 2."""
    return (np.random.default_rng(seed).standard_normal((n, V)) * 2).astype(np.float32)


def crafted(seed: int, V: int, tops, ladder=(), ts_ladder=()) -> np.ndarray:
    """One row: base logits with a ladder of runners-up (LADDER_TOP, LADDER_TOP - 1, ..) at the
    given ids, a second one for the timestamps (LADDER_TOP - 1.5, - 2.5, ..: the candidates when the
    timestamp rule fires; together they stay a whole logit below the first ladder's top, so they
    never fire it themselves), then tops = [(id, value)] overwritten."""
    r = base(seed, V)[0]
    for j, t in enumerate(ladder):
        r[t] = LADDER_TOP - j
    for j, t in enumerate(ts_ladder):
        r[t] = LADDER_TOP - 1.5 - j
    for t, v in tops:
        r[t] = v
    return r


def text_ladder(V: int, n: int = 9):
    """Runner-up ids spread over the chunks, clear of every edge the tests place a maximum at."""
    return [107 + (V // 11) * j for j in range(n)]


def chunk_size(V: int) -> int:
    return -(-V // CHUNKS)


# ---- bookkeeping scripts: one dominant logit per step -------------------------------------------
def script_logits(V: int, scripts, S: int, seed: int = 100) -> np.ndarray:
    """[S][B][V]: row b's step s has scripts[b][s] at TOP (None: every logit -inf)."""
    lg = base(seed, V, S * len(scripts)).reshape(S, len(scripts), V)
    for b, sc in enumerate(scripts):
        for s in range(S):
            t = sc[s] if s < len(sc) else sc[-1]
            if t is None:
                lg[s, b] = -np.inf
            else:
                lg[s, b, t] = TOP
    return lg


def bookkeeping_groups(V: int):
    """The scripted calls: dict(name, prm, scripts, S, seek, seek_end, state, forced, out_cap[, done]).
    Together they take every branch of W.bookkeep (sampler_ref.BRANCHES) and the not-live
    conventions."""
    sp, _ = vocab(V)
    eot, beg = sp["eot"], sp["beg"]
    ts = lambda k: beg + k
    T = TEXT
    z = (0, 0, 0, 0)
    g = []
    # default parameters, S = 6
    scripts = [
        [ts(10), T, T, ts(20), ts(20), eot],   # first timestamp, later ones, [eot] with a result
        [T, ts(30), T, T, T, T],               # seek_delta 61 in the state: time runs backwards at step 1
        [T, eot, T, T, T, T],                  # [eot] without a result: failed
        [T, eot, T, T, T, T],                  # ... but at the end of the audio: kept
        [T, T, T, T, T, T],                    # end of audio by the state's timestamp, no result yet: kept
        [ts(50), T, T, T, T, T],               # end of audio right after the first timestamp
        [T, None, T, T, T, T],                 # nothing survives at step 1
        [T, T, ts(40), ts(41), T, eot],        # a pair of timestamps after text, then text, then [eot]
    ]
    state = [z, (1, 61, 0, 0), z, z, (1, 2900, 0, 0), z, z, z]
    seek = [0, 0, 0, 0, 0, 2800, 0, 0]
    seek_end = [3000, 3000, 3000, 100, 3000, 3000, 3000, 3000]
    g.append(dict(name="default", prm=R.Prm(), scripts=scripts, S=6, seek=seek, seek_end=seek_end, state=state,
                  forced=None, out_cap=None))
    # forced tokens replace next_tok, not the record; one outside the vocabulary feeds [eot]; a row that
    # ends at this very step still feeds its forced token
    g.append(dict(name="forced", prm=R.Prm(), scripts=[[T, T], [T, T], [T, eot]], S=2, seek=0, seek_end=3000,
                  state=None, forced=[[T + 1, T + 2], [T + 1, V + 5], [T + 1, T + 2]], out_cap=None))
    g.append(dict(name="max_tokens", prm=R.Prm(max_tokens=2), scripts=[[ts(10), T, T, T], [T, T, T, T]], S=4, seek=0,
                  seek_end=3000, state=None, forced=None, out_cap=None))
    g.append(dict(name="no_ts", prm=R.Prm(no_ts=True), scripts=[[T, T, eot, T], [T, T, T, T]], S=4, seek=0,
                  seek_end=3000, state=None, forced=None, out_cap=None))
    g.append(dict(name="guard", prm=R.Prm(n_max=3), scripts=[[T] * 4] * 3, S=4, seek=0, seek_end=9000,
                  state=[z, (1, 1600, 1, 0), (1, 1000, 1, 0)], forced=None, out_cap=None))
    # steps at or past out_cap; a row that arrives already done
    g.append(dict(name="out_cap", prm=R.Prm(), scripts=[[T] * 4, [T, eot, T, T], [T] * 4], S=4, seek=0, seek_end=3000,
                  state=None, forced=None, out_cap=2, done=[0, 0, 1]))
    return g


REACHED = set(R.BRANCHES) | {"nothing_survives", "not_live_record", "past_out_cap"}


# ---- temperature rows ---------------------------------------------------------------------------
TEMPS, SEEDS, T_B, T_S = (0.2, 0.6, 1.0), (7, 8), 8, 4
ROW_KINDS = ("peaked", "flat", "ends", "rule", "one", "peaked", "flat", "rule")


def temperature_logits(V: int, T: float, seed: int) -> np.ndarray:
    """[T_S][T_B][V] logits whose val = logits / T are, by row: 8 tokens with 99 % of the mass; flat
    text; 60 % on id 0 and 39 % on V - 1; 400 timestamps that beat the best text token together but
    not alone; one survivor; then three more of these over other ids.  Timestamps of the other rows
    and [eot] lie far below, so that the timestamp-rule comparison is never close."""
    sp, smask = vocab(V)
    eot, beg = sp["eot"], sp["beg"]
    val = base(1000 + seed, V, T_S * T_B).reshape(T_S, T_B, V).astype(np.float64)
    g = np.random.default_rng(seed)
    free = np.flatnonzero(~smask[:eot])
    for s in range(T_S):
        for b, kind in enumerate(ROW_KINDS):
            r = val[s, b]
            r[beg:] = -25 + 0.5 * r[beg:]
            r[eot] = -28
            if kind == "flat":
                r[:eot] = 1.0
                r[g.choice(free, 500, replace=False)] = -np.inf   # -inf entries inside a draw set
                continue
            if kind == "one":
                r[:] = -np.inf
                r[TEXT + 3 * b + s] = 2.0
                continue
            rest = lambda ids: np.log(np.exp(np.delete(r, ids)[np.delete(~smask, ids)]).sum())
            if kind == "peaked":
                ids = g.choice(free, 8, replace=False)
                r[ids] = rest(ids) + np.log(99.0 / 8) + g.uniform(-0.3, 0.3, 8)
            elif kind == "ends":
                ids = np.array([0, V - 1])
                r[ids] = rest(ids) + np.log([60.0, 39.0])
            else:  # rule
                lo = 200 * (b == 7)
                r[beg + lo:beg + lo + 400] = 9.0 + g.uniform(-0.5, 0.5, 400)
                r[g.choice(free, 1)] = 10.0
    return (val * T).astype(np.float32)


def emulate_f32_cdf(val32: np.ndarray, draw: np.ndarray, M2: np.float32):
    """The sampling walk's f32 arithmetic (finalize_ts_kernel): thread t owns ids [t C, t C + C), adds
    its expf(val - M2) serially, the 1024 sums go through a 10-level Hillis-Steele scan, and a
    boundary inside a chunk is the scanned sum before the chunk plus the serial adds up to it.
    -> the cumulative sum after every id, normalised by the total (f64 of the f32 values)."""
    V = val32.size
    C = -(-V // TW)
    e = np.zeros(TW * C, np.float32)
    e[:V] = np.where(draw, np.exp(np.where(draw, val32 - M2, np.float32(0)).astype(np.float32)), np.float32(0))
    e = e.reshape(TW, C)
    z = np.cumsum(e, axis=1, dtype=np.float32)[:, -1].copy()
    o = 1
    while o < TW:
        z[o:] = z[o:] + z[:-o].copy()
        o <<= 1
    lo = np.concatenate([[np.float32(0)], z[:-1]]).astype(np.float32)
    c = np.cumsum(np.concatenate([lo[:, None], e], axis=1), axis=1, dtype=np.float32)[:, 1:]
    return c.reshape(-1)[:V].astype(np.float64) / np.float64(z[-1])
