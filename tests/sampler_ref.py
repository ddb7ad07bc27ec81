"""Float64 reference of the sampler kernels (spittle_amd/csrc/k_sample.hip) for
tests/test_gpu_sampler.py, on the inputs the spt_debug_sample_* hooks take.

  * Greedy token, beam candidates and bookkeeping are oracle/whisper_full.py's pick / topk /
    bookkeep as they are (pinned against HF transformers by tests/test_timestamp_rules_hf.py);
    replay() only drives them over S steps of B rows with the kernels' conventions for rows that
    are not live, forced tokens and rows where nothing survives.
  * Temperature sampling is stated here from its definition (whisper_process_logits +
    whisper_sample_token with the project's counter-based draw): sample().
  * kv_gather(): numpy indexing.
"""
from __future__ import annotations

import copy
from dataclasses import dataclass

import numpy as np

from oracle import whisper_full as W

M64 = (1 << 64) - 1


def u01(seed: int, b: int, step: int) -> float:
    """The draw of (seed, row, step): splitmix64's finaliser over a counter, top 24 bits -> [0, 1)."""
    z = (seed * 0x9E3779B97F4A7C15 + (b << 32) + step + 0x632BE59BD9B4E019) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return (z >> 40) / 16777216.0


def round_dtype(a, dtype: str) -> np.ndarray:
    """f32 -> the engine's storage dtype (round to nearest even) -> f32."""
    a = np.ascontiguousarray(a, np.float32)
    if dtype == "f32":
        return a.copy()
    if dtype == "f16":
        return a.astype(np.float16).astype(np.float32)
    u = a.view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) >> 16 << 16
    return (u & 0xFFFFFFFF).astype(np.uint32).view(np.float32).reshape(a.shape)


@dataclass
class Prm:
    """The fields of spittle_amd.sampler_debug.SampleParams the reference reads."""
    temperature: float = 0.0
    suppress_blank: bool = True
    no_ts: bool = False
    max_initial: int = 50
    n_max: int = 220
    max_tokens: int = 0
    seed: int = 0

    def w(self) -> W.Params:
        return W.Params(no_timestamps=bool(self.no_ts), suppress_blank=bool(self.suppress_blank),
                        max_tokens=self.max_tokens)


def rule_mask(step: int, toks: list, w: W.Window, prm, sp: dict, smask: np.ndarray, blank: int) -> np.ndarray:
    """whisper_process_logits' masked tokens of one row at one step (True = removed)."""
    eot, beg = sp["eot"], sp["beg"]
    m = np.array(smask, bool)
    if step == 0 and prm.suppress_blank:
        m[[eot, blank]] = True
    if prm.no_ts:
        m[beg:] = True
    if toks and toks[-1] >= beg:              # the last token was a timestamp
        if len(toks) < 2 or toks[-2] >= beg:  # ... and closed a pair: text next
            m[beg:] = True
        else:                                 # ... and opened one: a timestamp or [eot] next
            m[:eot] = True
    if step == 0 and prm.max_initial >= 0:
        m[beg + prm.max_initial + 1:] = True
    if w.has_ts:
        m[beg:beg + w.seek_delta // 2] = True
    return m


def _lse(v: np.ndarray) -> float:
    M = v.max()
    return float(np.log(np.exp(v - M).sum()) + M)


def sample(lg: np.ndarray, u: float, step: int, toks: list, w: W.Window, prm, sp: dict, smask: np.ndarray,
           blank: int) -> dict:
    """One temperature > 0 draw.  val = f32(lg) / f32(T) (the inputs' one f32 operation), then f64:
    lse over every unmasked token; the timestamp rule (summed timestamp probability above the
    best text token's); the draw set = the survivors, text removed when the rule fires; the draw is
    the inverse CDF of softmax(val) over the draw set in ascending id at u.
    -> dict(tok, plog, tid, rule, ids (the draw set), lo / hi (each member's CDF interval))."""
    beg = sp["beg"]
    val = (np.asarray(lg, np.float32) / np.float32(prm.temperature)).astype(np.float64)
    keep = ~rule_mask(step, toks, w, prm, sp, smask, blank) & np.isfinite(val)
    if not keep.any():
        return dict(tok=-2, plog=np.nan, tid=0, rule=False, ids=np.zeros(0, int), lo=np.zeros(0), hi=np.zeros(0))
    lse = _lse(val[keep])
    kt, ks = keep.copy(), keep.copy()
    kt[beg:] = False
    ks[:beg] = False
    rule = bool(ks.any() and (not kt.any() or _lse(val[ks]) > val[kt].max()))
    ids = np.flatnonzero(ks if rule else keep)
    p = np.exp(val[ids] - val[ids].max())
    cdf = np.cumsum(p) / p.sum()
    cdf[-1] = 1.0
    j = int(np.searchsorted(cdf, u, side="right"))
    tok = int(ids[j])
    tid = tok if tok >= beg else (int(np.flatnonzero(ks)[np.argmax(val[ks])]) if ks.any() else 0)
    return dict(tok=tok, plog=float(val[tok] - lse), tid=tid, rule=rule, ids=ids,
                lo=np.concatenate([[0.0], cdf[:-1]]), hi=cdf)


# the branches of W.bookkeep a step can take (labels only: the state itself comes from W.bookkeep)
BRANCHES = ("ts_first", "ts_later", "ts_backwards", "eot_result", "eot_no_result", "max_tokens", "end_of_audio",
            "end_of_audio_no_result_kept", "no_ts_complete", "guard_fail", "guard_pass")


def _branches(before: W.Window, after: W.Window, tok: int, i: int, seek: int, seek_end: int, prm, sp: dict) -> set:
    eot, beg = sp["eot"], sp["beg"]
    hts, sd, rl = before.has_ts, before.seek_delta, before.result_len
    out, status = set(), 0
    if tok > beg:
        if hts and sd > 2 * (tok - beg) and rl < i:
            out, status = {"ts_backwards"}, 2
        else:
            out.add("ts_later" if hts else "ts_first")
            hts, sd, rl = True, 2 * (tok - beg), i + 1
    end_audio = hts and seek + sd + 100 >= seek_end
    by_max = prm.max_tokens > 0 and i >= prm.max_tokens
    if status == 0 and (tok == eot or by_max or end_audio):
        status = 1
        if rl == 0 and not prm.no_ts:
            if seek + sd + 100 >= seek_end:
                out.add("end_of_audio_no_result_kept")
            else:
                out.add("eot_no_result")
                status = 2
        if status == 1:
            out |= {n for n, c in (("eot_result", tok == eot and rl > 0), ("max_tokens", by_max),
                                   ("end_of_audio", end_audio), ("no_ts_complete", prm.no_ts)) if c}
    elif status == 0 and i == prm.n_max - 1:
        status = 2 if rl == 0 or sd < 1500 else 0
        out.add("guard_fail" if status else "guard_pass")
    assert status == after.status, (out, status, after)
    return out


def replay(logits, prm, sp: dict, smask, blank: int, seek, seek_end, n_vocab=None, state=None, done=None,
           forced=None, out_cap=None, step=0, history=None) -> dict:
    """S steps of B rows as the token path of the hook runs them: logits [S][B][ldl].
    history: the [B][out_cap] initial out_tok when step > 0.  -> the hook's outputs (out_tok / out_plog
    / out_tid pre-filled with -9 / 0 / -9), float64, plus reached = the bookkeeping branches taken and min_margin = the smallest greedy
    decision gap W.pick reported."""
    lg = np.asarray(logits)
    S, B, ldl = lg.shape
    V = ldl if n_vocab is None else n_vocab
    eot = sp["eot"]
    cap = S + step if out_cap is None else out_cap
    seek = np.broadcast_to(seek, (B,))
    seek_end = np.broadcast_to(seek_end, (B,))
    st = np.zeros((B, 4), np.int64) if state is None else np.array(state, np.int64).reshape(B, 4)
    dn = np.zeros(B, np.int64) if done is None else np.array(done, np.int64).reshape(B)
    fc = None if forced is None else np.asarray(forced).reshape(B, -1)
    out_tok = np.full((B, cap), -9, np.int64) if history is None else np.array(history, np.int64)
    out_plog = np.zeros((B, cap))
    out_tid = np.full((B, cap), -9.0)
    next_tok = np.full(B, -9, np.int64)
    smask = np.asarray(smask, bool)
    wp = prm.w()
    reached, min_margin = set(), np.inf
    for s in range(S):
        i = step + s
        for b in range(B):
            live = i < cap and not dn[b]
            nxt = eot
            if live:
                w = W.Window(has_ts=bool(st[b, 0]), seek_delta=int(st[b, 1]), result_len=int(st[b, 2]))
                toks = [int(t) for t in out_tok[b, :i]]
                row = lg[s, b, :V]
                if prm.temperature > 0:
                    r = sample(row, u01(prm.seed, b, i), i, toks, w, prm, sp, smask, blank)
                    tok, plog, tid = r["tok"], r["plog"], r["tid"]
                elif (np.isfinite(row.astype(np.float64)) & ~rule_mask(i, toks, w, prm, sp, smask, blank)).any():
                    tok, plog, tid, mg = W.pick(row, i, toks, w, wp, sp, smask, blank, prm.max_initial)
                    min_margin = min(min_margin, mg)
                else:
                    tok = -2
                if tok == -2:  # nothing survives: the row fails
                    out_tok[b, i], out_plog[b, i], out_tid[b, i] = -2, np.nan, 0
                    st[b, 3], dn[b] = 2, 1
                    reached.add("nothing_survives")
                else:
                    out_tok[b, i], out_plog[b, i], out_tid[b, i] = tok, plog, tid
                    before = copy.copy(w)
                    W.bookkeep(w, tok, i, int(seek[b]), int(seek_end[b]), wp, sp, prm.n_max)
                    reached |= _branches(before, w, tok, i, int(seek[b]), int(seek_end[b]), prm, sp)
                    st[b] = [int(w.has_ts), w.seek_delta, w.result_len, w.status]
                    if w.status:
                        dn[b] = 1
                nxt = int(out_tok[b, i])
                if fc is not None and i < fc.shape[1]:
                    nxt = int(fc[b, i])
            elif i < cap:
                out_tok[b, i], out_plog[b, i], out_tid[b, i] = -1, -np.inf, -1
                reached.add("not_live_record")
            else:
                reached.add("past_out_cap")
            next_tok[b] = nxt if 0 <= nxt < V else eot
    return dict(out_tok=out_tok, out_plog=out_plog, out_tid=out_tid, state=st, done=dn, next_tok=next_tok,
                step=step + S, reached=reached, min_margin=min_margin)


def embed(next_tok, emb, pos, pos0_last: int, Tq: int, dtype: str) -> np.ndarray:
    """x of the last step: round_dtype(emb[next_tok]) + pos[min(pos0 + Tq, ctx - 1)], one f32 add
    (pos0_last: pos0 as the last step read it)."""
    pos = np.asarray(pos, np.float32)
    pn = min(pos0_last + Tq, pos.shape[0] - 1)
    return round_dtype(emb, dtype)[np.asarray(next_tok)] + pos[pn][None, :]


def beam(lg, row, step: int, k: int, prm, sp: dict, smask, blank: int):
    """W.topk for one row of the beam hook: row = (last, previous token, has_ts, seek_delta).
    -> (ids [8], lps [8], tid): the tail beyond the survivors is -1 / -inf."""
    last, pen, has_ts, sd = (int(v) for v in row)
    toks = [] if step == 0 else ([last] if step == 1 else [pen, last])
    w = W.Window(has_ts=bool(has_ts), seek_delta=sd)
    v = np.asarray(lg, np.float64)
    keep = np.isfinite(v) & ~rule_mask(step, toks, w, prm, sp, np.asarray(smask, bool), blank)
    ids, lps = np.full(8, -1, np.int64), np.full(8, -np.inf)
    if not keep.any():
        return ids, lps, 0
    out, _ = W.topk(np.asarray(lg), step, toks, w, prm.w(), sp, np.asarray(smask, bool), k, blank, prm.max_initial)
    for j, (t, lp, _tid) in enumerate(out):
        ids[j], lps[j] = t, lp
    ks = keep.copy()
    ks[:sp["beg"]] = False
    tid = int(np.flatnonzero(ks)[np.argmax(v[ks])]) if ks.any() else 0
    return ids, lps, tid


def kv_gather(src, dst, rows, pos0: int, dtype: str) -> np.ndarray:
    """dst row b <- src row rows[b] at positions < pos0 of [L][2][B][H][ctx][64], in dtype's storage."""
    s, out = round_dtype(src, dtype), round_dtype(dst, dtype)
    for b, r in enumerate(rows):
        out[:, :, b, :, :pos0] = s[:, :, r, :, :pos0]
    return out
