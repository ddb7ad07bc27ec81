"""Float64 reference of the no-speech probability (spittle_amd/csrc/k_sample.hip dec_no_speech, DESIGN
4.6) with a per-case error bar, the crafted rows the kernel test runs, the faults the bar must be able
to see, and whisper_full's window loop restated with the silence skip.

The probability of a row l [V] is softmax(l)[nosp] over the raw logits: exp(l[nosp] - m) / sum_n
exp(l[n] - m), m = max l; a -inf logit contributes 0; a row holding a NaN or +inf gives NaN.

The bar (first order in u = 2^-24, from the kernel's operation count, not from its output):
  * the row is cut into CHUNKS contiguous chunks of CS = ceil(V / CHUNKS) columns; chunk c computes
    e_n = expf(fl(l_n - m_c)) against its own maximum: one rounding of the difference, amplified by its
    magnitude (u |l_n - m_c|), plus expf's 1 ulp (<= 2u);
  * the chunk's sum s_c: TS_J sequential adds per thread, a 6-level xor butterfly, 4 waves added in
    order: depth 13 + 6 + 4 = 23 adds of positive terms (23 u);
  * the merge rescales s_c by expf(fl(m_c - M)) (u |m_c - M| + 2u), multiplies (u) and adds the 16
    chunks in order (16 u);
  * the numerator expf(fl(l_nosp - M)) (u |l_nosp - M| + 2u) and the division (u).
Each term of the denominator enters with its weight w_n = exp(l_n - M) / Z.  1.05 covers the second
order; 2^-125 covers a result or a term flushed below the smallest normal f32.
"""
from __future__ import annotations

import numpy as np

CHUNKS, TS_T, TS_J = 16, 256, 13          # k_sample.hip / kernels.h
MAX_V = CHUNKS * TS_T * TS_J              # 53248
U = 2.0 ** -24
SUM_DEPTH = TS_J + 6 + TS_T // 64
VOCABS = (17, 4096, 51864, 51865, 51866, 53248)


def chunk_size(V: int) -> int:
    return (V + CHUNKS - 1) // CHUNKS


def prob(row, nosp: int) -> float:
    """float64 softmax(row)[nosp]; NaN for a row holding a NaN or +inf"""
    l = np.asarray(row, np.float64)
    if np.isnan(l).any() or np.isposinf(l).any():
        return float("nan")
    M = l.max()
    with np.errstate(invalid="ignore"):
        e = np.where(np.isneginf(l), 0.0, np.exp(l - M))
    return float(e[nosp] / e.sum())


def bar(row, nosp: int) -> float:
    """the kernel's error bound on prob(row, nosp) (module docstring); 0 where the result is NaN"""
    l = np.asarray(row, np.float64)
    V = l.size
    p = prob(l, nosp)
    if not np.isfinite(p):
        return 0.0
    M = l.max()
    fin = ~np.isneginf(l)
    w = np.zeros(V)
    w[fin] = np.exp(l[fin] - M)
    Z = w.sum()
    CS = chunk_size(V)
    dist = np.zeros(V)                    # |l_n - m_c| + |m_c - M| of each finite term
    for c in range(CHUNKS):
        a, b = c * CS, min(V, (c + 1) * CS)
        if a >= b or not fin[a:b].any():
            continue
        mc = l[a:b][fin[a:b]].max()
        dist[a:b] = np.where(fin[a:b], np.abs(np.where(fin[a:b], l[a:b], mc) - mc) + abs(mc - M), 0.0)
    denom = float((w * (U * dist + 2 * U)).sum() / Z) + (SUM_DEPTH + 3 + CHUNKS) * U
    numer = (U * abs(l[nosp] - M) + 2 * U) if fin[nosp] else 0.0
    return 1.05 * p * (denom + numer + U) + 2.0 ** -125


# ----------------------------------------------------------------------------- crafted rows
def positions(V: int) -> dict:
    """the nosp columns the cases use: the row's ends and the two sides of a chunk boundary"""
    CS = chunk_size(V)
    k = (V - 1) // CS                     # the last chunk that holds a column
    assert k >= 1, "the cases need at least two chunks with columns"
    edge = CS * max(1, k // 2)            # the first column of a chunk in the middle of the row
    return {"first": 0, "last": V - 1, "chunk_end": edge - 1, "chunk_begin": edge}


def rows(V: int, nosp: int, pad: int = 5, seed: int = 0):
    """-> (names, logits [n][V + pad] f32): the row shapes and contents of the issue's table for one
    (V, nosp); the pad columns hold +1e30 and NaN alternately and must never be read"""
    rng = np.random.Generator(np.random.PCG64(seed * 100003 + V * 7 + nosp))
    base = (3.0 * rng.standard_normal(V)).astype(np.float32)
    out = {}
    out["equal"] = np.full(V, 1.25, np.float32)
    r = base.copy(); r[nosp] = np.delete(base, nosp).max() + 80.0 if V > 1 else 0.0; out["max_by_80"] = r
    r = base.copy(); r[nosp] = base.max() - 80.0; out["80_below"] = r
    r = base.copy(); r[nosp] = -np.inf; out["nosp_minus_inf"] = r
    r = np.full(V, -np.inf, np.float32); r[nosp] = base[nosp]; r[(nosp + V // 2) % V] = base[nosp] + 1.0
    out["minus_inf_elsewhere"] = r
    out["offset_plus_1e4"] = (base + np.float32(1e4)).astype(np.float32)
    out["offset_minus_1e4"] = (base - np.float32(1e4)).astype(np.float32)
    out["random"] = base.copy()
    r = base.copy(); r[(nosp + 3) % V] = np.nan; out["nan_row"] = r
    r = base.copy(); r[(nosp + 5) % V] = np.inf; out["plus_inf_row"] = r
    names = list(out)
    lg = np.empty((len(names), V + pad), np.float32)
    for i, n in enumerate(names):
        lg[i, :V] = out[n]
        lg[i, V:] = [1e30 if j % 2 == 0 else np.nan for j in range(pad)]
    return names, lg


# ----------------------------------------------------------------------------- faults (the power check)
def fault_prob(row_padded, V: int, nosp: int, fault: str, suppress=None) -> float:
    """what a wrong kernel would return (float64), for the faults DESIGN 4.6 lists"""
    full = np.asarray(row_padded, np.float64)
    l = full[:V].copy()
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        if fault == "no_max_subtraction":
            e = np.exp(l.astype(np.float32)).astype(np.float64)   # f32 exp of the raw logit
            return float(e[nosp] / e.sum())
        if fault == "suppressed_logits":
            l[np.asarray(suppress, bool)] = -np.inf
            return prob(l, nosp)
        if fault == "temperature":
            return prob(l / 0.2, nosp)
        if fault == "drop_last_tail":     # the last chunk stops at a multiple of the thread count
            CS = chunk_size(V)
            a = ((V - 1) // CS) * CS
            keep = a + (V - a) // TS_T * TS_T
            M = l.max()
            e = np.where(np.isneginf(l), 0.0, np.exp(l - M))
            return float(e[nosp] / e[:keep].sum())
        if fault == "read_pad":
            return prob(full, nosp)
        if fault == "merge_without_rescale":
            CS = chunk_size(V)
            M = l.max()
            z = 0.0
            for c in range(CHUNKS):
                a, b = c * CS, min(V, (c + 1) * CS)
                if a < b and np.isfinite(l[a:b]).any():
                    z += np.exp(l[a:b] - l[a:b].max()).sum()
            return float(np.exp(l[nosp] - M) / z)
    raise ValueError(fault)


FAULTS = ("no_max_subtraction", "suppressed_logits", "temperature", "drop_last_tail", "read_pad",
          "merge_without_rescale")


# ----------------------------------------------------------------------------- the rule
def skip_rule(p: float, avg: float, no_speech_thold: float, logprob_thold: float) -> bool:
    """the threshold is on iff 0 < thold < 1; strict > and strict <; a NaN is never above"""
    if not (0.0 < no_speech_thold < 1.0):
        return False
    return bool(p > no_speech_thold and avg < logprob_thold)


def ln_prob(logits, nosp: int) -> float:
    l = np.asarray(logits, np.float64)
    M = l.max()
    return float(l[nosp] - M - np.log(np.exp(l - M).sum()))


def transcribe(m, pcm, p, no_speech_thold: float = 0.0, prompt=(), lang_tok: int = -1):
    """oracle.whisper_full.transcribe restated with the no-speech probability of every window and the
    skip rule.  -> dict(windows = [dict(seek, seek_delta, i0, n_tokens, skipped, ln_p, p, avg, prefix)],
    segments, tokens, kept)."""
    from oracle import oracle as O
    from oracle import whisper_full as WF
    sp = O.special_tokens(m.dims.n_vocab)
    eot, beg = sp["eot"], sp["beg"]
    multi = sp["n_langs"] > 0
    no_ts = p.no_timestamps or (m.dims.n_dec == 2 and m.dims.n_vocab != 51866)
    pp = WF.Params(**{**p.__dict__, "no_timestamps": no_ts})
    init = [sp["sot"]]
    if multi:
        init += [lang_tok if lang_tok >= 0 else sp["sot"] + 1, sp["translate"] if p.translate else sp["transcribe"]]
    if no_ts:
        init.append(sp["not"])
    n_max = m.dims.n_text_ctx // 2 - 4
    seek, seek_end = 0, WF.n_len_org(len(pcm))
    past = list(prompt)
    mel_all = O.mel_full(pcm, m.dims.n_mels)
    wins, segs, all_toks, kept = [], [], [], []
    while seek + 100 < seek_end:
        if seek > 0 and seek + 500 >= seek_end:
            past = []
        pf = []
        if past and p.n_max_text_ctx > 0:
            n_take = min(p.n_max_text_ctx, m.dims.n_text_ctx // 2, len(past))
            pf = [sp["prev"]] + past[len(past) - n_take:]
        enc = m.encode(O.mel_window(mel_all, seek))
        lnp = ln_prob(m.logits(enc, pf + init), sp["nosp"])
        steps = min(n_max, m.dims.n_text_ctx + 1 - len(pf) - len(init))
        if p.beam_size > 1:
            decs = WF.decode_window_beam(m, enc, pf + init, seek, seek_end, pp, steps)
        else:
            decs = [WF.decode_window(m, enc, pf + init, seek, seek_end, pp, steps)]

        def scored(w):  # whisper_sequence_score + the entropy check: (failed, score, avg)
            if w.status == 2:
                return True, -np.inf
            rl = w.result_len
            if rl == 0:
                return False, -np.inf
            toks_ = [s.tok for s in w.steps]
            cnt = {}
            for t in toks_[max(0, rl - 32):rl]:
                cnt[t] = cnt.get(t, 0) + 1
            n = sum(cnt.values())
            ent = -sum(c / n * np.log(c / n) for c in cnt.values())
            sc = sum(s.plog for s in w.steps[:rl]) / rl
            if rl > 32 and ent < p.entropy_thold:
                return True, sc
            return False, sc

        best, best_score = 0, -np.inf
        flags = [scored(w) for w in decs]
        for d, (f, sc) in enumerate(flags):
            if not f and best_score < sc:
                best, best_score = d, sc
        w = decs[best]
        failed = flags[best][0]
        avg = flags[best][1] if w.status != 2 else -np.inf   # full.cpp score(): avg is set unless failed before
        skipped = skip_rule(np.exp(lnp), avg, no_speech_thold, p.logprob_thold)
        toks = [s.tok for s in w.steps]
        tids = [s.tid for s in w.steps]
        n_keep = 0 if skipped else len(toks) if failed else min(w.result_len, len(toks))
        toks, tids = toks[:n_keep], tids[:n_keep]
        base = len(all_toks)
        adv = w.seek_delta if w.seek_delta > 0 else 3000
        wins.append(dict(seek=seek, seek_delta=adv, i0=base, n_tokens=n_keep, skipped=int(skipped), ln_p=lnp,
                         p=float(np.exp(lnp)), avg=float(avg), prefix=list(pf), window=w))
        all_toks += toks
        kept += w.steps[:n_keep]
        past = (pf[1:] if pf else []) + ([] if skipped else [s.tok for s in w.steps[:w.result_len]])
        if toks:
            i0, t0, text, i = 0, seek + 2 * (tids[0] - beg), "", 0
            while i < len(toks):
                if toks[i] < eot:
                    text += f"[{toks[i]}]"
                if toks[i] > beg:
                    t1 = seek + 2 * (tids[i] - beg)
                    if text:
                        segs.append((t0, t1, text, base + i0, i - i0 + 1))
                    text = ""
                    while i < len(toks) and toks[i] > beg:
                        i += 1
                    i -= 1
                    t0, i0 = t1, i + 1
                i += 1
            if text:
                segs.append((t0, seek + w.seek_delta, text, base + i0, len(toks) - i0))
        seek += adv
    return dict(windows=wins, segments=segs, tokens=all_toks, kept=kept)
