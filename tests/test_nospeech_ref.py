"""CPU checks of tests/nospeech_ref.py: the float64 no-speech probability and its bar on the crafted
rows, the bar's power against the faults DESIGN 4.6 lists, an f32 restatement of the kernel's
summation order inside the bar, the skip rule's boundaries, and the restated window loop against
oracle.whisper_full.transcribe."""
import math

import numpy as np
import pytest

from tests import nospeech_ref as R


def _all_cases():
    for V in R.VOCABS:
        for pos, nosp in R.positions(V).items():
            names, lg = R.rows(V, nosp)
            for i, n in enumerate(names):
                yield V, pos, nosp, n, lg[i]


CASES = list(_all_cases())


def test_positions_sit_on_a_chunk_boundary():
    for V in R.VOCABS:
        p, CS = R.positions(V), R.chunk_size(V)
        assert p["first"] == 0 and p["last"] == V - 1
        assert p["chunk_begin"] % CS == 0 and p["chunk_end"] == p["chunk_begin"] - 1 and 0 < p["chunk_begin"] < V
    assert R.MAX_V == 53248 and R.chunk_size(53248) == R.TS_T * R.TS_J


def test_reference_values():
    for V, pos, nosp, name, row in CASES:
        p = R.prob(row[:V], nosp)
        if name == "equal":
            assert p == pytest.approx(1.0 / V, rel=1e-12)
        elif name == "max_by_80":
            assert 1.0 - p < V * math.exp(-80.0)
        elif name == "80_below":
            assert 0.0 < p <= math.exp(-80.0)
        elif name == "nosp_minus_inf":
            assert p == 0.0
        elif name == "minus_inf_elsewhere":
            assert p == pytest.approx(1.0 / (1.0 + math.e), rel=1e-6)
        elif name in ("nan_row", "plus_inf_row"):
            assert math.isnan(p)
        elif name.startswith("offset"):
            assert 0.0 < p < 1.0
    # the max subtraction: an offset row is the random row's softmax up to the rounding of the sum in f32
    for V in R.VOCABS:
        nosp = R.positions(V)["last"]
        names, lg = R.rows(V, nosp)
        a = lg[names.index("random"), :V].astype(np.float64)
        assert R.prob(a + 1e4, nosp) == pytest.approx(R.prob(a, nosp), rel=1e-9)


def test_bar_is_tight_and_positive():
    """a few hundred u at the most: the bar is no licence"""
    for V, pos, nosp, name, row in CASES:
        p, b = R.prob(row[:V], nosp), R.bar(row[:V], nosp)
        if math.isnan(p):
            assert b == 0.0
            continue
        assert b > 0.0
        assert b <= p * 200 * R.U + 2.0 ** -125, (V, pos, name, b / max(p, 1e-300))


def _kernel_f32(row, V, nosp):
    """dec_no_speech's arithmetic restated in numpy float32, in its summation order"""
    f = np.float32
    CS = R.chunk_size(V)
    l = np.asarray(row[:V], f)
    cm, cs = [], []
    for c in range(R.CHUNKS):
        n0, n1 = c * CS, min(V, (c + 1) * CS)
        idx = n0 + np.arange(R.TS_T)[:, None] + R.TS_T * np.arange(R.TS_J)[None, :]   # [tid][j]
        inb = idx < n1
        v = l[np.minimum(idx, V - 1)]
        bad = bool((inb & (np.isnan(v) | np.isposinf(v))).any())
        m = f(np.max(np.where(inb & ~np.isnan(v), v, f(-np.inf)))) if inb.any() else f(-np.inf)
        with np.errstate(invalid="ignore", over="ignore"):
            e = np.where(inb & np.isfinite(m), np.exp((v - m).astype(f)).astype(f), f(0))
        t = np.zeros(R.TS_T, f)
        for j in range(R.TS_J):
            t = (t + e[:, j]).astype(f)
        t = t.reshape(R.TS_T // 64, 64)
        o = 32
        while o:
            t = (t + t[:, np.arange(64) ^ o]).astype(f)
            o >>= 1
        z = f(0)
        for wv in range(R.TS_T // 64):
            z = f(z + t[wv, 0])
        cm.append(m)
        cs.append(f(np.nan) if bad else z)
    M = f(max(cm))
    z = f(0)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(R.CHUNKS):
            if np.isfinite(cm[c]) or np.isnan(cs[c]):
                z = f(z + f(cs[c] * f(np.exp(f(cm[c] - M)))))
        return f(f(np.exp(f(l[nosp] - M))) / z)


def test_f32_restatement_is_inside_the_bar():
    worst = 0.0
    for V, pos, nosp, name, row in CASES:
        if V in (51864, 51865) and pos != "last":
            continue  # the same paths as 51866; kept on the GPU, trimmed here for time
        want, got = R.prob(row[:V], nosp), float(_kernel_f32(row, V, nosp))
        if math.isnan(want):
            assert math.isnan(got), (V, pos, name)
            continue
        b = R.bar(row[:V], nosp)
        assert abs(got - want) <= b, (V, pos, name, got, want, b)
        worst = max(worst, abs(got - want) / b)
    print(f"largest |f32 restatement - f64| / bar = {worst:.3f}")


def test_every_fault_moves_the_reference_by_100_bars():
    for fault in R.FAULTS:
        seen = 0.0
        for V, pos, nosp, name, row in CASES:
            want = R.prob(row[:V], nosp)
            if math.isnan(want):
                continue
            sup = np.zeros(V, bool)
            sup[nosp] = True
            got = R.fault_prob(row, V, nosp, fault, suppress=sup)
            moved = math.inf if not math.isfinite(got) else abs(got - want) / R.bar(row[:V], nosp)
            seen = max(seen, moved)
        assert seen >= 100.0, (fault, seen)


def test_rule_boundaries():
    assert R.skip_rule(0.61, -1.5, 0.6, -1.0)
    assert not R.skip_rule(0.6, -1.5, 0.6, -1.0)            # p == thold: strict >
    assert not R.skip_rule(0.61, -1.0, 0.6, -1.0)           # avg == logprob_thold: strict <
    assert not R.skip_rule(float("nan"), -1.5, 0.6, -1.0)   # a NaN is never above the threshold
    assert not R.skip_rule(0.61, float("nan"), 0.6, -1.0)
    assert R.skip_rule(0.61, -math.inf, 0.6, -1.0)          # a decoder without a result
    assert not R.skip_rule(0.99, -5.0, 0.0, -1.0)           # 0: off
    assert not R.skip_rule(1.0, -5.0, 1.0, -1.0)            # >= 1: off
    assert not R.skip_rule(0.99, -5.0, 1.5, -1.0)
    assert not R.skip_rule(0.99, -5.0, 0.5, -20.0)          # "never": nothing is that improbable


def test_restated_loop_is_the_oracles_with_the_threshold_off():
    from oracle import oracle as O
    from oracle import whisper_full as WF
    m = O.Model(O.dims_for("tiny.en", 1, 3), 1234, O.W_F32)
    pcm = O.synth_audio(5, 16000 * 12)
    p = WF.Params(max_tokens=8)   # short windows: every step recomputes the decoder over its prefix
    wins, segs, toks, kept = WF.transcribe(m, pcm, p)
    r = R.transcribe(m, pcm, p, 0.0)
    assert r["tokens"] == toks and r["segments"] == segs
    assert [w["seek"] for w in r["windows"]] == [s for s, _ in wins]
    assert all(not w["skipped"] and 0.0 < w["p"] < 1.0 for w in r["windows"])
    # a threshold under every window's probability with logprob_thold above every average: all skipped,
    # the seek loop unchanged
    lo = min(w["p"] for w in r["windows"]) / 2
    s = R.transcribe(m, pcm, WF.Params(max_tokens=8, logprob_thold=1.0), lo)
    assert s["tokens"] == [] and s["segments"] == [] and all(w["skipped"] for w in s["windows"])
    assert [w["seek"] for w in s["windows"]][0] == 0
    m.close()
