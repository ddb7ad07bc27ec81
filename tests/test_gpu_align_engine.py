"""DTW token timestamps through the engine (spt_transcribe_aligned) on
synthetic:tiny.en:enc=2:dec=2.

Against HF transformers (tests/golden/tiny_en_align.npz, written by tests/golden/make_golden_align.py):
the f32 engine's alignment-head probabilities, read back with spt_debug_align_last, lie within
8 x p_noise (relative) of HF's, p_noise being the largest relative difference between HF's own float32
and float64 runs -- the reference's error, not the engine's.  Random weights give a flat matrix, so
the path is not compared with HF's; instead the device path is exactly the f32 reference DTW of the
device's own matrix, and its cost on HF's matrix is within 2 x len x bar_m of HF's path's, bar_m being
the p bar carried through the normalisation (align_ref.norm_bars with 8 x p_noise as the unit).

The fixture's HF encoder runs with the tanh GELU on its two convolutions, as whisper.cpp, the oracle
and the engine do (HF hard-codes the erf form there whatever activation_function says: DESIGN.md 7;
make_golden_align.py asserts that its encoder is then the oracle's within 5e-6 relative L2).  With HF's erf
stem the same comparison gave 1.41e-3 (5 s) and 8.43e-4 (30 s), all of it that one activation: HF's own
decoder fed the oracle's encoder output moved p by 1.40e-3.  Seen on an MI355X against the bar of 5.19e-5
(p_noise 6.49e-6): 1.01e-5 at 5 s / n = 3, 1.36e-5 at 30 s / n = 11; the device path costs exactly what
HF's path costs on HF's matrix.

The fixture's text is fed through forced_tokens (n = 3 and n = 11), so the sampler's choices do not steer
the decode; the tokens recorded (and aligned) are still the sampler's, and are asserted equal to HF's.

Invariance and sanity in f32 / bf16 / f16: token times bitwise equal alone and in a batch and with
SPT_NO_GRAPH on and off (a process each), the result equal to spt_transcribe's, every window's times
non-decreasing and inside [seek, seek + 2 M], custom heads, a second window, a window of timestamp tokens
only (no token times), the test hooks allowed, and a beam / temperature-fallback call followed by an
unchanged plain call."""
import os

import numpy as np
import pytest

from oracle import oracle as O
from spittle_amd import TranscriptionError, WhisperEngine, WhisperInferenceParams, WhisperModelParams
from tests import align_ref as A

pytestmark = pytest.mark.gpu

SPEC = "synthetic:tiny.en:enc=2:dec=2"
GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "tiny_en_align.npz"))
P_NOISE = float(GOLD["p_noise"])
DT = ("f32", "bf16", "f16")


@pytest.fixture(scope="module", params=DT)
def eng(request):
    e = WhisperEngine(WhisperModelParams(dtype=request.param, max_batch=5))
    e.load_model(SPEC)
    yield e
    e.unload_model()


@pytest.fixture(scope="module")
def eng32():
    e = WhisperEngine(WhisperModelParams(dtype="f32", max_batch=2))
    e.load_model(SPEC)
    yield e
    e.unload_model()


def _greedy(n, forced=None):
    """whisper_full without timestamps or fallback, ending after n tokens: make_golden_align.py's greedy loop.
    forced [utterances][n]: the tokens fed step by step (teacher forcing), whatever the sampler chose."""
    return WhisperInferenceParams(no_timestamps=True, temperature_inc=0.0, max_new_tokens=n - 1,
                                  forced_tokens=None if forced is None else np.asarray(forced, np.int32))


_runs = {}


def _aligned(eng32, case):
    """One aligned call per fixture case: (result, p, m, path)."""
    if case not in _runs:
        n = len(GOLD[f"{case}_tokens"])
        x = O.synth_audio(0, int(GOLD[f"{case}_n_samples"]))
        # the text is fixed through forced_tokens: every step is fed the fixture's token, so a sampler
        # choice that differed from HF's would show in that one result token and not steer the rest
        r = eng32.transcribe_samples_aligned(x, _greedy(n, [GOLD[f"{case}_tokens"]]))
        _runs[case] = (r,) + tuple(eng32.debug_align_last())
    return _runs[case]


@pytest.mark.parametrize("case", ["s5", "s30"])
def test_probabilities_against_hf(eng32, case):
    toks = [int(t) for t in GOLD[f"{case}_tokens"]]
    r, p, m, _ = _aligned(eng32, case)
    assert r.tokens == toks, (r.tokens, toks, GOLD[f"{case}_gaps"])
    assert [t[0] for t in r.token_times] == list(range(len(toks)))
    hp, hm = GOLD[f"{case}_p"].astype(np.float64), GOLD[f"{case}_m"]
    assert p.shape == hp.shape == (6, len(toks) + 1, hm.shape[1]) and m.shape == hm.shape
    rel = float(np.max(np.abs(p - hp) / hp))
    print(f"{case}: largest relative difference of p {rel:.3e}, p_noise {P_NOISE:.3e}, bar {8 * P_NOISE:.3e}")
    assert rel <= 8 * P_NOISE


@pytest.mark.parametrize("case", ["s5", "s30"])
def test_path_against_hf(eng32, case):
    r, p, m, path = _aligned(eng32, case)
    hp, hm, hpath = GOLD[f"{case}_p"].astype(np.float64), GOLD[f"{case}_m"], GOLD[f"{case}_path"]
    # the device path is the f32 reference DTW of the device's own matrix, exactly
    ti, tj = A.dtw(-m, np.float32)
    assert np.array_equal(path[:, 0], ti) and np.array_equal(path[:, 1], tj)
    t0, t1 = A.token_times(A.jumps(ti, tj), 0)
    assert [t[1] for t in r.token_times] == list(t0) and [t[2] for t in r.token_times] == list(t1)
    # and on HF's matrix it costs no more than HF's own path, within the bar on m along the path
    bar_m = float((A.norm_bars(hp)[2] * (8 * P_NOISE / (4 * A.U32))).max())
    gap = A.path_cost(-hm, ti, tj) - A.path_cost(-hm, hpath[:, 0], hpath[:, 1])
    print(f"{case}: path cost above HF's {gap:.3e}, allowed {2 * max(len(ti), len(hpath)) * bar_m:.3e}")
    assert gap <= 2 * max(len(ti), len(hpath)) * bar_m


def _same(a, b):
    assert a.tokens == b.tokens and a.text == b.text and a.n_windows == b.n_windows and a.n_fallbacks == b.n_fallbacks
    assert np.array_equal(a.top1.view(np.uint32), b.top1.view(np.uint32))
    assert np.array_equal(a.top2.view(np.uint32), b.top2.view(np.uint32))
    assert [(s.start, s.end, s.text, s.i0, s.n_tokens) for s in a.segments] == \
           [(s.start, s.end, s.text, s.i0, s.n_tokens) for s in b.segments]


def _sane_windows(r, n_samples):
    """A call without timestamp tokens: window k starts at seek = 3000 k and is one segment.  Its token
    times are non-decreasing and lie in [seek, seek + 2 M], M = min(3000, seek_end - seek) / 2."""
    _sane(r, n_samples)
    seek_end = 1 + (n_samples - 200) // 160
    assert len(r.segments) == r.n_windows
    for k, sg in enumerate(r.segments):
        seek = 3000 * k
        M = min(3000, seek_end - seek) // 2
        win = [t for t in r.token_times if sg.i0 <= t[0] < sg.i0 + sg.n_tokens]
        assert win, k
        t0 = [t[1] for t in win]
        assert t0 == sorted(t0), (k, t0)
        assert all(seek <= t[1] <= t[2] <= seek + 2 * M for t in win), (k, seek, M, win)
        assert all(a[2] == b[1] for a, b in zip(win, win[1:]))  # a token ends where the next one starts


def _sane(r, n_samples):
    """One time per text token, ordered, inside the audio; nothing for timestamp and eot tokens."""
    sp = O.special_tokens(51864)
    text = [i for i, t in enumerate(r.tokens) if t < sp["eot"]]
    assert [t[0] for t in r.token_times] == text
    end = 1 + (n_samples - 200) // 160
    for _, t0, t1, p in r.token_times:
        assert 0 <= t0 <= t1 <= end and 0.0 <= p <= 1.0
    assert r.words == []  # a synthetic model has no vocabulary


def test_alone_and_in_a_batch(eng):
    xs = [O.synth_audio(0, 80000), O.synth_audio(1, 480000), O.synth_audio(2, 160000)]
    prm = WhisperInferenceParams(temperature_inc=0.0)  # timestamps on, greedy
    alone = [eng.transcribe_samples_aligned(x, prm) for x in xs]
    both = eng.transcribe_batch_aligned(xs, prm)
    for a, b, x in zip(alone, both, xs):
        _same(a, b)
        assert a.token_times == b.token_times and len(a.token_times) > 0
        _sane(a, x.size)
        _same(a, eng.transcribe_samples(x, prm))  # the result is spt_transcribe's
    # without timestamp tokens the windows are known, so every window's range and order can be held
    g = _greedy(9)
    alone = [eng.transcribe_samples_aligned(x, g) for x in xs]
    for a, b, x in zip(alone, eng.transcribe_batch_aligned(xs, g), xs):
        _same(a, b)
        assert a.token_times == b.token_times
        _sane_windows(a, x.size)


def test_times_follow_the_windows(eng):
    """45 s: the second window's tokens lie beyond its seek, each window's times are non-decreasing."""
    x = O.synth_audio(3, 720000)
    r = eng.transcribe_samples_aligned(x, _greedy(6))
    assert r.n_windows == 2 and len(r.segments) == 2  # without timestamps: one segment per window
    _sane_windows(r, x.size)
    cut = r.segments[1].i0
    first, second = [t for t in r.token_times if t[0] < cut], [t for t in r.token_times if t[0] >= cut]
    assert first and second
    for win, seek in ((first, 0), (second, 3000)):
        t0 = [t[1] for t in win]
        assert t0 == sorted(t0) and all(seek <= t[1] <= t[2] <= seek + 3000 for t in win)
    assert second[-1][2] > 3000


def test_custom_heads(eng):
    x = O.synth_audio(0, 80000)
    base = eng.transcribe_samples_aligned(x, _greedy(5))
    assert eng.debug_align_last()[0].shape[0] == 6  # the top half of two layers: layer 1, six heads
    eng.set_alignment_heads([(1, 2)])
    one = eng.transcribe_samples_aligned(x, _greedy(5))
    p1 = eng.debug_align_last()[0]
    assert p1.shape[0] == 1
    eng.set_alignment_heads([(0, 3), (1, 2), (1, 0)])
    assert eng.debug_align_last()[0].shape[0] == 1  # the last alignment stays readable
    three = eng.transcribe_samples_aligned(x, _greedy(5))
    p3 = eng.debug_align_last()[0]
    assert p3.shape[0] == 3 and np.array_equal(p3[1], p1[0])  # sorted by layer: (0, 3), (1, 2), (1, 0)
    for bad in ([(2, 0)], [(0, 6)], [(-1, 0)], [(1, 2), (1, 2)]):
        with pytest.raises(TranscriptionError):
            eng.set_alignment_heads(bad)
    assert eng.transcribe_samples_aligned(x, _greedy(5)).token_times == three.token_times  # a refused list changes nothing
    eng.set_alignment_heads([])
    again = eng.transcribe_samples_aligned(x, _greedy(5))
    assert again.token_times == base.token_times and one.tokens == base.tokens


@pytest.fixture(scope="module", params=DT)
def eng_ts(request):
    """Three decoder layers: whisper_full forces <|notimestamps|> on two-layer models of this vocabulary, so the
    model that must produce timestamp tokens has three (alignment heads: layers 1 and 2)."""
    e = WhisperEngine(WhisperModelParams(dtype=request.param, max_batch=2))
    e.load_model("synthetic:tiny.en:enc=2:dec=3")
    yield e
    e.unload_model()


def test_window_of_timestamp_tokens_only(eng_ts):
    """1.025 s of audio with timestamps on and any first timestamp allowed (max_initial_ts = 30): on this clip
    the timestamps together outweigh the likeliest text token, so the first token is a timestamp, after which
    less than a second is left (seek + seek_delta + 100 >= seek_end) and the window's result is that one
    token.  No text token: no replay, no token times, and the result is still spt_transcribe's."""
    sp = O.special_tokens(51864)
    eng = eng_ts
    x = O.synth_audio(4, 16400)
    prm = WhisperInferenceParams(temperature_inc=0.0, max_initial_ts=30.0)
    r = eng.transcribe_samples_aligned(x, prm)
    assert r.n_windows == 1 and len(r.tokens) >= 1 and all(t >= sp["eot"] for t in r.tokens), r.tokens
    assert r.token_times == [] and r.words == []
    _same(r, eng.transcribe_samples(x, prm))
    # beside an utterance that has text, in one call: the other's times are what they are alone
    y = O.synth_audio(5, 16400)  # the same length, and a text token first
    both = eng.transcribe_batch_aligned([x, y], prm)
    assert both[0].token_times == [] and both[0].tokens == r.tokens
    assert both[1].token_times == eng.transcribe_samples_aligned(y, prm).token_times != []


def test_hooks_stay_allowed(eng):
    """forced_tokens and SPT_IGNORE_EOT are refused by spt_transcribe on the whisper_full path and allowed by
    the aligned call; forcing changes what is fed, so (past the first token) what is decoded and aligned."""
    x = O.synth_audio(0, 80000)
    free = eng.transcribe_samples_aligned(x, _greedy(6))
    f = np.array([[100, 200, 300, 400, 500, 600]], np.int32)
    forced = eng.transcribe_samples_aligned(x, _greedy(6, f))
    assert forced.tokens[0] == free.tokens[0] and forced.tokens != free.tokens
    assert len(forced.token_times) == len([t for t in forced.tokens if t < O.special_tokens(51864)["eot"]])
    _sane_windows(forced, x.size)
    ign = WhisperInferenceParams(no_timestamps=True, temperature_inc=0.0, max_new_tokens=5, ignore_eot=True)
    assert eng.transcribe_samples_aligned(x, ign).token_times == free.token_times
    with pytest.raises(TranscriptionError):
        eng.transcribe_samples(x, WhisperInferenceParams(temperature_inc=0.2, forced_tokens=f))
    with pytest.raises(TranscriptionError):
        eng.transcribe_samples_aligned(x, WhisperInferenceParams(beam_size=2, temperature_inc=0.0, forced_tokens=f))


_NO_GRAPH_SCRIPT = """
import json, sys
import torch; torch.cuda.init()
from oracle import oracle as O
from spittle_amd import WhisperEngine, WhisperInferenceParams, WhisperModelParams
out = {}
for dt in ("f32", "bf16", "f16"):
    e = WhisperEngine(WhisperModelParams(dtype=dt, max_batch=2)); e.load_model("%s")
    for name, n in (("s5", 80000), ("s30", 480000)):
        r = e.transcribe_samples_aligned(O.synth_audio(0, n), WhisperInferenceParams(temperature_inc=0.0))
        out[dt + name] = [r.tokens, [list(t[:3]) + [float(t[3]).hex()] for t in r.token_times], e.call_stats()["decoder_passes"]]
    e.unload_model()
print("RESULT" + json.dumps(out))
"""


def test_graph_and_eager_passes_give_the_same_times():
    """SPT_NO_GRAPH is read once per process, so each setting runs in a process of its own: the decode is
    graph-replayed in one and eager in the other, the alignment's replay is eager in both, and tokens,
    token times and probabilities are bitwise equal in every dtype."""
    import json
    import subprocess
    import sys
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    got = []
    for no_graph in (False, True):
        env = {k: v for k, v in os.environ.items() if k != "SPT_NO_GRAPH"}
        if no_graph:
            env["SPT_NO_GRAPH"] = "1"
        run = subprocess.run([sys.executable, "-c", _NO_GRAPH_SCRIPT % SPEC], cwd=root, env=env, capture_output=True,
                             text=True, timeout=120)
        assert run.returncode == 0, run.stderr[-2000:]
        got.append(json.loads(next(l for l in run.stdout.splitlines() if l.startswith("RESULT"))[6:]))
    assert got[0] == got[1]
    assert all(len(v[1]) > 0 for v in got[0].values())


@pytest.mark.parametrize("kind", ["beam", "fallback"])
def test_cache_reuse_is_safe(eng, kind):
    """A beam-5 call and a temperature-fallback call are aligned once, for the decoder kept, and a plain
    call after the alignment is bitwise what it was before: the replay's use of the decode group's
    cache and step state leaves nothing behind."""
    x = O.synth_audio(4, 240000)
    plain = WhisperInferenceParams(temperature_inc=0.0)
    before = eng.transcribe_samples(x, plain)
    prm = WhisperInferenceParams(beam_size=5, temperature_inc=0.0) if kind == "beam" else \
        WhisperInferenceParams(temperature_inc=0.4, logprob_thold=0.0, best_of=3, seed=7)
    ref = eng.transcribe_samples(x, prm)
    r = eng.transcribe_samples_aligned(x, prm)
    _same(r, ref)
    _sane(r, x.size)
    if kind == "fallback":
        assert r.n_fallbacks > 0
    _same(eng.transcribe_samples(x, plain), before)
