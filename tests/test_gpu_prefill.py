"""SPT_BLOCK_PREFILL through the public interface: a prompt prefix of at least P_min = 17
positions (the measured crossover; the 9-token oracle cases run on contexts built with
SPT_BLOCK_PREFILL_MIN=8, the constructor-time switch, so that the block pass is held to the oracle at P = 10 too) goes through the decoder in one block pass per sequence slice (GEMMs + the prefill attention
kernels) instead of ceil(P / 4) chunked passes.  Small synthetic models only.

Bars are those of the existing prompt and large-v3 tests (copied here, the old files are untouched):
  f32 tiny / tiny.en         tokens equal until the oracle's top-1 / top-2 gap falls below 2e-3, top-1
                             within 2e-3 on the agreed prefix (tests/test_gpu_parity.py _check_greedy)
  bf16 large-v3 2 + 2        margin 0.1, top-1 within 0.05 (test_transcribe_bf16_teacher_forced)
  f16 large-v3 2 + 2         margin 0.5, top-1 within 0.25 (test_transcribe_f16_teacher_forced)
An empty agreed prefix fails.  The audio seeds were picked on the CPU from the oracle alone so that each
case's agreed prefix covers at least 8 of the 12 tokens decoded (AUDIO below).  Against the chunked path
the results differ in the low bits (another accumulation order), so flag on is compared with flag off up
to the first step whose flag-off gap is below the same margin.  What must be bitwise is: a sequence in a
batch against itself alone, a sliced workspace against an unsliced one, and a plain call after a flagged
one against a plain call on a fresh context."""
import math

import numpy as np
import pytest

from oracle import ggml as G
from oracle import oracle as O
from oracle import whisper_full as W

pytestmark = pytest.mark.gpu

SEED = 1234
FLAGS = O.SUPPRESS_BLANK | O.NO_TIMESTAMPS | O.IGNORE_EOT
N_TOK = 12
P_MIN = 17
TINY_EN, TINY, LARGE22 = "synthetic:tiny.en", "synthetic:tiny", "synthetic:large-v3:enc=2:dec=2"
# (spec, dtype) -> oracle config, layers, decision margin, top-1 bound
MODELS = {(TINY_EN, "f32"): ("tiny.en", None, 2e-3, 2e-3), (TINY, "f32"): ("tiny", None, 2e-3, 2e-3),
          (LARGE22, "bf16"): ("large-v3", 2, 0.1, 0.05), (LARGE22, "f16"): ("large-v3", 2, 0.5, 0.25)}
# audio seed per (spec, dtype, prompt tokens), from the oracle alone: the first seed from 40 up whose
# first 10 decisions all clear the margin (5 s of synth_audio)
AUDIO = {(LARGE22, "bf16", 9): 43, (LARGE22, "f16", 9): 43, (LARGE22, "f16", 223): 41}
N_PAST = (9, 64, 223, 300)  # 300: the last-224 rule, P = 225


def _f16(x):
    return np.ascontiguousarray(x, np.float32).astype(np.float16).astype(np.float32)


def _params(**kw):
    from spittle_amd import WhisperInferenceParams
    kw.setdefault("language", "en")
    kw.setdefault("no_timestamps", True)
    kw.setdefault("temperature_inc", 0.0)
    kw.setdefault("ignore_eot", True)
    kw.setdefault("max_new_tokens", N_TOK)
    return WhisperInferenceParams(**kw)


def _engine(spec, dtype, max_batch=4, p_min=None, **kw):
    """p_min: SPT_BLOCK_PREFILL_MIN for this context (read once, by the constructor)."""
    import os
    from spittle_amd import WhisperEngine, WhisperModelParams
    old = os.environ.pop("SPT_BLOCK_PREFILL_MIN", None)
    if p_min is not None:
        os.environ["SPT_BLOCK_PREFILL_MIN"] = str(p_min)
    try:
        e = WhisperEngine(WhisperModelParams(dtype=dtype, max_batch=max_batch, seed=SEED, **kw))
        e.load_model(spec)
    finally:
        os.environ.pop("SPT_BLOCK_PREFILL_MIN", None)
        if old is not None:
            os.environ["SPT_BLOCK_PREFILL_MIN"] = old
    return e


def _past(n):
    return [int(v) for v in np.random.default_rng(5 + n).integers(0, 50000, n)]


def _audio(seed):
    return O.synth_audio(seed, 5 * 16000)


@pytest.fixture(scope="module")
def eng():
    cache = {}

    def get(spec, dtype, p_min=None):
        if (spec, dtype, p_min) not in cache:
            cache[(spec, dtype, p_min)] = _engine(spec, dtype, p_min=p_min)
        return cache[(spec, dtype, p_min)]

    yield get
    for e in cache.values():
        e.unload_model()


@pytest.fixture(scope="module")
def ref():
    """Oracle models (an f16 engine's reference: W_F32 with the engine-dtype tensors rounded to f16, as
    tests/test_gpu_whisper_f16.py builds it) and their encoder outputs, once each."""
    O.set_threads(16)
    models, encs = {}, {}

    def model(spec, dtype):
        if (spec, dtype) not in models:
            cfg, nl, _, _ = MODELS[(spec, dtype)]
            dims = O.dims_for(cfg, nl, nl)
            if dtype == "bf16":
                om = O.Model(dims, SEED, O.W_BF16)
            else:
                om = O.Model(dims, SEED, O.W_F32)
                if dtype == "f16":
                    t = om.tensors()
                    tids = {tid for tid, name, ne in G.tensor_table(dims) if len(ne) >= 2 and name not in G._F32_ALWAYS}
                    for tid in sorted(tids):
                        om.set_tensor(tid, _f16(t[tid]))
            models[(spec, dtype)] = om
        return models[(spec, dtype)]

    def enc(spec, dtype, seed):
        if (spec, dtype, seed) not in encs:
            om = model(spec, dtype)
            encs[(spec, dtype, seed)] = om.encode(O.mel(_audio(seed), om.dims.n_mels))
        return encs[(spec, dtype, seed)]

    model.enc = enc
    yield model
    for om in models.values():
        om.close()


def _agreed(gap, margin):
    """Steps before the first decision whose gap is below the margin."""
    return next((i for i, g in enumerate(gap) if g < margin), len(gap))


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float32)).view(np.uint32)


def _same(a, b, what):
    assert a.tokens == b.tokens, what
    assert np.array_equal(_bits(a.top1), _bits(b.top1)), what
    assert np.array_equal(_bits(a.top2), _bits(b.top2)), what


# ---------------------------------------------------------------------------------- the path is taken
def test_the_block_path_is_taken(eng):
    e = eng(TINY, "f32")
    x = _audio(40)
    on = e.transcribe_samples(x, _params(prompt_tokens=_past(64), block_prefill=True))
    s_on, c_on = e.prefill_stats(), e.call_stats()
    assert s_on["block_passes"] >= 1 and s_on["chunk_passes"] == 0 and s_on["block_rows"] == 65, s_on
    off = e.transcribe_samples(x, _params(prompt_tokens=_past(64)))
    s_off, c_off = e.prefill_stats(), e.call_stats()
    assert s_off["block_passes"] == 0 and s_off["block_rows"] == 0 and s_off["chunk_passes"] == math.ceil(65 / 4), s_off
    assert c_off["decoder_passes"] - c_on["decoder_passes"] == math.ceil(65 / 4) - 1, (c_off, c_on)
    assert len(on.tokens) == len(off.tokens) == N_TOK
    # below P_min the flag changes nothing
    a = e.transcribe_samples(x, _params(prompt_tokens=_past(3), block_prefill=True))
    s = e.prefill_stats()
    assert s["block_passes"] == 0 and s["chunk_passes"] == 1, s
    _same(a, e.transcribe_samples(x, _params(prompt_tokens=_past(3))), "P = 4 < P_min")
    # both sides of P_min: 15 prompt tokens + [prev] stay chunked, 16 take the block pass
    e.transcribe_samples(x, _params(prompt_tokens=_past(15), block_prefill=True))
    assert e.prefill_stats() == {"block_passes": 0, "block_rows": 0, "chunk_passes": 4}
    e.transcribe_samples(x, _params(prompt_tokens=_past(16), block_prefill=True))
    assert e.prefill_stats() == {"block_passes": 1, "block_rows": 17, "chunk_passes": 0}
    # no prefix at all: nothing to prefill
    e.transcribe_samples(x, _params(block_prefill=True))
    assert e.prefill_stats() == {"block_passes": 0, "block_rows": 0, "chunk_passes": 0}


# ------------------------------------------------------------------------------------ against the oracle
@pytest.mark.parametrize("n_past", N_PAST)
@pytest.mark.parametrize("spec,dtype", list(MODELS), ids=lambda v: v.replace("synthetic:", ""))
def test_against_the_oracle(eng, ref, spec, dtype, n_past):
    _, _, margin, bound = MODELS[(spec, dtype)]
    seed = AUDIO.get((spec, dtype, n_past), 40)
    om = ref(spec, dtype)
    past = _past(n_past)
    tk, t1, t2 = om.decode(ref.enc(spec, dtype, seed), O.default_prompt(om.dims.n_vocab, 0, past=past), N_TOK, FLAGS)
    k = _agreed(np.asarray(t1) - np.asarray(t2), margin)
    assert k >= 8, f"the oracle's decisions clear the margin for {k} steps only: pick another seed"
    e = eng(spec, dtype, 8 if n_past + 1 < P_MIN else None)
    r = e.transcribe_samples(_audio(seed), _params(prompt_tokens=past, block_prefill=True))
    s = e.prefill_stats()
    assert s["block_passes"] == 1 and s["block_rows"] == min(n_past, 224) + 1 and s["chunk_passes"] == 0, s
    got = np.array(r.tokens)
    assert len(got) == N_TOK
    d = np.abs(np.asarray(r.top1)[:k] - np.asarray(t1)[:k])
    print(f"{spec} {dtype} P={min(n_past, 224) + 1}: agreed prefix {k}, max |d top1| {d.max():.5f} (bound {bound})")
    assert (got[:k] == np.asarray(tk)[:k]).all(), (got, tk)
    assert d.max() < bound, d


# ------------------------------------------------------------------------------- flag on against flag off
@pytest.mark.parametrize("spec,dtype", list(MODELS), ids=lambda v: v.replace("synthetic:", ""))
def test_flag_on_against_flag_off(eng, spec, dtype):
    _, _, margin, _ = MODELS[(spec, dtype)]
    e = eng(spec, dtype)
    x, past = _audio(40), _past(64)
    off = e.transcribe_samples(x, _params(prompt_tokens=past))
    on = e.transcribe_samples(x, _params(prompt_tokens=past, block_prefill=True))
    k = _agreed(np.asarray(off.top1) - np.asarray(off.top2), margin)
    assert k > 0, "the flag-off call's first decision is already uncertain: nothing to compare"
    assert on.tokens[:k] == off.tokens[:k], (on.tokens, off.tokens)
    print(f"{spec} {dtype}: agreed prefix {k}, max |d top1| {np.abs(np.asarray(on.top1)[:k] - np.asarray(off.top1)[:k]).max():.6f}")


# ------------------------------------------------------------------------------------- batch and slicing
def _long(seed, seconds=45):
    n = seconds * 16000
    return np.concatenate([O.synth_audio(seed + k) for k in range((n + 479999) // 480000)])[:n]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_batch_rows_are_bitwise_their_single_runs(eng, dtype):
    """Four 45 s utterances on the seek loop: each second window carries its own prompt_past (mixed
    prefixes, grouped by length), and each utterance's result in the batch is bitwise its result alone.
    Unlike the other cases this one decodes without ignore_eot and with 16 tokens per window: the seek loop
    refuses the hook, and the windows' own lengths are what makes the prefixes differ; 16 tokens put every
    second window's prefix at P_min or above."""
    e = eng(TINY, dtype)
    xs = [_long(200 + 10 * i) for i in range(4)]
    p = _params(ignore_eot=False, max_new_tokens=16, block_prefill=True)
    together = e.transcribe_batch(xs, p)
    assert e.prefill_stats()["block_passes"] >= 1 and e.prefill_stats()["chunk_passes"] == 0, e.prefill_stats()
    for i, (x, r) in enumerate(zip(xs, together)):
        alone = e.transcribe_samples(x, p)
        assert alone.n_windows == r.n_windows == 2
        _same(alone, r, f"utterance {i}")


def test_sliced_workspace_is_bitwise(monkeypatch):
    """B x P = 4 x 65 rows through a workspace of 225 rows runs as two slices (3 + 1 sequences) and gives
    the bits of the default workspace, where it is one pass."""
    xs = [_audio(40 + i) for i in range(4)]
    p = _params(prompt_tokens=_past(64), block_prefill=True)
    whole = _engine(TINY, "bf16")
    try:
        a = whole.transcribe_batch(xs, p)
        assert whole.prefill_stats() == {"block_passes": 1, "block_rows": 260, "chunk_passes": 0}
    finally:
        whole.unload_model()
    monkeypatch.setenv("SPT_BLOCK_PREFILL_ROWS", "1")  # read once, by the constructor: one whole prefix (225 rows)
    sliced = _engine(TINY, "bf16")
    monkeypatch.delenv("SPT_BLOCK_PREFILL_ROWS")
    try:
        b = sliced.transcribe_batch(xs, p)
        assert sliced.prefill_stats() == {"block_passes": 2, "block_rows": 260, "chunk_passes": 0}
    finally:
        sliced.unload_model()
    for i, (x, y) in enumerate(zip(a, b)):
        _same(x, y, f"row {i}")


# ------------------------------------------------------------------------------------------ whisper_full
def _full_params(**kw):
    from spittle_amd import WhisperInferenceParams
    kw.setdefault("language", "en")
    kw.setdefault("temperature_inc", 0.0)
    return WhisperInferenceParams(**kw)


GAP = 2e-3


def _compare(r, wins, segs, toks):
    """tests/test_gpu_full.py's comparison: equal until the oracle's first small-gap step."""
    steps = []
    for _, w in wins:
        steps += w.steps
    gaps = [s.margin for s in steps]
    got = list(r.tokens)
    if all(g > GAP for g in gaps):
        assert got == toks
        assert [(int(round(s.start * 100)), int(round(s.end * 100)), s.text) for s in r.segments] == \
               [(a, b, t) for a, b, t, _, _ in segs]
        return True
    k = next(i for i, g in enumerate(gaps) if g <= GAP)
    assert min(k, len(toks)) > 0, "the oracle's first decision is already uncertain: nothing to compare"
    assert got[:min(k, len(toks))] == toks[:min(k, len(toks))]
    return False


def _long_tiny(seconds=75, seed=72):
    n = seconds * 16000
    return np.concatenate([O.synth_audio(seed + k) for k in range((n + 479999) // 480000)])[:n]


def _expected_prefill(info, n_prompt, seek_end, best_of):
    """From the call's window records alone: every window's decode runs below temperature 0.5 (0, 0.2,
    0.4: the first min(n_fallbacks + 1, 3) of the temperatures tried; above, whisper_full drops the
    prompt) carry the prefix [prev] + the last <= 224 tokens of its prompt_past.  prompt_past is the call's
    prompt tokens, then after each window the conditioning tokens of the temperature it was kept at (none
    at 0.5 and above) plus the window's tokens; it is cleared within 5 s of the end.  The greedy run has one
    row, a sampled one best_of rows on one window."""
    seen, want, rows, chunks = n_prompt, 0, 0, 0
    for w in info:
        past = 0 if (w["seek"] > 0 and w["seek"] + 500 >= seek_end) else min(seen, 224)
        runs = min(w["n_fallbacks"] + 1, 3)
        if past > 0 and past + 1 >= P_MIN:
            want += runs
            rows += (past + 1) * (1 + best_of * (runs - 1))
        elif past > 0:  # a prefix below P_min stays on the chunked passes
            chunks += runs * math.ceil((past + 1) / 4)
        seen = (past if w["temperature"] < 0.5 else 0) + w["n_tokens"]
    return {"block_passes": want, "block_rows": rows, "chunk_passes": chunks}


def test_whisper_full_long_utterance():
    """75 s on synthetic:tiny with the loop's own parameters (temperature fallback in steps of 0.2, best_of 5
    sampled decoders on one window through the window map, no token limit): every decode run below temperature
    0.5 whose prefix has at least P_min positions is one block pass, counted from window_info.  Sampled
    runs draw from the device stream, so they are held to determinism; the same utterance without fallback
    is held to the oracle's whisper_full under tests/test_gpu_full.py's bars."""
    e = _engine(TINY, "f32", 8)
    om = O.Model(O.dims_for("tiny"), SEED, O.W_F32)
    try:
        x, prompt = _long_tiny(), _past(20)
        seek_end = W.n_len_org(len(x))
        p = _full_params(temperature_inc=0.2, prompt_tokens=prompt, block_prefill=True, seed=7)
        r = e.transcribe_samples(x, p)
        stats, info = e.prefill_stats(), e.window_info()
        assert r.n_windows >= 3 and len(info) == r.n_windows
        want = _expected_prefill(info, len(prompt), seek_end, 5)
        print(f"loop's own parameters: windows {[(w['seek'], w['n_fallbacks'], w['temperature'], w['n_tokens']) for w in info]}, "
              f"seek_end {seek_end}, prefill {stats}, expected {want}")
        assert want["block_passes"] >= 3, (want, info)
        assert stats == want, (stats, want)
        assert r.n_fallbacks > 0, "no window fell back: the sampled runs (best_of rows on one window) did not run"
        again = e.transcribe_samples(x, p)
        assert again.tokens == r.tokens and np.array_equal(_bits(again.top1), _bits(r.top1))
        assert e.prefill_stats() == stats
        # without fallback: one greedy run per window, against the oracle
        r0 = e.transcribe_samples(x, _full_params(max_new_tokens=16, prompt_tokens=prompt, block_prefill=True))
        stats0, info0 = e.prefill_stats(), e.window_info()
        wins, segs, toks, kept = W.transcribe(om, x, W.Params(max_tokens=16), prompt=prompt)
        assert len(wins) >= 3 and r0.n_windows >= 3
        if _compare(r0, wins, segs, toks):
            assert r0.n_windows == len(wins)
            for i, s in enumerate(kept):
                assert abs(r0.top1[i] - s.plog) < GAP and int(r0.top2[i]) == s.tid, i
        # (a greedy decoder that fails keeps every token in its record but hands only result_len of them
        # to prompt_past, so here the rows are not derivable from the records; the passes are)
        want0 = _expected_prefill(info0, len(prompt), seek_end, 5)
        assert want0["block_passes"] >= 3 and stats0["block_passes"] == want0["block_passes"], (stats0, want0)
        assert stats0["block_rows"] >= P_MIN * stats0["block_passes"]
    finally:
        e.unload_model()
        om.close()


def test_whisper_full_beam_with_a_prompt():
    """Beam 2 on one 10 s window with prompt tokens: the beams' rows share the window, the prefix runs as
    a block pass, and the result matches the oracle's beam search under the beam test's bars."""
    e = _engine(TINY_EN, "f32", 8)
    om = O.Model(O.dims_for("tiny.en"), SEED, O.W_F32)
    try:
        x = O.synth_audio(90, 10 * 16000)
        past = _past(64)
        r = e.transcribe_samples(x, _full_params(beam_size=2, max_new_tokens=16, prompt_tokens=past, block_prefill=True))
        s = e.prefill_stats()
        assert s["block_passes"] == 1 and s["block_rows"] == 2 * 65 and s["chunk_passes"] == 0, s
        wins, segs, toks, kept = W.transcribe(om, x, W.Params(max_tokens=16, beam_size=2), prompt=past)
        if _compare(r, wins, segs, toks):
            for i, st in enumerate(kept):
                assert abs(r.top1[i] - st.plog) < GAP and int(r.top2[i]) == st.tid, i
        assert r.n_windows >= 1
    finally:
        e.unload_model()
        om.close()


# ----------------------------------------------------------------------------------------- no state leaks
def test_no_state_leaks_between_flagged_and_plain_calls():
    x, past = _audio(40), _past(64)
    plain, flagged = _params(prompt_tokens=past), _params(prompt_tokens=past, block_prefill=True)
    fresh = _engine(TINY, "bf16")
    try:
        want_plain = fresh.transcribe_samples(x, plain)
    finally:
        fresh.unload_model()
    fresh = _engine(TINY, "bf16")
    try:
        want_flag = fresh.transcribe_samples(x, flagged)
    finally:
        fresh.unload_model()
    e = _engine(TINY, "bf16")
    try:
        _same(e.transcribe_samples(x, flagged), want_flag, "flagged, first call")
        _same(e.transcribe_samples(x, plain), want_plain, "plain after flagged")
        _same(e.transcribe_samples(x, flagged), want_flag, "flagged after plain")
        full = _full_params(max_new_tokens=16)
        a = e.transcribe_samples(x, full)
        e.transcribe_samples(x, _full_params(max_new_tokens=16, prompt_tokens=past, block_prefill=True))
        _same(e.transcribe_samples(x, full), a, "whisper_full, plain after flagged")
    finally:
        e.unload_model()


def test_quant_resident_context_ignores_the_flag(tmp_path):
    dims = O.dims_for("tiny.en", 2, 2)
    base = O.Model(dims, SEED, O.W_F32)
    path = str(tmp_path / "ggml-tiny.en-q5_0.bin")
    G.write_model(path, dims, O.mel_filters(dims.n_mels), G.synth_vocab(O.special_tokens(dims.n_vocab)["eot"]),
                  base.tensors(), G.Q5_0)
    base.close()
    e = _engine(path, "bf16", quant_resident=True)
    try:
        assert e.weight_residency()["resident_weights"] > 0
        x, past = _audio(40), _past(64)
        off = e.transcribe_samples(x, _params(prompt_tokens=past))
        on = e.transcribe_samples(x, _params(prompt_tokens=past, block_prefill=True))
        s = e.prefill_stats()
        assert s["block_passes"] == 0 and s["chunk_passes"] == math.ceil(65 / 4), s
        _same(on, off, "quant-resident: flag on against flag off")
    finally:
        e.unload_model()
