"""The no-speech probability and the silence skip in the engine against the oracle.

Models are ggml files written by oracle.ggml.write_model from the oracle's weights with ONE tensor changed
on both sides: the decoder's final LayerNorm bias (tensor 13) gets + ALPHA * E[nosp] / |E[nosp]|^2, which
raises the <|nospeech|> logit by ALPHA and leaves decoding alone (nosp is always suppressed for sampling).
Without it the synthetic weights put the probability near 1e-6 and no threshold could sit among the windows.

Bars on |ln p_gpu - ln p_oracle| (both terms of ln p = l[nosp] - lse(l) move by at most max |dl|, the
logit bars of test_gpu_parity.py): f32 2 x 2e-3, bf16 2 x 0.25; the f16 engine takes bf16's bar (f16 carries
three more mantissa bits than bf16, and its file's matrices are held exactly).

Every decision test first asserts on the ORACLE's values alone that each window's ln p and average
log-probability are further from their thresholds than the bar, and that every decoding step's decision gap
is above 2e-3: a drift is then a failed precondition, not a flaky comparison."""
import math

import numpy as np
import pytest

from tests import nospeech_ref as R
from oracle import ggml as G
from oracle import oracle as O
from oracle import whisper_full as WF

pytestmark = pytest.mark.gpu

SEED, ALPHA, GAP = 1234, 14.0, 2e-3
MEDIUM = O.Dims(80, 1024, 16, 2, 2, 51865, 1500, 448)
#         dims                          file   engine  oracle    bar on |d ln p|
MODELS = {"tiny.en": (("tiny.en", 2, 2), G.F32, "f32", O.W_F32, 2 * 2e-3),      # two decoder layers: no_timestamps forced
          "tiny.en3": (("tiny.en", 2, 3), G.F32, "f32", O.W_F32, 2 * 2e-3),     # three: timestamps on
          "tiny": (("tiny", 2, 2), G.F32, "f32", O.W_F32, 2 * 2e-3),            # multilingual
          "large-bf16": (("large-v3", 2, 2), G.F16, "bf16", O.W_BF16, 2 * 0.25),
          "medium-f16": (MEDIUM, G.F16, "f16", O.W_F32, 2 * 0.25)}


def _bf16(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def _engine(path, dtype, max_batch=5):
    from spittle_amd import WhisperEngine, WhisperModelParams
    e = WhisperEngine(WhisperModelParams(dtype=dtype, max_batch=max_batch, seed=SEED))
    e.load_model(path)
    return e


class Built:
    def __init__(self, tmp, name):
        cfg, wtype, self.dtype, wd, self.bar = MODELS[name]
        self.dims = dims = O.dims_for(*cfg) if isinstance(cfg, tuple) else cfg
        self.sp = O.special_tokens(dims.n_vocab)
        base = O.Model(dims, SEED, O.W_F32)
        t = base.tensors()
        base.close()
        E = t[10].reshape(dims.n_vocab, dims.d)[self.sp["nosp"]].astype(np.float64)
        t[13] = (t[13].astype(np.float64) + ALPHA * E / (E @ E)).astype(np.float32)
        self.path = str(tmp / f"ggml-{name}.bin")
        deq = G.write_model(self.path, dims, O.mel_filters(dims.n_mels), G.synth_vocab(self.sp["eot"]), t, wtype)
        self.om = O.Model(dims, SEED, wd)
        rnd = {tid for tid, nm, ne in G.tensor_table(dims) if len(ne) >= 2 and nm not in G._F32_ALWAYS} \
            if self.dtype == "bf16" else set()
        for tid, v in deq.items():
            self.om.set_tensor(tid, _bf16(v) if tid in rnd else v)
        self.e = _engine(self.path, self.dtype)
        self.multi = self.sp["n_langs"] > 0
        self.lang = self.sp["sot"] + 1 if self.multi else -1
        self._lnp = {}

    def init(self, no_ts=True):
        p = [self.sp["sot"]] + ([self.lang, self.sp["transcribe"]] if self.multi else [])
        return p + ([self.sp["not"]] if no_ts else [])

    def oracle_lnp(self, key, x, seek=0, prefix=(), no_ts=True):
        """ln p of the window at `seek` of x for the prompt prefix + init (cached by key)"""
        k = (key, seek, tuple(prefix), no_ts)
        if k not in self._lnp:
            enc = self.om.encode(O.mel_window(O.mel_full(x, self.dims.n_mels), seek))
            self._lnp[k] = R.ln_prob(self.om.logits(enc, list(prefix) + self.init(no_ts)), self.sp["nosp"])
        return self._lnp[k]


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("nospeech")
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Built(tmp, name)
        return cache[name]

    yield get
    for b in cache.values():
        b.e.unload_model()
        b.om.close()


def _params(**kw):
    from spittle_amd import WhisperInferenceParams
    kw.setdefault("language", "en")
    kw.setdefault("temperature_inc", 0.0)
    kw.setdefault("max_new_tokens", 6)
    return WhisperInferenceParams(**kw)


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float32)).view(np.uint32)


def _same(a, b, what):
    assert a.tokens == b.tokens, what
    assert np.array_equal(_bits(a.top1), _bits(b.top1)) and np.array_equal(_bits(a.top2), _bits(b.top2)), what
    assert a.text == b.text and a.language == b.language and a.n_windows == b.n_windows, what
    assert a.n_fallbacks == b.n_fallbacks, what
    assert [(s.start, s.end, s.text, s.i0, s.n_tokens) for s in a.segments] == \
           [(s.start, s.end, s.text, s.i0, s.n_tokens) for s in b.segments], what


def _long():
    """75 s whose middle 30 s are silent: three windows with different probabilities"""
    x = O.synth_audio(5, 75 * 16000).copy()
    x[30 * 16000:60 * 16000] = 0
    return x


_REF = {}


def _ref(b, name, p, thold):
    """the restated loop's result, computed once per (model, parameters)"""
    k = (name, tuple(sorted(p.__dict__.items())), thold)
    if k not in _REF:
        _REF[k] = R.transcribe(b.om, _long(), p, thold)
    return _REF[k]


def _preconditions(ref, bar, thold, logprob_thold):
    for w in ref["windows"]:
        if 0.0 < thold < 1.0:
            assert abs(w["ln_p"] - math.log(thold)) > bar, ("ln p too close to the threshold", w["seek"], w["p"])
        assert abs(w["avg"] - logprob_thold) > GAP, ("avg too close to logprob_thold", w["seek"], w["avg"])
        assert all(s.margin > GAP for s in w["window"].steps), ("an uncertain decoding step", w["seek"])


def _check_against_ref(b, r, info, ref):
    assert list(r.tokens) == ref["tokens"]
    # (the file's vocabulary spells the text; the oracle writes "[id]": the tokens above carry it)
    assert [(int(round(s.start * 100)), int(round(s.end * 100)), s.i0, s.n_tokens) for s in r.segments] == \
           [(a, z, i0, n) for a, z, _, i0, n in ref["segments"]]
    assert r.n_windows == len(ref["windows"]) == len(info)
    for g, w in zip(info, ref["windows"]):
        assert (g["utterance"], g["seek"], g["seek_delta"], g["i0"], g["n_tokens"], g["skipped"]) == \
               (0, w["seek"], w["seek_delta"], w["i0"], w["n_tokens"], w["skipped"]), (g, w["seek"])
        assert abs(math.log(g["no_speech_prob"]) - w["ln_p"]) <= b.bar, (g, w["ln_p"])
        assert g["n_fallbacks"] == 0 and g["temperature"] == 0.0
        if math.isfinite(w["avg"]):
            assert abs(g["avg_logprob"] - w["avg"]) <= GAP, (g, w["avg"])
        else:
            assert g["avg_logprob"] == -math.inf


# ----------------------------------------------------------------------------- 1. the probability
@pytest.mark.parametrize("name", ["tiny.en", "tiny", "large-bf16", "medium-f16"])
def test_probability_matches_the_oracle(models, name):
    b = models(name)
    nb = 5 if name == "large-bf16" else 4    # B = 5 on large-v3 geometry: the fused cross-Q path
    batch = [O.synth_audio(i) for i in range(nb)]
    p = _params(no_timestamps=True, no_speech_prob=True, max_new_tokens=4)
    alone = []
    for i in range(nb):                                          # B = 1: every utterance alone
        b.e.transcribe_samples(batch[i], p)
        (w,) = b.e.window_info()
        assert math.isnan(w["avg_logprob"]) and not w["skipped"] and w["seek"] == 0      # the fast path
        want = b.oracle_lnp(("synth", i), batch[i])
        print(f"{name} B=1 utt {i}: p={w['no_speech_prob']:.6g} oracle={math.exp(want):.6g} "
              f"|d ln p|={abs(math.log(w['no_speech_prob']) - want):.3g} bar={b.bar}")
        assert abs(math.log(w["no_speech_prob"]) - want) <= b.bar
        alone.append(w["no_speech_prob"])
    for B in sorted({4, nb}):
        b.e.transcribe_batch(batch[:B], p)
        info = b.e.window_info()
        assert [w["utterance"] for w in info] == list(range(B))
        for i, w in enumerate(info):
            assert abs(math.log(w["no_speech_prob"]) - b.oracle_lnp(("synth", i), batch[i])) <= b.bar, (B, i)
        got = [w["no_speech_prob"] for w in info]
        assert np.array_equal(_bits(got), _bits(alone[:B])), (B, got, alone)   # every row's bits are its bits alone
    if name == "large-bf16":
        assert b.e.xq_stats()["fused_launches"] > 0 and b.e.xq_stats()["fallbacks"] == 0


# ----------------------------------------------------------------------------- 2. the rule
RULE = {"some": (0.3, -2.45), "none": (0.8, -1.0), "all": (0.05, -1.0), "never": (0.05, -20.0)}


@pytest.mark.parametrize("case", list(RULE))
@pytest.mark.parametrize("name", ["tiny.en", "tiny.en3"])
def test_rule_against_the_restated_loop(models, name, case):
    b = models(name)
    thold, lp = RULE[case]
    ref = _ref(b, name, WF.Params(max_tokens=6, logprob_thold=lp), thold)
    _preconditions(ref, b.bar, thold, lp)
    n_skip = sum(w["skipped"] for w in ref["windows"])
    if name == "tiny.en":   # finite averages everywhere: the four outcomes as named
        assert {"some": 0 < n_skip < len(ref["windows"]), "none": n_skip == 0, "all": n_skip == len(ref["windows"]),
                "never": n_skip == 0}[case], (case, n_skip)
    r = b.e.transcribe_samples(_long(), _params(no_speech_thold=thold, logprob_thold=lp))
    _check_against_ref(b, r, b.e.window_info(), ref)


# ----------------------------------------------------------------------------- 3. beam
@pytest.mark.parametrize("name,case", [("tiny.en3", (0.3, -1.0)), ("tiny.en3", (0.8, -1.0)), ("tiny.en", (0.3, -1.0))])
def test_beam_under_the_same_rule(models, name, case):
    b = models(name)
    thold, lp = case
    ref = _ref(b, name, WF.Params(max_tokens=4, logprob_thold=lp, beam_size=3), thold)
    _preconditions(ref, b.bar, thold, lp)
    r = b.e.transcribe_samples(_long(), _params(no_speech_thold=thold, logprob_thold=lp, beam_size=3, max_new_tokens=4))
    _check_against_ref(b, r, b.e.window_info(), ref)


# ----------------------------------------------------------------------------- 4. fallback on
PROMPT = [1000, 2000, 3000]   # prompt_tokens: the first window's prompt_past


def _walk_fallback(b, x, r, info, prompt):
    """every window's probability against the oracle's for the prompt of the temperature kept: with the
    [prev] prefix below 0.5, without it at or above.  -> (windows matched with their prefix, windows that
    had a prefix and lost it, windows that never had one)"""
    seek_end = WF.n_len_org(len(x))
    past, known = list(prompt), True
    n_pref = n_lost = n_none = 0
    for w in info:
        assert abs(w["temperature"] - 0.2 * w["n_fallbacks"]) < 1e-5 and 0 <= w["n_fallbacks"] <= 5
        if w["seek"] > 0 and w["seek"] + 500 >= seek_end:
            past, known = [], True
        toks = list(r.tokens[w["i0"]:w["i0"] + w["n_tokens"]])
        got = math.log(w["no_speech_prob"])
        # the prefixes prompt_past may have held: exactly `past`, or, after a decoder kept at the last
        # temperature (it may have failed: prompt_past took its result_len, not its token count), a head of it
        cands = [past] if known else [past[:k] for k in range(len(past), 0, -1)]
        with_pf = [b.oracle_lnp("long", x, w["seek"], [b.sp["prev"]] + c[-224:]) for c in cands if c]
        bare = b.oracle_lnp("long", x, w["seek"])
        if w["temperature"] >= 0.5 or not past:        # the prompt lost (or never had) its prompt_past prefix
            assert abs(got - bare) <= b.bar, (w, bare)
            if with_pf:
                # the value is the kept run's, not the t = 0 run's: every prefix that run can have had is
                # further from the oracle's bare value than twice the bar, so the engine's misses it by a bar
                assert all(abs(v - bare) > 2 * b.bar for v in with_pf), ("precondition: the prefix moves ln p", w["seek"])
                assert all(abs(got - v) > b.bar for v in with_pf), (w, with_pf)
                n_lost += 1
                print(f"seek {w['seek']} t={w['temperature']:.1f}: without the prefix |d ln p| = {abs(got - bare):.3g}, "
                      f"with it {min(abs(got - v) for v in with_pf):.3g}")
            else:
                n_none += 1
            past, known = toks, w["n_fallbacks"] < 5
        else:
            errs = [abs(got - v) for v in with_pf]
            assert min(errs) <= b.bar, (w, errs)
            n_pref += 1
            past, known = ([c for c in cands if c][int(np.argmin(errs))] + toks), True
            print(f"seek {w['seek']} t={w['temperature']:.1f}: with the prefix |d ln p| = {min(errs):.3g}, "
                  f"without it {abs(got - bare):.3g}")
    return n_pref, n_lost, n_none


def test_fallback_records_the_kept_temperature_and_its_prompt(models):
    b = models("tiny.en")
    x = _long()
    # logprob_thold -2.4: some windows are kept at t = 0 with their prefix, others fall back
    r = b.e.transcribe_samples(x, _params(temperature_inc=0.2, best_of=5, no_speech_prob=True, logprob_thold=-2.4))
    info = b.e.window_info()
    assert r.n_windows == len(info) >= 3 and r.n_fallbacks == sum(w["n_fallbacks"] for w in info)
    n_pref, n_lost, n_none = _walk_fallback(b, x, r, info, [])
    print(f"logprob_thold -2.4: with a prefix {n_pref}, lost it {n_lost}, never had one {n_none}; fallbacks {r.n_fallbacks}")
    assert n_pref >= 1 and n_none >= 1 and r.n_fallbacks >= 1, (n_pref, n_lost, n_none, r.n_fallbacks)


def test_fallback_above_half_reports_the_prompt_without_its_prefix(models):
    """logprob_thold 0: no average reaches it, so every window falls back to the last temperature, 1.0, whose
    prompt has no prompt_past prefix.  With prompt_tokens the FIRST window already has a prefix to lose (and
    the later ones have the tokens before them): the value reported is the bare prompt's, and it misses
    the t = 0 run's, which had the prefix, by more than the bar."""
    b = models("tiny.en")
    x = _long()
    r = b.e.transcribe_samples(x, _params(temperature_inc=0.2, best_of=5, no_speech_prob=True, logprob_thold=0.0,
                                          prompt_tokens=PROMPT))
    info = b.e.window_info()
    assert r.n_windows == len(info) >= 3 and r.n_fallbacks == 5 * len(info)
    assert all(w["n_fallbacks"] == 5 and abs(w["temperature"] - 1.0) < 1e-5 for w in info)
    n_pref, n_lost, n_none = _walk_fallback(b, x, r, info, PROMPT)
    print(f"logprob_thold 0: with a prefix {n_pref}, lost it {n_lost}, never had one {n_none}")
    assert n_pref == 0 and n_lost >= 1, (n_pref, n_lost, n_none)
    # the same call at temperature_inc 0 keeps the t = 0 run: its first window reports the value WITH the prefix
    b.e.transcribe_samples(x, _params(no_speech_prob=True, logprob_thold=0.0, prompt_tokens=PROMPT))
    w0 = b.e.window_info()[0]
    want = b.oracle_lnp("long", x, 0, [b.sp["prev"]] + PROMPT)
    assert w0["temperature"] == 0.0 and abs(math.log(w0["no_speech_prob"]) - want) <= b.bar, (w0, want)
    assert abs(math.log(w0["no_speech_prob"]) - math.log(info[0]["no_speech_prob"])) > b.bar


# ----------------------------------------------------------------------------- 5. nothing else moves
def _both(e, call, **kw):
    a = call(_params(**kw))
    xa = e.xq_stats()
    b = call(_params(no_speech_prob=True, **kw))
    return a, b, xa, e.xq_stats()


@pytest.mark.parametrize("name", ["tiny.en3", "large-bf16"])
def test_flag_alone_changes_nothing(models, name):
    b = models(name)
    e = b.e
    nb = 5
    batch = [O.synth_audio(i) for i in range(nb)]
    for B in (1, 4, nb):                                                    # the fast path
        ra, rb, xa, xb = _both(e, lambda p: e.transcribe_batch(batch[:B], p), no_timestamps=True, max_new_tokens=8,
                               ignore_eot=True)
        for u, v in zip(ra, rb):
            _same(u, v, f"fast path B = {B}")
        assert xa == xb, (B, xa, xb)
        info = e.window_info()
        assert len(info) == B and all(math.isnan(w["avg_logprob"]) for w in info)
        assert abs(math.log(info[0]["no_speech_prob"]) - b.oracle_lnp(("synth", 0), batch[0])) <= b.bar
    x8 = O.synth_audio(5, 128000)
    calls = {"whisper_full defaults": (lambda p: [e.transcribe_samples(x8, p)], dict(temperature_inc=0.2, max_new_tokens=220)),
             "beam": (lambda p: [e.transcribe_samples(x8, p)], dict(beam_size=3)),
             "initial_prompt": (lambda p: [e.transcribe_samples(x8, p)], dict(initial_prompt=" hello world")),
             "aligned": (lambda p: [e.transcribe_samples_aligned(x8, p)], dict())}
    if b.multi:
        calls["auto-detect"] = (lambda p: [e.transcribe_samples(x8, p)], dict(language=None))
    for what, (call, kw) in calls.items():
        ra, rb, xa, xb = _both(e, call, **kw)
        _same(ra[0], rb[0], what)
        assert xa == xb, (what, xa, xb)
        assert ra[0].token_times == rb[0].token_times and ra[0].words == rb[0].words, what
        assert all(0.0 < w["no_speech_prob"] < 1.0 for w in e.window_info()), what
    if name == "tiny.en3":   # a plain call after flagged calls is a fresh engine's
        fresh = _engine(b.path, b.dtype)
        for kw in (dict(no_timestamps=True, max_new_tokens=8), dict(temperature_inc=0.2, max_new_tokens=220)):
            _same(e.transcribe_samples(x8, _params(**kw)), fresh.transcribe_samples(x8, _params(**kw)), kw)
            assert all(math.isnan(w["no_speech_prob"]) for w in e.window_info())
        fresh.unload_model()


# ----------------------------------------------------------------------------- 6. skip with alignment
def test_skipped_window_has_no_words(models):
    """two one-window utterances in one aligned call; the threshold sits between their probabilities, so
    one is dropped whole and the other's tokens, times and words are those of the call without a threshold"""
    b = models("tiny.en3")
    xs = [O.synth_audio(1), O.synth_audio(2)]
    lnp = [b.oracle_lnp(("synth", i), x, no_ts=False) for i, x in zip((1, 2), xs)]
    thold, lp = 0.45, -1.0
    refs = [R.transcribe(b.om, x, WF.Params(max_tokens=6, logprob_thold=lp), thold) for x in xs]
    for ref in refs:
        _preconditions(ref, b.bar, thold, lp)
    assert [w["skipped"] for ref in refs for w in ref["windows"]] == [1, 0] and lnp[0] > math.log(thold) > lnp[1]
    plain = b.e.transcribe_batch_aligned(xs, _params(logprob_thold=lp))
    got = b.e.transcribe_batch_aligned(xs, _params(logprob_thold=lp, no_speech_thold=thold))
    info = b.e.window_info()
    assert [(w["utterance"], w["skipped"], w["n_tokens"]) for w in info] == [(0, 1, 0), (1, 0, len(got[1].tokens))]
    assert got[0].tokens == [] and got[0].segments == [] and got[0].token_times == [] and got[0].words == []
    assert got[0].n_windows == 1 and plain[0].tokens
    _same(got[1], plain[1], "the utterance that was kept")
    assert got[1].token_times == plain[1].token_times and got[1].words == plain[1].words and got[1].token_times


# ----------------------------------------------------------------------------- 7. refusals
def test_refusals(models):
    import torch
    from spittle_amd import _lib as L
    from spittle_amd.engine import TranscriptionError
    b = models("tiny.en")
    dev = torch.zeros(480000, dtype=torch.float32, device="cuda")
    dev.copy_(torch.from_numpy(O.synth_audio(0)))
    torch.cuda.synchronize()
    fast = dict(no_timestamps=True, max_new_tokens=4)
    with pytest.raises(TranscriptionError) as e:
        b.e.transcribe_batch_device(dev.data_ptr(), 480000, [480000], _params(no_speech_thold=0.5, **fast))
    assert e.value.status == L.SPT_ERR_INVALID_ARG
    assert b.e.window_info() == []       # a call that fails leaves no records, not the previous call's
    r = b.e.transcribe_batch_device(dev.data_ptr(), 480000, [480000], _params(no_speech_prob=True, **fast))   # the flag alone
    (w,) = b.e.window_info()
    assert len(r[0].tokens) > 0 and math.isnan(w["avg_logprob"])
    assert abs(math.log(w["no_speech_prob"]) - b.oracle_lnp(("synth", 0), O.synth_audio(0))) <= b.bar
    ip = L.InferParams()
    L.load().spt_default_infer_params(__import__("ctypes").byref(ip))
    for bad in (-0.5, float("nan")):   # the library's own check, past the Python mirror's
        ip.no_speech_thold = bad
        C = __import__("ctypes")
        x = np.zeros(16000, np.float32)
        ptrs = (C.POINTER(C.c_float) * 1)(x.ctypes.data_as(C.POINTER(C.c_float)))
        out = (C.POINTER(L.Result) * 1)()
        st = L.load().spt_transcribe_batch(b.e._ctx, ptrs, (C.c_size_t * 1)(x.size), 1, C.byref(ip), out)
        assert st == L.SPT_ERR_INVALID_ARG and not out[0]
        assert b.e.window_info() == []
    # an enabled threshold with the fast path's parameters runs whisper_full (avg_logprob is finite)
    b.e.transcribe_samples(O.synth_audio(0), _params(no_speech_thold=0.999, **fast))
    assert all(math.isfinite(w["avg_logprob"]) and 0 < w["no_speech_prob"] < 1 for w in b.e.window_info())
