"""GPU tests of the SenseVoice engine against its torch restatement (tests/sensevoice_torch.py) on
sensevoice-test-small with the restatement's seeded weights.

Bars.  E_EMUL holds, per audio case, figures measured on the CPU by

    python scripts/sensevoice_measure_ref.py

    (features rel-L2, features max-abs, encoder rel-L2, encoder max-abs, max |logit(emulate_f16) - logit(f32)|)

The encoder and logit figures are sensevoice_torch(emulate_f16=True) against its f32 run.  The engine
stores no f16 before the first LayerNorm, so for the features that difference is identically zero;
their figure is the restatement's own f32 error against its f64 run instead.  A GPU bar is 4 x the
figure (accumulation order, the device's exp / log / sin); bar_m = 4 x the logit figure is the margin
below which a row's argmax is not asserted, and top-1 logits must be within bar_m / 2.  None of these
comes from the engine's output.  Every figure is printed before it is asserted (pytest -s).

    case      R   feat rel   feat max   enc rel    enc max    logit     bar_m    rows under bar_m (CPU, f32)
    400       5   1.137e-06  1.055e-05  7.394e-04  2.443e-03  2.284e-02 9.137e-02  0.000
    1360      6   1.203e-06  3.417e-05  7.258e-04  2.709e-03  2.248e-02 8.991e-02  0.000
    57999    64   2.112e-06  2.440e-04  5.596e-04  2.424e-03  2.058e-02 8.231e-02  0.016
    58000    65   1.492e-06  1.047e-04  5.625e-04  2.527e-03  2.466e-02 9.865e-02  0.015
    160000  171   1.447e-06  1.541e-04  5.587e-04  2.489e-03  2.350e-02 9.398e-02  0.023

With seed 42 the f32 restatement has 28 / 29 / 63 blank rows and 23 / 22 / 48 repeated labels in the three
longer cases, and no argmax differs between f16 emulation and f32."""
import numpy as np
import pytest
import torch

from spittle_amd import _lib as L
from spittle_amd import (Language, SenseVoiceEngine, SenseVoiceInferenceParams, SenseVoiceModelParams,
                         TranscriptionError)
from tests import sensevoice_torch as ST

pytestmark = pytest.mark.gpu

# python scripts/sensevoice_measure_ref.py  (see the module docstring)
E_EMUL = {
    400: (1.137e-06, 1.055e-05, 7.394e-04, 2.443e-03, 2.284e-02),
    1360: (1.203e-06, 3.417e-05, 7.258e-04, 2.709e-03, 2.248e-02),
    57999: (2.112e-06, 2.440e-04, 5.596e-04, 2.424e-03, 2.058e-02),
    58000: (1.492e-06, 1.047e-04, 5.625e-04, 2.527e-03, 2.466e-02),
    160000: (1.447e-06, 1.541e-04, 5.587e-04, 2.489e-03, 2.350e-02),
}
D = ST.TEST_SMALL


def bar_m(n):
    return 4.0 * E_EMUL[n][4]


def rel_l2(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def make_engine(max_batch=4, weights=None, spec=ST.SPEC, max_samples=max(ST.CASES)):
    e = SenseVoiceEngine()
    e.load_model_with_params(spec, SenseVoiceModelParams(max_batch=max_batch, max_samples=max_samples))
    assert e.missing_tensors() > 0
    e.load_state_dict(weights if weights is not None else ST.make_weights(D))
    assert e.missing_tensors() == 1   # the CMVN pair
    e.set_cmvn(*ST.make_cmvn(D))
    assert e.missing_tensors() == 0
    return e


class Rig:
    def __init__(self):
        self.pcm = {n: ST.audio(n, ci) for ci, n in enumerate(ST.CASES)}
        self.W = ST.to_torch(ST.make_weights(D))
        self.cmvn = tuple(torch.from_numpy(v) for v in ST.make_cmvn(D))
        self.eng = make_engine()
        self.ref, self.alone, self.frames = {}, {}, {}

    def want(self, n):
        """the f32 restatement's (features, encoder output, logits), computed once"""
        if n not in self.ref:
            with torch.no_grad():
                self.ref[n] = tuple(t.numpy() for t in ST.forward(self.W, self.cmvn, self.pcm[n], D))
        return self.ref[n]

    def run_alone(self, n):
        if n not in self.alone:
            self.alone[n] = self.eng.transcribe_samples(self.pcm[n])
        return self.alone[n]

    def debug_frames(self, n):
        if n not in self.frames:
            self.frames[n] = self.eng.debug_frames(self.pcm[n])
        return self.frames[n]


@pytest.fixture(scope="module")
def rig():
    r = Rig()
    yield r
    r.eng.unload_model()


def test_features(rig):
    for n in ST.CASES:
        got, want = rig.eng.debug_features(rig.pcm[n]), rig.want(n)[0]
        assert got.shape == want.shape == (ST.n_rows(n) - 4, 560)
        e = E_EMUL[n]
        rl, mx = rel_l2(got, want), float(np.abs(got - want).max())
        print(f"parity n={n} features: rel_l2 {rl:.3e} (bar {4 * e[0]:.3e}) max_abs {mx:.3e} (bar {4 * e[1]:.3e})")
        assert np.isfinite(got).all()
        assert rl <= 4 * e[0] and mx <= 4 * e[1], (n, rl, mx)


def test_encoder(rig):
    for n in ST.CASES:
        got, want = rig.eng.debug_encode(rig.pcm[n]), rig.want(n)[1]
        assert got.shape == want.shape == (ST.n_rows(n), D.d)
        e = E_EMUL[n]
        rl, mx = rel_l2(got, want), float(np.abs(got - want).max())
        print(f"parity n={n} encoder: rel_l2 {rl:.3e} (bar {4 * e[2]:.3e}) max_abs {mx:.3e} (bar {4 * e[3]:.3e})")
        assert np.isfinite(got).all()
        assert rl <= 4 * e[2] and mx <= 4 * e[3], (n, rl, mx)


def test_row_argmax(rig):
    for n in ST.CASES:
        ids, t1, t2 = rig.debug_frames(n)
        lg = rig.want(n)[2]
        bm, mg = bar_m(n), ST.margins(lg)
        want_ids = lg.argmax(axis=1)
        asserted = mg > bm
        err = float(np.abs(t1 - lg.max(axis=1)).max())
        print(f"parity n={n} rows {len(ids)}: |d top1| {err:.3e} (bar {bm / 2:.3e}) exempt {(~asserted).sum()} "
              f"mismatches among asserted {(ids[asserted] != want_ids[asserted]).sum()}")
        assert len(ids) == ST.n_rows(n)
        assert asserted.any() and (~asserted).mean() <= 0.10, (n, (~asserted).mean())
        assert (ids[asserted] == want_ids[asserted]).all(), n
        assert err <= bm / 2, (n, err)
        assert (t1 >= t2).all()


def test_collapse_is_exact(rig):
    """tokens, frames and prefix labels are the greedy collapse of the engine's own per-row ids"""
    seen_blank = seen_repeat = 0
    for n in ST.CASES:
        ids, t1, t2 = rig.debug_frames(n)
        prefix, tok, frame = ST.ctc_collapse(ids, D.n_prefix, D.blank)
        r = rig.run_alone(n)
        body = ids[D.n_prefix:]
        seen_blank += int((body == D.blank).sum())
        seen_repeat += int((body[1:] == body[:-1]).sum())
        print(f"collapse n={n}: {len(tok)} tokens of {len(body)} rows, prefix {prefix}")
        assert r.prefix == prefix and r.tokens == tok and r.frames == frame, n
        at = np.array(frame, np.int64) + D.n_prefix
        assert np.array_equal(r.top1, t1[at]) and np.array_equal(r.top2, t2[at]), n
        assert len(tok) <= ST.n_rows(n) - 4
        assert r.text == "".join(f"[{t}]" for t in tok)
    assert seen_blank > 0 and seen_repeat > 0


def same(a, b):
    return (a.tokens == b.tokens and a.frames == b.frames and a.prefix == b.prefix and
            np.array_equal(a.top1, b.top1) and np.array_equal(a.top2, b.top2))


def test_batch_equals_alone(rig):
    """every batch row is bitwise what it is alone; R = 5, 64, 65 and 171 side by side exercise the
    length masks of the FSMN, the attention's key tiles and the collapse"""
    for order in ((400, 160000, 57999, 58000), (58000, 57999, 400, 160000), (160000, 1360, 160000, 400)):
        res = rig.eng.transcribe_batch([rig.pcm[n] for n in order])
        for n, r in zip(order, res):
            assert same(r, rig.run_alone(n)), (order, n)


def test_stale_workspace_does_not_leak(rig):
    fresh = make_engine(max_batch=1)
    try:
        want = fresh.transcribe_samples(rig.pcm[400])
        want_enc = fresh.debug_encode(rig.pcm[400])
    finally:
        fresh.unload_model()
    rig.eng.transcribe_batch([rig.pcm[160000], rig.pcm[160000]])
    assert same(rig.eng.transcribe_samples(rig.pcm[400]), want)
    rig.eng.debug_encode(rig.pcm[160000])
    assert np.array_equal(rig.eng.debug_encode(rig.pcm[400]), want_enc)


def test_language_and_itn_rows(rig):
    n = 57999
    ft = torch.from_numpy(rig.want(n)[0])
    base = rig.eng.debug_encode(rig.pcm[n])
    e = E_EMUL[n]
    for lang, itn in ((Language.English, True), (Language.Korean, False), (Language.Cantonese, True)):
        with torch.no_grad():
            want = ST.encoder(rig.W, ST.input_rows(rig.W, ft, D, lang.value, itn), D).numpy()
        got = rig.eng.debug_encode(rig.pcm[n], SenseVoiceInferenceParams(language=lang, use_itn=itn))
        rl, mx = rel_l2(got, want), float(np.abs(got - want).max())
        print(f"language {lang.name} itn {itn}: rel_l2 {rl:.3e} max_abs {mx:.3e}; against auto {rel_l2(got, base):.3e}")
        assert rl <= 4 * e[2] and mx <= 4 * e[3]
        assert rel_l2(got, base) > 8 * e[2]   # the query rows did change
    with pytest.raises(TranscriptionError, match="language") as ei:
        rig.eng.transcribe_samples(rig.pcm[400], SenseVoiceInferenceParams(language=6))
    assert ei.value.status == L.SPT_ERR_INVALID_ARG


def test_lengths(rig):
    e = rig.eng
    rig.run_alone(1360)   # a device pass first: its timings must not survive the next call
    r = e.transcribe_samples(rig.pcm[400][:399])
    assert r.text == "" and r.tokens == [] and r.frames == [] and r.prefix == [-1, -1, -1, -1]
    t = e.timings()
    assert t["batch"] == 0 and t["total_ms"] == 0.0   # no device pass ran
    res = e.transcribe_batch([np.zeros(10, np.float32), rig.pcm[1360]])
    assert res[0].tokens == [] and same(res[1], rig.run_alone(1360))
    with pytest.raises(TranscriptionError, match="longer than max_samples") as ei:
        e.transcribe_samples(np.zeros(max(ST.CASES) + 1, np.float32))
    assert ei.value.status == L.SPT_ERR_INVALID_ARG
    assert e.n_rows(399) == 0 and [e.n_rows(n) for n in ST.CASES] == [5, 6, 64, 65, 171]


def test_error_paths_with_a_context(rig):
    for dt in ("f32", "bf16"):
        with pytest.raises(TranscriptionError) as ei:
            SenseVoiceEngine().load_model_with_params("synthetic:sensevoice-test-small", SenseVoiceModelParams(dtype=dt))
        assert ei.value.status == L.SPT_ERR_UNSUPPORTED
    m = SenseVoiceEngine()
    m.load_model_with_params(ST.SPEC, SenseVoiceModelParams(max_batch=1, max_samples=16000))
    try:
        w = ST.make_weights(D)
        del w["encoder.tp_encoders.0.self_attn.fsmn_block.weight"]
        m.load_state_dict(w)
        assert m.missing_tensors() == 2   # that tensor and the CMVN pair
        with pytest.raises(TranscriptionError, match="not set") as ei:
            m.transcribe_samples(rig.pcm[1360])
        assert ei.value.status == L.SPT_ERR_INVALID_ARG
        m.set_cmvn(*ST.make_cmvn(D))
        assert m.missing_tensors() == 1
        with pytest.raises(TranscriptionError, match="not set"):
            m.debug_encode(rig.pcm[1360])
        with pytest.raises(TranscriptionError, match="has 2816 elements, got 3"):
            m.load_state_dict({"encoder.tp_encoders.0.self_attn.fsmn_block.weight": np.zeros(3, np.float32)})
        with pytest.raises(TranscriptionError, match="unknown tensor"):
            m.load_state_dict({"encoder.nope": np.zeros(3, np.float32)})
        with pytest.raises(TranscriptionError, match="560 elements"):
            m.set_cmvn(np.zeros(80, np.float32), np.ones(80, np.float32))
        assert m.tensor_numel("ctc.ctc_lo.weight") == 500 * 256
        assert m.transcribe_samples(np.zeros(100, np.float32)).tokens == []   # nothing to run: no error
    finally:
        m.unload_model()
    # text through set_vocab: tags dropped, the leading space stripped
    toks = rig.run_alone(57999).tokens
    pieces = [f"▁p{i}" for i in range(D.vocab)]
    pieces[toks[0]] = "<|en|>"
    rig.eng.set_vocab(pieces)
    try:
        text = rig.eng.transcribe_samples(rig.pcm[57999]).text
        assert text == " ".join(f"p{t}" for t in toks if t != toks[0])
    finally:
        rig.eng.set_vocab([])


def test_pad_columns_take_no_part():
    """V = 500 is padded to 512 GEMM columns whose logit is 0; with zero CTC weights and a bias of -50
    everywhere every real logit is -50, so a pad column would win the argmax if it took part"""
    w = ST.make_weights(D)
    w["ctc.ctc_lo.weight"] = np.zeros_like(w["ctc.ctc_lo.weight"])
    w["ctc.ctc_lo.bias"] = np.full_like(w["ctc.ctc_lo.bias"], -50.0)
    e = make_engine(max_batch=1, weights=w, max_samples=58000)
    try:
        pcm = ST.audio(58000, 3)
        ids, t1, t2 = e.debug_frames(pcm)
        assert len(ids) == 65 and (ids == 0).all() and (ids < 500).all()
        assert (t1 == -50.0).all() and (t2 == -50.0).all()
        r = e.transcribe_samples(pcm)
        assert r.tokens == [] and r.prefix == [0, 0, 0, 0]
    finally:
        e.unload_model()


def test_synthetic_small_full_depth():
    pcm = ST.audio(160000, 4)
    e = SenseVoiceEngine()
    e.load_model_with_params("synthetic:sensevoice-small:seed=5", SenseVoiceModelParams(max_batch=1, max_samples=160000))
    try:
        info = e.info()
        assert (info["d"], info["n_heads"], info["head_dim"], info["ff"]) == (512, 4, 128, 2048)
        assert (info["n_enc0_layers"], info["n_enc_layers"], info["n_tp_layers"], info["n_vocab"]) == (1, 49, 20, 25055)
        assert info["dtype"] == L.SPT_DTYPE_F16 and e.missing_tensors() == 0 and info["input_dim"] == 560
        r = e.transcribe_samples(pcm, SenseVoiceInferenceParams(language=Language.English, use_itn=True))
        t = e.timings()
        print(f"sensevoice-small 10 s: {len(r.tokens)} tokens, rows {t['rows']}, front end {t['frontend_ms']:.2f} ms, "
              f"encoder {t['encoder_ms']:.2f} ms, ctc {t['ctc_ms']:.2f} ms, weights {info['weight_bytes'] / 1e6:.0f} MB")
        assert t["rows"] == 171 and t["batch"] == 1
        assert len(r.tokens) <= 171 - 4 and all(0 < k < 25055 for k in r.tokens)
        assert np.isfinite(r.top1).all() and np.isfinite(r.top2).all()
        assert np.isfinite(e.debug_encode(pcm)).all()
    finally:
        e.unload_model()
