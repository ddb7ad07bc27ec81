"""GPU tests of the Moonshine engine against the HF fixtures (tests/golden/moonshine_*.npz, written by
tests/golden/make_golden_moonshine.py; reference restated in tests/moonshine_torch.py).

Bars.  E_EMUL holds, per fixture and audio case, the error of moonshine_torch(emulate_f16=True)
against the f32 fixture, measured on the CPU by

    python scripts/moonshine_measure_ref.py

(stem rel-L2, stem max-abs, encoder rel-L2, encoder max-abs, max |logit(emulate_f16) - logit(f32)|).
The stem / encoder bar is 4 x e_emul (accumulation order, the device's tanh / erf / exp); bar_m =
4 x the logit figure is the margin below which a decode step's argmax is not asserted, and the
teacher-forced logits must be within bar_m / 2.  None of these comes from the engine's output.
Every figure is printed before it is asserted (pytest -s)."""
import math
import os

import numpy as np
import pytest

from spittle_amd import _lib as L
from spittle_amd import (MoonshineEngine, MoonshineInferenceParams, MoonshineModelParams, TranscriptionError)
from tests import moonshine_torch as MT

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

# python scripts/moonshine_measure_ref.py  (see the module docstring)
E_EMUL = {
    "moonshine_small": {
        895: (4.278e-04, 3.004e-03, 5.947e-04, 2.072e-03, 2.362e-03),
        16000: (4.297e-04, 3.853e-03, 5.815e-04, 2.811e-03, 2.583e-03),
        32077: (4.324e-04, 3.733e-03, 5.719e-04, 3.016e-03, 2.519e-03),
        160000: (4.326e-04, 3.797e-03, 5.594e-04, 3.019e-03, 2.945e-03),
    },
    "moonshine_tiny2": {
        895: (3.912e-04, 2.016e-03, 5.865e-04, 2.409e-03, 1.697e-03),
        16000: (4.457e-04, 2.393e-03, 5.671e-04, 2.706e-03, 2.189e-03),
        32077: (4.415e-04, 2.659e-03, 5.661e-04, 2.966e-03, 1.892e-03),
        160000: (4.341e-04, 2.911e-03, 5.759e-04, 2.953e-03, 2.075e-03),
    },
}


def bar_m(name, n):
    return 4.0 * E_EMUL[name][n][4]


def rel_l2(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def make_engine(name, eos=None, max_batch=4):
    D, spec, seed, std = MT.FIXTURES[name]
    e = MoonshineEngine()
    e.load_model_with_params(spec + (f":eos={eos}" if eos is not None else ""),
                             MoonshineModelParams(max_batch=max_batch, max_samples=max(MT.CASES)))
    assert e.missing_tensors() > 0
    e.load_state_dict(MT.make_weights(D, seed, std))
    assert e.missing_tensors() == 0
    return e


class Rig:
    def __init__(self, name):
        self.name = name
        self.D = MT.FIXTURES[name][0]
        self.fx = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
        self.pcm = {n: MT.audio(n, ci) for ci, n in enumerate(MT.CASES)}
        self.eng = make_engine(name)
        self.alone = {}

    def tokens(self, n):
        return [int(t) for t in self.fx[f"c{n}_tokens"]]

    def run_alone(self, n):
        if n not in self.alone:
            self.alone[n] = self.eng.transcribe_samples(self.pcm[n])
        return self.alone[n]

    def safe_prefix(self, n):
        """steps before the first one whose reference margin is below bar_m"""
        low = MT.margins(self.fx[f"c{n}_logits"]) < bar_m(self.name, n)
        return int(np.argmax(low)) if low.any() else len(low)


@pytest.fixture(scope="module", params=list(MT.FIXTURES))
def rig(request):
    r = Rig(request.param)
    yield r
    r.eng.unload_model()


def test_stem_and_encoder(rig):
    for n in MT.CASES:
        rows = MT.fixture_rows(MT.frame_counts(n)[2])
        e = E_EMUL[rig.name][n]
        for what, got, k in (("stem", rig.eng.debug_stem(rig.pcm[n]), 0), ("enc", rig.eng.debug_encode(rig.pcm[n]), 2)):
            assert got.shape == (MT.frame_counts(n)[2], rig.D.d)
            want = rig.fx[f"c{n}_{what}"]
            rl, mx = rel_l2(got[rows], want), float(np.abs(got[rows] - want).max())
            print(f"parity {rig.name} n={n} {what}: rel_l2 {rl:.3e} (bar {4 * e[k]:.3e}) max_abs {mx:.3e} (bar {4 * e[k + 1]:.3e})")
            assert np.isfinite(got).all()
            assert rl <= 4 * e[k] and mx <= 4 * e[k + 1], (rig.name, n, what, rl, mx)


def test_teacher_forced_logits(rig):
    for n in MT.CASES:
        toks, want = rig.tokens(n), rig.fx[f"c{n}_logits"]
        got = rig.eng.debug_logits(rig.pcm[n], [rig.D.bos] + toks[:-1])
        bm = bar_m(rig.name, n)
        mg = MT.margins(want)
        err = float(np.abs(got - want).max())
        print(f"parity {rig.name} n={n} logits: max_abs {err:.3e} (bar {bm / 2:.3e}) steps {len(toks)} below bar_m {(mg < bm).sum()}")
        assert (mg < bm).mean() <= 0.25
        assert err <= bm / 2, (rig.name, n, err)
        am = got.argmax(axis=1)
        for s in range(len(toks)):
            if mg[s] >= bm:
                assert am[s] == toks[s], (rig.name, n, s)


def test_free_running_decode(rig):
    for n in MT.CASES:
        toks, safe = rig.tokens(n), rig.safe_prefix(n)
        r = rig.run_alone(n)
        print(f"decode {rig.name} n={n}: {len(r.tokens)} tokens, compared prefix {safe} of {len(toks)}, n_steps {rig.eng.timings()['n_steps']}")
        assert safe >= 0.75 * len(toks)
        assert r.tokens[:safe] == toks[:safe], (rig.name, n)
        assert len(r.tokens) == MT.max_tokens(n) and not r.hit_eos
        assert (r.top1 >= r.top2).all()
    assert len(rig.run_alone(160000).tokens) == math.ceil(6.5 * 10) == 65


def test_eos_and_max_tokens(rig):
    """eos = the fixture's token at step 4, in a case where that token does not occur before step 4:
    the result is the first 4 tokens, eos itself is not recorded."""
    n = next(n for n in (32077, 160000, 16000) if rig.tokens(n)[4] not in rig.tokens(n)[:4])
    toks = rig.tokens(n)
    assert rig.safe_prefix(n) > 4
    e = make_engine(rig.name, eos=toks[4], max_batch=1)
    try:
        r = e.transcribe_samples(rig.pcm[n])
        print(f"eos {rig.name} n={n}: token {toks[4]} -> {len(r.tokens)} tokens, n_steps {e.timings()['n_steps']}")
        assert r.tokens == toks[:4] and r.hit_eos
        assert 5 <= e.timings()["n_steps"] <= min(16, len(toks))
        r3 = e.transcribe_samples(rig.pcm[n], MoonshineInferenceParams(max_tokens=3))
        assert r3.tokens == toks[:3] and not r3.hit_eos and e.timings()["n_steps"] == 3
    finally:
        e.unload_model()


def test_batch_equals_alone(rig):
    """Every batch row is computed exactly as alone, in two orders: the same tokens and bitwise the same
    top-1 / top-2 logits at every step (they pass through the stem, the encoder, the cross K/V and
    every decode step, so this is stronger than comparing encoder rows within the test-1 bar).  The
    895-sample row next to the 10 s row exercises the length masks; the 10 s rows of a second batch
    push every element-wise kernel past one trip of its grid."""
    for order in ((895, 160000, 16000, 32077), (32077, 16000, 160000, 895), (160000, 160000, 160000, 160000)):
        res = rig.eng.transcribe_batch([rig.pcm[n] for n in order])
        for n, r in zip(order, res):
            a = rig.run_alone(n)
            assert r.tokens == a.tokens, (rig.name, order, n)
            assert np.array_equal(r.top1, a.top1) and np.array_equal(r.top2, a.top2), (rig.name, order, n)


def test_stale_workspace_does_not_leak(rig):
    """a long utterance, then a short one in the same engine: bitwise the fresh engine's result"""
    fresh = make_engine(rig.name, max_batch=1)
    try:
        want = fresh.transcribe_samples(rig.pcm[895])
        want_enc = fresh.debug_encode(rig.pcm[16000])
    finally:
        fresh.unload_model()
    rig.eng.transcribe_batch([rig.pcm[160000], rig.pcm[160000]])
    got = rig.eng.transcribe_samples(rig.pcm[895])
    assert got.tokens == want.tokens and np.array_equal(got.top1, want.top1) and np.array_equal(got.top2, want.top2)
    rig.eng.debug_encode(rig.pcm[160000])
    assert np.array_equal(rig.eng.debug_encode(rig.pcm[16000]), want_enc)


def test_boundaries(rig):
    e = rig.eng
    rig.run_alone(16000)  # a device pass first: its timings must not survive the next call
    r = e.transcribe_samples(rig.pcm[895][:894])
    assert r.text == "" and r.tokens == [] and not r.hit_eos
    t = e.timings()
    assert t["n_steps"] == 0 and t["batch"] == 0 and t["total_ms"] == 0.0  # no device pass ran
    res = e.transcribe_batch([np.zeros(10, np.float32), rig.pcm[16000]])
    assert res[0].tokens == [] and res[1].tokens == rig.run_alone(16000).tokens
    with pytest.raises(TranscriptionError, match="longer than max_samples") as ei:
        e.transcribe_samples(np.zeros(max(MT.CASES) + 1, np.float32))
    assert ei.value.status == L.SPT_ERR_INVALID_ARG
    for dt in ("f32", "bf16"):
        with pytest.raises(TranscriptionError) as ei:
            MoonshineEngine().load_model_with_params("synthetic:moonshine-test-small", MoonshineModelParams(dtype=dt))
        assert ei.value.status == L.SPT_ERR_UNSUPPORTED
    # a missing tensor is an error, not garbage
    D, spec, seed, std = MT.FIXTURES[rig.name]
    m = MoonshineEngine()
    m.load_model_with_params(spec, MoonshineModelParams(max_batch=1, max_samples=16000))
    w = MT.make_weights(D, seed, std)
    del w["model.decoder.layers.1.mlp.fc1.bias"]
    m.load_state_dict(w)
    assert m.missing_tensors() == 1
    with pytest.raises(TranscriptionError, match="not set"):
        m.transcribe_samples(rig.pcm[16000])
    with pytest.raises(TranscriptionError):
        m.load_state_dict({"model.decoder.layers.1.mlp.fc1.bias": np.zeros(3, np.float32)})
    with pytest.raises(TranscriptionError, match="unknown tensor"):
        m.load_state_dict({"model.decoder.nope": np.zeros(3, np.float32)})
    m.unload_model()
    # text through set_vocab: specials dropped, byte pieces joined, the leading space stripped
    toks = rig.run_alone(16000).tokens
    pieces = [f"p{i}" for i in range(D.vocab)]
    pieces[0], pieces[1], pieces[2] = "<unk>", "<s>", "</s>"
    assert toks[0] > 2
    pieces[toks[0]] = "▁héllo"
    e.set_vocab(pieces)
    try:
        text = e.transcribe_samples(rig.pcm[16000]).text
        want = "".join(pieces[t] for t in toks if t > 2).replace("▁", " ")
        assert text == (want[1:] if want.startswith(" ") else want) and text.startswith("héllo")
    finally:
        e.set_vocab([])
    assert e.transcribe_samples(rig.pcm[895]).text == "".join(f"[{t}]" for t in rig.run_alone(895).tokens)


def test_synthetic_base_is_deterministic():
    pcm = MT.audio(32000, 9)
    out = []
    for _ in range(2):
        e = MoonshineEngine()
        mp = MoonshineModelParams.variant("base")
        mp.max_batch, mp.max_samples = 1, 32000
        e.load_model_with_params("synthetic:moonshine-base:seed=5", mp)
        info = e.info()
        assert (info["d"], info["n_heads"], info["head_dim"], info["rotary_dim"], info["ff"]) == (416, 8, 52, 46, 1664)
        assert (info["n_enc_layers"], info["n_dec_layers"], info["n_vocab"], info["bos"], info["eos"]) == (8, 8, 32768, 1, 2)
        assert info["dtype"] == L.SPT_DTYPE_F16 and e.missing_tensors() == 0
        r = e.transcribe_samples(pcm)
        assert 1 <= len(r.tokens) <= 13 and np.isfinite(r.top1).all()
        out.append(r)
        e.unload_model()
    assert out[0].tokens == out[1].tokens and np.array_equal(out[0].top1, out[1].top1)
