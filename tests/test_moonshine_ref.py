"""The torch restatement of Moonshine (tests/moonshine_torch.py) against the HF fixtures, and the
margin precondition of the GPU tests, on the reference alone (no device, no transformers).

Measured with `python scripts/moonshine_measure_ref.py` (torch f32 against HF f32, 16 threads):
stem max-abs 0.0 (the same torch convolutions; up to 1e-7 with another thread count), encoder <= 1.5e-6,
logits <= 2.2e-6, the same tokens in every case.  The bars below are ~10 x those round-off figures
(values reach 4: one f32 ulp there is 4.8e-7)."""
import os

import numpy as np
import pytest
import torch

from tests import moonshine_torch as MT

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
STEM_BAR, ENC_BAR, LOGIT_BAR = 2e-5, 2e-5, 2e-5
_cache = {}


def _run(name):
    """each fixture's reference outputs, computed once and shared"""
    if name in _cache:
        return _cache[name]
    D, _spec, seed, std = MT.FIXTURES[name]
    fx = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    W = MT.to_torch(MT.make_weights(D, seed, std))
    out = {}
    with torch.no_grad():
        for ci, n in enumerate(MT.CASES):
            pcm = MT.audio(n, ci)
            toks = [int(t) for t in fx[f"c{n}_tokens"]]
            st = MT.stem(W, pcm, D)
            en = MT.encoder(W, st, D)
            lg = MT.decoder_logits(W, en, [D.bos] + toks[:-1], D)
            st16 = MT.stem(W, pcm, D, True)
            en16 = MT.encoder(W, st16, D, True)
            lg16 = MT.decoder_logits(W, en16, [D.bos] + toks[:-1], D, True)
            out[n] = (st.numpy(), en.numpy(), lg.numpy(), lg16.numpy(), W, en, st16.numpy(), en16.numpy())
    _cache[name] = (D, fx, out)
    return _cache[name]


@pytest.mark.parametrize("name", list(MT.FIXTURES))
def test_torch_reproduces_hf_fixture(name):
    D, fx, out = _run(name)
    assert int(fx["seed"]) == MT.FIXTURES[name][2] and float(fx["std"]) == MT.FIXTURES[name][3]
    for n in MT.CASES:
        st, en, lg = out[n][:3]
        t3 = MT.frame_counts(n)[2]
        rows = MT.fixture_rows(t3)
        assert st.shape == (t3, D.d) and en.shape == (t3, D.d)
        assert np.abs(st[rows] - fx[f"c{n}_stem"]).max() <= STEM_BAR
        assert np.abs(en[rows] - fx[f"c{n}_enc"]).max() <= ENC_BAR
        assert lg.shape == fx[f"c{n}_logits"].shape == (MT.max_tokens(n), D.vocab)
        assert np.abs(lg - fx[f"c{n}_logits"]).max() <= LOGIT_BAR
        assert lg.argmax(axis=1).tolist() == fx[f"c{n}_tokens"].tolist()
    assert MT.frame_counts(32077) == (500, 165, 82) and MT.frame_counts(895)[2] == 1 and MT.frame_counts(894)[2] == 0


@pytest.mark.parametrize("name", list(MT.FIXTURES))
def test_greedy_loop_reproduces_hf_tokens(name):
    D, fx, out = _run(name)
    for n in (895, 16000, 32077):  # the 65-step case is covered step by step above
        W, en = out[n][4], out[n][5]
        with torch.no_grad():
            toks, hit, rows = MT.greedy(W, en, D, MT.max_tokens(n))
        assert toks == fx[f"c{n}_tokens"].tolist() and not hit and int(fx[f"c{n}_hit_eos"]) == 0
        assert len(set(fx[f"c{n}_tokens"].tolist())) > 1 or n == 895  # not one repeated token


@pytest.mark.parametrize("name", list(MT.FIXTURES))
def test_margin_precondition_of_the_gpu_tests(name):
    """bar_m = 4 x max |logit(emulate_f16) - logit(f32)|: at most 25 % of a case's decode steps may have a
    reference margin below it, the free-running comparison's safe prefix must be >= 75 % of the
    sequence, and the constants the GPU test carries (E_EMUL) must be this measurement."""
    from tests.test_gpu_moonshine import E_EMUL
    D, fx, out = _run(name)
    for n in MT.CASES:
        lg, lg16 = out[n][2], out[n][3]
        d_emu = float(np.abs(lg16 - lg).max())
        bar_m = 4 * d_emu
        mg = MT.margins(fx[f"c{n}_logits"])
        low = mg < bar_m
        first = int(np.argmax(low)) if low.any() else len(low)
        print(f"{name} n={n}: emu-f32 {d_emu:.3e} bar_m {bar_m:.3e} below {low.mean():.3f} safe prefix {first}/{len(low)}")
        assert low.mean() <= 0.25
        assert first >= 0.75 * len(low)
        rows = MT.fixture_rows(MT.frame_counts(n)[2])
        measured = []
        for got, key in ((out[n][6], "stem"), (out[n][7], "enc")):
            want = fx[f"c{n}_{key}"]
            measured += [float(np.linalg.norm(got[rows] - want) / np.linalg.norm(want)), float(np.abs(got[rows] - want).max())]
        measured.append(d_emu)
        print("    e_emul", " ".join(f"{v:.3e}" for v in measured))
        for const, v in zip(E_EMUL[name][n], measured):
            assert abs(const - v) <= 0.1 * v + 1e-6, (name, n, E_EMUL[name][n], measured)
