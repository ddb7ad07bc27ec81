"""CPU checks of the SenseVoice restatement (tests/sensevoice_torch.py), the GPU tests' reference: its
fbank against an independent Kaldi-compatible one (HF transformers' audio_utils.spectrogram, stored in
tests/golden/sensevoice_fbank.npz by tests/golden/make_golden_sensevoice.py), and each component
against a torch built-in or a hand-written table."""
import os

import numpy as np
import pytest
import torch

from tests import sensevoice_torch as ST
from tests.golden.make_golden_sensevoice import fixture_rows

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(ROOT, "tests", "golden", "sensevoice_fbank.npz"))


def test_frame_counts(fx):
    want = {400: 1, 1360: 7, 57999: 360, 58000: 361, 160000: 998, 480000: 2998}
    for n, T in want.items():
        assert ST.n_frames(n) == T == int(fx[f"c{n}_frames"]) == 1 + (n - 400) // 160
    assert ST.n_frames(399) == 0
    assert [ST.n_rows(n) for n in ST.CASES] == [5, 6, 64, 65, 171] and ST.n_rows(480000) == 504


def test_fbank_matches_the_hf_fixture(fx):
    """The restatement's f32 fbank against the fixture (computed in f64 by HF, stored as f32).  The bar
    per length is 4 x the restatement's own f32-vs-f64 difference, measured here and, when this was
    written, max-abs 2.5e-05 / 7.6e-05 / 6.2e-04 / 2.5e-04 / 4.1e-04 / 2.5e-03 for n = 400 / 1360 /
    57999 / 58000 / 160000 / 480000 (log-mel values near 22; the largest differences sit in bins
    whose power is a small remainder beside a tone).  4 x allows for a different summation order.
    The f64 run itself must agree with the fixture to the fixture's f32 rounding (1e-5)."""
    for ci, n in enumerate(ST.FIXTURE_LENGTHS):
        pcm = ST.audio(n, ci)
        a32, a64 = ST.fbank(pcm).numpy(), ST.fbank(pcm, torch.float64).numpy()
        rows = fixture_rows(a32.shape[0])
        want = fx[f"c{n}_fbank"]
        own = float(np.abs(a32 - a64).max())
        err32, err64 = float(np.abs(a32[rows] - want).max()), float(np.abs(a64[rows] - want).max())
        print(f"fbank n={n}: f32-vs-f64 {own:.3e}, f32 vs fixture {err32:.3e} (bar {4 * own:.3e}), f64 vs fixture {err64:.3e}")
        assert a32.shape == (ST.n_frames(n), 80) and want.shape == (len(rows), 80)
        assert err64 <= 1e-5
        assert err32 <= 4 * own


def test_lfr_index_tables():
    # T = 1: one row, every block reads frame 0
    assert ST.lfr_index(1).tolist() == [[0] * 7]
    # T = 7: three copies of frame 0 in front, the tail filled with frame 6
    assert ST.lfr_index(7).tolist() == [[0, 0, 0, 0, 1, 2, 3], [3, 4, 5, 6, 6, 6, 6]]
    # T = 361: 61 rows; row i reads frames 6 i - 3 .. 6 i + 3 clamped to [0, 360]
    t = ST.lfr_index(361).tolist()
    assert len(t) == 61
    assert t[0] == [0, 0, 0, 0, 1, 2, 3] and t[1] == [3, 4, 5, 6, 7, 8, 9] and t[2] == [9, 10, 11, 12, 13, 14, 15]
    assert t[59] == [351, 352, 353, 354, 355, 356, 357] and t[60] == [357, 358, 359, 360, 360, 360, 360]
    assert ST.lfr_index(360).shape == (60, 7) and ST.lfr_index(360)[59].tolist() == [351, 352, 353, 354, 355, 356, 357]
    # the rows themselves: LFR row = the indexed fbank frames side by side, then CMVN
    D = ST.TEST_SMALL
    cm = tuple(torch.from_numpy(v) for v in ST.make_cmvn(D))
    pcm = ST.audio(1360, 1)
    fb, ft = ST.fbank(pcm), ST.features(pcm, cm, D)
    assert ft.shape == (2, 560)
    assert torch.equal(ft[1, 80:160], (fb[4] + cm[0][80:160]) * cm[1][80:160])
    assert torch.equal(ft[1, 480:], (fb[6] + cm[0][480:]) * cm[1][480:])


def test_fsmn_is_a_depthwise_conv():
    g = torch.Generator().manual_seed(3)
    for R, d, shift in ((5, 16, 0), (64, 32, 0), (23, 8, 2), (23, 8, -1)):
        v, w = torch.randn(R, d, generator=g), torch.randn(d, 1, 11, generator=g)
        conv = torch.nn.Conv1d(d, d, 11, groups=d, bias=False)
        with torch.no_grad():
            conv.weight.copy_(w)
            padded = torch.nn.functional.pad(v.t()[None], (5 + shift, 5 - shift))
            want = conv(padded)[0].t() + v
        assert torch.allclose(ST.fsmn(v, w, shift), want, atol=1e-5, rtol=1e-5)


def test_attention_core_is_sdpa():
    g = torch.Generator().manual_seed(4)
    for R, H in ((5, 2), (65, 2), (171, 4)):
        q, k, v = (torch.randn(R, H * 128, generator=g) for _ in range(3))
        sp = lambda t: t.reshape(R, H, 128).transpose(0, 1)[None]  # noqa: E731
        want = torch.nn.functional.scaled_dot_product_attention(sp(q), sp(k), sp(v))[0].transpose(0, 1).reshape(R, H * 128)
        assert torch.allclose(ST.attention_core(q, k, v, H), want, atol=2e-5, rtol=1e-4)
        emu = ST.attention_core(q, k, v, H, emu=True)
        assert torch.equal(emu, emu.half().float()) and torch.allclose(emu, want, atol=4e-3, rtol=4e-3)


def test_ctc_collapse_is_unique_consecutive():
    rng = np.random.default_rng(6)
    for R in (4, 5, 6, 64, 171):
        ids = rng.integers(0, 4, R)          # few classes: many repeats and blanks
        prefix, tok, frame = ST.ctc_collapse(ids, 4, 0)
        body = torch.from_numpy(ids[4:])
        u, counts = torch.unique_consecutive(body, return_counts=True)
        starts = torch.cumsum(counts, 0) - counts
        keep = u != 0
        assert prefix == ids[:4].tolist()
        assert tok == u[keep].tolist() and frame == starts[keep].tolist()
    assert ST.ctc_collapse([3, 0, 0, 7], 4, 0) == ([3, 0, 0, 7], [], [])
    assert ST.ctc_collapse([3, 0, 0, 7, 5, 5, 0, 5], 4, 0) == ([3, 0, 0, 7], [5, 5], [0, 3])


def test_positions_and_query_rows():
    D = ST.TEST_SMALL
    W = ST.to_torch(ST.make_weights(D))
    pe = ST.positions(3, 560)
    inv = np.exp(-np.arange(280) * np.log(10000.0) / 279.0)
    assert np.allclose(pe[:, :280].numpy(), np.sin(np.arange(1, 4)[:, None] * inv[None]), atol=1e-6)
    assert np.allclose(pe[:, 280:].numpy(), np.cos(np.arange(1, 4)[:, None] * inv[None]), atol=1e-6)
    ft = torch.zeros(2, 560)
    x = ST.input_rows(W, ft, D, language=2, use_itn=True) - ST.positions(6, 560)
    rows = [4, 1, 2, 14]
    for r, er in enumerate(rows):
        assert torch.allclose(x[r], W["embed.weight"][er] * 16.0, atol=1e-5)
    assert torch.allclose(x[4:], torch.zeros(2, 560), atol=1e-6)
    y = ST.input_rows(W, ft, D) - ST.positions(6, 560)
    assert torch.allclose(y[0], W["embed.weight"][0] * 16.0, atol=1e-5) and torch.allclose(y[3], W["embed.weight"][15] * 16.0, atol=1e-5)


def test_weights_cover_the_engine_table():
    s = ST.tensor_shapes(ST.SMALL)
    assert len(s) == 1 + 13 * 70 + 6
    assert s["encoder.encoders0.0.self_attn.linear_q_k_v.weight"] == (1536, 560)
    assert s["encoder.encoders.48.self_attn.fsmn_block.weight"] == (512, 1, 11)
    assert s["encoder.tp_encoders.19.feed_forward.w_2.weight"] == (512, 2048)
    assert s["ctc.ctc_lo.weight"] == (25055, 512) and s["embed.weight"] == (16, 560)
    total = sum(int(np.prod(v)) for v in s.values())
    assert 230e6 < total < 240e6   # about 234 M parameters
