"""CPU checks of the token-alignment reference (tests/align_ref.py) and cases (tests/align_cases.py):
the restatement equals HF transformers' _median_filter, normalisation and _dynamic_time_warping on
every case, each crafted case catches the fault it is built for, and the conditions the GPU bars of
tests/test_gpu_align.py rest on hold for the reference alone."""
import numpy as np
import pytest
import torch
from transformers.models.whisper.generation_whisper import _dynamic_time_warping, _median_filter

from tests import align_cases as K
from tests import align_ref as A
from tests import attn_ref as R


def _hf_matrix(p):
    """HF _extract_token_timestamps' normalise + median + head mean on p [A][N][M] (float64)."""
    w = torch.tensor(np.asarray(p, np.float64))
    std = torch.std(w, dim=-2, keepdim=True, unbiased=False)
    mean = torch.mean(w, dim=-2, keepdim=True)
    return _median_filter((w - mean) / std, 7).mean(dim=0).numpy()


def _first_frames(ti, tj):
    return np.array([tj[ti == r].min() for r in range(ti.max() + 1)])


# ------------------------------------------------------------------------------------------- DTW
@pytest.mark.parametrize("c", K.DTW_CASES, ids=lambda c: c["id"])
def test_dtw_equals_hf(c):
    m = K.dtw_inputs(c["id"])
    assert np.all(m * 8 == np.round(m * 8)) and np.abs(m).max() <= 8  # every f32 sum is exact
    ti, tj = K.dtw_ref(c["id"])
    hi, hj = _dynamic_time_warping(-m.astype(np.float64))
    assert np.array_equal(ti, hi) and np.array_equal(tj, hj)
    di, dj = A.dtw(-m, np.float64)  # exact sums: f32 and f64 agree
    assert np.array_equal(ti, di) and np.array_equal(tj, dj)
    jump = A.jumps(ti, tj)
    hf_jump = hj[np.pad(np.diff(hi), (1, 0), constant_values=1).astype(bool)]
    assert np.array_equal(jump, hf_jump) and np.array_equal(jump, _first_frames(ti, tj))
    assert len(jump) == c["N"] and np.all(np.diff(jump) >= 0)


def test_dtw_float_case_equals_hf():
    m = K.dtw_float_inputs()
    ti, tj = A.dtw(-m, np.float32)
    hi, hj = _dynamic_time_warping(-m.astype(np.float64))
    assert np.array_equal(ti, hi) and np.array_equal(tj, hj)


def test_dtw_cases_discriminate():
    """A take-the-minimum DTW gives another path on the constructed tie and on several random cases,
    and ties of all kinds occur."""
    seen = {}
    differs = []
    for c in K.DTW_CASES:
        x = -K.dtw_inputs(c["id"])
        for kind, n in A.tie_kinds(x).items():
            seen[kind] = seen.get(kind, 0) + n
        mi, mj = A.dtw(x, np.float32, rule="min")
        ti, tj = K.dtw_ref(c["id"])
        if not (np.array_equal(mi, ti) and np.array_equal(mj, tj)):
            differs.append(c["id"])
    assert "2x2-c0==c1<c2" in differs and "226x1500-fine" in differs and len(differs) >= 4
    assert all(seen[k] > 0 for k in ("c0==c1<c2", "c0==c2<c1", "c1==c2<c0", "all")), seen
    assert A.tie_kinds(-K.dtw_inputs("2x2-c0==c1<c2"))["c0==c1<c2"] == 1


# ---------------------------------------------------------------------------- normalise + median
def test_median_filter_equals_hf():
    rng = np.random.default_rng(7)
    for M in (1, 3, 4, 5, 7, 8, 50):
        z = rng.normal(size=(2, 5, M))
        assert np.array_equal(A.median_filter(z), _median_filter(torch.tensor(z), 7).numpy())


@pytest.mark.parametrize("c", K.NORM_CASES, ids=lambda c: c["id"])
def test_norm_case(c):
    p = K.norm_inputs(c["id"]).astype(np.float64)
    mean, std = A.stats(p)
    flat = std == 0
    assert int(flat.sum()) == (1 if c["id"] == K.NORM_FLAT else 0)
    # the condition the propagated bar rests on: every other column's std >= 1e-3 of its largest p
    assert np.all((std >= 1e-3 * p.max(-2, keepdims=True)) | flat)
    m = A.matrix(p)
    if not flat.any():
        assert np.allclose(m, _hf_matrix(p), rtol=0, atol=1e-12)
    else:  # HF's z is 0 / 0 = NaN down the flat column (its sort then ranks the NaN last); the rule here is z = 0
        w = torch.tensor(p)
        hf_z = (w - w.mean(-2, keepdim=True)) / torch.std(w, dim=-2, keepdim=True, unbiased=False)
        assert bool(torch.isnan(hf_z[2, :, 1]).all()) and int(torch.isnan(hf_z).sum()) == c["N"]
        assert np.all(A.normalise(p)[2, :, 1] == 0) and np.isfinite(m).all()
    bz, bmed, bm = A.norm_bars(p)
    assert bm.shape == m.shape and np.all(bm > 0) and np.all(bm < 1e-2)  # the bars are far below z's scale of 1


# --------------------------------------------------------------------------------------- align_qk
@pytest.mark.parametrize("c", [c for c in K.QK_CASES if c["M"] == 50 and c["Tq"] == 4], ids=lambda c: c["id"])
def test_qk_case(c):
    q, k, peak = K.qk_inputs(c["id"])
    s = K.QK_SETS[c["set"]]
    for dtype in K.DT:
        qr, kr = R.round_dtype(q, dtype), R.round_dtype(k, dtype)
        for b in range(s["B"]):
            w = b if s["kvrow"] is None else s["kvrow"][b]
            sc = R.scores(qr[b], kr[w])
            assert np.abs(sc).max() <= 64.0  # peaked, within 64 log2 units
            assert np.array_equal(sc.argmax(-1), peak[b])
        full = K.qk_ref(c["id"], dtype, full=True)
        for p, tol in full:
            assert np.allclose(p.sum(-1), 1.0, rtol=0, atol=1e-12) and np.all(tol > 0)
        if c["T"] % 32:  # the padded keys, admitted, move p by more than 100 bars everywhere
            for (p, tol), (pf, _) in zip(K.qk_ref(c["id"], dtype), K.qk_ref(c["id"], dtype, fault="admit_pad")):
                assert np.all(np.abs(p - pf) > 100 * tol)
    if s["kvrow"] is not None:  # the window map matters: another window, another p
        (p0, tol0), _ = K.qk_ref(c["id"], "f32")
        heads = list(s["heads"])
        wrong = A.probs(q[0, heads], k[0, heads], K.qk_M(c)[0])
        assert np.abs(p0 - wrong).max() > 100 * tol0.max()


def test_sharp_case_jumps():
    g = K.SHARP
    q, k = K.sharp_inputs()
    heads = list(g["heads"])
    m = A.matrix(A.probs(q[0, heads], k[0, heads], g["M"]))
    ti, tj = A.dtw(-m.astype(np.float32), np.float32)
    assert np.array_equal(A.jumps(ti, tj), 10 * np.arange(g["n_rows"]))
    t0, t1 = A.token_times(A.jumps(ti, tj), 300)
    assert np.array_equal(t0, 300 + 20 * np.arange(5)) and np.array_equal(t1, t0 + 20)
