"""The token-alignment kernels alone (align_qk, align_norm, align_dtw of k_align.hip) against the
float64 / exact-f32 reference of tests/align_ref.py, through the context-free hooks spt_debug_align_*
(no engine, no model).  Inputs are crafted (tests/align_cases.py); tests/test_align_ref.py has checked
the reference against HF transformers and each case against the fault it is built for.

Bars (none is taken from what the kernels give):
  align_qk    4 x attn_ref.rel_bound_f32 x p per probability, on the dtype-rounded inputs (so only the
              f32 arithmetic is under test); the untruncated rows sum to 1 within the same bound
  align_norm  propagated per element from reference quantities: 4 u32 (|p| + |mean|) (2 + |z|) / std on
              z, the largest such bar in the 7-wide window on the median, the mean over the heads on m
  align_dtw   none: path, jumps and length equal the reference's
The largest error seen per kernel, as a fraction of its bar, is printed by each test."""
import numpy as np
import pytest

from spittle_amd import align_debug as D
from tests import align_cases as K
from tests import align_ref as A

pytestmark = pytest.mark.gpu


def _hold(name, got, ref, tol):
    """got within tol of ref everywhere (NaN fails)."""
    got = np.asarray(got, np.float64)
    err = np.where(np.isfinite(got), np.abs(got - ref), np.inf)
    with np.errstate(invalid="ignore", divide="ignore"):
        frac = float(np.max(np.where(err == 0, 0.0, err / tol)))
    print(f"{name}: largest error {frac:.3f} of its bar")
    assert frac <= 1.0, f"{name}: {frac:.3f} of the bar"


# --------------------------------------------------------------------------------------- align_qk
@pytest.mark.parametrize("dtype", K.DT)
@pytest.mark.parametrize("c", K.QK_CASES, ids=lambda c: c["id"])
def test_align_qk(c, dtype):
    s = K.QK_SETS[c["set"]]
    q, k, _ = K.qk_inputs(c["id"])
    Ms = K.qk_M(c)
    N_cap = c["pos0"] + c["Tq"] + 1  # one row more than the pass reaches
    got = D.qk(K.rows_pack(q), k, s["heads"], Ms, Tq=c["Tq"], pos0=c["pos0"], kvrow=s["kvrow"], N_cap=N_cap,
               pad_value=K.PAD, dtype=dtype)
    assert got.shape == (s["B"], len(s["heads"]), N_cap, max(Ms))
    rows = slice(c["pos0"], c["pos0"] + c["Tq"])
    for b, (ref, tol) in enumerate(K.qk_ref(c["id"], dtype)):
        _hold(f"align_qk {dtype}", got[b, :, rows, :Ms[b]], ref, tol)
        # nothing else of the workspace is written: the other rows, and the keys from M[b] on
        untouched = np.ones(got.shape[1:], bool)
        untouched[:, rows, :Ms[b]] = False
        assert np.isnan(got[b][untouched]).all()


@pytest.mark.parametrize("dtype", K.DT)
@pytest.mark.parametrize("cid", ["T1500-heads-Tq4at0-M50", "T1500-map-Tq3at221-M750", "T1024-map-Tq1at0-M4"])
def test_align_qk_rows_sum_to_one(cid, dtype):
    """Every key kept (M = n_audio_ctx): the probabilities are the reference's and each row sums to 1."""
    c = K.QK_BY_ID[cid]
    s = K.QK_SETS[c["set"]]
    q, k, _ = K.qk_inputs(cid)
    got = D.qk(K.rows_pack(q), k, s["heads"], c["T"], Tq=c["Tq"], pos0=c["pos0"], kvrow=s["kvrow"], pad_value=K.PAD,
               dtype=dtype)
    for b, (ref, tol) in enumerate(K.qk_ref(cid, dtype, full=True)):
        rows = got[b, :, c["pos0"]:c["pos0"] + c["Tq"], :]
        _hold(f"align_qk {dtype} (all keys)", rows, ref, tol)
        _hold(f"align_qk {dtype} row sums", rows.astype(np.float64).sum(-1), 1.0, tol.sum(-1))


# -------------------------------------------------------------------------------------- align_norm
def _hold_norm(name, p, stat, m):
    """stat and m of one sequence (p [A][N][M] as the device saw it) against the reference."""
    p64 = p.astype(np.float64)
    mean, std = A.stats(p64)
    # the statistics: a few f32 roundings of quantities no larger than the column's largest p
    u = 4 * A.U32 * np.abs(p64).max(-2)
    _hold(name + " mean", stat[:, 0], mean[:, 0], u)
    _hold(name + " std", stat[:, 1], std[:, 0], u)
    assert np.array_equal(stat[:, 1] == 0, std[:, 0] == 0)
    _, _, bar_m = A.norm_bars(p64)
    _hold(name, m, A.matrix(p64), bar_m)


@pytest.mark.parametrize("c", K.NORM_CASES, ids=lambda c: c["id"])
def test_align_norm(c):
    p = K.norm_inputs(c["id"])
    stat, m = D.norm(p[None])
    _hold_norm("align_norm", p, stat[0], m[0])
    if c["id"] == K.NORM_FLAT:  # z = 0 down the std = 0 column, so the other heads alone make m there
        q = p.copy()
        q[2] = 0.0  # every column of head 2 flat
        _, m0 = D.norm(q[None])
        assert np.isfinite(m0).all()
        _hold("align_norm (flat head)", m0[0], A.matrix(q.astype(np.float64)), A.norm_bars(q.astype(np.float64))[2])


def test_align_norm_ragged():
    """Two sequences of different N and M in one workspace: each is its own reference, and nothing is
    written outside its N x M."""
    g = K.NORM_RAGGED
    p = K.norm_ragged_inputs()
    stat, m = D.norm(p, N=g["N"], M=g["M"])
    for b in range(2):
        N, M = g["N"][b], g["M"][b]
        _hold_norm("align_norm ragged", p[b, :, :N, :M], stat[b, :, :, :M], m[b, :N, :M])
        out = np.ones(m[b].shape, bool)
        out[:N, :M] = False
        assert np.isnan(m[b][out]).all() and np.isnan(stat[b, :, :, M:]).all()
    alone = D.norm(p[1:2, :, :g["N"][1], :g["M"][1]])[1]
    assert np.array_equal(alone[0], m[1, :g["N"][1], :g["M"][1]])  # bitwise the sequence alone


# --------------------------------------------------------------------------------------- align_dtw
def _same_path(got, ti, tj):
    path, jump, ln = got
    assert ln == len(ti), (ln, len(ti))
    assert np.array_equal(path[:, 0], ti) and np.array_equal(path[:, 1], tj)
    assert np.array_equal(jump, A.jumps(ti, tj))


@pytest.mark.parametrize("c", K.DTW_CASES, ids=lambda c: c["id"])
def test_align_dtw(c):
    (got,) = D.dtw(K.dtw_inputs(c["id"])[None])
    _same_path(got, *K.dtw_ref(c["id"]))


def test_align_dtw_float():
    """Unrounded floats: the device path is the f32 reference's on the same f32 matrix."""
    m = K.dtw_float_inputs()
    (got,) = D.dtw(m[None])
    _same_path(got, *A.dtw(-m, np.float32))


def test_align_dtw_ragged():
    g = K.DTW_RAGGED
    m = K.dtw_ragged_inputs()
    got = D.dtw(m, N=g["N"], M=g["M"])
    for b in range(2):
        _same_path(got[b], *A.dtw(-m[b, :g["N"][b], :g["M"][b]], np.float32))


# ------------------------------------------------------------------------ the three kernels in a row
@pytest.mark.parametrize("dtype", K.DT)
def test_sharp_alignment(dtype):
    """Row r attends the frames [10 r, 10 r + 10): two align_qk passes (4 + 2 rows) fill the workspace,
    align_norm and align_dtw follow, and the jumps are 10 r exactly."""
    g = K.SHARP
    q, k = K.sharp_inputs()
    n, M = g["n_rows"], g["M"]
    p = np.full((1, len(g["heads"]), n, M), np.nan, np.float32)
    for pos0, Tq in g["chunks"]:
        part = D.qk(K.rows_pack(q[:, :, pos0:pos0 + Tq]), k, g["heads"], M, Tq=Tq, pos0=pos0, N_cap=n, pad_value=K.PAD,
                    dtype=dtype)
        p[:, :, pos0:pos0 + Tq] = part[:, :, pos0:pos0 + Tq]
    assert np.isfinite(p).all()
    _, m = D.norm(p)
    (got,) = D.dtw(m)
    _same_path(got, *A.dtw(-m[0], np.float32))  # the device path is the reference DTW of the device's own m
    assert np.array_equal(got[1], 10 * np.arange(n))
