"""CPU checks behind tests/test_gpu_gemm.py: the float64 reference of tests/gemm_ref.py
against torch in float64, the exactness budget and the sensitivity every exact case of tests/gemm_cases.py
is built for, the inputs of the other cases, and every refusal of spt_debug_gemm and spt_debug_layernorm
(they are made before the hooks look for a device)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from spittle_amd import _lib as L
from spittle_amd import gemm_debug as D
from spittle_amd.engine import TranscriptionError
from tests import gemm_cases as K
from tests import gemm_ref as R

t64 = lambda a: torch.from_numpy(np.asarray(a, np.float64))  # noqa: E731


# ------------------------------------------------------------------------------------- the reference
def _close(a, b, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))) <= 1e-12, what


def test_reference_against_torch():
    rng = np.random.default_rng(0)
    A, W, bias = rng.standard_normal((2, 37, 96)), rng.standard_normal((48, 96)), rng.standard_normal(48)
    y = rng.standard_normal((2, 37, 48))
    lin = F.linear(t64(A), t64(W), t64(bias))
    _close(R.gemm("bias", A, W, bias), lin, "bias")
    _close(R.gemm("relu", A, W, bias), F.relu(lin), "relu")
    _close(R.gemm("gelu", A, W, bias), F.gelu(lin, approximate="tanh"), "gelu")
    _close(R.gemm("swish", A, W, bias), F.silu(lin), "swish")
    _close(R.gemm("gelu_pos", A, W, bias, pos=y), F.gelu(lin, approximate="tanh") + t64(y), "gelu_pos")
    _close(R.gemm("resid", A, W, bias, alpha=0.5, resid=y), t64(y) + 0.5 * lin, "resid")
    _close(R.gemm("bias_f32", A, W, bias, alpha=2.0), 2.0 * lin, "bias_f32")
    _close(R.gemm("partial", A, W), F.linear(t64(A), t64(W)), "partial")
    x = 20.0 * rng.standard_normal(4000)
    _close(R.gelu(x), F.gelu(t64(x), approximate="tanh"), "gelu far out")
    _close(R.swish(x), F.silu(t64(x)), "swish far out")
    for d in (4, 252, 1536):
        x, w, b = rng.standard_normal((5, d)) + 3.0, rng.standard_normal(d), rng.standard_normal(d)
        _close(R.layernorm(x, w, b), F.layer_norm(t64(x), (d,), t64(w), t64(b), 1e-5), f"layernorm {d}")
        sl, pb = rng.standard_normal((3, 5, d)), rng.standard_normal(d)
        v = t64(x) + 0.5 * (t64(sl).sum(0) + t64(pb))
        _close(R.pend(x, sl, pb, 0.5), v, "pend")


def test_rows_and_kv_index_restates_the_layouts():
    flat = np.arange(100)
    assert R.rows(flat, 3, 4, 3, 6, 2, 40)[1, 2].tolist() == list(range(51, 57))  # 3 + 40 + 2 * 4, rows overlap
    B, H, T, N = 2, 2, 33, 512
    idx = R.kv_index(N, B, H, T)
    assert idx.shape == (B * T, N) and len(np.unique(idx)) == idx.size and idx.max() < 2 * R.kv_layer_elems(B, H, T)
    # row b * T + t, column l * 2 d + kvi * d + h * 64 + e, as kernels.h kv_offset places it
    assert idx[1 * T + 32, 1 * 256 + 1 * 128 + 1 * 64 + 5] == R.kv_layer_elems(B, H, T) + ((1 * B + 1) * H + 1) * 4096 + 2048 + 5


# ------------------------------------------------------------------------------------ the exact cases
EXACT = K.GEMM_EXACT + K.GEMM_SKINNY + K.GEMM_CONV + K.GEMM_KV + K.GEMM_TAIL


@pytest.mark.parametrize("c", EXACT, ids=lambda c: c["id"])
def test_exact_case_budget_and_sensitivity(c):
    b = K.build(c)
    dtype, epi, M, N, Kk = c["dtype"], c["epi"], c["M"], c["N"], b.L.K
    S, amax = K.SLAB[dtype], K.AMAX[dtype]
    A3, W = b.A3.astype(np.float64), b.W.astype(np.float64)
    # integers that are exact in the dtype, A over the whole range with the lowest bit set
    assert np.array_equal(b.A, np.round(b.A)) and np.array_equal(b.W, np.round(b.W))
    assert np.abs(A3).max() <= amax and (A3[A3 != 0] % 2 == 1).all()
    if A3.size >= 4096:
        assert np.abs(A3).max() > 0.95 * amax and np.abs(A3[A3 != 0]).min() <= 0.05 * amax and (np.abs(A3) > amax // 2).mean() > 0.3
    # the budget: every partial sum, in any order, is an integer below 2^24 -- also with alpha applied
    mag = R.abs_product(A3, W, b.bias)
    resid = 0.0 if b.resid is None else np.abs(b.resid)
    assert (mag + resid).max() < 2 ** 24
    assert b.alpha in (0.5, 1.0, 2.0)
    if b.alpha == 0.5:      # units of one half
        assert (mag + 2 * resid).max() < 2 ** 24
    else:
        assert (b.alpha * mag + resid).max() < 2 ** 24
    ref = b.ref if epi != "partial" else b.ref.sum(0)[None]
    assert np.array_equal(ref, np.round(2 * ref) / 2) and np.abs(ref).max() < 2 ** 24
    # every 128-byte K slab contributes to every output element (the conv stem's first and last rows
    # read the caller's zero pad rows: their outer taps are zero by construction)
    inner = slice(1, M - 1) if c["conv"] else slice(None)
    for s in range(Kk // S):
        part = A3[:, inner, s * S:(s + 1) * S] @ W[:, s * S:(s + 1) * S].T
        assert (part != 0).all(), f"slab {s}"
    if b.bias is not None:
        assert len(np.unique(b.bias)) == N
    # no two rows and no two columns agree anywhere (an f16 store cannot hold that many distinct values:
    # those cases check the rounding and the clamp of the store, the f32 ones the place)
    lin = R.product(A3, W) + (0.0 if b.bias is None else b.bias.astype(np.float64))
    if dtype == "f16" and epi not in R.F32_OUT:
        if epi == "kvsplit" and c["kv_T"] >= 31:  # sums beyond +-65504 come back clamped, not inf
            assert (np.abs(lin) > 65504).any() and (R.store(b.ref, epi, dtype) == 65504).any()
    else:
        v = lin.reshape(-1, N)
        assert not len(K._collisions(v)) and not len(K._collisions(v.T))
    # every written element once, inside C, and a margin of elements that must stay
    assert len(np.unique(b.idx)) == b.idx.size and b.idx.min() >= 0 and b.idx.max() < b.C_in.size
    assert b.idx.size < b.C_in.size or (c["batch"] == 1 and not c["ldc_pad"] and not c["c_pad"])


def test_exact_cases_reach_every_listed_edge():
    def seen(v, key):
        return sorted({c[key] for c in EXACT if c["variant"] == v and c["kind"] == "exact"})
    assert seen(1, "M") == [1, 65, 127, 128, 129, 300, 1100] and seen(4, "M") == seen(5, "M") == [1, 63, 64, 65, 129, 130, 300, 1100]
    assert seen(2, "M") == [1, 255, 256, 257, 300] and seen(3, "M") == [1, 15, 16, 17, 33, 48, 49, 64]
    assert seen(1, "N") == seen(4, "N") == [128, 384] and seen(5, "N") == [64, 192] and seen(2, "N") == [256, 512]
    assert seen(3, "N") == [16, 48] and seen(3, "ksplit") == [1, 2, 4]
    for v in (1, 4, 5):
        for dtype in K.DT:
            ks = {c["K"] for c in EXACT if c["variant"] == v and c["dtype"] == dtype}
            assert {K._k(k, dtype) for k in (64, 128, 192, 320)} <= ks
            assert {c["epi"] for c in EXACT if c["variant"] == v and c["dtype"] == dtype} >= set(K.EXACT_EPI)
    assert {c["K"] // c["ksplit"] for c in K.GEMM_SKINNY} == {128, 256, 512, 640}
    # grids that are no multiple of 8
    for c in EXACT:
        if c.get("wgs") == "odd":
            tm, tn = {1: (128, 128), 4: (64, 128), 5: (64, 64)}[c["variant"]]
            assert (-(-c["M"] // tm) * (c["N"] // tn)) % 8
    assert {c["kv_T"] for c in K.GEMM_KV} == {1, 31, 33, 50}
    assert {R.EPI[e] for e in (0, 1, 3, 5, 6, 7, 8)} == set(R.SKINNY_EPI) == \
        {c["epi"] for c in K.GEMM_SKINNY + K.GEMM_ACT + K.GEMM_ROUNDED if c["variant"] == 3}


@pytest.mark.parametrize("c", K.GEMM_ROUNDED + K.GEMM_ACT, ids=lambda c: c["id"])
def test_rounded_and_activation_inputs(c):
    b = K.build(c)
    tiny = 2.0 ** -14 if c["dtype"] == "f16" else 2.0 ** -126
    for a in (b.A, b.W):
        assert np.isfinite(a).all() and ((a == 0) | (np.abs(a) >= tiny)).all(), "normal numbers only"
        assert np.array_equal(a, R.round_dtype(a, c["dtype"]))
    if c["kind"] == "act":
        x, e4 = b.x, R.round_dtype(np.float32([1e4]), c["dtype"])[0]
        assert np.array_equal(R.product(b.A3, b.W), x), "the pre-activation value is the selected entry of W"
        inside = x[np.abs(x) <= 12]
        assert inside.min() == -12 and inside.max() == 12 and np.diff(np.unique(inside)).max() <= (0.13 if c["dtype"] == "bf16" else 0.02)
        assert (x == 0).any() and np.signbit(b.W[b.W == 0]).any() and (x == e4).any() and (x == -e4).any()
        if c["dtype"] != "f16":  # the cube overflows f32
            with np.errstate(over="ignore"):
                assert (np.abs(x.astype(np.float32)) ** 3 == np.inf).sum() >= 4
        kind = "swish" if c["epi"] == "swish" else "gelu"
        bar = R.act_bar(kind, x, b.ref, b.out_dtype)
        assert np.isfinite(bar).all() and (bar > 0).all() and np.isfinite(b.ref).all()
        # away from the flush-to-zero floor the bar is relative: 4 x at most 2.5e-4 (far out in the
        # negative tail, where |u| ~ 100 scales the argument's seven roundings), 4 x 8 ulp near 0
        big = np.abs(R.swish(x) if kind == "swish" else R.gelu(x)) > 1e-30
        assert (R.act_rel(kind, x)[big] < 2.5e-4).all() and (R.act_rel(kind, x)[np.abs(x) <= 1] < 16 * R.U32).all()


# ---------------------------------------------------------------------------------------- LayerNorm
def test_layernorm_rows_are_what_they_claim():
    for d in K.LN_D:
        o = K.ln_inputs(d, 9)
        assert set(o.types) == set(K.ROW_TYPES)
        ref = R.layernorm(o.x, o.w, o.b)
        bar = R.ln_bar(o.x, o.w, o.b, "f32")
        for m, t in enumerate(o.types):
            if t == "constant":
                assert np.array_equal(ref[m], o.b.astype(np.float64)), "a constant row normalises to b"
            if t == "mean1000":
                assert abs(o.x[m].mean() - 1000) < 1 and 0.5 < o.x[m].std() < 2 or d == 4
        op = K.ln_inputs(d, 9, 3, 8)
        v = R.pend(op.x, op.slabs, op.pbias, op.alpha)
        assert np.array_equal(R.slabs(op.slab_flat, 3, op.stride, 9, d), op.slabs) and op.stride > 9 * d
        for m, t in enumerate(op.types):
            if t == "constant":
                assert (v[m] == 1 + 0.5 * (3 + 2)).all()
                assert np.array_equal(R.layernorm(v, op.w, op.b)[m], op.b.astype(np.float64))
        assert np.isfinite(bar).all()
    assert {K.row_type(0, di) for di in range(len(K.LN_D))} == set(K.ROW_TYPES)  # M = 1 meets every type


def test_one_pass_variance_misses_the_bar_on_mean_1000_rows():
    """var = E[x^2] - mean^2 accumulated in f32 is wrong by >= 100 bars on the rows of mean 1000 and
    deviation 1; the two-pass formula in f32 stays inside."""
    for d in (256, 1024, 1536):
        o = K.ln_inputs(d, 9)
        ref, bar = R.layernorm(o.x, o.w, o.b), R.ln_bar(o.x, o.w, o.b, "f32")
        rows = [m for m, t in enumerate(o.types) if t == "mean1000"]
        miss = np.max(np.abs(R.layernorm_onepass_f32(o.x, o.w, o.b) - ref)[rows] / bar[rows])
        assert miss >= 100, (d, miss)
        x32 = o.x.astype(np.float32)
        mean = x32.mean(-1, keepdims=True, dtype=np.float32)
        a = x32 - mean
        two = a / np.sqrt((a * a).mean(-1, keepdims=True, dtype=np.float32) + np.float32(1e-5)) * o.w + o.b
        assert np.max(np.abs(two - ref) / bar) <= 1.0


# ------------------------------------------------------------------------------------- the refusals
def _ok_gemm(**over):
    """A valid 128 x 128 x 128 bf16 call, with `over` applied."""
    kw = dict(A=np.zeros(128 * 128, np.float32), W=np.zeros((128, 128), np.float32), C_in=np.zeros(128 * 128, np.float32),
              M=128, N=128, K=128, dtype="bf16", epi="bias", variant=1)
    kw.update(over)
    A, W, C_in = kw.pop("A"), kw.pop("W"), kw.pop("C_in")
    return D.gemm(A, W, C_in, **kw)


def _rejects(word, fn, *a, **kw):
    with pytest.raises(TranscriptionError) as e:
        fn(*a, **kw)
    assert e.value.status == L.SPT_ERR_INVALID_ARG and word in e.value.message, e.value.message


z = lambda *s: np.zeros(s, np.float32)  # noqa: E731


def test_gemm_refuses_null_and_ranges():
    _rejects("null", _ok_gemm, A=None)
    _rejects("null", _ok_gemm, C_in=None)
    _rejects("dtype is", _ok_gemm, dtype=7)
    _rejects("epilogue 0..8", _ok_gemm, epi=9)
    _rejects("variant 0..5", _ok_gemm, variant=6)
    _rejects("M, N, K >= 1", _ok_gemm, M=0)
    _rejects("batch 1..65535", _ok_gemm, batch=0)
    _rejects("ksplit 1..65535", _ok_gemm, ksplit=0)
    _rejects("negative offset", _ok_gemm, a_off=-8)
    _rejects("ldw >= K", _ok_gemm, W=z(128, 64), ldw=64)


def test_gemm_refuses_what_the_launcher_throws_on():
    _rejects("split-K needs EPI_PARTIAL", _ok_gemm, ksplit=2)
    _rejects("split-K needs EPI_PARTIAL", _ok_gemm, epi="partial", K=192, W=z(128, 192), A=z(128 * 192), ksplit=5)
    _rejects("unsupported shape", _ok_gemm, N=64, W=z(64, 128))            # N % 128
    _rejects("unsupported shape", _ok_gemm, K=96, W=z(128, 96))            # K bytes % 128
    _rejects("unsupported shape", _ok_gemm, variant=5, N=32, W=z(32, 128))
    _rejects("skinny variant needs", _ok_gemm, variant=3, dtype="f32", K=128)
    _rejects("skinny variant needs", _ok_gemm, variant=3)                   # M = 128 > 64
    _rejects("skinny variant needs", _ok_gemm, variant=3, M=16, N=24, W=z(24, 128))
    _rejects("skinny variant needs", _ok_gemm, variant=3, M=16, K=64, W=z(128, 64))


def test_gemm_refuses_skinny_batch():
    """launch_skinny has no grid z: batch > 1 used to compute item 0 only."""
    _rejects("batch == 1", _ok_gemm, variant=3, M=16, batch=2, sA=16 * 128, sC=16 * 128)


def test_gemm_refuses_an_epilogue_the_variant_lacks():
    _rejects("bad epilogue for the skinny", _ok_gemm, variant=3, M=16, epi="gelu_pos", pos=z(16, 128))
    _rejects("bad epilogue for the skinny", _ok_gemm, variant=3, M=16, epi="kvsplit", kv=(1, 16, 1))
    _rejects("256 x 256 tile is bf16 / f16", _ok_gemm, variant=2, dtype="f32")
    _rejects("would not run the 256 x 256", _ok_gemm, variant=2)            # N = 128
    _rejects("needs pos", _ok_gemm, epi="gelu_pos")
    _rejects("batch == 1", _ok_gemm, epi="partial", batch=2, sA=128 * 128, sC=128 * 128, A=z(2 * 128 * 128), C_in=z(2 * 128 * 128))


def test_gemm_refuses_accesses_outside_the_arrays():
    _rejects("A read beyond", _ok_gemm, A=z(128 * 128 - 1))
    _rejects("A read beyond", _ok_gemm, a_off=8)
    _rejects("A read beyond", _ok_gemm, batch=2, sA=128 * 128, sC=128 * 128, C_in=z(2 * 128 * 128))
    _rejects("A read beyond", _ok_gemm, lda=64, A=z(127 * 64 + 127))        # the last row's K elements
    _rejects("C written beyond", _ok_gemm, C_in=z(128 * 128 - 1))
    _rejects("C written beyond", _ok_gemm, c_off=1)
    _rejects("ldc below N", _ok_gemm, ldc=64)
    _rejects("batch items of C overlap", _ok_gemm, batch=2, sA=0, sC=128)
    _rejects("last split-K slab", _ok_gemm, epi="partial", K=256, A=z(128 * 256), W=z(128, 256), ksplit=2,
             c_split=128 * 128, C_in=z(2 * 128 * 128 - 1))
    _rejects("slabs of C overlap", _ok_gemm, epi="partial", K=256, A=z(128 * 256), W=z(128, 256), ksplit=2, c_split=64,
             C_in=z(2 * 128 * 128))
    kv = dict(epi="kvsplit", N=256, W=z(256, 128), M=66, A=z(66 * 128))
    _rejects("M == kv_B * kv_T", _ok_gemm, **kv, kv=(2, 32, 2), C_in=z(R.kv_layer_elems(2, 2, 32)))
    _rejects("N % (2 * kv_H * 64)", _ok_gemm, **kv, kv=(2, 33, 4), C_in=z(R.kv_layer_elems(2, 4, 33)))
    _rejects("kv_B, kv_T, kv_H >= 1", _ok_gemm, **kv, kv=(0, 33, 2), C_in=z(64))
    _rejects("beyond c_count", _ok_gemm, **kv, kv=(2, 33, 2), C_in=z(R.kv_layer_elems(2, 2, 33) - 1))
    _rejects("beyond c_count", _ok_gemm, **kv, kv=(2, 33, 2), C_in=z(R.kv_layer_elems(2, 2, 33)), c_off=64)


def test_gemm_refuses_misaligned_operands():
    """Every kernel stages A and W in 16-byte pieces; the 256 x 256 epilogue stores C and reads pos in them."""
    _rejects("16-byte aligned", _ok_gemm, a_off=4, A=z(128 * 128 + 4))                       # 8 bytes in
    _rejects("16-byte aligned", _ok_gemm, lda=132, A=z(128 * 132))
    _rejects("16-byte aligned", _ok_gemm, ldw=132, W=z(128, 132))
    _rejects("16-byte aligned", _ok_gemm, batch=2, sA=128 * 128 + 4, sC=128 * 128, A=z(2 * 128 * 128 + 4), C_in=z(2 * 128 * 128))
    _rejects("16-byte aligned", _ok_gemm, variant=3, M=16, a_off=4, A=z(16 * 128 + 4))
    g2 = dict(variant=2, M=64, N=256, W=z(256, 128), A=z(64 * 128))
    _rejects("256 x 256 tile needs", _ok_gemm, **g2, c_off=4, C_in=z(64 * 256 + 4))          # bf16 C 8 bytes in
    _rejects("256 x 256 tile needs", _ok_gemm, **g2, ldc=260, C_in=z(64 * 260))
    _rejects("256 x 256 tile needs", _ok_gemm, **g2, epi="resid", ldc=258, C_in=z(64 * 258))
    _rejects("256 x 256 tile needs", _ok_gemm, **g2, epi="bias_f32", c_off=2, C_in=z(64 * 256 + 2))
    _rejects("256 x 256 tile needs", _ok_gemm, **g2, batch=2, sA=0, sC=64 * 256 + 4, C_in=z(2 * 64 * 256 + 4))
    _rejects("256 x 256 tile needs", _ok_gemm, variant=2, M=64, N=256, K=256, W=z(256, 256), A=z(64 * 256), epi="partial", ksplit=2,
             c_split=64 * 256 + 2, C_in=z(2 * 64 * 256 + 2))
    # the 128 x 128 tile stores element by element: the same C is accepted (and then needs a device)
    try:
        _ok_gemm(variant=1, M=64, N=256, W=z(256, 128), A=z(64 * 128), ldc=260, C_in=z(64 * 260))
    except TranscriptionError as e:
        assert e.status == L.SPT_ERR_DEVICE and not torch.cuda.is_available()


def _ok_ln(mode, **over):
    kw = dict(x=z(4, 256), w=z(256), b=z(256), dtype="f32")
    if mode:
        kw.update(slab=z(2 * 4 * 256), ks=2, slab_stride=4 * 256, pbias=z(256), alpha=1.0)
    if mode == 2:
        kw.update(w2=z(256), b2=z(256))
    kw.update(over)
    return D._ln(mode, kw.pop("x"), kw.pop("w"), kw.pop("b"), kw.pop("dtype"), **kw)


def test_layernorm_refuses_bad_shapes():
    for mode in (0, 1, 2):
        _rejects("d % 4", _ok_ln, mode, M=4, d=254)
        _rejects("M >= 1", _ok_ln, mode, M=0, d=256)
        _rejects("d too large", _ok_ln, mode, x=z(1, 1540), M=1, d=1540, w=z(1540), b=z(1540))
        _rejects("dtype is", _ok_ln, mode, dtype=9)
    _rejects("layernorm_pend2: d too large", _ok_ln, 2, x=z(1, 1028), w=z(1028), b=z(1028), w2=z(1028), b2=z(1028),
             pbias=z(1028), slab=z(2 * 1028), slab_stride=1028)
    _rejects("mode 0..2", _ok_ln, 3)
    _rejects("null", _ok_ln, 0, w=None)


def test_layernorm_refuses_split_counts():
    for ks in (0, 3, 5, 16):
        _rejects("split count must be 1, 2, 4 or 8", _ok_ln, 2, ks=ks, slab=z(16 * 4 * 256))
    _rejects("1..64 slabs", _ok_ln, 1, ks=0)
    _rejects("1..64 slabs", _ok_ln, 1, ks=65, slab=z(65 * 4 * 256))


def test_layernorm_refuses_null_pbias():
    """The kernels read pbias unconditionally."""
    for mode in (1, 2):
        _rejects("null pbias", _ok_ln, mode, pbias=None)


def test_layernorm_refuses_slabs_outside_the_array():
    for mode in (1, 2):
        _rejects("beyond slab_count", _ok_ln, mode, slab=z(2 * 4 * 256 - 1))
        _rejects("beyond slab_count", _ok_ln, mode, slab_stride=4 * 256 + 4)
        _rejects("slab_stride >= 0, % 4", _ok_ln, mode, slab_stride=4 * 256 + 2, slab=z(4096))
        _rejects("slab_stride >= 0, % 4", _ok_ln, mode, slab_stride=-4)
        _rejects("null slabs", _ok_ln, mode, slab=None)
    _rejects("pend2 needs", _ok_ln, 2, w2=None)


def test_hooks_without_gpu_report_device_error():
    """A valid call on a machine without a GPU is SPT_ERR_DEVICE; with one it runs."""
    calls = [lambda: _ok_gemm(), lambda: _ok_gemm(variant=3, M=16), lambda: _ok_ln(0)[1], lambda: _ok_ln(1)[1],
             lambda: _ok_ln(2)[1]]
    for call in calls:
        if torch.cuda.is_available():
            assert np.isfinite(call()).all()
            continue
        with pytest.raises(TranscriptionError) as e:
            call()
        assert e.value.status == L.SPT_ERR_DEVICE and e.value.message


def test_exported_and_declared():
    for fn in ("spt_debug_gemm", "spt_debug_layernorm"):
        assert fn in L.EXPORTS
        import ctypes as C
        assert getattr(L.load(), fn).restype is C.c_int
