"""CPU-only: what tests/test_gpu_gemv.py relies on.  The float64 reference of tests/gemv_ref.py against torch
float64; every refusal of spt_debug_gemv and spt_debug_dec_step (made on the host before any launch) and the
status of a valid call without a device; the preconditions the cases' checks assume; and the sensitivity of
the checks: each named fault, applied to the reference, moves an output by >= 100 bars, or changes a value
the GPU test asserts exactly."""
import numpy as np
import pytest
import torch

from spittle_amd import _lib as L
from spittle_amd import gemv_debug as D
from spittle_amd.engine import TranscriptionError
from tests import gemv_cases as K
from tests import gemv_ref as R

NO_GPU = not torch.cuda.is_available()


def _t(x):
    return torch.from_numpy(np.asarray(x, np.float64))


# ------------------------------------------------------------------------------------------ the reference
def test_reference_against_torch():
    F = torch.nn.functional
    rng = np.random.default_rng(1)
    for K_, N, Rr in ((128, 40, 5), (1536, 192, 17)):
        a = rng.standard_normal((Rr, K_))
        W = rng.standard_normal((N, K_)).astype(np.float32)
        bias = rng.standard_normal(N)
        resid = rng.standard_normal((Rr, N))
        y, _ = R.linear(a, np.zeros_like(a), W, "f32", bias, resid)
        want = (F.linear(_t(a), _t(W), _t(bias)) + _t(resid)).numpy()
        assert np.max(np.abs(y - want)) < 1e-12 * np.max(np.abs(want))
        g, _ = R.gelu_out(y, np.zeros_like(y), "f32")
        assert np.max(np.abs(g - F.gelu(_t(y), approximate="tanh").numpy())) < 1e-12 * np.max(np.abs(g))
        w, b = rng.uniform(0.5, 1.5, K_), rng.uniform(-1, 1, K_)
        ln = R.layernorm(a * 3 + 1, w, b)
        assert np.max(np.abs(ln - F.layer_norm(_t(a * 3 + 1), (K_,), _t(w), _t(b), 1e-5).numpy())) < 1e-12 * np.max(np.abs(ln))
    # the merge is a softmax-weighted mean over the chunks: o_c / l_c weighted by softmax2(m_c + log2 l_c)
    p = K.make_partials(rng, 5, 3, 4).astype(np.float64)
    p[0, 0, 1, :64] = 0.0
    o, m, l = _t(p[..., :64]), _t(p[..., 64]), _t(p[..., 65])
    wgt = torch.softmax((m + torch.log2(l)) * np.log(2.0), dim=2)
    want = (wgt[..., None] * torch.nan_to_num(o / l[..., None])).sum(2).reshape(5, 192).numpy()
    got = R.attn_merge(p)
    assert np.max(np.abs(got - want)) < 1e-12 * np.max(np.abs(want))
    # float32 sums in order against torch float32
    x, ps = rng.standard_normal(500).astype(np.float32), rng.standard_normal((4, 500)).astype(np.float32)
    t = torch.from_numpy(x.copy())
    for q in ps:
        t = t + torch.from_numpy(q)
    assert (R.sum_f32(x, ps).view(np.uint32) == t.numpy().view(np.uint32)).all()


# ------------------------------------------------------------------------------------------ refusals
def _refused(match, b, dtype="bf16", **over):
    with pytest.raises(TranscriptionError, match=match) as e:
        D.gemv(b.W, dtype=dtype, need_device=False, **{**b.kw, **over})
    assert e.value.status == L.SPT_ERR_INVALID_ARG


def test_gemv_hook_refusals():
    ln = K.build(K.pend_case("bias", 2, 384, 5))
    _refused("rows must be in 1..64", ln, R=0)
    _refused("rows must be in 1..64", ln, R=65)
    _refused("dtype is f32, bf16 or f16", ln, dtype=7)
    _refused("K alignment", ln, K=320)
    _refused("K split needs partial outputs", ln, ksplit=2)
    _refused("pending slab count must be 0, 1, 2 or 4", ln, n_pend=3)
    _refused("LayerNorm prologue needs K <= 1536 and LN parameters", ln, ln_w=None)
    _refused("unsupported mode / A source", ln, n_pend=1)                      # (GV_BIAS, LN_SRC(1)) is no pair
    _refused("unsupported mode / A source", ln, mode="bias_resid", n_pend=0, C_in=np.zeros(ln.c_count, np.float32))
    _refused("A read beyond a_count", ln, a_row0=4)
    _refused("A read beyond a_count", ln, lda=388)
    _refused("16-byte aligned", ln, a_row0=2)
    _refused("C written beyond c_count", ln, c_count=ln.c_count - 5)
    _refused("ldc below the columns written", ln, ldc=39)
    _refused("pending slabs and x_out belong to A_LN", K.build(K.case("bias_resid", "direct", 384, 40, 5)), x_out=True)
    big = K.build(K.pend_case("bias", 0, 1536, 1))
    _refused("A image exceeds the LDS budget", big, R=32, A=np.zeros(32 * 1536, np.float32))
    _refused("K too large for a staged A operand", big, dtype="f32")            # 24 super-steps, N < 4096
    _refused("K too large for a staged A operand", K.build(K.pend_case("bias", 0, 1280, 1)), dtype="f32")
    d = K.build(K.case("partial", "direct", 512, 40, 5, ksplit=4))
    _refused("K split exceeds the super-steps", d, ksplit=5)
    _refused("split-K slabs of C overlap", d, c_split=8)
    _refused("last split-K slab reaches beyond c_count", d, c_count=d.c_count - 5)
    _refused("residual rows into slab 0 need partial outputs", K.build(K.case("bias_resid", "direct", 384, 40, 5)),
             p_resid=np.zeros((5, 40), np.float32))
    wide = K.build(K.case("partial", "direct", 128 * 49, 16, 1))
    _refused("gemv: K too large", wide)
    at = K.build(K.case("bias_resid", "attn", 768, 40, 5, H=12, S=4))
    _refused("attention-merge prologue needs 2..4 or 8 chunks over all heads", at, S=5)
    _refused("attention-merge prologue needs 2..4 or 8 chunks over all heads", at, H=11)
    _refused("merge_first needs A_ATTN with 8 chunks", at, merge_first=True)
    qc = K.build(K.cache_cases()[1])
    _refused("pos0 \\+ Tq beyond ctx", qc, pos0=14)
    _refused("R = B \\* Tq", qc, B=3)
    _refused("N = 3 d", qc, cache_H=3)
    lg = K.build(K.logits_cases()[1])
    _refused("suppress shorter than", lg, suppress=lg.mask[:-1])
    _refused("n_tiles below 1", lg, n_tiles=0)


def _step_refused(match, op, **kw):
    with pytest.raises(TranscriptionError, match=match) as e:
        D.dec_step(op, need_device=False, **kw)
    assert e.value.status == L.SPT_ERR_INVALID_ARG


def _step_kw(**over):
    o = K.step_inputs(5, 2, 128)
    kw = dict(state=o["state"], dtype="bf16", B=2, Tq=1, d=128, ctx=o["ctx"], n_vocab=o["n_vocab"], emb=o["emb"], pos=o["pos"],
              part=K.step_parts(o), n_tiles=5, n_steps=3, done=o["done"], out_cap=8, eot=o["eot"])
    kw.update(over)
    return kw


def test_step_hook_refusals():
    _step_refused("op 0..3", 9, state=(0, 0, 0, 0))
    _step_refused("null state", "reset", state=None)
    _step_refused("negative pos0, step or arrive", "advance", state=(-1, 0, 0, 0))
    _step_refused("negative n_advance", "advance", state=(0, 0, 0, 0), n_advance=-1)
    _step_refused("eot outside", "finalize", **_step_kw(eot=72))
    _step_refused("n_steps 1..64", "finalize", **_step_kw(n_steps=0))
    _step_refused("starts from arrive == 0", "finalize", **_step_kw(state=(0, 0, 0, 1)))
    _step_refused("out_cap below 1", "finalize", **_step_kw(out_cap=0))
    _step_refused("packed embedding needs a bf16 or f16 engine", "finalize", **_step_kw(dtype="f32", emb_q=6, emb_blocks=b"x"))
    _step_refused("emb_blocks_bytes is not the size", "finalize", **_step_kw(emb_q=6, emb_blocks=b"x"))
    _step_refused("no resident layout", "finalize", **_step_kw(emb_q=2, emb_blocks=b"x"))
    tok = np.zeros(2, np.int32)
    _step_refused("pos0 \\+ Tq beyond ctx", "embed", **_step_kw(tok=tok, state=(16, 0, 0, 0)))
    _step_refused("token outside", "embed", **_step_kw(tok=np.array([0, 72], np.int32)))
    _step_refused("null tok", "embed", **_step_kw())


@pytest.mark.skipif(not NO_GPU, reason="a device is present")
def test_valid_calls_without_a_device():
    b = K.build(K.pend_case("bias", 2, 1280, 5))
    r = D.gemv(b.W, dtype="bf16", need_device=False, **b.kw)
    assert r.status == L.SPT_ERR_DEVICE
    assert (r.plan["nwv"], r.plan["ct"], r.plan["maxj"], r.plan["exact"], r.plan["rg"]) == (10, 1, 1, 1, 1)
    assert D.dec_step("finalize", need_device=False, **_step_kw()).status == L.SPT_ERR_DEVICE
    assert D.dec_step("reset", need_device=False, state=(1, 2, 3, 0)).status == L.SPT_ERR_DEVICE


def test_plans_without_a_device():
    """gemv_plan() through the hook (it fills `plan` before it looks for a device, so the answer is the same
    with and without one): the geometry of every shape class of gemv_shape."""
    def plan(c, dtype):
        b = K.build(c)
        try:
            p = D.gemv(b.W, dtype=dtype, need_device=False, **b.kw).plan
        except TranscriptionError as e:   # a device is present and something else went wrong
            raise AssertionError(e.message)
        return p["nwv"], p["ct"], p["maxj"], p["exact"], p["rg"]
    assert plan(K.pend_case("bias", 0, 128, 1), "bf16") == (4, 1, 2, 0, 1)
    assert plan(K.pend_case("bias", 0, 1280, 17), "f16") == (10, 1, 1, 1, 2)
    assert plan(K.pend_case("bias_gelu", 0, 1280, 33, N=4112), "bf16") == (10, 2, 2, 1, 4)
    assert plan(K.pend_case("bias_gelu", 0, 1024, 5, N=4112), "bf16") == (8, 2, 3, 0, 1)
    assert plan(K.pend_case("bias", 0, 1536, 5), "bf16") == (12, 1, 1, 1, 1)
    assert plan(K.pend_case("bias", 0, 768, 5), "f32") == (12, 1, 1, 1, 1)
    assert plan(K.pend_case("logits", 0, 384, 5), "bf16") == (4, 4, 4, 0, 1)
    assert plan(K.case("partial", "direct", 5120, 40, 5), "bf16") == (16, 1, 3, 0, 1)
    assert plan(K.case("partial", "direct", 5120, 40, 5, ksplit=4), "bf16") == (8, 1, 2, 0, 1)
    assert plan(K.case("bias_resid", "attn", 1536, 40, 5, H=24, S=8), "f16") == (12, 1, 1, 1, 1)


# ------------------------------------------------------------------------------------------ preconditions
def test_case_preconditions():
    for dtype in R.DTYPES:
        for c in K.attn_cases(dtype):
            p = K.build(c).apart
            m, l = p[..., 64], p[..., 65]
            live = np.isfinite(m)
            assert (l[live] > 0).all() and live.any(axis=2).all(), "l > 0 and never all chunks empty"
            assert not live[0, 0, 1] and np.isnan(p[0, 0, 1, :64]).all()
        for c in K.logits_cases():
            b = K.build(c)
            y, bar = K.expect(b, dtype)["C"]
            sup = R.suppressed(c["N"], b.mask, b.blank0, b.blank1, b.step)
            if c.get("ties"):
                w = R.round_t(b.W, dtype)
                for grp in K.TIE_GROUPS:
                    for n in grp[1:]:
                        assert (w[n] == w[grp[0]]).all(), "crafted ties tie after rounding to T"
                        assert (y[:, n] == y[:, grp[0]]).all()
                # an in-tile pair (33, 38 or its negation 49, 54) and the in-tile part of the triple lead their
                # tile by more than the bars in at least one row: there the lowest index must win and v2 == v1
                for n in (33, 200):
                    led = 0
                    for row in y:
                        lead = n if row[n] > 0 else n + 16
                        t0 = 16 * (lead // 16)
                        others = np.delete(row[t0:t0 + 16], [k - t0 for g in K.TIE_GROUPS for k in g if t0 <= k < t0 + 16])
                        led += int(row[lead] > others.max() + 4 * bar.max())
                    assert led >= 1, (dtype, c["id"], n)
            if c.get("blank") == "winners":
                # the blank columns win their rows by more than the bars: the rule decides the winner
                for row, col in ((0, c["blank0"]), (-1, c["blank1"])):
                    second = np.delete(y[row], [c["blank0"], c["blank1"]]).max()
                    assert y[row, col] - second > 4 * bar[row].max(), (dtype, c["id"])
            if c.get("mask") == "all_but_one":
                assert (~sup).sum() == 1
            if c.get("mask") == "last_word":
                assert sup[:(c["N"] // 32) * 32].sum() == 0 and sup.sum() == c["N"] % 32 - 1
            if c.get("mask") == "one_tile":
                assert sup[80:96].all() and sup.sum() == 16
    # the step hook's random partials have a unique winner per (step, sequence)
    for nt in K.STEP_TILES:
        o = K.step_inputs(nt, 5, 384)
        v1 = o["v"][0]
        s = np.sort(v1, axis=2)
        if nt > 1:
            assert (s[..., -1] > s[..., -2]).all()
        assert (o["v"][1] < o["n_vocab"]).all()


# ------------------------------------------------------------------------------------------ sensitivity
def _moved(exp, bad, key="C"):
    (ref, bar), (ref2, _) = exp[key][:2], bad[key][:2]
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.abs(ref - ref2) / bar
    return float(np.nanmax(np.where(np.isnan(ref2) & ~np.isnan(ref), np.inf, d)))


@pytest.mark.parametrize("dtype", R.DTYPES)
def test_faults_move_the_reference(dtype):
    # one slab dropped; a_row0 ignored
    for mode, n_pend in K.LN_PAIRS:
        if n_pend:
            b = K.build(K.pend_case(mode, n_pend, K.pend_k(dtype)[1], 5))
            exp, bad = K.expect(b, dtype), K.expect(b, dtype, "slab_dropped")
            assert _moved(exp, bad) >= 100.0, (mode, n_pend)
            assert (exp["x"] != bad["x"]).any()
    c = [c for c in K.logits_cases() if c["K"] == 384][0]
    b = K.build(c)
    assert _moved(K.expect(b, dtype), K.expect(b, dtype, "a_row0_ignored")) >= 100.0
    c = [c for c in K.direct_cases("bf16") if c.get("a_row0")][0]
    b = K.build(c)
    assert _moved(K.expect(b, dtype), K.expect(b, dtype, "a_row0_ignored")) >= 100.0
    # the cache: position off by one, K / V exchanged, b and t exchanged
    for c in K.cache_cases():
        if dtype == "f32" and c["R"] == 64 and c["H"] == 6:
            continue
        b = K.build(c)
        exp = K.expect(b, dtype)
        ref, bar, written = exp["cache"]
        for fault in ("cache_pos_off_by_one", "kv_exchanged", "b_t_exchanged"):
            ref2, _, written2 = K.expect(b, dtype, fault)["cache"]
            if fault == "b_t_exchanged" and (c["B"] == 1 or c["Tq"] == 1):
                continue
            if (written != written2).any():
                continue   # the untouched-elements check sees it
            both = written & written2
            with np.errstate(invalid="ignore"):
                assert np.nanmax(np.abs(ref[both] - ref2[both]) / bar[both]) >= 100.0, (c["id"], fault)
        # off by one always moves which rows are written, unless it falls off the end: then a row is missing
        assert (written != K.expect(b, dtype, "cache_pos_off_by_one")["cache"][2]).any()
    # the merge
    for c in K.attn_cases(dtype)[:12]:
        b = K.build(c)
        exp = K.expect(b, dtype)
        assert _moved(exp, K.expect(b, dtype, "merge_unweighted")) >= 100.0
        bad = K.expect(b, dtype, "empty_chunk_not_skipped")
        assert np.isnan(bad["C"][0][0]).all() and not np.isnan(exp["C"][0]).any()


def test_faults_change_the_exact_checks():
    dtype = "bf16"
    hit = {f: 0 for f in ("blank_at_step_1", "mask_bit_shifted", "v2_second_distinct", "tie_to_higher_index")}
    for c in K.logits_cases():
        b = K.build(c)
        y = K.expect(b, dtype)["C"][0].astype(np.float32)
        sup = R.suppressed(c["N"], b.mask, b.blank0, b.blank1, b.step)
        for f in ("blank_at_step_1", "mask_bit_shifted"):
            sup2 = R.suppressed(c["N"], b.mask, b.blank0, b.blank1, b.step, f)
            hit[f] += int(any((R.parts_words(*R.tile_top2(r, sup)) != R.parts_words(*R.tile_top2(r, sup2))).any() for r in y))
        for f in ("v2_second_distinct", "tie_to_higher_index"):
            hit[f] += int(any((R.parts_words(*R.tile_top2(r, sup)) != R.parts_words(*R.tile_top2(r, sup, fault=f))).any()
                              for r in y))
    assert all(v > 0 for v in hit.values()), hit
    # the step hook: ties across tiles, v2 from the multiset, the position clamp
    o = K.step_inputs(63, 5, 384, ctx=16, pos0=13)
    v1, i1, v2 = o["v"]
    v1[0, :, 62] = v1[0, :, 31] = 9.0
    kw = dict(B=5, n_tiles=63, n_vocab=o["n_vocab"], eot=o["eot"], ignore_eot=False, forced=None, forced_len=0, done=o["done"],
              out_cap=8, Tq=1, ctx=16, emb_t=o["emb"], pos=o["pos"])
    good = R.finalize_ref(K.step_parts(o), o["state"], **kw)
    for f in ("tie_to_higher_index", "v2_second_distinct", "pos_clamp_at_ctx"):
        bad = R.finalize_ref(K.step_parts(o), o["state"], fault=f, **kw)
        assert any((np.asarray(good[k]) != np.asarray(bad[k])).any() for k in ("out_tok", "out_top2", "x")), f
    assert tuple(good["state"]) == (16, 3, 44, 0)
