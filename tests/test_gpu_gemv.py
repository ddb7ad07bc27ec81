"""The decoder GEMV (dec_gemv.h through gemv() of k_dec.hip) with everything the decoder varies -- pending
slabs, x_out, the reload rows, the attention-merge prologue, the K/V cache geometry, live suppression, the
final LayerNorm's row selection, the f32 instances -- and the small kernels of the step (dec_embed,
dec_finalize, dec_advance, dec_reset), alone, through spt_debug_gemv and spt_debug_dec_step (no engine, no
model), against the float64 reference of tests/gemv_ref.py on the cases of tests/gemv_cases.py.

Exact by construction, zero tolerance: x_out against the float32 sum in order; a launch with pending slabs
against the launch on the summed rows; the residual fold of GV_PARTIAL; merge_first against the A_ATTN
prologue; every cache element outside the appended rows (still 0xFF); the top-2 partials as a function of the
returned logits; everything the step hook returns.  The rounded parts are held to bars DESIGN.md 2f derives
(none from what a kernel gives); tests/test_gemv_ref.py has checked, on the CPU, the cases' preconditions and
that each named fault moves an output by >= 100 bars.  The last test prints the largest error per (mode,
source, dtype) as a fraction of its bar; DESIGN.md 2f holds the table measured on an MI355X.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from spittle_amd import _lib as L
from spittle_amd import gemv_debug as D
from spittle_amd.engine import TranscriptionError
from tests import gemv_cases as K
from tests import gemv_ref as R
from tests import qgemv_ref as Q

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SWITCHES = ("SPT_GV_LOGITS_CT", "GV_EXACT_LN", "SPT_GV_EXACT12", "SPT_GV_EXACT12_DIRECT", "SPT_GV_CT2_MIN")
DT = R.DTYPES
DT16 = ("bf16", "f16")

_seen = {}


@pytest.fixture(autouse=True)
def _production_geometry():
    """The launcher's A/B switches are read once per process and select another geometry for the whole run:
    an exported one is refused rather than cleared."""
    for name in SWITCHES:
        assert name not in os.environ, f"{name} selects another GEMV geometry for the whole process"


def _on_device(fn, *a, **kw):
    """A device error ends the session: nothing more is launched on a GPU that has faulted."""
    try:
        return fn(*a, **kw)
    except TranscriptionError as e:
        if e.status == L.SPT_ERR_DEVICE:
            pytest.exit(f"device error, no further launches: {e.message}", returncode=3)
        raise


def _hold(name, got, ref, bar):
    got = np.asarray(got, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        frac = float(np.max(np.where(np.isfinite(got), np.abs(got - ref), np.inf) / bar))
    _seen[name] = max(_seen.get(name, 0.0), frac)
    print(f"{name}: largest error {frac:.3f} of its bar")
    assert frac <= 1.0, f"{name}: {frac:.3f} of the bar"


def _same_bits(a, b, what):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape, what
    bad = a.view(np.uint32) != b.view(np.uint32)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} differ, first at {tuple(np.argwhere(bad)[0])}: " \
                          f"{a[bad][0]!r} against {b[bad][0]!r}"


def _still_ff(v, what):
    """Elements no launch wrote: the 0xFF fill (a NaN in every dtype once converted to f32)."""
    v = np.asarray(v)
    assert np.isnan(v).all(), f"{what}: {int((~np.isnan(v)).sum())} elements written that the launch must not touch"


def _launch(b, dtype, **over):
    return _on_device(D.gemv, b.W, dtype=dtype, **{**b.kw, **over})


def _slabs(b, flatC):
    """The elements of C the launch writes: [ksplit][R][ncol] (or [R][ncol]), and the mask of the rest."""
    ks = b.case.get("ksplit", 1)
    idx = np.stack([b.c_idx + s * b.c_split for s in range(ks)])
    keep = np.ones(flatC.size, bool)
    keep[idx.ravel()] = False
    got = flatC[idx]
    return (got if b.case["mode"] == "partial" else got[0]), keep


def _check(b, dtype, r, name=None, exp=None):
    """One launch against the reference: C within its bar, what it must not write untouched, x_out exact."""
    c = b.case
    exp = K.expect(b, dtype) if exp is None else exp
    got, keep = _slabs(b, r.C)
    ref, bar = exp["C"]
    _hold(name or f"{c['mode']} {c['a_src']} {dtype}", got, ref, bar)
    if c["mode"] == "bias_resid":
        _same_bits(r.C[keep], b.C_in[keep], f"{c['id']}: elements of C the launch must not write")
    else:
        _still_ff(r.C[keep], f"{c['id']}: C outside the rows and columns")
    if r.x_out is not None:
        used = np.zeros(r.x_out.size, bool)
        used[((np.arange(c["R"])[:, None] * b.lda + b.a_row0) + np.arange(c["K"])[None, :]).ravel()] = True
        _same_bits(r.x_out[used], exp["x"][used], f"{c['id']}: x_out against x + p0 + p1 + .. in float32")
        _still_ff(r.x_out[~used], f"{c['id']}: x_out outside the rows")
    return exp


def _check_cache(b, dtype, r, exp):
    c = b.case
    ref, bar, written = exp["cache"]
    _still_ff(r.cache[~written], f"{c['id']}: cache rows outside pos0 .. pos0 + Tq - 1")
    _hold(f"qkv_cache cache {dtype}", r.cache[written], ref[written], bar[written])
    if c.get("clamp") and dtype == "f16":
        pos = c["pos0"]
        assert r.cache[0, 0, 0, pos, 5] == 65504.0 and r.cache[1, 0, 0, pos, 9] == -65504.0, "to_cache's f16 clamp"


def _check_parts(b, r, logits):
    """Every tile's (v1, i1, v2) is a pure function of the returned logits, the mask, blank* and step."""
    c = b.case
    sup = R.suppressed(c["N"], b.mask, b.blank0, b.blank1, b.step)
    for row in range(c["R"]):
        want = R.parts_words(*R.tile_top2(logits[row], sup))
        got = r.part[row]
        assert (got[:, 3] == 0).all(), "the partial's pad word"
        bad = (got[:, :3] != want[:, :3]).any(axis=1)
        assert not bad.any(), f"{c['id']} row {row}: tile {int(np.flatnonzero(bad)[0])} gives " \
                              f"{got[bad][0]} against {want[bad][0]}"


# ------------------------------------------------------------------------------------------ pending slabs
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("mode,n_pend", K.LN_PAIRS)
def test_pending_slabs(mode, n_pend, dtype):
    """LN_SRC(n_pend) at every K and R: x_out is the float32 sum in order; the launch on the summed rows with
    no slabs (x_out off) writes the same bits; both hold the float64 bar.  R = 5 on 4 waves and R = 17 on 8 /
    10 / 12 waves take the second-round rows, which reload their slabs."""
    for Kk in K.pend_k(dtype):
        for Rr in K.ROWS:
            b = K.build(K.pend_case(mode, n_pend, Kk, Rr))
            r = _launch(b, dtype)
            exp = _check(b, dtype, r)
            r0 = _launch(b, dtype, A=exp["x"], pend=None, n_pend=0, x_out=False)
            _same_bits(r0.C, r.C, f"{b.case['id']}: slabs against pre-summed rows")
            if mode == "qkv_cache":
                _check_cache(b, dtype, r, exp)
                _same_bits(r0.cache, r.cache, f"{b.case['id']}: cache, slabs against pre-summed rows")
            if mode == "logits":
                logits = _slabs(b, r.C)[0]
                _check_parts(b, r, logits)
                assert (r0.part == r.part).all()


@pytest.mark.parametrize("dtype", DT)
def test_two_tile_shapes(dtype):
    """N = 4112: two column tiles per workgroup (10 waves x 2 tiles at 10 super-steps, 8 waves x 2 tiles else)."""
    for Kk in ((640, 1024) if dtype == "f32" else (1280, 1024)):
        b = K.build(K.pend_case("bias_gelu", 0, Kk, 5, N=4112))
        r = _launch(b, dtype)
        assert r.plan["ct"] == 2, r.plan
        _check(b, dtype, r, f"bias_gelu ln two tiles {dtype}")
    b = K.build(K.pend_case("bias", 2, 640 if dtype == "f32" else 1280, 17, N=4112))
    _check(b, dtype, _launch(b, dtype), f"bias ln two tiles {dtype}")


# ------------------------------------------------------------------------------------------ direct
@pytest.mark.parametrize("dtype", DT)
def test_direct_and_residual_fold(dtype):
    """A_DIRECT in the three dtypes (ldc > N, the pad columns untouched; lda / a_row0), and the fold:
    GV_PARTIAL with p_resid writes slab 0 = float32(slab 0 without + residual), the other slabs unchanged."""
    for c in K.direct_cases(dtype):
        b = K.build(c)
        r = _launch(b, dtype)
        _check(b, dtype, r)
        if c["mode"] == "partial":
            r0 = _launch(b, dtype, p_resid=None)
            with_, keep = _slabs(b, r.C)
            without, _ = _slabs(b, r0.C)
            _same_bits(with_[0], (without[0] + b.resid).astype(np.float32), f"{c['id']}: slab 0 with the residual folded in")
            _same_bits(with_[1:], without[1:], f"{c['id']}: the other slabs")
            _seen[f"residual fold exact {dtype}"] = 0.0


@pytest.mark.parametrize("dtype", DT)
def test_f32_refusals_and_plans(dtype):
    """What gemv_plan() gives: the geometry per shape, and for f32 the refusal of a staged A operand at
    K = 1280 / 1536 below N = 4096 (20 / 24 super-steps: no 16-wave instance carries an image)."""
    if dtype == "f32":
        for Kk in (1280, 1536):
            b = K.build(K.pend_case("bias", 0, Kk, 1))
            with pytest.raises(TranscriptionError, match="K too large for a staged A operand"):
                D.gemv(b.W, dtype=dtype, **b.kw)
    want = {"f32": {64: (4, 1, 2, 0), 640: (10, 1, 1, 1), 768: (12, 1, 1, 1), 1024: (8, 1, 2, 0)},
            "bf16": {128: (4, 1, 2, 0), 1280: (10, 1, 1, 1), 1536: (12, 1, 1, 1), 384: (4, 1, 2, 0)},
            "f16": {128: (4, 1, 2, 0), 1280: (10, 1, 1, 1), 1536: (12, 1, 1, 1), 384: (4, 1, 2, 0)}}[dtype]
    for Kk, geom in want.items():
        b = K.build(K.pend_case("bias", 0, Kk, 1))
        p = _launch(b, dtype).plan
        assert (p["nwv"], p["ct"], p["maxj"], p["exact"]) == geom, (Kk, p)


# ------------------------------------------------------------------------------------------ A_ATTN
@pytest.mark.parametrize("dtype", DT)
def test_attention_merge(dtype):
    """ATTN_SRC(2 / 3 / 4 / 8): the merged image projected, an empty chunk skipped, all mass in the last chunk;
    S = 8: dec_attn_part_merge + the A_DIRECT projection writes the same bits (merge_first)."""
    for c in K.attn_cases(dtype):
        b = K.build(c)
        r = _launch(b, dtype)
        _check(b, dtype, r, f"bias_resid attn S{c['S']} {dtype}")
        if c["S"] == 8:
            _same_bits(r.merged, r.C, f"{c['id']}: merge kernel + A_DIRECT against the A_ATTN prologue")
            _seen[f"merge_first exact {dtype}"] = 0.0


# ------------------------------------------------------------------------------------------ QKV cache
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("H", K.CACHE_H)
def test_qkv_cache_geometry(H, dtype):
    """pos0 > 0, Tq > 1, ctx > 1, B > 1: k and v of row b * Tq + t land at position pos0 + t of (part, b, h),
    everything else of the cache is still 0xFF, K and V are not exchanged, f16 clamps at +-65504."""
    for c in K.cache_cases():
        if c["H"] != H:
            continue
        b = K.build(c)
        if dtype == "f32" and c["R"] == 64 and H == 6:   # 64 rows x 388 x 4 bytes: beyond the image budget
            with pytest.raises(TranscriptionError, match="A image exceeds the LDS budget"):
                D.gemv(b.W, dtype=dtype, **b.kw)
            continue
        r = _launch(b, dtype)
        exp = _check(b, dtype, r)
        _check_cache(b, dtype, r, exp)


# ------------------------------------------------------------------------------------------ logits
@pytest.mark.parametrize("dtype", DT)
def test_logits_suppression_and_partials(dtype):
    """GV_LOGITS with live masks (none, half, all but one column, one whole tile, bits only in the last partial
    word), the blank rule at step 0 against step 1 on the columns that would win, exact ties inside a tile and
    across tiles, the last of Tq = 3 rows read with the other rows huge."""
    for c in K.logits_cases():
        b = K.build(c)
        r = _launch(b, dtype)
        _check(b, dtype, r)
        logits = _slabs(b, r.C)[0]
        _check_parts(b, r, logits)
        if c.get("ties"):
            for grp in K.TIE_GROUPS:
                for n in grp[1:]:
                    _same_bits(logits[:, n], logits[:, grp[0]], f"{c['id']}: duplicate rows of W give equal logits")
        if c.get("blank") == "winners":
            got1 = R.merge_parts(r.part[0])[1]
            assert (got1 == c["blank0"]) == (c["step"] == 1), "the blank rule holds at step 0 only"
    _seen[f"partials exact {dtype}"] = 0.0


# ------------------------------------------------------------------------------------------ the step hook
def _step_check(o, dtype, parts, **kw):
    args = dict(state=o["state"], dtype=dtype, B=o["B"], Tq=o["Tq"], d=o["d"], ctx=o["ctx"], n_vocab=o["n_vocab"],
                emb=o["emb"], pos=o["pos"], part=parts, n_tiles=o["n_tiles"], n_steps=o["n_steps"], forced=o["forced"],
                done=o["done"], ignore_eot=o["ignore_eot"], out_cap=o["out_cap"], eot=o["eot"])
    emb_t = kw.pop("emb_t", None)
    args.update(kw)
    r = _on_device(D.dec_step, "finalize", **args)
    want = R.finalize_ref(parts, o["state"], B=o["B"], n_tiles=o["n_tiles"], n_vocab=o["n_vocab"], eot=o["eot"],
                          ignore_eot=o["ignore_eot"], forced=o["forced"],
                          forced_len=0 if o["forced"] is None else o["forced"].shape[1], done=o["done"],
                          out_cap=o["out_cap"], Tq=o["Tq"], ctx=o["ctx"],
                          emb_t=R.emb_rows(o["emb"], dtype) if emb_t is None else emb_t, pos=o["pos"])
    assert (r.next_tok == want["next_tok"]).all(), (r.next_tok, want["next_tok"])
    assert (r.out_tok == want["out_tok"]).all(), (r.out_tok, want["out_tok"])
    for k in ("out_top1", "out_top2"):
        g, w = getattr(r, k), want[k]
        assert (np.isnan(g) == np.isnan(w)).all() and (g[~np.isnan(w)] == w[~np.isnan(w)]).all(), k
    assert (r.done == want["done"]).all()
    _same_bits(r.x, want["x"], "the next pass's embedded rows")
    assert (r.state.astype(np.int64) == want["state"]).all(), (r.state, want["state"])
    return r, want


@pytest.mark.parametrize("B", K.STEP_B)
@pytest.mark.parametrize("n_tiles", K.STEP_TILES)
def test_finalize_reduction(n_tiles, B):
    """dec_finalize three times over [B][n_tiles] partials (n_tiles below, at and beyond FIN_T = 1024): the
    state advances once per step whatever B (pos0 + Tq, step + 1, epoch + 1, arrive back at 0); ties across
    tiles go to the lowest index; v2 may be another tile's v1."""
    dtype = DT[(n_tiles + B) % 3]
    o = K.step_inputs(n_tiles, B, 384 if B == 5 else 1280 if n_tiles == 63 else 384)
    v1, i1, v2 = o["v"]
    if n_tiles > 1:
        hi, lo = n_tiles - 1, n_tiles // 2
        v1[0, :, hi] = v1[0, :, lo] = 9.0          # step 0: a tie across tiles, the lower index wins
        v1[1, :, lo], v2[1, :, lo] = 9.0, -5.0     # step 1: v2 comes from another tile's v1
        v1[1, :, hi] = 8.5
    r, want = _step_check(o, dtype, K.step_parts(o))
    if n_tiles > 1:
        assert (r.out_tok[:, 0] == i1[0, :, n_tiles // 2]).all() and (r.out_top2[:, 0] == 9.0).all()
        assert (r.out_top2[:, 1] == 8.5).all()
    _seen["dec_finalize exact"] = 0.0


@pytest.mark.parametrize("dtype", DT)
def test_finalize_rules(dtype):
    """out_cap, done rows, forced tokens inside / past forced_len and out of range, eot with and without
    ignore_eot, all partials invalid, the position clamp below / at / beyond ctx - 1."""
    B, nt = 5, 63
    for ignore_eot in (False, True):
        for pos0, ctx in ((3, 16), (12, 16), (13, 16), (20, 16)):   # pos0 + Tq + steps against ctx - 1 = 15
            o = K.step_inputs(nt, B, 384, seed=pos0, ctx=ctx, pos0=pos0, step0=1, out_cap=3, ignore_eot=ignore_eot)
            v1, i1, v2 = o["v"]
            o["done"][1] = 1                                   # a done row: -1 / -inf / -inf, next = eot
            v1[0, 2, 0], i1[0, 2, 0] = 50.0, o["eot"]          # sequence 2 chooses eot at the first step
            i1[:, 3, :], v1[:, 3, :], v2[:, 3, :] = R.INVALID, -np.inf, -np.inf   # sequence 3: nothing valid
            o["forced"] = np.array([[5, 6], [5, 6], [5, 6], [5, 6], [5, o["n_vocab"] + 3]], np.int32)   # forced_len 2
            # steps 1, 2 are recorded (out_cap 3), step 3 is not; forced covers step 1 only (step < forced_len)
            _step_check(o, dtype, K.step_parts(o))
    _seen[f"dec_finalize rules exact {dtype}"] = 0.0


@pytest.mark.parametrize("dtype", DT)
def test_embed_advance_reset(dtype):
    for Tq in (1, 3):
        for pos0 in (0, 7):
            for d in (384, 1280):
                rng = np.random.default_rng([Tq, pos0, d])
                B, nv, ctx = 5, 200, 12
                emb = rng.standard_normal((nv, d)).astype(np.float32)
                pos = rng.standard_normal((ctx, d)).astype(np.float32)
                tok = rng.integers(0, nv, B * Tq).astype(np.int32)
                r = _on_device(D.dec_step, "embed", state=(pos0, 2, 9, 0), dtype=dtype, B=B, Tq=Tq, d=d, ctx=ctx, n_vocab=nv,
                               emb=emb, pos=pos, tok=tok)
                _same_bits(r.x, R.embed_ref(tok, Tq, pos0, R.emb_rows(emb, dtype), pos), "dec_embed")
                assert tuple(r.state) == (pos0, 2, 9, 0), "dec_embed leaves the state"
    r = _on_device(D.dec_step, "advance", state=(5, 2, 9, 0), n_advance=4)
    assert tuple(r.state) == (9, 2, 10, 0), "dec_advance: pos0 + n, epoch + 1"
    r = _on_device(D.dec_step, "reset", state=(5, 2, 9, 3))
    assert tuple(r.state) == (0, 0, 9, 0), "dec_reset leaves the epoch"
    _seen[f"dec_embed exact {dtype}"] = 0.0


@pytest.mark.parametrize("dtype", DT16)
@pytest.mark.parametrize("qt", ["q5_0", "q4_1"])
def test_packed_embedding(qt, dtype):
    """The QE instances: a token embedding resident in its packed ggml blocks reads as
    round_t(dequant(blocks)) + pos, bit for bit, in dec_embed and in dec_finalize."""
    t = Q.TYPES[qt]
    nv, d, ctx, B = 72, 384, 8, 5
    rng = np.random.default_rng([t, 5])
    nb = nv * d // 32
    codes = rng.integers(0, 32 if Q.Q5[t] else 16, (nb, 32), dtype=np.uint8)
    sc = (rng.uniform(0.5, 1.5, nb) * 2.0 ** -6 * rng.choice([-1.0, 1.0], nb)).astype(np.float32)
    mn = (rng.uniform(-1, 1, nb) * 2.0 ** -3).astype(np.float32)
    blocks = Q.make_blocks(t, codes, sc, mn)
    emb_t = R.round_t(Q.dequant(blocks, t).reshape(nv, d), dtype)
    pos = rng.standard_normal((ctx, d)).astype(np.float32)
    tok = rng.integers(0, nv, B).astype(np.int32)
    r = _on_device(D.dec_step, "embed", state=(2, 0, 0, 0), dtype=dtype, B=B, Tq=1, d=d, ctx=ctx, n_vocab=nv,
                   emb_blocks=blocks, emb_q=t, pos=pos, tok=tok)
    _same_bits(r.x, R.embed_ref(tok, 1, 2, emb_t, pos), "dec_embed over packed blocks")
    o = K.step_inputs(5, B, d, ctx=ctx, pos0=2)
    o["pos"] = pos
    _step_check(o, dtype, K.step_parts(o), emb=None, emb_blocks=blocks, emb_q=t, emb_t=emb_t)


# ------------------------------------------------------------------------------------------ the switches
def _child_cases(dtype):
    ks = (640, 768) if dtype == "f32" else (1280, 1536)
    out = [K.pend_case("bias", 2, k, 17) for k in ks] + [K.pend_case("bias_gelu", 0, ks[0], 5, N=4112)]
    out += [K.case("bias_resid", "direct", ks[1], 40, 5), K.case("bias_resid", "attn", ks[1], 40, 5, H=ks[1] // 64, S=8,
                                                                merge_first=True)]
    out += [K.case("logits", "ln", ks[0], 1000, 5, n_pend=1, mask="half", ties=True)]
    return out


def _child(path):
    """Run in a fresh process: the child cases through gemv_debug, everything returned into `path`."""
    out = {}
    for dtype in DT:
        for c in _child_cases(dtype):
            r = D.gemv(K.build(c).W, dtype=dtype, **K.build(c).kw)
            out[f"{dtype}:{c['id']}:C"] = r.C
            out[f"{dtype}:{c['id']}:plan"] = np.array([r.plan[k] for k in D.PLAN_FIELDS])
            for k in ("x_out", "part", "merged"):
                if getattr(r, k) is not None:
                    out[f"{dtype}:{c['id']}:{k}"] = getattr(r, k)
    np.savez(path, **out)


def test_process_wide_switches(tmp_path):
    """Each switch of gemv_shape is read once per process: one fresh child each runs a small case list.
    SPT_GV_LOGITS_CT=8 must give the default's logits and partials bit for bit (dec_gemv.h's claim); the other
    four select another K order and are held to the float64 bar and to the exact checks.  The first child that
    does not exit 0 ends the test: no further one is started."""
    mine = {(dt, c["id"]): _launch(K.build(c), dt) for dt in DT for c in _child_cases(dt)}
    code = "import sys; from tests.test_gpu_gemv import _child; _child(sys.argv[1])"
    for name, value in (("SPT_GV_LOGITS_CT", "8"), ("GV_EXACT_LN", "0"), ("SPT_GV_EXACT12", "0"),
                        ("SPT_GV_EXACT12_DIRECT", "0"), ("SPT_GV_CT2_MIN", "16")):
        path = str(tmp_path / f"{name}.npz")
        env = dict(os.environ, **{name: value})
        env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
        r = subprocess.run([sys.executable, "-c", code, path], env=env, cwd=ROOT, timeout=120, capture_output=True, text=True)
        assert r.returncode == 0, f"{name}={value}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}"
        theirs = np.load(path)
        changed = 0
        for dt in DT:
            for c in _child_cases(dt):
                b = K.build(c)
                key = f"{dt}:{c['id']}"

                class Rr:
                    pass
                rr = Rr()
                rr.C = theirs[key + ":C"]
                rr.x_out = theirs[key + ":x_out"] if key + ":x_out" in theirs else None
                rr.part = theirs[key + ":part"] if key + ":part" in theirs else None
                _check(b, dt, rr, f"{name}={value} {c['mode']} {c['a_src']} {dt}")
                if c["mode"] == "logits":
                    _check_parts(b, rr, _slabs(b, rr.C)[0])
                if c.get("merge_first"):
                    _same_bits(theirs[key + ":merged"], rr.C, f"{key} under {name}: merge_first")
                changed += int(tuple(theirs[key + ":plan"]) != tuple(mine[dt, c["id"]].plan[k] for k in D.PLAN_FIELDS))
                if name == "SPT_GV_LOGITS_CT" and c["mode"] == "logits":
                    assert int(theirs[key + ":plan"][1]) == 8
                    _same_bits(rr.C, mine[dt, c["id"]].C, f"{key}: logits under SPT_GV_LOGITS_CT=8 against the default")
                    assert (rr.part == mine[dt, c["id"]].part).all(), "partials under SPT_GV_LOGITS_CT=8"
        assert changed, f"{name}={value} changed no case's geometry"
    _seen["SPT_GV_LOGITS_CT=8 exact"] = 0.0


def test_report_largest_errors():
    """What the kernels gave, as a fraction of each bar (DESIGN.md 2f holds the table)."""
    assert _seen, "this test reports what the tests above saw"
    for name in sorted(_seen):
        print(f"{name:52s} {_seen[name]:.3f}")
    assert max(_seen.values()) <= 1.0
