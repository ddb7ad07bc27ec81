"""The GEMM tiles (k_gemm.hip: the 128 x 128 ring and its 64 x 128 / 64 x 64 instantiations, the 256 x 256
tile in its three schedules, the skinny kernel) and the LayerNorm kernels (k_norm.hip) alone against the
float64 reference of tests/gemm_ref.py, through the context-free hooks spt_debug_gemm and
spt_debug_layernorm (no engine, no model).

Inputs are crafted (tests/gemm_cases.py).  The exact cases hold small integers: every partial sum in any
order is exact in f32, so the tolerance is zero and any dropped, duplicated or misplaced element fails;
every element of C the launch must not write is compared with what the caller put there.
tests/test_gemm_ref.py has checked, on the CPU, the budget and the sensitivity of each case.

Bars of the other cases (none is taken from what the kernels give):
  rounded     4 x (K + 2) 2^-24 (sum |a w| + |bias|) per element (+ half an ulp of a 16-bit output)
  activation  4 x the linear bound of common.h's gelu_tanh / swish at the exact pre-activation value
  LayerNorm   4 x the linear bound of the two-pass f32 algorithm, evaluated from the row
The largest error seen per kernel, case class and dtype, as a fraction of its bar, is printed by the last
test of the file; DESIGN.md 2e holds the table measured on an MI355X.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from spittle_amd import _lib as L
from spittle_amd import gemm_debug as D
from spittle_amd.engine import TranscriptionError
from tests import gemm_cases as K
from tests import gemm_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
KERNEL = {0: "auto", 1: "128x128", 2: "256x256", 3: "skinny", 4: "64x128", 5: "64x64"}
ONCE_PER_PROCESS = ("SPT_GEMM128", "SPT_GEMM_NT_STAGES", "SPT_GEMM_NT_RASTER")
PER_LAUNCH = ("SPT_G2_STAGGER", "SPT_G2_PP", "SPT_GEMM_F32_SMALL", "SPT_GEMM_F32_T128MIN", "SPT_GEMM_BF16_T256G")

_seen = {}


@pytest.fixture(autouse=True)
def _production_variant(monkeypatch):
    """No A/B switch of the launcher left in the environment: those read once per process select another
    kernel for the whole run, so an exported one is refused rather than cleared."""
    for name in ONCE_PER_PROCESS:
        assert name not in os.environ, f"{name} selects another GEMM kernel for the whole process"
    for name in PER_LAUNCH:
        monkeypatch.delenv(name, raising=False)


def _hold(name, got, ref, tol):
    """got within tol of ref everywhere (NaN fails); the largest error / tol goes into _seen[name]."""
    got = np.asarray(got, np.float64)
    frac = float(np.max(np.where(np.isfinite(got), np.abs(got - ref), np.inf) / tol))
    _seen[name] = max(_seen.get(name, 0.0), frac)
    print(f"{name}: largest error {frac:.3f} of its bar")
    assert frac <= 1.0, f"{name}: {frac:.3f} of the bar"


def _same_bits(a, b, what):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape, what
    bad = a.view(np.uint32) != b.view(np.uint32)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} differ, first at {tuple(np.argwhere(bad)[0])}: " \
                          f"{a[bad][0]!r} against {b[bad][0]!r}"


def _on_device(fn, *a, **kw):
    """A device error ends the session: nothing more is launched on a GPU that has faulted."""
    try:
        return fn(*a, **kw)
    except TranscriptionError as e:
        if e.status == L.SPT_ERR_DEVICE:
            pytest.exit(f"device error, no further launches: {e.message}", returncode=3)
        raise


def _launch(b, **over):
    """The case's launch -> (the elements it writes, in the shape of b.idx; the whole C buffer)."""
    out = _on_device(D.gemm, b.A, b.W, b.C_in, **{**b.kw, **over})
    return out[b.idx], out


def _untouched(b, out):
    """Every element of C outside the case's writes holds the caller's bits: rows >= M of a tail tile, the
    pad columns of ldc > N, the rows before and after a batch item, the keys from kv_T to the next 32."""
    keep = np.ones(out.size, bool)
    keep[b.idx.ravel()] = False
    _same_bits(out[keep], b.C_in[keep], f"{b.case['id']}: elements the launch must not write")


def _exact(c, **over):
    b = K.build(c)
    got, out = _launch(b, **over)
    _untouched(b, out)
    _same_bits(got, R.store(b.ref, c["epi"], c["dtype"]), f"{c['id']}: the {KERNEL[c['variant']]} kernel against float64")
    _seen[f"{KERNEL[c['variant']]} exact {c['dtype']}"] = 0.0
    return got


def _bar(b):
    """The rounded cases' bar, per element, in the shape of b.ref."""
    c = b.case
    if c["epi"] == "partial":
        Kc = b.L.K // c["ksplit"]
        return np.stack([R.gemm_bar(b.A3[0][:, s * Kc:(s + 1) * Kc], b.W[:, s * Kc:(s + 1) * Kc], None, Kc, b.ref[s], "f32")
                         for s in range(c["ksplit"])])
    mag = R.abs_product(b.A3, b.W, b.bias)
    lin = 4.0 * (b.L.K + 2) * R.U32 * (abs(b.alpha) * mag + (0.0 if b.resid is None else np.abs(b.resid)))
    return lin + R.half_ulp(b.ref, b.out_dtype)


# ----------------------------------------------------------------------------------------- exact cases
def test_one_tile_is_exact():
    """The simplest case first: one 128 x 128 tile, one K slab, small integers.  If this is not bit-exact
    the MFMA path itself rounds integers, and nothing below can be held at zero tolerance."""
    for dtype in K.DT:
        _exact(K.case(1, dtype, 128, 128, 64, "bias_f32"))


@pytest.mark.parametrize("c", K.GEMM_EXACT, ids=lambda c: c["id"])
def test_gemm_exact(c):
    _exact(c)


@pytest.mark.parametrize("c", K.GEMM_SKINNY, ids=lambda c: c["id"])
def test_gemm_skinny_exact(c):
    _exact(c)


@pytest.mark.parametrize("c", K.GEMM_CONV, ids=lambda c: c["id"])
def test_gemm_conv_stem_exact(c):
    """Overlapping rows (lda < K), batch 2 with strides, C one row into each item's M + 2 rows."""
    _exact(c)


@pytest.mark.parametrize("c", K.GEMM_KV, ids=lambda c: c["id"])
def test_gemm_kvsplit_exact(c):
    """Every (layer, k / v, b, h, t, e) at its kv_offset, the keys from kv_T to the next 32 untouched, and
    in f16 sums beyond +-65504 clamped, not inf."""
    got = _exact(c)
    assert np.isfinite(got).all()


# --------------------------------------------------------------------------------------- rounded cases
@pytest.mark.parametrize("c", K.GEMM_ROUNDED, ids=lambda c: c["id"])
def test_gemm_rounded(c):
    b = K.build(c)
    got, out = _launch(b)
    _untouched(b, out)
    _hold(f"{KERNEL[c['variant']]} rounded {c['dtype']}", got, b.ref, _bar(b))


# ------------------------------------------------------------------------------------ activation cases
def _act_check(c, got, b):
    kind = "swish" if c["epi"] == "swish" else "gelu"
    ref, x = b.ref, b.x
    bar = R.act_bar(kind, x, ref, b.out_dtype)
    if b.pos is not None:  # the activation's error scales with its own value, not with the sum (they may
        # cancel); the add of a nonzero pos rounds once more
        bar = R.act_bar(kind, x, R.gelu(x), "f32") + 4.0 * R.U32 * np.abs(ref) * (b.pos[None] != 0)
    assert np.isfinite(got).all(), "an activation of a finite value is finite"
    # the sign of x where the result is not below the flush-to-zero floor (a pre-activation -0 does not
    # exist: the accumulator starts at +0); zero at zero
    act = R.act(c["epi"], x)
    firm = (np.abs(act) > (np.abs(x) + 1.0) * R.TINY + R.half_ulp(act, b.out_dtype)) & (b.pos is None or b.pos[None] == 0)
    assert (np.signbit(got[firm]) == np.signbit(x[firm])).all(), "sign"
    assert (got[(x == 0) & (ref == 0)] == 0).all()
    _hold(f"{KERNEL[c['variant']]} {c['epi']} {c['dtype']}", got, ref, bar)


@pytest.mark.parametrize("c", K.GEMM_ACT, ids=lambda c: c["id"])
def test_gemm_activation(c):
    b = K.build(c)
    got, out = _launch(b)
    _untouched(b, out)
    _act_check(c, got, b)


# ------------------------------------------------------------------------ the 256 x 256 tile's schedules
SCHEDULES = ({}, {"SPT_G2_STAGGER": "0"}, {"SPT_G2_PP": "0"})
G2_CASES = K.GEMM_TAIL + [c for c in K.GEMM_ACT if c["variant"] == 2 and c["epi"] == "gelu_pos"] + \
    [c for c in K.GEMM_ROUNDED if c["variant"] == 2] + [c for c in K.GEMM_KV if c["variant"] == 2 and c["kv_T"] == 33]


@pytest.mark.parametrize("c", G2_CASES, ids=lambda c: c["id"])
def test_g2_schedules(c, monkeypatch):
    """Default (ping-pong), SPT_G2_PP=0 (staggered) and SPT_G2_STAGGER=0 (lock-step), read per launch: each
    held to the reference, all three the same bits.  M = 257: the pre-loaded residual / pos rows of the
    tail tile are clamped, and rows >= M stay untouched."""
    b = K.build(c)
    outs = []
    for env in SCHEDULES:
        with monkeypatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            got, out = _launch(b)
        _untouched(b, out)
        if c["kind"] == "act":
            _act_check(c, got, b)
        elif c["kind"] == "rounded":
            _hold(f"256x256 rounded {c['dtype']}", got, b.ref, _bar(b))
        else:
            _same_bits(got, R.store(b.ref, c["epi"], c["dtype"]), f"{c['id']} under {env}")
        outs.append(out)
    _same_bits(outs[1], outs[0], "lock-step against ping-pong")
    _same_bits(outs[2], outs[0], "staggered against ping-pong")


# --------------------------------------------------------------------------------- cross-tile equality
@pytest.mark.parametrize("dtype", K.DT)
@pytest.mark.parametrize("epi", R.EPI)
def test_tiles_write_the_same_bits(epi, dtype):
    """M = 300, N = 512, K = 192: every tile shape accepts it, and every epilogue writes the same bits from
    each (k_gemm.hip's claim: every C element is the same MFMA chain in every tile shape)."""
    cases = K.cross_cases(dtype, epi)
    outs = []
    for c in cases:
        b = K.build(c)
        got, out = _launch(b)
        _untouched(b, out)
        outs.append(out)
    b = K.build(cases[0])
    got = outs[0][b.idx]
    if epi in ("gelu", "gelu_pos", "swish"):  # (held to their bar on exact pre-activation values above)
        assert np.isfinite(got).all()
    else:
        _hold(f"128x128 rounded {dtype}", got, b.ref, _bar(b))
    for c, out in zip(cases[1:], outs[1:]):
        _same_bits(out, outs[0], f"{epi} {dtype}: the {KERNEL[c['variant']]} tile against 128 x 128")


# ------------------------------------------------------------------------------------------ LayerNorm
def _constant_rows(o, y, b, dtype, what):
    for m, t in enumerate(o.types):
        if t == "constant":
            _same_bits(y[m], R.round_dtype(b, dtype), f"{what}: a constant row gives b exactly")


@pytest.mark.parametrize("dtype", K.DT)
@pytest.mark.parametrize("d", K.LN_D)
def test_layernorm(d, dtype):
    for M in K.LN_M:
        o = K.ln_inputs(d, M)
        y = _on_device(D.layernorm, o.x, o.w, o.b, dtype)
        _hold(f"layernorm {dtype}", y, R.layernorm(o.x, o.w, o.b), R.ln_bar(o.x, o.w, o.b, dtype))
        _constant_rows(o, y, o.b, dtype, f"layernorm d={d} M={M}")


@pytest.mark.parametrize("dtype", K.DT)
@pytest.mark.parametrize("d", K.LN_D)
def test_layernorm_pend(d, dtype):
    """x + alpha (slabs + pbias), then the LayerNorm; write_x on: x comes back summed, off: bit-identical.
    ks = 3 takes the runtime-loop instance; slab_stride > M d."""
    di = K.LN_D.index(d)
    for i, M in enumerate(K.LN_M):
        for ks in (K.LN_KS[(i + di) % 5], K.LN_KS[(i + di + 2) % 5]):
            o = K.ln_inputs(d, M, ks, 8)
            v = R.pend(o.x, o.slabs, o.pbias, o.alpha)
            err = R.pend_err(o.x, o.slabs, o.pbias, o.alpha)
            ref, bar = R.layernorm(v, o.w, o.b), R.ln_bar(v, o.w, o.b, dtype, err)
            for write_x in (True, False):
                x, y = _on_device(D.layernorm_pend, o.x, o.slab_flat, ks, o.stride, o.pbias, o.alpha, o.w, o.b, dtype, write_x)
                _hold(f"layernorm_pend {dtype}", y, ref, bar)
                _constant_rows(o, y, o.b, dtype, f"layernorm_pend d={d} M={M} ks={ks}")
                if write_x:
                    _hold("layernorm_pend x", x, v, 4.0 * err)
                else:
                    _same_bits(x, o.x, "write_x off: x comes back as given")


@pytest.mark.parametrize("dtype", K.DT)
@pytest.mark.parametrize("d", [d for d in K.LN_D if d <= 1024])
def test_layernorm_pend2(d, dtype):
    """y and y2 equal, bit for bit, layernorm_pend (f32, x not written) followed by layernorm (k_norm.hip's
    claim), and both are held to the reference."""
    di = K.LN_D.index(d)
    for i, M in enumerate(K.LN_M):
        ks = (1, 2, 4, 8)[(i + di) % 4]
        o = K.ln_inputs(d, M, ks, 8)
        y, y2 = _on_device(D.layernorm_pend2, o.x, o.slab_flat, ks, o.stride, o.pbias, o.alpha, o.w, o.b, o.w2, o.b2, dtype)
        _, y_two = _on_device(D.layernorm_pend, o.x, o.slab_flat, ks, o.stride, o.pbias, o.alpha, o.w, o.b, "f32", False)
        _same_bits(y, y_two, "pend2's y against layernorm_pend")
        _same_bits(y2, _on_device(D.layernorm, y_two, o.w2, o.b2, dtype), "pend2's y2 against layernorm_pend + layernorm")
        v = R.pend(o.x, o.slabs, o.pbias, o.alpha)
        ref = R.layernorm(v, o.w, o.b)
        bar = R.ln_bar(v, o.w, o.b, "f32", R.pend_err(o.x, o.slabs, o.pbias, o.alpha))
        _hold("layernorm_pend2 y", y, ref, bar)
        _hold(f"layernorm_pend2 y2 {dtype}", y2, R.layernorm(ref, o.w2, o.b2), R.ln_bar(ref, o.w2, o.b2, dtype, bar / 4.0))


# ----------------------------------------------------------------------- the process-wide switches
CHILD_CASES = [c for c in K.GEMM_EXACT if c["variant"] == 1 and c["M"] <= 300]


def _child(path):
    """Run in a fresh process: the variant-1 exact cases through gemm_debug, their C buffers into `path`."""
    np.savez(path, **{c["id"]: _launch(K.build(c))[1] for c in CHILD_CASES})


def test_process_wide_switches(tmp_path):
    """SPT_GEMM_NT_STAGES=3 / 4 (the counted vmcnt(8) / vmcnt(16) rings) and SPT_GEMM_NT_RASTER=1 are read
    once per process: one fresh child each runs the variant-1 exact cases; the parent holds what it wrote
    to the reference and to its own default-setting bits.  The first child that does not exit 0 ends the
    test: no further one is started."""
    mine = {c["id"]: _launch(K.build(c))[1] for c in CHILD_CASES}
    code = "import sys; from tests.test_gpu_gemm import _child; _child(sys.argv[1])"
    for name, value in (("SPT_GEMM_NT_STAGES", "3"), ("SPT_GEMM_NT_STAGES", "4"), ("SPT_GEMM_NT_RASTER", "1")):
        path = str(tmp_path / f"{name}_{value}.npz")
        env = dict(os.environ, **{name: value})
        env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
        r = subprocess.run([sys.executable, "-c", code, path], env=env, cwd=ROOT, timeout=120, capture_output=True, text=True)
        assert r.returncode == 0, f"{name}={value}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}"
        theirs = np.load(path)
        for c in CHILD_CASES:
            b = K.build(c)
            out = theirs[c["id"]]
            _untouched(b, out)
            _same_bits(out[b.idx], R.store(b.ref, c["epi"], c["dtype"]), f"{c['id']} under {name}={value}")
            _same_bits(out, mine[c["id"]], f"{c['id']}: {name}={value} against the default")
        _seen[f"128x128 exact {name}={value}"] = 0.0


def test_report_largest_errors():
    """What the kernels gave, as a fraction of each bar (DESIGN.md 2e holds the table)."""
    assert _seen, "this test reports what the tests above saw"
    for name in sorted(_seen):
        print(f"{name:44s} {_seen[name]:.3f}")
    assert max(_seen.values()) <= 1.0
