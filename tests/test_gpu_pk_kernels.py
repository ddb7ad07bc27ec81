"""The Parakeet encoder kernels of k_pk.hip alone -- rel_attn_kernel (f32, bf16, f16), rel_attn_mfma_kernel<64>
and <128>, conv_module_kernel, conv0_kernel, dwconv_kernel, relpos_kernel -- against the float64 reference of
tests/pk_ref.py; dec_kernel in its LSTM, PRED and JOINT modes with place_lstm_kernel / place_blocked_kernel;
state_init_kernel + joint_fin_kernel against its TDT state machine; and the engine's whole five-launch decode step
against its greedy loop -- through the context-free hooks spt_debug_pk_rel_attn, spt_debug_pk_conv,
spt_debug_pk_relpos, spt_debug_pk_dec_stage, spt_debug_pk_tdt and spt_debug_pk_tdt_steps (no engine, no model).

Inputs are crafted (tests/pk_cases.py); tests/test_pk_ref.py has checked, on the CPU, the reference, each
case's preconditions and its sensitivity to the faults it names.  Exact cases (the subsampling convolutions on
small integers, padded rows, guard elements) are compared at zero tolerance.  Bars of the others (DESIGN.md
9.8; none is taken from what the kernels give) are pk_ref.rel_attn_bar, conv_module_bar and relpos_bar.  The
largest error seen per kernel and dtype, as a fraction of its bar, is printed by the last test of the file;
DESIGN.md 9.8 holds the table measured on an MI355X."""
import os

import numpy as np
import pytest

from spittle_amd import _lib as L
from spittle_amd import pk_debug as D
from spittle_amd.engine import TranscriptionError
from tests import pk_cases as K
from tests import pk_ref as R

pytestmark = pytest.mark.gpu

_seen = {}


@pytest.fixture(autouse=True)
def _production_variant():
    """SPT_PK_ATTN_VALU is read once per process; the hook names its kernel, so the switch must not be needed."""
    assert "SPT_PK_ATTN_VALU" not in os.environ


def _hold(name, got, ref, tol):
    """got within tol of ref everywhere (NaN fails); the largest error / tol goes into _seen[name]."""
    got = np.asarray(got, np.float64)
    err = np.where(np.isfinite(got), np.abs(got - ref), np.inf)
    frac = float(np.max(np.where(err == 0, 0.0, err / np.maximum(tol, 1e-300))))
    _seen[name] = max(_seen.get(name, 0.0), frac)
    print(f"{name}: largest error {frac:.3f} of its bar")
    assert frac <= 1.0, f"{name}: {frac:.3f} of the bar"


def _on_device(fn, *a, **kw):
    """A device error ends the session: nothing more is launched on a GPU that has faulted."""
    try:
        return fn(*a, **kw)
    except TranscriptionError as e:
        if e.status == L.SPT_ERR_DEVICE:
            pytest.exit(f"device error, no further launches: {e.message}", returncode=3)
        raise


def _guard_untouched(y, owned):
    assert y.size > owned and np.isnan(y[owned:]).all(), "an element past the launch's own was written"


# ------------------------------------------------------------------------------------- attention
ATTN = [(c["id"], kern, dt, dk) for c in K.ATTN_CASES for kern, dt, dk in K.attn_kernels(c)]


@pytest.mark.parametrize("cid,kern,dtype,dk", ATTN)
def test_rel_attn(cid, kern, dtype, dk):
    x = K.attn_inputs(cid, dk)
    B, Tp, d = x["B"], x["Tp"], K.H * dk
    kw = {k: x[k] for k in ("B", "Tp", "H", "dk", "ldp", "p_off", "p_bstride")}
    mfma = kern == "mfma"
    r = R.rel_attn(R.round_dtype(x["qkv"], dtype), R.round_dtype(x["p"], dtype), x["pu"], x["pv"], x["lens"], mfma=mfma,
                   parts=True, **kw)
    bar = R.rel_attn_bar(r["out"], r["amax"], r["vmax"], r["nvis"], dk=dk, dtype=dtype, mfma=mfma)
    _, out = _on_device(D.rel_attn, x["qkv"], x["p"], x["pu"], x["pv"], x["lens"], dtype=dtype, variant=kern, guard=d, **kw)
    _guard_untouched(out, B * Tp * d)                      # the row past B * Tp
    got = out[:B * Tp * d].reshape(B, Tp, d)
    for b in range(B):                                     # padded rows: exact zeros
        pad = got[b, int(x["lens"][b, 3]):]
        assert (pad == 0).all() and not np.signbit(pad).any(), f"utterance {b}: a row >= T3 is not +0"
    _hold(f"rel_attn {kern}{dk if mfma else ''} {dtype}", got.reshape(B * Tp, d), r["out"], bar)


def test_rel_attn_auto_picks_the_mfma_kernel():
    """pk_rel_attn's choice (variant auto): f16 at head dim 64 / 128 is bitwise the MFMA kernel, anything else the
    VALU kernel."""
    for dk, dtype, same in ((64, "f16", "mfma"), (128, "f16", "mfma"), (72, "f16", "valu"), (64, "bf16", "valu")):
        x = K.attn_inputs("pad-T33-bd", dk)
        kw = {k: x[k] for k in ("B", "Tp", "H", "dk", "ldp", "p_off", "p_bstride")}
        run = lambda v: _on_device(D.rel_attn, x["qkv"], x["p"], x["pu"], x["pv"], x["lens"], dtype=dtype, variant=v, **kw)[1]  # noqa: E731
        assert (run("auto").view(np.uint32) == run(same).view(np.uint32)).all(), (dk, dtype)


# ----------------------------------------------------------------------------------- conv module
@pytest.mark.parametrize("dtype", K.DT)
@pytest.mark.parametrize("family", K.CM_FAMILIES)
@pytest.mark.parametrize("cid", [c["id"] for c in K.CM_CASES])
def test_conv_module(cid, family, dtype):
    x = K.cm_inputs(cid, family)
    B, Tp, d = x["B"], x["Tp"], x["d"]
    a = R.round_dtype(x["a"], dtype)
    ref, z, mag = R.conv_module(a, x["lens"], x["dw_w"], x["dw_b"], *x["bn"], Tp, parts=True)
    bar = R.conv_module_bar(a, z, mag, x["bn"], dtype)
    _, y, owned = _on_device(D.conv, "conv_module", x["a"], x["lens"], x["dw_w"], x["dw_b"], bn=x["bn"], dtype=dtype, B=B,
                             Tp=Tp, C_=d, guard=d)
    _guard_untouched(y, owned)
    got = y[:owned].reshape(B, Tp, d)
    for b in range(B):
        assert (got[b, int(x["lens"][b, 3]):] == 0).all(), f"utterance {b}: a row >= T3 is not zero"
    _hold(f"conv_module {family} {dtype}", got.reshape(B * Tp, d), ref, bar)


# ----------------------------------------------------------------------------------- subsampling
@pytest.mark.parametrize("dtype", K.DT)
@pytest.mark.parametrize("mode", K.SUB_MODES)
@pytest.mark.parametrize("cid", [c["id"] for c in K.SUB_CASES])
def test_subsampling_exact(cid, mode, dtype):
    """Small integers: zero tolerance in every dtype."""
    x = K.sub_inputs(cid, mode)
    if mode == "conv0":
        ref = R.conv0(x["x"], x["lens"], x["w"], x["bias"])
    else:
        ref = R.dwconv(x["x"], x["lens"], x["col"], x["w"], x["bias"])
    _, y, owned = _on_device(D.conv, mode, x["x"], x["lens"], x["w"], x["bias"], dtype=dtype, B=x["B"], Tp=x["Tp"], F=x["F"],
                             C_=x["C"], guard=x["C"])
    _guard_untouched(y, owned)
    assert owned == ref.size
    bad = y[:owned].reshape(ref.shape) != ref
    assert not bad.any(), f"{int(bad.sum())} of {bad.size} differ, first at {tuple(np.argwhere(bad)[0])}"


# ---------------------------------------------------------------------------------------- relpos
@pytest.mark.parametrize("dtype", K.DT)
@pytest.mark.parametrize("Tp,d", K.RELPOS_CASES)
def test_relpos(Tp, d, dtype):
    ref = R.relpos(Tp, d)
    _, pe = _on_device(D.relpos, Tp, d, dtype=dtype, guard=d)
    _guard_untouched(pe, ref.size)
    got = pe[:ref.size].reshape(ref.shape)
    assert (got[Tp - 1] == np.tile([0.0, 1.0], d // 2)).all()        # position 0: (0, 1, 0, 1, ..) exactly
    _hold(f"relpos {dtype}", got, ref, R.relpos_bar(Tp, d, ref, dtype))


# ------------------------------------------------------------------------------- TDT bookkeeping
@pytest.mark.parametrize("cid", [c["id"] for c in K.TDT_CASES])
def test_tdt_rules(cid):
    """pk_state_init and joint_fin_kernel step by step on crafted partials: every PkState field, xemb, fecur and
    the four output arrays with their guard element after every step, bit for bit."""
    x = K.tdt_inputs(cid)
    kw = {k: x[k] for k in ("V", "max_symbols", "cap", "T3p")}
    ref = R.tdt_run(x["part"], x["dur"], x["lens"], x["emb"], x["fe"], **kw)
    got = _on_device(D.tdt, x["part"], x["dur"], x["lens"], x["emb"], x["fe"], **kw)
    for s in range(ref["state"].shape[0]):
        assert (got["state"][s] == ref["state"][s]).all(), \
            f"state after step {s - 1} {R.STATE_FIELDS}: {got['state'][s].tolist()} against {ref['state'][s].tolist()}"
    for k in ("xemb", "fecur", "out_tok", "out_frame", "out_t1", "out_t2"):
        g, r = np.ascontiguousarray(got[k]).view(np.uint32), np.ascontiguousarray(ref[k]).view(np.uint32)
        bad = g != r
        assert not bad.any(), f"{k}: {int(bad.sum())} words differ, first at {tuple(np.argwhere(bad)[0])}"


# ------------------------------------------------------------------------------ the decode stages
def _bits_equal(a, b, what):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    bad = a.view(np.uint32) != b.view(np.uint32)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} differ, first at {tuple(np.argwhere(bad)[0])}"


@pytest.mark.parametrize("P,B", K.DEC_SHAPES)
def test_dec_lstm(P, B):
    """pk_place_lstm twice + the LSTM stage: rows with upd = 0 return h and c bitwise, the others within the bar."""
    x = K.lstm_inputs(P, B)
    h, c, g, mag = R.lstm_cell(x["x"], x["h"], x["c"], x["W_ih"], x["W_hh"], x["b_ih"], x["b_hh"], x["upd"], parts=True)
    bh, bc = R.lstm_bar(x["c"], g, mag)
    got = _on_device(D.dec_stage, "lstm", x["W_ih"], x["b_ih"], D.state_rows(x["upd"]), B=B, P=P, W2=x["W_hh"], b1=x["b_hh"],
                     xin=x["x"], h_in=x["h"], c_in=x["c"])
    off = x["upd"] == 0
    _bits_equal(got["h_out"][off], x["h"][off], "h of rows with upd = 0")
    _bits_equal(got["c_out"][off], x["c"][off], "c of rows with upd = 0")
    _hold("dec lstm h f32", got["h_out"][~off], h[~off], bh[~off])
    _hold("dec lstm c f32", got["c_out"][~off], c[~off], bc[~off])


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("P,B", K.DEC_SHAPES)
def test_dec_pred(P, B, exact):
    """pk_place_blocked + the prediction stage: gp of rows with upd = 0 bitwise as pre-filled; the others exact on
    integers, within (P + 2) 2^-24 (sum |x w| + |b|) on seeded inputs."""
    x = K.pred_inputs(P, B, exact)
    ref = R.pred_proj(x["x"], x["W"], x["b"], x["gp"], x["upd"])
    got = _on_device(D.dec_stage, "pred", x["W"], x["b"], D.state_rows(x["upd"]), B=B, P=P, xin=x["x"], gp=x["gp"])["gp"]
    off = x["upd"] == 0
    _bits_equal(got[off], x["gp"][off], "gp of rows with upd = 0")
    if exact:
        _bits_equal(got, ref.astype(np.float32), "gp")
    else:
        _hold("dec pred f32", got[~off], ref[~off], ((P + 2) * R.U32 * R.dot_abs(x["x"], x["W"], x["b"]))[~off])


def _check_part(part, dur, logits, V, bar=None):
    """The joint stage's partials of every row against tile_top2 of the reference logits: exact, or (bar given) the
    values within the bar and the index equal wherever the reference's lead exceeds two bars."""
    B = logits.shape[0]
    f = part.view(np.float32)
    for r in range(B):
        v1, i1, v2 = R.tile_top2(logits[r], V)
        live = np.isfinite(v1)
        assert (np.isneginf(f[r, ~live, 0]) & np.isneginf(f[r, ~live, 2])).all(), "a tile without a token"
        gi = part[r, :, 1].view(np.int32)
        if bar is None:
            assert (f[r, live, 0] == v1[live]).all() and (gi[live] == i1[live]).all() and (f[r, :, 2] == v2).all(), r
            assert (dur[r] == logits[r, V + 1:]).all(), r
        else:
            tb = np.array([bar[r, 64 * t:min(64 * t + 64, V + 1)].max() if live[t] else 0.0 for t in range(len(v1))])
            _hold("dec joint top-2 f32", np.concatenate([f[r, live, 0], f[r, live & np.isfinite(v2), 2]]),
                  np.concatenate([v1[live], v2[live & np.isfinite(v2)]]), np.concatenate([tb[live], tb[live & np.isfinite(v2)]]))
            with np.errstate(invalid="ignore"):  # a tile without a token: -inf - -inf, not sure
                sure = live & (v1 - v2 > 2 * tb)
            assert (gi[sure] == i1[sure]).all(), r
            _hold("dec joint dur f32", dur[r], logits[r, V + 1:], bar[r, V + 1:])
        assert (part[r, :, 3] == 0).all()


@pytest.mark.parametrize("kind", ["exact", "rounded"])
@pytest.mark.parametrize("P,B", K.DEC_SHAPES)
def test_dec_joint(P, B, kind):
    V = 61
    x = K.joint_inputs(P, B, V, kind)
    logits, xr = R.joint(x["fe"], x["gp"], x["W"], x["b"], V, K.N_DUR)
    got = _on_device(D.dec_stage, "joint", x["W"], x["b"], D.state_rows(np.ones(B)), B=B, P=P, fe=x["fe"], gp=x["gp"], V=V,
                     n_dur=K.N_DUR)
    bar = None if kind == "exact" else (P + 2) * R.U32 * R.dot_abs(xr, x["W"], x["b"])
    _check_part(got["part"], got["dur"], logits, V, bar)


@pytest.mark.parametrize("V", K.JOINT_V)
def test_dec_joint_vocabularies_and_bias_patterns(V):
    """N = V + 1 + n_dur at every layout of the blank and the durations over the 64-wide tiles: the exact family,
    then the logits set through the bias with W = 0; the stage's own partials go through joint_fin_kernel
    (spt_debug_pk_tdt, one step) and must give the stated token, best and runner-up."""
    P, B = 128, 9
    x = K.joint_inputs(P, B, V, "exact")
    logits, _ = R.joint(x["fe"], x["gp"], x["W"], x["b"], V, K.N_DUR)
    got = _on_device(D.dec_stage, "joint", x["W"], x["b"], D.state_rows(np.ones(B)), B=B, P=P, fe=x["fe"], gp=x["gp"], V=V,
                     n_dur=K.N_DUR)
    _check_part(got["part"], got["dur"], logits, V)
    N = V + 1 + K.N_DUR
    for pat in range(6):
        b, want = K.joint_bias_case(V, pat)
        z = np.zeros((1, P), np.float32)
        g = _on_device(D.dec_stage, "joint", np.zeros((N, P), np.float32), b, D.state_rows([1]), B=1, P=P, fe=z, gp=z + 1, V=V,
                       n_dur=K.N_DUR)
        _check_part(g["part"], g["dur"], b[None].astype(np.float64), V)
        t = _on_device(D.tdt, g["part"].view(np.float32)[None], g["dur"][None], np.array([[0, 0, 0, 4]]), np.zeros((V + 1, 8), np.float32),
                       np.zeros((4, 8), np.float32), V=V, max_symbols=10, cap=2, T3p=4)
        if want[0] == V:
            assert t["state"][1, 0, 4] == 0 and t["state"][1, 0, 2] == 0, pat            # the blank: nothing emitted
        else:
            assert (int(t["out_tok"][0, 0]), float(t["out_t1"][0, 0]), float(t["out_t2"][0, 0])) == want, pat


def test_tdt_whole_steps():
    """The engine's five launches per step, 14 steps at P = 128, B = 9, V = 61: the joint stage's own partials feed
    joint_fin_kernel.  Every decision's lead is >= 100 bars (tests/test_pk_ref.py), so the states, tokens and frames
    must be equal; the best and the runner-up logit within the joint's bar."""
    x, S = K.steps_inputs(), K.STEPS
    kw = dict(V=S["V"], n_dur=K.N_DUR, max_symbols=S["max_symbols"], cap=S["cap"], T3p=S["T3p"], n_steps=S["n_steps"])
    ref = R.tdt_steps(**x, **kw)
    got = _on_device(D.tdt_steps, **x, **kw)
    for s in range(ref["state"].shape[0]):
        assert (got["state"][s] == ref["state"][s]).all(), \
            f"state after step {s - 1} {R.STATE_FIELDS}: {got['state'][s].tolist()} against {ref['state'][s].tolist()}"
    assert (got["out_tok"] == ref["out_tok"]).all() and (got["out_frame"] == ref["out_frame"]).all()
    w = ref["out_tok"] >= 0
    assert np.isnan(got["out_t1"][~w]).all() and np.isnan(got["out_t2"][~w]).all()       # the guard and the unused slots
    _hold("tdt whole step t1, t2 f32", np.concatenate([got["out_t1"][w], got["out_t2"][w]]),
          np.concatenate([ref["out_t1"][w], ref["out_t2"][w]]), 4 * ref["bar"])


def test_zz_report():
    """The largest error of each kernel and dtype as a fraction of its bar (DESIGN.md 9.8 holds the table)."""
    for name in sorted(_seen):
        print(f"{name:40s} {_seen[name]:.3f}")
    assert _seen
