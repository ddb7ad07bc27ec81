"""The Whisper attention kernels alone (enc_attention of k_attn.hip; dec_self_attn, dec_cross_attn,
dec_cross_attn_vw and dec_attn_part_merge of k_dec.hip) against the float64 reference of
tests/attn_ref.py, through the context-free hooks spt_debug_attn_* (no engine, no model).

Inputs are crafted (tests/attn_cases.py): peaked scores within 64 log2 units, a recognisable V per
key, poisoned cache rows and padded keys that would win.  tests/test_attn_ref.py has checked, on the
CPU, that each case moves by at least 100 tolerances under the fault it is built for.

Bars (none is taken from what the kernels give):
  decoder kernels, f32 encoder   4 x the linear f32 bound of attn_ref.rel_bound_f32 x max |v| over the
                                 keys the row sees (+ half an ulp of a 16-bit output at the reference)
  16-bit encoder                 3 u max |v|, u = 2^-9 (bf16) / 2^-11 (f16)
Partials are merged here in float64 and held to the f32 part of the bar.  The largest error seen per
kernel and dtype, as a fraction of its bar, is printed by the last test of the file.  Seen on an
MI355X: f32 kernels <= 0.003 (f32 encoder 0.015); 16-bit decoder outputs <= 0.954 (bf16) / 0.724 (f16),
which is the output's own rounding; 16-bit encoder 0.953 (bf16), 0.950 (bf16 SUM = 3), 0.469 (f16).
"""
import os

import numpy as np
import pytest

from spittle_amd import attn_debug as D
from tests import attn_cases as K
from tests import attn_ref as R

pytestmark = pytest.mark.gpu

_seen = {}


def _hold(name, got, ref, tol):
    """got within tol of ref everywhere (NaN fails); the largest error / tol goes into _seen[name]."""
    got = np.asarray(got, np.float64)
    frac = float(np.max(np.where(np.isfinite(got), np.abs(got - ref), np.inf) / tol))
    _seen[name] = max(_seen.get(name, 0.0), frac)
    print(f"{name}: largest error {frac:.3f} of its bar")
    assert frac <= 1.0, f"{name}: {frac:.3f} of the bar"


def _same_bits(a, b, what):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), what


# ------------------------------------------------------------------------------------------ encoder
ENC_VARIANTS = (("f32", 4), ("bf16", 4), ("bf16", 3), ("f16", 4))


@pytest.mark.parametrize("variant", ENC_VARIANTS, ids=lambda v: f"{v[0]}-sum{v[1]}")
@pytest.mark.parametrize("c", K.ENC_CASES, ids=lambda c: c["id"])
def test_enc_attention(c, variant, monkeypatch):
    dtype, sm = variant
    # the production variant: no A/B switch of the launcher left in the environment (SPT_ATTN_Q32 is
    # read once per process, so an exported one is refused rather than cleared)
    assert "SPT_ATTN_Q32" not in os.environ, "SPT_ATTN_Q32 selects another encoder kernel for the whole process"
    for name in ("SPT_ATTN_SWZ", "SPT_ATTN_QL", "SPT_ATTN_FULLDMA"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("SPT_ATTN_SUM", str(sm))  # read per launch; only the bf16 launcher branches on it
    q, k, v, _ = K.enc_inputs(c["id"])
    got = K.enc_unpack(D.enc(K.enc_pack(q, k, v), c["B"], c["T"], K.H, dtype=dtype), c["B"], c["T"])
    ref, tol, _ = K.enc_ref(c["id"], dtype, sum4=(sm == 4))
    _hold(f"enc_attention {dtype}" + (" SUM=3" if sm == 3 else ""), got, ref, tol)


# ------------------------------------------------------------------------------- decoder self-attention
@pytest.mark.parametrize("dtype", K.DT)
@pytest.mark.parametrize("c", K.SELF_CASES, ids=lambda c: c["id"])
def test_dec_self_attn(c, dtype):
    q, k, v, _ = K.self_inputs(c["id"])
    got = K.rows_unpack(D.self_attn(K.rows_pack(q), np.stack([k, v]), c["pos0"], c["Tq"], dtype=dtype), c["B"], c["Tq"])
    ref, tol, _ = K.self_ref(c["id"], dtype)
    _hold(f"dec_self_attn {dtype}", got, ref, tol)


# ------------------------------------------------------------------------------ decoder cross-attention
def _cross(c, dtype, **kw):
    q, k, v, _ = K.cross_inputs(c["id"])
    args = dict(Tq=c["Tq"], b0=c["b0"], kvrow=c["kvrow"], share=c["share"], pad_value=K.PAD, dtype=dtype)
    args.update(kw)
    return D.cross(K.rows_pack(q), k, v, **args)


def _rows(part, c):
    """[B*Tq][H][..] -> [B][H][Tq][..]."""
    p = np.asarray(part)
    return np.moveaxis(p.reshape((c["B"], c["Tq"]) + p.shape[1:]), 1, 2)


@pytest.mark.parametrize("dtype", K.DT)
@pytest.mark.parametrize("c", K.CROSS_CASES, ids=lambda c: c["id"])
def test_dec_cross_attn(c, dtype):
    ref, tol, _, _ = K.cross_ref(c["id"], dtype)
    tol32 = tol - R.half_ulp(ref, dtype)  # partials are f32: no output rounding
    out = _cross(c, dtype)
    _hold(f"dec_cross_attn {dtype}", K.rows_unpack(out, c["B"], c["Tq"]), ref, tol)

    # the one-wave-per-workgroup kernel: its 8 partials merged in float64, and by dec_attn_part_merge
    part = _cross(c, dtype, mode="vw")
    assert np.isfinite(part[..., :64]).all() and not np.isnan(part).any()
    _hold(f"dec_cross_attn_vw {dtype}", _rows(K.part_merge(part), c), ref, tol32)
    merged = _cross(c, dtype, mode="vw_merge")
    _hold(f"dec_attn_part_merge {dtype}", K.rows_unpack(merged, c["B"], c["Tq"]), ref, tol)
    _same_bits(merged, out, "vw + merge against the 8-wave kernel")
    if c["Tq"] == 1:
        _same_bits(_cross(c, dtype, mode="vw_pq"), part, "per_query partials against vw's")
        _same_bits(_cross(c, dtype, mode="vw_pq_merge"), out, "per_query + merge against the 8-wave kernel")

    if c["share"] == 1:  # key chunks: the float64 merge of the partials is their only check
        for S in (2, 3, 4):
            ps = _cross(c, dtype, splits=S)
            assert ps.shape == (c["B"] * c["Tq"], K.H, S, 66)
            _hold(f"dec_cross_attn splits {dtype}", _rows(K.part_merge(ps), c), ref, tol32)
            _, _, _, want = K.cross_ref(c["id"], dtype, None, S)
            for s, (a, e) in enumerate(K.chunk_edges(c["T"], S, K.key_block(dtype, c["Tq"]))):
                o, m, l = ps[:, :, s, :64], ps[:, :, s, 64], ps[:, :, s, 65]
                if a == e:  # an empty chunk takes no part: m = -inf, l = 0
                    assert np.all(m == -np.inf) and np.all(l == 0) and np.all(o == 0), (S, s)
                else:  # |dm| <= 12 2^-24 sum|q k| log2(e) / 8 < 1e-4 at these magnitudes
                    assert np.abs(_rows(m, c) - want[s][1]).max() < 1e-4 and np.all(l > 0), (S, s)
    else:
        # a row is bitwise the same whether alone or in a shared window
        q, k, v, _ = K.cross_inputs(c["id"])
        qp = K.rows_pack(q)
        for b in range(c["B"]):
            alone = D.cross(qp[b * c["Tq"]:(b + 1) * c["Tq"]], k, v, Tq=c["Tq"], b0=K.cross_window(c, b),
                            pad_value=K.PAD, dtype=dtype)
            _same_bits(alone, out[b * c["Tq"]:(b + 1) * c["Tq"]], f"row {b} alone against its shared window")


def test_zz_report_largest_errors():
    """Not a check of its own: prints the table DESIGN.md 2c records (run the file with -s)."""
    for name in sorted(_seen):
        print(f"{name:40s} {_seen[name]:.3f}")
    assert all(f <= 1.0 for f in _seen.values())
