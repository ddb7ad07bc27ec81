"""The fp8 cross K/V kernels alone (k_dec_f8.hip: kv_quant_f8, kv_dequant_f8, dec_cross_attn_f8,
dec_cross_attn_vw_f8, merged by dec_attn_part_merge) through spt_debug_attn_cross_quant, against the numpy
quantiser and the float64 reference of tests/f8kv_ref.py.

The cases are DESIGN 2c's cross cases (every T_enc of the list, both row shapes, the three window maps)
with neighbouring keys' scales 4 apart.  The device's scales and dequantised rows are the numpy
quantiser's bit for bit; the outputs and the float64-merged partials lie within bars derived from the
kernel's operation counts and the case's magnitudes (f8kv_ref.tol_of), none from a measurement; the three
launch shapes give the same bits; a row in a shared window has the bits it has alone; and the keys that
pad the last block -- which dequantise to pad_value, 32 or NaN -- change no bit.

    python -m pytest tests/test_gpu_f8kv_attn.py -m gpu -s    prints each kernel's largest error / bar"""
import numpy as np
import pytest

from spittle_amd import f8kv_debug as FD
from tests import attn_cases as K
from tests import attn_ref as R
from tests import f8kv_ref as F

pytestmark = pytest.mark.gpu

_seen = {}


def _hold(name, got, ref, tol):
    got = np.asarray(got, np.float64)
    frac = float(np.max(np.where(np.isfinite(got), np.abs(got - ref), np.inf) / tol))
    _seen[name] = max(_seen.get(name, 0.0), frac)
    print(f"{name}: largest error {frac:.3f} of its bar")
    assert frac <= 1.0, f"{name}: {frac:.3f} of the bar"


def _same_bits(a, b, what):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), what


def _run(c, dtype, **kw):
    q, k, v, _ = F.inputs(c["id"])
    args = dict(Tq=c["Tq"], b0=c["b0"], kvrow=c["kvrow"], share=c["share"], pad_value=K.PAD, dtype=dtype)
    args.update(kw)
    return FD.cross_f8(K.rows_pack(q), k, v, **args)


def _rows(part, c):
    p = np.asarray(part)
    return np.moveaxis(p.reshape((c["B"], c["Tq"]) + p.shape[1:]), 1, 2)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("c", F.CASES, ids=lambda c: c["id"])
def test_cross_attn_f8(c, dtype):
    ref, tol, _ = F.ref(c["id"], dtype)
    tol32 = tol - R.half_ulp(ref, dtype)  # partials are f32: no output rounding
    kq, vq, ks, vs, _, _ = F.quantised(c["id"], dtype)

    r = _run(c, dtype)
    # the device quantiser and the kernels' conversion: the numpy quantiser's bits
    _same_bits(r.k_scale, ks, "K scales")
    _same_bits(r.v_scale, vs, "V scales")
    _same_bits(r.kq, kq, "dequantised K")
    _same_bits(r.vq, vq, "dequantised V")
    out = r.out
    _hold(f"dec_cross_attn_f8 {dtype}", K.rows_unpack(out, c["B"], c["Tq"]), ref, tol)

    part = _run(c, dtype, mode="vw").part
    assert np.isfinite(part[..., :64]).all() and not np.isnan(part).any()
    _hold(f"dec_cross_attn_vw_f8 {dtype}", _rows(K.part_merge(part), c), ref, tol32)
    # a wave with no key block (blocks w, w + 8, ..): m = -inf, l = 0, o = 0
    nblk = -(-c["T"] // 32)
    for w in range(8):
        o, m, l = part[:, :, w, :64], part[:, :, w, 64], part[:, :, w, 65]
        if w >= nblk:
            assert np.all(m == -np.inf) and np.all(l == 0) and np.all(o == 0), w
        else:
            assert np.all(np.isfinite(m)) and np.all(l > 0), w
    merged = _run(c, dtype, mode="vw_merge").out
    _hold(f"dec_attn_part_merge (f8) {dtype}", K.rows_unpack(merged, c["B"], c["Tq"]), ref, tol)
    _same_bits(merged, out, "vw + merge against the 8-wave kernel")
    if c["Tq"] == 1:
        _same_bits(_run(c, dtype, mode="vw_pq").part, part, "per_query partials against vw's")
        _same_bits(_run(c, dtype, mode="vw_pq_merge").out, out, "per_query + merge against the 8-wave kernel")

    # the padded keys' scale (and so their dequantised value) is used nowhere
    if c["T"] % 32:
        _same_bits(_run(c, dtype, pad_value=float("nan")).out, out, "pad_value NaN against 32")
        _same_bits(_run(c, dtype, mode="vw", pad_value=float("nan")).part, part, "pad_value NaN against 32 (vw)")

    if c["share"] > 1:  # a row is bitwise the same whether alone or in a shared window
        q, k, v, _ = F.inputs(c["id"])
        qp = K.rows_pack(q)
        for b in range(0, c["B"], max(1, c["share"] // 2)):  # two rows of every window
            alone = FD.cross_f8(qp[b * c["Tq"]:(b + 1) * c["Tq"]], k, v, Tq=c["Tq"], b0=K.cross_window(c, b),
                                pad_value=K.PAD, dtype=dtype).out
            _same_bits(alone, out[b * c["Tq"]:(b + 1) * c["Tq"]], f"row {b} alone against its shared window")
    else:  # a row's bits in a batch are its bits alone
        q, k, v, _ = F.inputs(c["id"])
        qp = K.rows_pack(q)
        b = c["B"] - 1
        alone = FD.cross_f8(qp[b * c["Tq"]:(b + 1) * c["Tq"]], k, v, Tq=c["Tq"], b0=K.cross_window(c, b), pad_value=K.PAD,
                            dtype=dtype).out
        _same_bits(alone, out[b * c["Tq"]:(b + 1) * c["Tq"]], f"row {b} alone against its batch")


def test_zz_report_largest_errors():
    """Not a check of its own: prints the table DESIGN.md 2h records (run the file with -s)."""
    for name in sorted(_seen):
        print(f"{name:40s} {_seen[name]:.3f}")
    assert all(f <= 1.0 for f in _seen.values())
