"""The block prefill's attention kernels alone (dec_prefill_self_attn, dec_prefill_cross_attn of
k_prefill.hip) against the float64 reference of tests/attn_ref.py, through the context-free hooks
spt_debug_attn_prefill_self / _cross (no engine, no model).

Inputs are crafted (tests/prefill_cases.py): peaked scores within 64 log2 units, a recognisable V per key,
keys past a query's limit that score +100, padded keys that would win, a self cache that goes in as NaN.
tests/test_prefill_ref.py has checked, on the CPU, that each case moves by at least 100 tolerances under
the fault it is built for.

Bars (none is taken from what the kernels give):
  f32          4 x attn_ref.rel_bound_f32(chain = 66) x max |v| over the keys the row sees
  bf16 / f16   that plus 3 u max |v|, u = 2^-9 / 2^-11
The largest error seen per kernel and dtype, as a fraction of its bar, is printed by the last test."""
import numpy as np
import pytest

from spittle_amd import prefill_debug as D
from tests import attn_cases as K
from tests import attn_ref as R
from tests import prefill_cases as PC

pytestmark = pytest.mark.gpu

_seen = {}
NAN_BITS = np.uint32(0x7FC00000)  # survives the round trip through bf16 and f16 storage bit for bit


def _hold(name, got, ref, tol):
    got = np.asarray(got, np.float64)
    assert not np.isnan(got).any(), f"{name}: NaN in the output"
    frac = float(np.max(np.where(np.isfinite(got), np.abs(got - ref), np.inf) / tol))
    _seen[name] = max(_seen.get(name, 0.0), frac)
    print(f"{name}: largest error {frac:.3f} of its bar")
    assert frac <= 1.0, f"{name}: {frac:.3f} of the bar"


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _run_self(cid, dtype, only=None):
    """-> (out [B][H][P][64], cache after [2][B][H][ctx][64], cache before); only: one sequence alone."""
    c = PC.SELF_BY_ID[cid]
    q, k, v, _ = PC.self_inputs(cid)
    if only is not None:
        q, k, v = (x[only:only + 1] for x in (q, k, v))
    B, P = q.shape[0], c["P"]
    cache = np.full((2, B, PC.H, PC.CTX, 64), 0, np.uint32)
    cache[:] = NAN_BITS
    cache = cache.view(np.float32)
    with np.errstate(over="ignore"):
        out, after = D.self_attn(PC.self_pack(q, k, v), cache, P, dtype=dtype)
    return K.enc_unpack(out, B, P), after, cache


SELF_RUNS = [(c, dt) for c in PC.SELF_CASES for dt in PC.DT if dt == "f16" or not c["big"]]


@pytest.mark.parametrize("c,dtype", SELF_RUNS, ids=lambda x: x["id"] if isinstance(x, dict) else x)
def test_prefill_self_attn(c, dtype):
    P = c["P"]
    q, k, v, _ = PC.self_inputs(c["id"])
    got, after, before = _run_self(c["id"], dtype)
    # rows >= P come back bit for bit (they went in as NaN), rows < P hold the host-rounded K and V
    assert np.array_equal(_bits(after[:, :, :, P:]), _bits(before[:, :, :, P:])), "cache rows from P up were written"
    with np.errstate(over="ignore"):
        want = np.stack([PC.stored(k, dtype), PC.stored(v, dtype)])
    assert np.array_equal(_bits(after[:, :, :, :P]), _bits(want)), "cache rows below P are not the stored K and V"
    ref, tol, _ = PC.self_ref(c["id"], dtype)
    _hold(f"dec_prefill_self_attn {dtype}", got, ref, tol)


@pytest.mark.parametrize("dtype", PC.DT)
@pytest.mark.parametrize("c", PC.CROSS_CASES, ids=lambda c: c["id"])
def test_prefill_cross_attn(c, dtype):
    q, k, v, _ = PC.cross_inputs(c["id"])
    out = D.cross(K.rows_pack(q), k, v, c["P"], b0=c["b0"], kvrow=c["kvrow"], share=c["share"], pad_value=K.PAD, dtype=dtype)
    ref, tol, _ = PC.cross_ref(c["id"], dtype)
    _hold(f"dec_prefill_cross_attn {dtype}", K.rows_unpack(out, c["B"], c["P"]), ref, tol)


@pytest.mark.parametrize("dtype", PC.DT)
def test_a_sequence_alone_has_the_same_bits(dtype):
    """A sequence's rows at B = 3 are bitwise its rows at B = 1 (self and cross), and a row on a shared
    window is bitwise the row computed alone on that window."""
    got, after, _ = _run_self("P161-B3", dtype)
    for b in range(3):
        one, after1, _ = _run_self("P161-B3", dtype, only=b)
        assert np.array_equal(_bits(got[b]), _bits(one[0])), f"self b={b}"
        assert np.array_equal(_bits(after[:, b, :, :161]), _bits(after1[:, 0, :, :161])), f"self cache b={b}"
    c = PC.CROSS_BY_ID["T257-P65-B3"]
    q, k, v, _ = PC.cross_inputs(c["id"])
    full = K.rows_unpack(D.cross(K.rows_pack(q), k, v, c["P"], b0=c["b0"], pad_value=K.PAD, dtype=dtype), 3, c["P"])
    for b in range(3):
        one = D.cross(K.rows_pack(q[b:b + 1]), k, v, c["P"], b0=c["b0"] + b, pad_value=K.PAD, dtype=dtype)
        assert np.array_equal(_bits(full[b]), _bits(K.rows_unpack(one, 1, c["P"])[0])), f"cross b={b}"
    c = PC.CROSS_BY_ID["T257-P5-share5"]
    q, k, v, _ = PC.cross_inputs(c["id"])
    full = K.rows_unpack(D.cross(K.rows_pack(q), k, v, c["P"], b0=0, kvrow=c["kvrow"], share=5, pad_value=K.PAD, dtype=dtype),
                         c["B"], c["P"])
    for b in (0, 4, 5, 9):
        one = D.cross(K.rows_pack(q[b:b + 1]), k, v, c["P"], b0=PC.cross_window(c, b), pad_value=K.PAD, dtype=dtype)
        assert np.array_equal(_bits(full[b]), _bits(K.rows_unpack(one, 1, c["P"])[0])), f"shared window b={b}"


def test_zz_report_largest_errors():
    for name in sorted(_seen):
        print(f"SEEN {name}: {_seen[name]:.3f} of its bar")
    assert _seen, "no kernel test ran before the report"
