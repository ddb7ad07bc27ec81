"""The decoder GEMV over a matrix resident in its packed ggml blocks (k_dec_q.hip) against the same launch
on the weights expanded at load (k_dec.hip) and against float64, the kernels alone through
spt_debug_qgemv (no engine, no model).

Per case (tests/qgemv_ref.py: the shapes at which each launch configuration exists, the decoder's (mode,
A source) pairs, both 16-bit dtypes, q5_0 and q4_1, q5_1 on one shape per pair):
  1. the two launches' outputs are the same bits, the logits' top-2 partials too;
  2. both are within the case's bar of the float64 reference (bars: qgemv_ref's docstring; none is taken
     from what the kernels give).  This is also the plain GEMV's first check against float64.
tests/test_qresident_ref.py has checked on the CPU that each named dequantisation fault moves each of
these references by at least 100 bars.  The last test prints the largest error seen per (mode, dtype) as a
fraction of its bar."""
import functools

import numpy as np
import pytest

from spittle_amd import qgemv_debug as D
from tests import qgemv_ref as Q

pytestmark = pytest.mark.gpu

_seen = {}
ALL_TYPES = dict(Q.TYPES, q5_1=Q.Q5_1)


@functools.lru_cache(maxsize=4)
def _inputs(c, t):
    return Q.make_inputs(c, t)


def _params():
    out = []
    first = set()
    for c in Q.CASES:
        for tn in ALL_TYPES:
            if tn == "q5_1":   # optional type: the first shape of each pair
                if (c.mode, c.a_src) in first:
                    continue
                first.add((c.mode, c.a_src))
            for dt in Q.DTYPES:
                out.append(pytest.param(c, tn, dt, id=f"{c.id}-{tn}-{dt}"))
    return out


@pytest.mark.parametrize("c,tname,dtype", _params())
def test_packed_is_bitwise_plain_and_both_hold_float64(c, tname, dtype):
    t = ALL_TYPES[tname]
    inp = _inputs(c, t)
    r = D.qgemv(inp.blocks, t, c.N, c.K, inp.act, mode=c.mode, a_src=c.a_src, ln_w=inp.ln_w, ln_b=inp.ln_b,
                bias=inp.bias, resid=inp.resid, ksplit=c.ksplit, dtype=dtype, want_unpacked=False)
    assert r.plain.shape == r.packed.shape
    same = np.array_equal(r.plain.view(np.uint32), r.packed.view(np.uint32))
    ref, bar = Q.reference(c, inp, t, dtype)
    assert ref.shape == r.plain.shape
    fr = {}
    for name, got in (("plain", r.plain), ("packed", r.packed)):
        g = got.astype(np.float64)
        err = np.where(np.isfinite(g), np.abs(g - ref), np.inf)
        fr[name] = float(np.max(err / np.maximum(bar, 1e-300)))   # a bar of 0: an output of exact zeros
    key = (c.mode, dtype)
    _seen[key] = max(_seen.get(key, 0.0), fr["plain"], fr["packed"])
    print(f"{c.id}-{tname}-{dtype}: bitwise {same}; largest error / bar: plain {fr['plain']:.3f}, packed {fr['packed']:.3f}")
    assert same, "the packed launch's output differs from the plain launch's"
    if c.mode == "logits":
        assert np.array_equal(r.top_plain, r.top_packed), "top-2 partials differ"
        # a partial is its tile's best logit and index: the tile of the row's best logit holds the row's argmax
        best = np.argmax(r.plain, axis=1)
        for row in range(c.R):
            tp = r.top_plain[row, best[row] // 16]
            assert int(tp[1]) == int(best[row]) and tp[0] == r.plain[row, best[row]].view(np.uint32)
    assert fr["plain"] <= 1.0, f"plain launch: {fr['plain']:.3f} of the bar"
    assert fr["packed"] <= 1.0, f"packed launch: {fr['packed']:.3f} of the bar"


def test_report_largest_errors():
    for (mode, dtype), f in sorted(_seen.items()):
        print(f"{mode:10s} {dtype}: largest error {f:.3f} of its bar")
