"""spt_debug_xq_fused: the argument errors that need no device return SPT_ERR_INVALID_ARG with a message,
before the hook looks for one."""
import ctypes as C

import numpy as np
import pytest

from spittle_amd import _lib as L

D = 1280


def _call(dtype=L.SPT_DTYPE_BF16, B=2, H=20, T=256, lds=0, touch=2, null=None):
    lib = L.load()
    fp = C.POINTER(C.c_float)
    bufs = dict(x=np.zeros((B if 0 < B <= 16 else 1, D), np.float32), ln_w=np.ones(D, np.float32),
                ln_b=np.zeros(D, np.float32), wq=np.zeros((4, D), np.float32), bias=np.zeros(D, np.float32),
                k=np.zeros(64, np.float32), v=np.zeros(64, np.float32), q=np.zeros(D, np.float32),
                out=np.zeros(D, np.float32))  # never read: every case here is refused first
    p = {n: (None if n == null else a.ctypes.data_as(fp)) for n, a in bufs.items()}
    err = C.create_string_buffer(256)
    st = lib.spt_debug_xq_fused(0, dtype, p["x"], p["ln_w"], p["ln_b"], p["wq"], p["bias"], p["k"], p["v"], 0.0, B, H, T,
                                lds, touch, p["q"], p["out"], err, 256)
    return st, err.value.decode()


@pytest.mark.parametrize("kw", [
    dict(dtype=L.SPT_DTYPE_F32), dict(H=2), dict(H=16), dict(B=0), dict(B=17), dict(T=255), dict(T=1537), dict(lds=-1),
    dict(lds=3), dict(touch=1), dict(touch=4),
    *[dict(null=n) for n in ("x", "ln_w", "ln_b", "wq", "bias", "k", "v", "q", "out")],
], ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_refused_before_any_device(kw):
    st, msg = _call(**kw)
    assert st == L.SPT_ERR_INVALID_ARG, (st, msg)
    assert msg, "no message"


def test_exported_and_declared():
    assert "spt_debug_xq_fused" in L.EXPORTS
    assert L.load().spt_debug_xq_fused.restype is C.c_int
