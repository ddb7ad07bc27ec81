"""Quantised decoder weights resident in HBM, the parts that need no device: the packed layout is lossless
(spt_debug_qgemv's host side against spt_debug_ggml_dequant, bit for bit, on crafted blocks), the hook
refuses bad arguments before it looks for a device, and the float64 references of
tests/test_gpu_qgemv.py's cases notice each mistake an in-register dequantisation can make."""
import ctypes as C

import numpy as np
import pytest

from oracle import ggml as G
from spittle_amd import _lib as L
from spittle_amd import qgemv_debug as D
from spittle_amd.engine import TranscriptionError
from tests import qgemv_ref as Q

# scales and minima: f16 subnormals, negatives, 2^-14, 1 and 2 (|d| <= 2: nothing overflows f16)
SPECIAL = np.array([2.0 ** -24, -(2.0 ** -24), 3 * 2.0 ** -24, 2.0 ** -14, -(2.0 ** -14), 1.0, -1.0, 2.0, -2.0],
                   np.float32)


def _crafted(t):
    """Every code value at every one of a block's 32 positions, under every (d, m) of SPECIAL."""
    nc = 32 if Q.Q5[t] else 16
    rot = (np.arange(nc)[:, None] + np.arange(32)[None, :]) % nc          # block c: code (c + j) % nc at j
    assert all(set(rot[:, j]) == set(range(nc)) for j in range(32))
    ms = SPECIAL if Q.HAS_M[t] else SPECIAL[:1]
    codes = np.tile(rot, (len(SPECIAL) * len(ms), 1))
    d = np.repeat(np.repeat(SPECIAL, len(ms)), nc)
    m = np.repeat(np.tile(ms, len(SPECIAL)), nc)
    nb = codes.shape[0]
    assert nb % 4 == 0
    return Q.make_blocks(t, codes, d, m), nb // 4, 128


def _host_dequant(raw, t, n):
    lib = L.load()
    out = np.zeros(n, np.float32)
    buf = (C.c_char * len(raw)).from_buffer_copy(raw)
    st = lib.spt_debug_ggml_dequant(t, C.cast(buf, C.c_void_p), n, out.ctypes.data_as(C.POINTER(C.c_float)))
    assert st == L.SPT_OK
    return out


def _call(raw, t, N, K, **kw):
    kw.setdefault("need_device", False)
    kw.setdefault("dtype", "bf16")
    R = kw.pop("R", 2)
    act = kw.pop("act", np.ones((R, K), np.float32))
    ln = np.ones(max(K, 1), np.float32)
    return D.qgemv(raw, t, N, K, act, ln_w=kw.pop("ln_w", ln), ln_b=kw.pop("ln_b", ln), R=R, **kw)


@pytest.mark.parametrize("t", [Q.Q5_0, Q.Q4_1, Q.Q5_1], ids=["q5_0", "q4_1", "q5_1"])
def test_packing_is_lossless(t):
    raw, N, K = _crafted(t)
    want = _host_dequant(raw, t, N * K)
    r = _call(raw, t, N, K)
    assert r.status in (L.SPT_OK, L.SPT_ERR_DEVICE)
    assert np.array_equal(r.unpacked.reshape(-1).view(np.uint32), want.view(np.uint32))
    # the test-side restatements compute the same bits (the references of the GPU cases rest on them)
    assert np.array_equal(Q.dequant(raw, t).view(np.uint32), want.view(np.uint32))
    assert np.array_equal(G.dequantize(raw, t, N * K).view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("t", [Q.Q5_0, Q.Q4_1], ids=["q5_0", "q4_1"])
def test_packing_is_lossless_on_a_case_tensor(t):
    c = Q.Case("bias", "ln", 384, 40, 5)
    inp = Q.make_inputs(c, t)
    r = _call(inp.blocks, t, c.N, c.K)
    assert np.array_equal(r.unpacked.reshape(-1).view(np.uint32), _host_dequant(inp.blocks, t, c.N * c.K).view(np.uint32))


def test_argument_errors_come_before_any_launch():
    t = Q.Q5_0
    raw = Q.make_blocks(t, np.zeros((16 * 4, 32), np.int64), np.ones(64, np.float32))
    N, K = 16, 128

    def status(**kw):
        a = dict(raw=raw, t=t, N=N, K=K)
        a.update(kw)
        try:
            return _call(a.pop("raw"), a.pop("t"), a.pop("N"), a.pop("K"), **a).status
        except TranscriptionError as e:
            return e.status

    assert status() in (L.SPT_OK, L.SPT_ERR_DEVICE)                       # the valid call
    assert status(K=112, raw=raw[:16 * 3 * 22 + 11]) == L.SPT_ERR_INVALID_ARG   # ragged K: no whole blocks
    assert status(K=96, raw=raw[:16 * 3 * 22]) == L.SPT_ERR_INVALID_ARG   # whole blocks, not a multiple of 128
    assert status(raw=raw[:-22]) == L.SPT_ERR_INVALID_ARG                 # a block short
    assert status(raw=raw + b"\0") == L.SPT_ERR_INVALID_ARG
    for bad in (G.Q5_K, G.Q8_0, G.Q4_0, G.F16, 99):
        assert status(t=bad) == L.SPT_ERR_UNSUPPORTED, bad
    assert status(dtype="f32") == L.SPT_ERR_UNSUPPORTED
    assert status(dtype=7) == L.SPT_ERR_INVALID_ARG
    assert status(raw=None) == L.SPT_ERR_INVALID_ARG                      # null buffers
    assert status(act=None) == L.SPT_ERR_INVALID_ARG
    assert status(ln_w=None) == L.SPT_ERR_INVALID_ARG
    assert status(R=0) == L.SPT_ERR_INVALID_ARG
    assert status(R=65, act=np.ones((65, K), np.float32)) == L.SPT_ERR_INVALID_ARG
    assert status(N=0) == L.SPT_ERR_INVALID_ARG
    assert status(mode="partial", a_src="ln") == L.SPT_ERR_INVALID_ARG    # not a pair of the decoder's table
    assert status(mode="bias", a_src="direct") == L.SPT_ERR_INVALID_ARG
    assert status(mode="bias_resid", a_src="direct") == L.SPT_ERR_INVALID_ARG   # no residual rows
    assert status(ksplit=2) == L.SPT_ERR_INVALID_ARG                      # K split needs partial outputs
    assert status(mode="partial", a_src="direct", ksplit=2) == L.SPT_ERR_INVALID_ARG  # above the one super-step
    assert status(mode="qkv_cache") == L.SPT_ERR_INVALID_ARG              # N = 16 is not 3 d
    assert status(device=-1) in (L.SPT_ERR_INVALID_ARG, L.SPT_ERR_DEVICE)
    # a LayerNorm source beyond its bounds: K > 1536, and an image above the LDS budget
    big = Q.make_blocks(t, np.zeros((16 * 52, 32), np.int64), np.ones(16 * 52, np.float32))
    assert status(raw=big, K=1664) == L.SPT_ERR_INVALID_ARG
    b1536 = Q.make_blocks(t, np.zeros((16 * 48, 32), np.int64), np.ones(16 * 48, np.float32))
    assert status(raw=b1536, K=1536, R=33, act=np.ones((33, 1536), np.float32)) == L.SPT_ERR_INVALID_ARG


def _case_params():
    return [pytest.param(c, tn, id=f"{c.id}-{tn}") for c in Q.CASES for tn in Q.TYPES]


@pytest.mark.parametrize("c,tname", _case_params())
def test_reference_notices_each_fault(c, tname):
    """Each named fault moves the float64 reference of each GPU case by at least 100 of the case's own
    tolerances on some output (both dtypes), so a kernel with that fault cannot pass test_gpu_qgemv."""
    t = Q.TYPES[tname]
    inp = Q.make_inputs(c, t)
    for dtype in Q.DTYPES:
        ref, bar = Q.reference(c, inp, t, dtype)
        assert np.all(np.isfinite(ref)) and np.all(bar >= 0)   # 0: an output of exact zeros
        for fault in Q.FAULTS:
            if not Q.fault_applies(t, fault):
                continue
            bad, _ = Q.reference(c, inp, t, dtype, fault)
            moved = np.max(np.abs(bad - ref) / np.maximum(bar, 1e-300))
            assert moved >= 100.0, (dtype, fault, float(moved))
