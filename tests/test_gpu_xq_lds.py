"""The fused cross-Q + cross-attention launch with key blocks staged in LDS by its loader wave.

Kernel alone, through spt_debug_xq_fused: for dtype in {bf16, f16}, B in {1, 5, 8} and T_enc in
  256   8 key blocks: every wave has one, both staged slots hold clamped duplicates that nobody reads;
  257   9 blocks: wave 0 has two;
  800   25 blocks: 3 or 4 per wave, the edge of "block 3 exists";
  1500  47 blocks: 6 per wave, wave 7 has 5;
  1536  the 48-block maximum,
the attention output with 1 and with 2 staged blocks per wave is bitwise the output with none, and each is
bitwise attn_debug.cross(mode="8wave") on the q the launch returned, with the same k and v
(tests/test_gpu_attn.py holds that kernel to float64).  Staging changes where a block's bytes wait, not
which blocks process() sees or in which order, so nothing but equality is acceptable.

The scores are the peaked constructions of tests/attn_cases.py (qk, values, cross_peaks): every (row, head)
peaks at one key, 8 log2 units above its neighbours in code, so a wrong block, a stale one or two blocks
swapped move the output by many ulps.  The hook takes residual rows, not q: row b is 1000 e_b, whose
LayerNorm is alpha at b and beta elsewhere, column b of Wq is the crafted q of row b over (alpha - beta),
and the bias cancels beta times the sum of the columns, so q comes out as crafted up to the dtype's rounding.

Every case runs twice back to back, the second time with other K/V (the heads reversed).  LDS often
survives between launches on a compute unit, so a ds_read that beat its DMA would tend to return the first
launch's rows.  This raises the chance of seeing such a race; it does not prove its absence.  The proof is
the ordering argument written in DESIGN 4.1j (the loader's vmcnt(0), then a barrier the readers pass).

Engine level: synthetic:large-v3:enc=2:dec=2, 16 steps, (bf16, 8), (bf16, 5), (f16, 8): tokens, top-1 and
top-2 under SPT_XQ_LDS in {1, 2} are bitwise those under SPT_XQ_LDS=0 and under SPT_XQ_FUSE=0, with the
fused launch taken once per layer of every one-token pass and no fallback.
"""
import contextlib
import functools
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests import attn_cases as AC

pytestmark = pytest.mark.gpu

H, D = 20, 1280
T_ENC = (256, 257, 800, 1500, 1536)
ROWS = (1, 5, 8)


@functools.lru_cache(maxsize=2)
def _kv(T):
    """k, v [8][H][T][64] and the crafted q [8][H*64] (rows b < B of every B share them)."""
    nbits = max(1, int(T - 1).bit_length())
    pk = AC.cross_peaks(T) + [16 * 32 + 5, 17 * 32 - 1, 24 * 32, 25 * 32 - 1, 40 * 32 + 7, T - 33]  # staged blocks' keys
    pk = [p for p in pk if 0 <= p < T]
    k, v = (np.zeros((8, H, T, 64), np.float32) for _ in range(2))
    q = np.zeros((8, H, 64), np.float32)
    n = 0
    for b in range(8):
        for h in range(H):
            _, kk = AC.qk(31000 + 100 * b + h, [0], np.arange(T), nbits, 4.0)
            k[b, h], v[b, h] = kk, AC.values(b, h, T)
            qq, _ = AC.qk(32000 + 100 * b + h, [pk[n % len(pk)]], [0], nbits, 4.0)
            qq[:, 63] = AC.GUARD
            q[b, h] = qq[0]
            n += 1
    return k, v, q.reshape(8, H * 64)


def _weights(q, B):
    """x, ln_w, ln_b, wq, bias whose LN2 + cross-Q projection is q[:B] (see the module docstring)."""
    x = np.zeros((B, D), np.float32)
    x[np.arange(B), np.arange(B)] = 1000.0
    r = x[0].astype(np.float64)
    a = (r - r.mean()) / np.sqrt(r.var() + 1e-5)
    alpha, beta = a[0], a[1]
    wq = np.zeros((D, D), np.float64)
    wq[:, :B] = q[:B].T.astype(np.float64) / (alpha - beta)
    bias = -beta * wq.sum(1)
    return x, np.ones(D, np.float32), np.zeros(D, np.float32), wq.astype(np.float32), bias.astype(np.float32)


@pytest.mark.parametrize("T", T_ENC)
@pytest.mark.parametrize("B", ROWS)
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_staged_blocks_change_no_bit(dtype, B, T):
    from spittle_amd import attn_debug as A
    k, v, q = _kv(T)
    w = _weights(q, B)
    for launch in range(2):  # back to back; the second launch's K/V: the heads reversed
        kk = np.ascontiguousarray(k[:B] if launch == 0 else k[:B, ::-1])
        vv = np.ascontiguousarray(v[:B] if launch == 0 else v[:B, ::-1])
        got = {lds: A.xq_fused(*w, kk, vv, lds=lds, touch=2, pad_value=AC.PAD, dtype=dtype) for lds in (0, 1, 2)}
        q0, out0 = got[0]
        assert np.isfinite(q0).all() and np.isfinite(out0).all(), (launch, "NaN: an output nobody wrote")
        # the crafted q arrived (each element within the dtype's rounding of three factors)
        assert np.allclose(q0, q[:B], rtol=0.03, atol=0.02), (launch, np.abs(q0 - q[:B]).max())
        ref = A.cross(q0, kk, vv, mode="8wave", pad_value=AC.PAD, dtype=dtype)
        for lds in (0, 1, 2):
            ql, outl = got[lds]
            assert np.array_equal(ql.view(np.uint32), q0.view(np.uint32)), (launch, lds, "q")
            bad = np.argwhere(outl.view(np.uint32) != ref.view(np.uint32))
            assert bad.size == 0, (launch, lds, "rows / heads differing from the 8-wave kernel",
                                   sorted({(int(r), int(c) // 64) for r, c in bad})[:8])
            assert np.array_equal(outl.view(np.uint32), out0.view(np.uint32)), (launch, lds)


def test_touch_off_changes_no_bit():
    from spittle_amd import attn_debug as A
    k, v, q = _kv(1500)
    w = _weights(q, 8)
    base = A.xq_fused(*w, k, v, lds=0, touch=2, pad_value=AC.PAD, dtype="bf16")[1]
    for lds in (0, 2):
        out = A.xq_fused(*w, k, v, lds=lds, touch=0, pad_value=AC.PAD, dtype="bf16")[1]
        assert np.array_equal(out.view(np.uint32), base.view(np.uint32)), lds


# ------------------------------------------------------------------------------------------ engine
SEED = 1234
LARGE22 = "synthetic:large-v3:enc=2:dec=2"
N_STEPS = 16


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _run(dtype, B, fuse, lds):
    from spittle_amd import WhisperEngine, WhisperInferenceParams, WhisperModelParams
    with _env(SPT_XQ_FUSE=None if fuse else "0", SPT_XQ_LDS=None if lds is None else str(lds)):
        e = WhisperEngine(WhisperModelParams(dtype=dtype, max_batch=B, seed=SEED))
        e.load_model(LARGE22)
        try:
            xs = [O.synth_audio(40 + i, 5 * 16000) for i in range(B)]
            res = e.transcribe_batch(xs, WhisperInferenceParams(language="en", no_timestamps=True, temperature_inc=0.0,
                                                               ignore_eot=True, max_new_tokens=N_STEPS))
            rows = [(list(r.tokens), np.asarray(r.top1).copy(), np.asarray(r.top2).copy()) for r in res]
            return rows, e.xq_stats(), e.call_stats()
        finally:
            e.unload_model()


@pytest.mark.parametrize("dtype,B", [("bf16", 8), ("bf16", 5), ("f16", 8)])
def test_engine_bitwise_under_every_setting(dtype, B):
    chain, xq, _ = _run(dtype, B, False, None)
    assert xq == {"fused_launches": 0, "fallbacks": 0}, xq
    assert all(len(r[0]) == N_STEPS and np.isfinite(r[1]).all() for r in chain)
    for lds in (0, 1, 2):
        rows, xq, cs = _run(dtype, B, True, lds)
        one_token_passes = cs["decoder_passes"] - cs["engine_calls"]
        assert cs["engine_calls"] == 1 and one_token_passes == N_STEPS - 1, (lds, cs)
        assert xq == {"fused_launches": one_token_passes * 2, "fallbacks": 0}, (lds, xq)  # dec=2 layers
        for i, ((tk_a, t1_a, t2_a), (tk_b, t1_b, t2_b)) in enumerate(zip(rows, chain)):
            assert tk_a == tk_b, (lds, i)
            assert np.array_equal(t1_a.view(np.uint32), t1_b.view(np.uint32)), (lds, i)
            assert np.array_equal(t2_a.view(np.uint32), t2_b.view(np.uint32)), (lds, i)
