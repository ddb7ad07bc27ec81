"""GPU tests of the Parakeet encoder's int8 mode (SPT_DTYPE_I8) against the numpy
restatement of its arithmetic (tests/pk_int8_ref.py).

The integer path is exact, so it is tested to equality: the quantised input q, the zero point and
the int32 accumulators equal the reference's, the scale s_a bitwise.  The float tail
y = float(acc) * (s_a * s_w[n]) + bias is held to 2 f32 ulp (it is the reference's operations in
the reference's order), and to 1e-6 relative + 1e-7 absolute after ReLU / Swish (an exp).

  1. the three kernels alone (spt_parakeet_debug_qgemm) over odd row counts, several utterances
     with different ranges, N not a multiple of the tile, K of one and many MFMA steps, int8 and
     uint8-per-channel weights, asymmetric W (a swapped lane map cannot pass);
  2. every quantised GEMM of the real pipeline, layer 0 and 1, through a tap on its input and
     stored output (real layouts, the stacked q / k / v, linear_pos, the residual products);
  3. a model directory's stored integers are what the GEMM multiplies (int8 and uint8 per channel);
  4. a batched utterance equals the same utterance alone, bitwise;
  5. the whole encoder against the whole reference, within 1.5 x the reference's own sensitivity
     to a 1e-6 relative perturbation of each quantised layer's input (measured, not fixed);
  6. the error paths."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

from oracle import parakeet as P
from oracle.oracle import synth_audio
from tests import onnx_parakeet, pk_int8_ref as R
from tests.test_gpu_parakeet import OUT  # where the Parakeet tests keep their parity records

pytestmark = pytest.mark.gpu

SEED = 7
ACT_REL, ACT_ABS = 1e-6, 1e-7


def _engine(spec, dtype="i8", **kw):
    from spittle_amd import ParakeetEngine, ParakeetModelParams
    e = ParakeetEngine()
    kw.setdefault("max_batch", 4)
    kw.setdefault("max_seconds", 8.0)
    e.load_model_with_params(spec, ParakeetModelParams(dtype=dtype, seed=SEED, **kw))
    return e


@pytest.fixture(scope="module")
def small8():
    P.set_threads(16)
    e = _engine("synthetic:parakeet-test-small")
    d = P.dims_for("test-small")
    om = P.Model(d, seed=SEED, wdtype=P.W_F32)
    yield e, om, d
    e.unload_model()
    om.close()


@pytest.fixture(scope="module")
def mel3():
    return P.mel(synth_audio(3, 16000 * 3))


def _check_y(got, ref, act, what):
    """print each figure, then hold it to the bar"""
    if act is None:
        u = int(R.ulp_diff(got, ref).max())
        print(f"{what}: y max ulp {u}")
        assert u <= 2, (what, u)
    else:
        err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
        bar = ACT_REL * np.abs(ref.astype(np.float64)) + ACT_ABS
        print(f"{what}: y ({act}) max err / bar {float((err / bar).max()):.3f}")
        assert (err <= bar).all(), (what, float((err / bar).max()))


def _check_exact(g, r, what):
    assert np.array_equal(g["q"], r["q"]), (what, "q", int((g["q"] != r["q"]).sum()))
    assert np.array_equal(g["za"], r["za"]), (what, "za", g["za"], r["za"])
    assert np.array_equal(g["sa"].view(np.int32), r["sa"].view(np.int32)), (what, "sa", g["sa"], r["sa"])
    assert np.array_equal(g["acc"], r["acc"]), (what, "acc", int(np.abs(g["acc"].astype(np.int64) - r["acc"]).max()))


def _weights(rng, N, K, form):
    """asymmetric integer weights: (stored integers [N][K], scales, zero points)"""
    if form == "int8":
        return rng.integers(-127, 128, (N, K)).astype(np.int16), np.array([0.0123], np.float32), np.zeros(1, np.int32)
    w = rng.integers(0, 256, (N, K)).astype(np.int16)
    w[0, :] = 255  # the extremes of the uint8 range next to an extreme zero point
    w[1, :] = 0
    zp = rng.integers(0, 256, N).astype(np.int32)
    zp[0], zp[1] = 0, 255
    return w, rng.uniform(0.001, 0.02, N).astype(np.float32), zp


GROUPS = {1: [1], 13: [13], 70: [13, 38, 19]}


# ------------------------------------------------------------------ 1. the kernels, exact
@pytest.mark.parametrize("form", ["int8", "uint8pc"])
@pytest.mark.parametrize("K", [64, 192, 1024])
@pytest.mark.parametrize("N", [48, 256])
@pytest.mark.parametrize("M", [1, 13, 70])
def test_kernel_exact(M, N, K, form):
    from spittle_amd.parakeet import debug_qgemm
    rng = np.random.default_rng(1000 * M + 10 * N + K + (form == "int8"))
    a = rng.standard_normal((M, K)).astype(np.float32)
    m = 0
    for i, n in enumerate(GROUPS[M]):  # every utterance its own range and offset
        a[m:m + n] = a[m:m + n] * np.float32(1 + 4 * i) + np.float32(i * 0.7 - 0.3)
        m += n
    w, s, zp = _weights(rng, N, K, form)
    bias = rng.standard_normal(N).astype(np.float32)
    for act in (None, "relu", "swish"):
        b = None if (act is None and K == 64) else bias
        g = debug_qgemm(a, GROUPS[M], w, s, zp, b, act)
        r = R.qlinear(a, GROUPS[M], w, s, zp, b, act)
        _check_exact(g, r, (M, N, K, form, act))
        _check_y(g["y"], r["y"], act, f"kernel M{M} N{N} K{K} {form}")


def test_kernel_hand_made_rounding():
    """range 255 -> scale 1: 0.5, 1.5, 2.5 round to 0, 2, 2 (half to even); one-sided ranges give
    zero points 0 and 255; both ends saturate; K = 4096 of extreme values stays inside int32"""
    from spittle_amd.parakeet import debug_qgemm
    rng = np.random.default_rng(5)
    K, N = 64, 16
    w, s, zp = _weights(rng, N, K, "uint8pc")
    rows = np.zeros((4, K), np.float32)
    rows[0, :5] = [0.0, 0.5, 1.5, 2.5, 255.0]          # group 0: range [0, 255]
    rows[1] = np.linspace(1.0, 3.0, K)                  # group 1: all positive
    rows[2] = -np.linspace(1.0, 3.0, K)                 # group 2: all negative
    rows[3, :3] = [-1.0, 0.0, 2.0]                      # group 3: both ends
    g = debug_qgemm(rows, [1, 1, 1, 1], w, s, zp)
    r = R.qlinear(rows, [1, 1, 1, 1], w, s, zp)
    _check_exact(g, r, "hand-made")
    assert g["sa"][0] == np.float32(1) and list(g["q"][0, :5]) == [0, 0, 2, 2, 255]
    assert g["za"][1] == 0 and g["q"][1].max() == 255
    assert g["za"][2] == 255 and g["q"][2].min() == 0
    assert g["za"][3] == 85 and g["q"][3, 0] == 0 and g["q"][3, 2] == 255
    _check_y(g["y"], r["y"], None, "hand-made")
    z = debug_qgemm(np.zeros((3, K), np.float32), [3], w, s, zp)  # an all-zero input: an all-zero product
    assert not z["acc"].any() and not z["y"].any()
    K = 4096
    a = np.full((2, K), 3.0, np.float32)
    a[1] = -3.0                                         # two utterances: q - z_a = 255 and -255
    for wv, zv in ((255, 0), (0, 255)):
        w = np.full((16, K), wv, np.int16)
        g = debug_qgemm(a, [1, 1], w, np.float32(0.01), np.array([zv], np.int32))
        r = R.qlinear(a, [1, 1], w, np.float32(0.01), np.array([zv]))
        _check_exact(g, r, ("K4096", wv))
        assert abs(int(g["acc"][0, 0])) == abs(int(g["acc"][1, 0])) == 255 * 255 * K


# ------------------------------------------------------------------ 2. every GEMM of the pipeline
def _site(om, d, tid):
    """-> (stored integers [N][K] in the engine's column order, scales [N], bias or None, act, alpha)
    of the quantised GEMM named by tensor tid, weights quantised by the load rule"""
    C_, D, ff = d.sub_ch, d.d, d.ff
    F3 = d.n_mels // 8
    W = lambda t, n, k: om.tensor(t).reshape(n, k)
    if tid in (5, 9):
        ws, act, alpha, bias = [W(tid, C_, C_)], "relu", None, om.tensor(tid + 1)
    elif tid == 11:  # columns (channel, freq) -> the engine's channel-last (freq, channel)
        w = W(11, D, C_ * F3).reshape(D, C_, F3).transpose(0, 2, 1).reshape(D, F3 * C_)
        ws, act, alpha, bias = [w], None, np.float32(math.sqrt(D)), om.tensor(12)
    else:
        off = (tid - 1000) % 64
        b = tid - off
        if off in (2, 33):
            ws, act, bias = [W(tid, ff, D)], "swish", om.tensor(tid + 1)
        elif off in (4, 35):
            ws, act, bias = [W(tid, D, ff)], None, None      # residual product: the next LayerNorm adds the bias
        elif off == 8:
            ws, act = [W(b + 8 + 2 * i, D, D) for i in range(3)], None
            bias = np.concatenate([om.tensor(b + 9 + 2 * i) for i in range(3)])
        elif off in (14, 29):
            ws, act, bias = [W(tid, D, D)], None, None
        elif off == 16:
            ws, act, bias = [W(tid, D, D)], None, None       # linear_pos has no bias
        elif off == 21:
            ws, act, bias = [W(tid, 2 * D, D)], None, om.tensor(tid + 1)
        else:
            raise AssertionError(tid)
        alpha = None
    qs, ss = [], []
    for w in ws:
        q, s, _ = R.quantize_weight(w)
        qs.append(q.astype(np.int16))
        ss.append(np.full(w.shape[0], s, np.float32))
    return np.concatenate(qs), np.concatenate(ss), bias, act, alpha


def _tap(e, mel, tid):
    e.debug_tap(tid)
    e.debug_encode(mel)
    return e.debug_tap_read()


def _check_site(a, y, bias_inc, w, s, zp, bias, act, alpha, what):
    assert bias_inc == (bias is not None), what
    assert a.shape[1] == w.shape[1] and y.shape == (a.shape[0], w.shape[0]), (what, a.shape, y.shape, w.shape)
    r = R.qlinear(a, [a.shape[0]], w, s, zp, bias, act)
    ref = r["y"] if alpha is None else (r["y"] * alpha).astype(np.float32)
    assert np.abs(ref).max() > 0
    _check_y(y, ref, act, what)


SITES = [5, 9, 11] + [1000 + 64 * l + o for l in (0, 1) for o in (2, 4, 8, 14, 16, 21, 29, 33, 35)]


@pytest.mark.parametrize("tid", SITES)
def test_pipeline_gemm_exact(small8, mel3, tid):
    e, om, d = small8
    a, y, bias_inc = _tap(e, mel3, tid)
    w, s, bias, act, alpha = _site(om, d, tid)
    _check_site(a, y, bias_inc, w, s, 0, bias, act, alpha, f"site {tid}")


def test_tap_does_not_change_the_output(small8, mel3):
    e, _, _ = small8
    plain = e.debug_encode(mel3)
    e.debug_tap(1002)
    assert np.array_equal(e.debug_encode(mel3), plain)
    assert np.array_equal(e.debug_encode(mel3), plain)  # disarmed after one capture


# ------------------------------------------------------------------ 3. a model directory's integers
@pytest.mark.parametrize("quant", ["int8", "uint8pc"])
def test_model_directory_integers_as_stored(tmp_path, mel3, quant):
    d = P.dims_for("test-small")
    om = P.Model(d, seed=SEED, wdtype=P.W_F32)
    onnx_parakeet.write_dir(str(tmp_path), om, d, quant=quant)
    e = _engine(str(tmp_path))
    for tid, N, K, act, bias in ((1002, d.ff, d.d, "swish", om.tensor(1003)), (1029, d.d, d.d, None, None)):
        q, s, zp, _ = onnx_parakeet.quantize(om.tensor(tid).reshape(N, K), quant, 0)  # what the writer stored
        a, y, bias_inc = _tap(e, mel3, tid)
        _check_site(a, y, bias_inc, q.astype(np.int16), np.broadcast_to(np.atleast_1d(s), (N,)),
                    np.broadcast_to(np.atleast_1d(zp).astype(np.int64), (N,)), bias, act, None, f"{quant} dir site {tid}")
    e.unload_model()
    om.close()


# ------------------------------------------------------------------ 4. batch invariance
def test_batched_row_equals_the_utterance_alone(small8):
    from spittle_amd import ParakeetInferenceParams, TimestampGranularity
    e, _, _ = small8
    prm = ParakeetInferenceParams(timestamp_granularity=TimestampGranularity.Token)
    pcms = [synth_audio(10, 16000), synth_audio(11, 16000 * 2 + 77)]
    rb = e.transcribe_batch(pcms, prm)
    encb = [e.debug_last_encoder(b) for b in range(2)]
    for _ in range(2):  # a repeated shape is captured, then replayed, as a hipGraph: the same bits
        e.transcribe_batch(pcms, prm)
        for b in range(2):
            assert np.array_equal(e.debug_last_encoder(b), encb[b])
    for b, pcm in enumerate(pcms):
        rs = e.transcribe_samples(pcm, prm)
        enc = e.debug_last_encoder(0)
        assert enc.shape == encb[b].shape and enc.shape[0] > 0
        assert np.array_equal(enc, encb[b]), (b, float(np.abs(enc - encb[b]).max()))
        assert list(rs.tokens) == list(rb[b].tokens) and list(rs.frames) == list(rb[b].frames)
        assert np.array_equal(rs.top1, rb[b].top1)


# ------------------------------------------------------------------ 5. the whole encoder
def test_whole_encoder_within_the_reference_sensitivity(small8, mel3):
    """Dynamic quantisation amplifies differences far below f32 LayerNorm noise: a flipped rounding
    early on re-draws every later layer's quantisation noise.  So the bar is the reference's own
    sensitivity -- the largest relative RMS change of its output over 5 seeds of a 1e-6 relative
    perturbation of every quantised layer's input, on the same audio -- times 1.5 (a sample of 5).
    Measured values: pk_i8_parity.json, next to the other Parakeet parity records."""
    from spittle_amd import ParakeetInferenceParams, TimestampGranularity
    e, om, d = small8
    ref = R.encode(om, d, mel3)
    sens = max(R.rel_rms(R.encode(om, d, mel3, perturb_seed=s), ref) for s in range(5))
    gap = R.rel_rms(ref, R.encode(om, d, mel3, mode="deq"))
    got = e.debug_encode(mel3)
    assert got.shape == ref.shape
    err = R.rel_rms(got, ref)
    pcm = synth_audio(3, 16000 * 3)
    r = e.transcribe_samples(pcm, ParakeetInferenceParams(timestamp_granularity=TimestampGranularity.Token))
    t, f, _, _ = om.decode(ref)
    i, margin = P.first_disagreement(list(r.tokens), list(r.frames), list(t), list(f), om.decode_gaps(ref)[4])
    rec = {"config": "parakeet-test-small synthetic seed 7, int8 mode, 3 s", "engine_rel_rms": err,
           "engine_max_abs": float(np.abs(got - ref).max()), "reference_sensitivity_rel_rms": sens,
           "int8_vs_dequantised_rel_rms": gap, "reference_tokens": len(t), "gpu_tokens": len(r.tokens),
           "prefix_agreement": i, "margin_at_departure": None if margin == float("inf") else float(margin)}
    print(rec)
    os.makedirs(OUT, exist_ok=True)
    json.dump(rec, open(os.path.join(OUT, "pk_i8_parity.json"), "w"), indent=1)
    assert err <= 1.5 * sens, (err, sens)


# ------------------------------------------------------------------ 6. errors
def test_errors(small8):
    from spittle_amd import TranscriptionError, _lib as L
    e, _, _ = small8
    lib = L.load()
    mp = L.ModelParams()
    lib.spt_default_model_params(C.byref(mp))
    mp.dtype = L.SPT_DTYPE_I8
    ctx, err = C.c_void_p(), C.create_string_buffer(256)
    assert lib.spt_ctx_create(b"synthetic:tiny.en", C.byref(mp), C.byref(ctx), err, 256) == L.SPT_ERR_INVALID_ARG
    assert not ctx.value
    for tid in (6, 1000, 1010, 1003, 90009, 1000 + 64 * 2 + 2):  # a bias, a LayerNorm, linear_k (named by linear_q), the joint, layer 2
        with pytest.raises(TranscriptionError) as x:
            e.debug_tap(tid)
        assert x.value.status == L.SPT_ERR_INVALID_ARG, tid
    f = _engine("synthetic:parakeet-test-small", "f32")
    with pytest.raises(TranscriptionError) as x:
        f.debug_tap(1002)
    assert x.value.status == L.SPT_ERR_UNSUPPORTED
    with pytest.raises(TranscriptionError) as x:
        f.debug_tap_read()
    assert x.value.status == L.SPT_ERR_UNSUPPORTED
    f.unload_model()
    assert e.info()["dtype"] == L.SPT_DTYPE_I8
