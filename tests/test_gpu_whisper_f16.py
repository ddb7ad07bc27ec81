"""The Whisper engine's fp16 mode (SPT_DTYPE_F16, ABI 14) against the CPU oracle.

Reference of an f16 engine: the oracle in W_F32 mode with every tensor the engine stores in its
dtype (the matrices, the conv kernels and the token embedding: oracle.ggml.tensor_table minus
_F32_ALWAYS, as tests/test_gpu_ggml.py computes it) replaced by its np.float16-rounded value.
Reference of a bf16 engine: the oracle in W_BF16 mode, as in the existing tests.

Bars:
  * weights: the same values on both sides -> the checksum tolerances of test_weights_match_oracle;
    an f16 file's tensors are held bit for bit (rel 1e-10 on the f64 checksums).
  * encoder: relative L2 error of the f16 engine <= the bf16 engine's on the same mel (f16 carries
    three more mantissa bits at every GEMM input), and below the project's bf16 bar 3e-2.
  * decoder, teacher-forced: top-1 logit within 0.25, tokens equal wherever the reference's
    top-1 / top-2 gap exceeds 0.5, and max |d top1| <= the bf16 engine's on the same audio.
  * batching: a row's tokens, top-1 and top-2 are bitwise those of its single-utterance run (a
    4-byte stride left over 2-byte data shows here).
Measured values are printed before each assertion (DESIGN 4.3 records them).
"""
import ctypes as C

import numpy as np
import pytest

from oracle import ggml as G
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SEED = 1234
FLAGS = O.SUPPRESS_BLANK | O.NO_TIMESTAMPS | O.IGNORE_EOT
TINY_EN = "synthetic:tiny.en"
TINY = "synthetic:tiny"
LARGE22 = "synthetic:large-v3:enc=2:dec=2"
LARGE12 = "synthetic:large-v3:enc=1:dec=2"
CFG = {TINY_EN: ("tiny.en", None), TINY: ("tiny", None), LARGE22: ("large-v3", 2)}


def _lib():
    from spittle_amd import _lib as L
    return L.load()


def _f16(x):
    return np.ascontiguousarray(x, np.float32).astype(np.float16).astype(np.float32)


def _bf16(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def _engine_dtype_tids(dims):
    """tensors the engine stores in its own dtype (f16-rounded in an f16 engine)"""
    return {tid for tid, name, ne in G.tensor_table(dims) if len(ne) >= 2 and name not in G._F32_ALWAYS}


def _engine(spec, dtype, max_batch=2, seed=SEED, **kw):
    from spittle_amd import WhisperEngine, WhisperModelParams
    e = WhisperEngine(WhisperModelParams(dtype=dtype, max_batch=max_batch, seed=seed, **kw))
    e.load_model(spec)
    return e


def _params(**kw):
    from spittle_amd import WhisperInferenceParams
    kw.setdefault("language", "en")
    kw.setdefault("no_timestamps", True)  # the device-resident greedy protocol (no fallback)
    kw.setdefault("temperature_inc", 0.0)
    return WhisperInferenceParams(**kw)


@pytest.fixture(scope="module")
def eng():
    cache = {}

    def get(spec, dtype, max_batch=2):
        key = (spec, dtype, max_batch)
        if key not in cache:
            cache[key] = _engine(spec, dtype, max_batch)
        return cache[key]

    yield get
    for e in cache.values():
        e.unload_model()


@pytest.fixture(scope="module")
def ref():
    """Oracle models and their encoder outputs, computed once per (spec, dtype[, audio seed])."""
    O.set_threads(16)
    models, encs = {}, {}

    def model(spec, dtype):
        if (spec, dtype) not in models:
            cfg, nl = CFG[spec]
            dims = O.dims_for(cfg, nl, nl)
            if dtype == "bf16":
                om = O.Model(dims, SEED, O.W_BF16)
            else:
                om = O.Model(dims, SEED, O.W_F32)
                t = om.tensors()
                for tid in sorted(_engine_dtype_tids(dims)):
                    om.set_tensor(tid, _f16(t[tid]))
            models[(spec, dtype)] = om
        return models[(spec, dtype)]

    def enc(spec, dtype, audio_seed):
        key = (spec, dtype, audio_seed)
        if key not in encs:
            om = model(spec, dtype)
            encs[key] = om.encode(O.mel(O.synth_audio(audio_seed), om.dims.n_mels))
        return encs[key]

    model.enc = enc
    yield model
    for om in models.values():
        om.close()


# ---------------------------------------------------------------- 1. the dtype is real
def test_f16_is_an_engine_dtype(eng):
    from spittle_amd import _lib as L
    f, b = eng(TINY_EN, "f16"), eng(TINY_EN, "bf16")
    assert f.info()["dtype"] == L.SPT_DTYPE_F16
    assert b.info()["dtype"] == L.SPT_DTYPE_BF16
    assert f.info()["weight_bytes"] == b.info()["weight_bytes"]
    # 1280 wide: the f32 engine refuses this width, the f16 engine runs every width bf16 runs
    e = _engine(LARGE12, "f16", 1)
    try:
        assert e.info()["dtype"] == L.SPT_DTYPE_F16 and e.info()["d"] == 1280
        r = e.transcribe_samples(O.synth_audio(3, 5 * 16000), _params(ignore_eot=True, max_new_tokens=4))
        assert len(r.tokens) == 4 and np.isfinite(np.asarray(r.top1)).all()
    finally:
        e.unload_model()


def test_i8_is_still_rejected():
    from spittle_amd import _lib as L
    lib = L.load()
    mp = L.ModelParams()
    lib.spt_default_model_params(C.byref(mp))
    mp.dtype = L.SPT_DTYPE_I8
    ctx, err = C.c_void_p(), C.create_string_buffer(256)
    assert lib.spt_ctx_create(TINY_EN.encode(), C.byref(mp), C.byref(ctx), err, 256) == L.SPT_ERR_INVALID_ARG
    assert not ctx.value


# ---------------------------------------------------------------- 2. weights
def test_weights_match_f16_rounded_oracle(eng):
    e = eng(TINY_EN, "f16")
    om = O.Model(O.dims_for("tiny.en"), SEED, O.W_F32)
    t = om.tensors()
    rnd = _engine_dtype_tids(om.dims)
    for tid in (1, 2, 3, 5, 6, 7, 10, 11, 100 + 2, 100 + 4, 100 + 13, 132 + 11, 5000 + 13, 5000 + 14, 5032 + 22, 5032 + 23):
        a, s = e.weight_checksum(tid)
        w = (_f16(t[tid]) if tid in rnd else t[tid]).astype(np.float64)
        assert a == pytest.approx(np.abs(w).sum(), rel=1e-10, abs=1e-9), tid
        assert s == pytest.approx(w.sum(), rel=1e-8, abs=1e-6), tid
    om.close()


# ---------------------------------------------------------------- 3. ggml files
class ModelFile:
    """A ggml file of the oracle's tiny.en weights (2 + 2 layers) written by oracle/ggml.py; deq: the
    values the file holds; scale: tensor id -> factor applied before writing."""

    def __init__(self, tmp, wtype, scale=None):
        self.dims = O.dims_for("tiny.en", 2, 2)
        self.wtype = wtype
        base = O.Model(self.dims, SEED, O.W_F32)
        self.tensors = base.tensors()
        for tid, f in (scale or {}).items():  # powers of two: exact
            self.tensors[tid] = (self.tensors[tid] * np.float32(f)).astype(np.float32)
        sp = O.special_tokens(self.dims.n_vocab)
        self.path = str(tmp / f"ggml-tiny.en-{wtype}.bin")
        self.deq = G.write_model(self.path, self.dims, O.mel_filters(self.dims.n_mels), G.synth_vocab(sp["eot"]),
                                 self.tensors, wtype)
        base.close()

    def host_dequant(self, tid):
        """the library's host dequantiser (spt_debug_ggml_dequant) on the tensor's file bytes"""
        name, ne = next((n, s) for t, n, s in G.tensor_table(self.dims) if t == tid)
        ty, n = G.tensor_type(name, ne, self.wtype), int(np.prod(ne))
        raw = G.quantize(self.tensors[tid], ty)
        out = np.empty(n, np.float32)
        buf = C.create_string_buffer(raw, len(raw))
        assert _lib().spt_debug_ggml_dequant(ty, buf, n, out.ctypes.data_as(C.POINTER(C.c_float))) == 0
        return out


GGML_TIDS = (1, 3, 10, 100 + 2, 100 + 13, 5000 + 13, 5000 + 14, 5032 + 22)


def test_f16_file_is_held_bit_for_bit(tmp_path):
    mf = ModelFile(tmp_path, G.F16)
    e, b = _engine(mf.path, "f16"), _engine(mf.path, "bf16")
    try:
        for tid in GGML_TIDS:
            w = mf.deq[tid].astype(np.float64)  # the file's own f16 values
            assert np.array_equal(_f16(mf.deq[tid]), mf.deq[tid]), tid
            a, s = e.weight_checksum(tid)
            assert a == pytest.approx(np.abs(w).sum(), rel=1e-10, abs=1e-9), tid
            assert s == pytest.approx(w.sum(), rel=1e-10, abs=1e-6), tid
        # the check discriminates: the bf16 engine rounds the same tensor from 11 to 8 significant bits
        tid = 100 + 2
        w = mf.deq[tid].astype(np.float64)
        a_bf, _ = b.weight_checksum(tid)
        assert a_bf == pytest.approx(np.abs(_bf16(mf.deq[tid]).astype(np.float64)).sum(), rel=1e-10)
        assert abs(a_bf - np.abs(w).sum()) > 1e-7 * np.abs(w).sum()
        # f32-typed tensors of the file (biases, LayerNorm, positions) stay f32 in an f16 engine
        a, _ = e.weight_checksum(7)
        assert a == pytest.approx(np.abs(mf.deq[7].astype(np.float64)).sum(), rel=1e-10)
    finally:
        e.unload_model()
        b.unload_model()


def test_q5_0_file_rounds_once_to_f16(tmp_path):
    mf = ModelFile(tmp_path, G.Q5_0)
    e = _engine(mf.path, "f16")
    try:
        for tid in GGML_TIDS:
            h = mf.host_dequant(tid)
            assert np.array_equal(h, mf.deq[tid]), tid
            w = _f16(h).astype(np.float64)
            a, s = e.weight_checksum(tid)
            assert a == pytest.approx(np.abs(w).sum(), rel=1e-10, abs=1e-9), tid
            assert s == pytest.approx(w.sum(), rel=1e-8, abs=1e-6), tid
        r = e.transcribe_samples(O.synth_audio(3, 5 * 16000), _params(ignore_eot=True, max_new_tokens=4))
        assert len(r.tokens) == 4
    finally:
        e.unload_model()


def test_kv_cache_stores_stay_finite(tmp_path):
    """f16 overflows at 65504.  A file whose decoder value projections (self and cross, layer 0) are
    scaled until the projected values pass that bound still decodes with finite logits: the two cache
    stores clamp to +-65504, so no Inf reaches AttnWave::process, where a masked or
    low-probability key would turn it into NaN (0 x Inf).  Nothing else is clamped: the attention
    outputs are averages of cache rows, finite again."""
    V_SELF, V_CROSS = 5000 + 5, 5000 + 14
    probe = ModelFile(tmp_path, G.F16)
    scale = {}
    for tid in (V_SELF, V_CROSS):  # the largest power of two that keeps the weights themselves below 2^15
        scale[tid] = 2.0 ** np.floor(np.log2(32768.0 / np.abs(probe.tensors[tid]).max()))
    mf = ModelFile(tmp_path, G.F16, scale)
    assert all(np.abs(mf.deq[tid]).max() < 65504 for tid in scale)
    # the projection does overflow f16: the cross values of the reference encoder output
    om = O.Model(mf.dims, SEED, O.W_F32)
    x = O.synth_audio(3)
    enc = om.encode(O.mel(x, 80))
    om.close()
    v = enc.astype(np.float64) @ mf.deq[V_CROSS].reshape(mf.dims.d, mf.dims.d).astype(np.float64).T
    print(f"cross V projection: max |v| {np.abs(v).max():.3e}, {(np.abs(v) > 65504).mean():.1%} of values past 65504")
    assert (np.abs(v) > 65504).mean() > 0.05
    e = _engine(mf.path, "f16")
    try:
        r = e.transcribe_samples(x, _params(ignore_eot=True, max_new_tokens=12))
        assert len(r.tokens) == 12 and min(r.tokens) >= 0
        assert np.isfinite(np.asarray(r.top1)).all() and np.isfinite(np.asarray(r.top2)).all()
    finally:
        e.unload_model()


# ---------------------------------------------------------------- 4. encoder
@pytest.mark.parametrize("spec", [TINY_EN, LARGE22])
def test_encoder_f16_beats_bf16(eng, ref, spec):
    mel = O.mel(O.synth_audio(3), ref(spec, "f16").dims.n_mels)
    err = {}
    for dtype in ("f16", "bf16"):
        g, o = eng(spec, dtype).debug_encode(mel), ref.enc(spec, dtype, 3)
        assert np.isfinite(g).all()
        err[dtype] = float(np.linalg.norm(g - o) / np.linalg.norm(o))
    print(f"{spec} encoder rel-L2 vs own reference: e_f16 {err['f16']:.3e}  e_bf16 {err['bf16']:.3e}")
    assert err["f16"] <= err["bf16"], err
    assert err["f16"] < 3e-2, err


# ---------------------------------------------------------------- 5. decoder, teacher-forced
@pytest.mark.parametrize("spec", [TINY, LARGE22])
def test_transcribe_f16_teacher_forced(eng, ref, spec):
    n = 24
    seeds = (3, 4)
    xs = [O.synth_audio(s) for s in seeds]
    dmax = {}
    for dtype in ("f16", "bf16"):
        om = ref(spec, dtype)
        refs = [om.decode(ref.enc(spec, dtype, s), O.default_prompt(om.dims.n_vocab), n, FLAGS) for s in seeds]
        forced = np.stack([r[0] for r in refs]).astype(np.int32)
        res = eng(spec, dtype).transcribe_batch(xs, _params(ignore_eot=True, max_new_tokens=n, forced_tokens=forced))
        dmax[dtype] = 0.0
        for (tk, t1, t2), r in zip(refs, res):
            got = np.array(r.tokens)
            assert len(got) == n
            d = np.abs(np.asarray(r.top1) - t1)
            dmax[dtype] = max(dmax[dtype], float(d.max()))
            if dtype == "f16":
                assert d.max() < 0.25, d
                clear = (t1 - t2) > 0.5
                assert (got[clear] == tk[clear]).all()
    print(f"{spec} teacher-forced max |d top1|: f16 {dmax['f16']:.4f}  bf16 {dmax['bf16']:.4f}")
    assert dmax["f16"] <= dmax["bf16"], dmax


# ---------------------------------------------------------------- 6. batch invariance, bitwise
def _same_bits(a, b, what):
    assert a.tokens == b.tokens, what
    assert np.array_equal(np.asarray(a.top1), np.asarray(b.top1)), what
    assert np.array_equal(np.asarray(a.top2), np.asarray(b.top2)), what


def test_batch_invariance_bitwise(eng):
    e = eng(TINY, "f16", 4)
    xs = [O.synth_audio(20 + i, n) for i, n in enumerate([480000, 300000, 20000])]
    p = _params(ignore_eot=True, max_new_tokens=16)
    together = e.transcribe_batch(xs, p)
    for i, (x, r) in enumerate(zip(xs, together)):
        _same_bits(e.transcribe_samples(x, p), r, i)


def test_batch_past_the_row_limit_bitwise():
    """max_batch 40 at large-v3 width: a decoder pass stages at most 38 rows (gemv_max_image_rows, the
    bf16 engine's figure: the same 2-byte image), so the batch is decoded as two groups."""
    mb = 40
    e = _engine(LARGE12, "f16", mb, seed=4321)
    try:
        xs = [O.synth_audio(300 + i, 5 * 16000) for i in range(mb)]
        p = _params(ignore_eot=True, max_new_tokens=8)
        batch = e.transcribe_batch(xs, p)
        assert len(batch) == mb
        _same_bits(e.transcribe_samples(xs[mb - 1], p), batch[mb - 1], mb - 1)
    finally:
        e.unload_model()


# ---------------------------------------------------------------- 7. whisper_full path
def _monotone(r):
    t = 0.0
    for s in r.segments:
        assert t <= s.start <= s.end, [(q.start, q.end) for q in r.segments]
        t = s.end


@pytest.mark.parametrize("kw", [{}, {"beam_size": 2}], ids=["default", "beam2"])
def test_whisper_full_f16(eng, kw):
    """Timestamps + temperature fallback (finalize_ts_kernel<f16>, the sampling walk) and beam search
    (the beam candidates, kv_gather<f16>) on the f16 engine: complete, monotone, repeatable."""
    from spittle_amd import WhisperInferenceParams
    e = eng(TINY, "f16", 4)
    x = O.synth_audio(120, 15 * 16000)
    p = WhisperInferenceParams(language="en", max_new_tokens=24, **kw)
    a, b = e.transcribe_samples(x, p), e.transcribe_samples(x, p)
    assert a.n_windows >= 1 and len(a.tokens) > 0 and len(a.segments) > 0
    assert np.isfinite(np.asarray(a.top1)).all()
    _monotone(a)
    assert a.tokens == b.tokens
    assert np.array_equal(np.asarray(a.top1), np.asarray(b.top1))
    assert [(s.start, s.end) for s in a.segments] == [(s.start, s.end) for s in b.segments]


def test_autodetect_f16_large_v3_dims(eng, ref):
    """The detected language equals the reference's wherever its top-2 language-logit gap exceeds
    0.25 (the bf16 test's rule)."""
    lib = _lib()
    codes = [lib.spt_language_code(i).decode() for i in range(100)]
    e, om = eng(LARGE22, "f16"), ref(LARGE22, "f16")
    seeds = (3, 4)
    res = e.transcribe_batch([O.synth_audio(s) for s in seeds], _params(language=None, ignore_eot=True, max_new_tokens=2))
    for s, r in zip(seeds, res):
        lid, probs = om.detect_language(ref.enc(LARGE22, "f16", s))
        lp = np.sort(np.log(probs))[::-1]
        print(f"audio {s}: reference language {codes[lid]} (gap {lp[0] - lp[1]:.3f}), engine {r.language}")
        assert r.language in codes
        if lp[0] - lp[1] > 0.25:
            assert r.language == codes[lid]


# ---------------------------------------------------------------- 8. replica load
def test_f16_weights_import_replicates_engine(eng):
    import torch
    from spittle_amd import TranscriptionError
    a = eng(LARGE22, "f16")
    b = _engine(LARGE22, "f16", 2, seed=SEED + 1, external_weights=True)
    try:
        x = O.synth_audio(3)
        p = _params(max_new_tokens=6, ignore_eot=True)
        with pytest.raises(TranscriptionError, match="weights not loaded"):
            b.transcribe_samples(x, p)
        n = a.info()["weight_bytes"]
        assert b.info()["weight_bytes"] == n
        buf = torch.empty(n, dtype=torch.uint8, device="cuda:0")
        a.export_weights(buf.data_ptr(), n)
        b.import_weights(buf.data_ptr(), n)
        back = torch.empty_like(buf)
        b.export_weights(back.data_ptr(), n)
        assert torch.equal(buf, back)
        ra, rb = a.transcribe_samples(x, p), b.transcribe_samples(x, p)
        assert list(ra.tokens) == list(rb.tokens)
        np.testing.assert_array_equal(np.array(ra.top1), np.array(rb.top1))
    finally:
        b.unload_model()
