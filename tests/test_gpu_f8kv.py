"""SPT_MODEL_CROSS_KV_F8 in the engine: the cross K/V cache kept as fp8 e4m3 records with one
f32 scale per key row, filled from 16-bit staging layers, read by the fp8 cross-attention kernels.

The flagged context's cache reads back as the numpy quantise -> dequantise of the unflagged context's, bit
for bit, in every layer; its bytes are within 0.54 of the 16-bit cache; teacher-forced against the oracle it
holds the bars of tests/test_gpu_prefill.py's table; a row's tokens and log-probabilities are its own in
any batch; whisper_full's paths run and do not change when SPT_MODEL_QUANT_RESIDENT is added; and what the
flag refuses is refused."""
import os
import subprocess

import numpy as np
import pytest

from oracle import ggml as G
from oracle import oracle as O
from spittle_amd import _lib as L
from spittle_amd import f8kv_debug as FD
from tests import attn_ref as R
from tests import f8kv_ref as F

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SEED = 1234
FLAGS = O.SUPPRESS_BLANK | O.NO_TIMESTAMPS | O.IGNORE_EOT
N_TOK = 12
TINY_EN, LARGE22 = "synthetic:tiny.en", "synthetic:large-v3:enc=2:dec=2"
# dtype -> decision margin, top-1 bound (tests/test_gpu_prefill.py's table for this model)
BARS = {"bf16": (0.1, 0.05), "f16": (0.5, 0.25)}
AUDIO_SEED = 43


def _params(**kw):
    from spittle_amd import WhisperInferenceParams
    kw.setdefault("language", "en")
    return WhisperInferenceParams(**kw)


def _fast(**kw):
    kw.setdefault("no_timestamps", True)
    kw.setdefault("temperature_inc", 0.0)
    kw.setdefault("ignore_eot", True)
    kw.setdefault("max_new_tokens", N_TOK)
    return _params(**kw)


def _engine(spec, dtype, f8, max_batch=5, **kw):
    from spittle_amd import WhisperEngine, WhisperModelParams
    e = WhisperEngine(WhisperModelParams(dtype=dtype, max_batch=max_batch, seed=SEED, cross_kv_f8=f8, **kw))
    e.load_model(spec)
    return e


@pytest.fixture(scope="module")
def eng():
    cache = {}

    def get(spec, dtype, f8, **kw):
        key = (spec, dtype, f8, tuple(sorted(kw.items())))
        if key not in cache:
            cache[key] = _engine(spec, dtype, f8, **kw)
        return cache[key]

    yield get
    for e in cache.values():
        e.unload_model()


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float32)).view(np.uint32)


def _same(a, b, what):
    assert a.tokens == b.tokens, what
    assert np.array_equal(_bits(a.top1), _bits(b.top1)), what
    assert np.array_equal(_bits(a.top2), _bits(b.top2)), what
    assert a.text == b.text and a.language == b.language and a.n_windows == b.n_windows, what
    assert a.n_fallbacks == b.n_fallbacks, what


# ------------------------------------------------------------------------------------------ the cache
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_cache_is_the_quantised_16_bit_cache(eng, dtype):
    off, on = eng(LARGE22, dtype, False), eng(LARGE22, dtype, True)
    batch = [O.synth_audio(i) for i in range(3)]
    p = _fast(max_new_tokens=2)
    off.transcribe_batch(batch, p)
    on.transcribe_batch(batch, p)
    n_dec = on.info()["n_dec"]
    for layer in range(n_dec):
        for window in (0, 2):
            k16, v16 = FD.cross_kv(off, layer, window)
            k8, v8 = FD.cross_kv(on, layer, window)
            assert np.isfinite(k16).all() and np.abs(k16).max() > 0
            for x16, x8, what in ((k16, k8, "K"), (v16, v8, "V")):
                want = F.dequant(*F.quant_rows(x16))  # x16 is the cache's own values: no rounding left
                assert np.array_equal(_bits(want), _bits(x8)), f"{dtype} layer {layer} window {window} {what}"


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_cross_kv_info(eng, dtype):
    off, on = eng(LARGE22, dtype, False), eng(LARGE22, dtype, True)
    a, b = off.cross_kv_info(), on.cross_kv_info()
    i = on.info()
    blocks = -(-i["n_audio_ctx"] // 32) * 5 * i["n_head"]
    assert a == {"format": 0, "cache_bytes": i["n_dec"] * blocks * 8192, "staging_bytes": 0}, a
    assert b["format"] == 1 and b["cache_bytes"] == i["n_dec"] * blocks * 4352, b
    assert b["cache_bytes"] <= 0.54 * a["cache_bytes"]
    cap = max(1, -(-i["n_dec"] // 8))
    assert 0 < b["staging_bytes"] <= cap * blocks * 8192, b
    # the arena changes by exactly the cache and the staging buffer (to its 256-byte carving) ...
    saved = a["cache_bytes"] - b["cache_bytes"] - b["staging_bytes"]
    assert abs(off.info()["workspace_bytes"] - on.info()["workspace_bytes"] - saved) <= 512
    # ... which is a saving from 3 decoder layers up (0.531 n + ceil(n / 8) < n): tiny.en has 4
    t_off, t_on = eng(TINY_EN, dtype, False), eng(TINY_EN, dtype, True)
    assert t_on.cross_kv_info()["staging_bytes"] * 4 == t_off.cross_kv_info()["cache_bytes"]
    assert t_on.info()["workspace_bytes"] < t_off.info()["workspace_bytes"]


# ------------------------------------------------------------------------------------ against the oracle
def _f16(x):
    return np.ascontiguousarray(x, np.float32).astype(np.float16).astype(np.float32)


@pytest.fixture(scope="module")
def oracle_run():
    """dtype -> (tokens, top1, top2) of the oracle on AUDIO_SEED, as tests/test_gpu_prefill.py builds its models."""
    O.set_threads(16)
    out = {}

    def get(dtype):
        if dtype not in out:
            dims = O.dims_for("large-v3", 2, 2)
            if dtype == "bf16":
                om = O.Model(dims, SEED, O.W_BF16)
            else:
                om = O.Model(dims, SEED, O.W_F32)
                t = om.tensors()
                tids = {tid for tid, name, ne in G.tensor_table(dims) if len(ne) >= 2 and name not in G._F32_ALWAYS}
                for tid in sorted(tids):
                    om.set_tensor(tid, _f16(t[tid]))
            enc = om.encode(O.mel(O.synth_audio(AUDIO_SEED, 5 * 16000), dims.n_mels))
            out[dtype] = om.decode(enc, O.default_prompt(dims.n_vocab, 0), N_TOK, FLAGS)
            om.close()
        return out[dtype]

    return get


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_against_the_oracle(eng, oracle_run, dtype):
    margin, bound = BARS[dtype]
    tk, t1, t2 = oracle_run(dtype)
    gap = np.asarray(t1) - np.asarray(t2)
    k = next((i for i, g in enumerate(gap) if g < margin), len(gap))
    assert k >= 8, f"the oracle's decisions clear the margin for {k} steps only: pick another seed"
    x = O.synth_audio(AUDIO_SEED, 5 * 16000)
    for f8 in (False, True):
        r = eng(LARGE22, dtype, f8).transcribe_samples(x, _fast())
        d = np.abs(np.asarray(r.top1)[:k] - np.asarray(t1)[:k])
        print(f"large-v3 2+2 {dtype} cross_kv_f8={f8}: agreed prefix {k}, max |d top1| {d.max():.5f} (bound {bound})")
        assert (np.array(r.tokens)[:k] == np.asarray(tk)[:k]).all(), (f8, r.tokens, tk)
        assert d.max() < bound, (f8, d)


# -------------------------------------------------------------------------------------- batch invariance
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_batch_rows_are_bitwise_their_single_runs(eng, dtype):
    e = eng(LARGE22, dtype, True)
    batch = [O.synth_audio(20 + i) for i in range(5)]
    single = [e.transcribe_samples(x, _fast()) for x in batch]
    assert e.xq_stats()["fused_launches"] == 0
    for B in (4, 5):
        rs = e.transcribe_batch(batch[:B], _fast())
        assert e.xq_stats() == {"fused_launches": 0, "fallbacks": 0}
        for i, r in enumerate(rs):
            _same(r, single[i], f"utterance {i} at B = {B}")


# ----------------------------------------------------------------------- whisper_full, with and without qresident
@pytest.fixture(scope="module")
def q5(tmp_path_factory):
    """A q5_0 large-v3 file with 2 + 2 layers, written as tests/test_gpu_qresident.py writes its files, and the
    flagged contexts on it without and with SPT_MODEL_QUANT_RESIDENT."""
    tmp = tmp_path_factory.mktemp("f8kv")
    dims = O.dims_for("large-v3", 2, 2)
    base = O.Model(dims, SEED, O.W_F32)
    vocab = G.synth_vocab(O.special_tokens(dims.n_vocab)["eot"])
    path = str(tmp / "ggml-large-q5_0.bin")
    G.write_model(path, dims, O.mel_filters(dims.n_mels), vocab, base.tensors(), G.Q5_0)
    base.close()
    a, b = _engine(path, "bf16", True), _engine(path, "bf16", True, quant_resident=True)
    assert b.weight_residency()["resident_weights"] > 0 and b.cross_kv_info()["format"] == 1
    yield a, b, path
    a.unload_model()
    b.unload_model()


AUDIO_8S = 128000
FULL = {
    "defaults-with-fallback": (5, dict()),
    "beam5": (6, dict(beam_size=5, temperature_inc=0.0)),
    "auto-detect": (7, dict(language=None, temperature_inc=0.0)),
    "initial_prompt": (8, dict(initial_prompt="Technical dictation. Common terms: Kubernetes, gRPC, MI355X. " * 3,
                               temperature_inc=0.0, block_prefill=True)),
}


@pytest.mark.parametrize("name", list(FULL))
def test_whisper_full_paths_run_and_combine_with_quant_resident(q5, name):
    a, b, _ = q5
    seed, kw = FULL[name]
    x = O.synth_audio(seed, AUDIO_8S)
    ra, rb = a.transcribe_samples(x, _params(**kw)), b.transcribe_samples(x, _params(**kw))
    assert len(ra.tokens) > 0
    _same(ra, rb, name)
    assert a.xq_stats()["fused_launches"] == 0
    if name == "defaults-with-fallback":  # a fallback ran: best_of 5 decoders shared the window's records
        assert ra.n_fallbacks > 0, ra.n_fallbacks
    if name == "initial_prompt":  # SPT_BLOCK_PREFILL is ignored: the chunked passes ran
        s = a.prefill_stats()
        assert s["block_passes"] == 0 and s["block_rows"] == 0 and s["chunk_passes"] > 0, s


def test_two_decode_groups(q5):
    """40 utterances at large-v3 width, where a decoder pass carries 38 rows (tests/test_gpu_full_large.py): the
    second group reads the records from its first window on.  Equal with SPT_MODEL_QUANT_RESIDENT added, and the
    utterances of the second group (rows 38, 39) are bitwise their single runs."""
    path = q5[2]
    a, b = _engine(path, "bf16", True, max_batch=40), _engine(path, "bf16", True, max_batch=40, quant_resident=True)
    try:
        batch = [O.synth_audio(30 + i) for i in range(40)]
        p = _fast(max_new_tokens=6)
        ra, rb = a.transcribe_batch(batch, p), b.transcribe_batch(batch, p)
        assert len(ra) == 40 and all(len(r.tokens) == 6 for r in ra)
        assert a.xq_stats()["fused_launches"] == 0
        for i in range(40):
            _same(ra[i], rb[i], f"utterance {i} of 40 with quant-resident weights")
        for i in (0, 37, 38, 39):
            _same(ra[i], a.transcribe_samples(batch[i], p), f"utterance {i} of 40 against its single run")
    finally:
        a.unload_model()
        b.unload_model()


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals(eng):
    from spittle_amd import TranscriptionError, WhisperEngine, WhisperModelParams
    e = WhisperEngine(WhisperModelParams(dtype="f32", max_batch=1, seed=SEED, cross_kv_f8=True))
    with pytest.raises(TranscriptionError) as ei:
        e.load_model(TINY_EN)
    assert ei.value.status == L.SPT_ERR_UNSUPPORTED
    on = eng(TINY_EN, "bf16", True)
    x = O.synth_audio(3)
    with pytest.raises(TranscriptionError) as ei:
        on.transcribe_samples_aligned(x, _params())
    assert ei.value.status == L.SPT_ERR_UNSUPPORTED and "CROSS_KV_F8" in str(ei.value)
    # the context still works, and block_prefill reports no block pass
    past = [int(v) for v in np.random.default_rng(5).integers(0, 50000, 64)]
    r = on.transcribe_samples(x, _fast(prompt_tokens=past, block_prefill=True))
    assert len(r.tokens) == N_TOK
    s = on.prefill_stats()
    assert s["block_passes"] == 0 and s["block_rows"] == 0 and s["chunk_passes"] == 17, s
    assert on.xq_stats() == {"fused_launches": 0, "fallbacks": 0}
    assert on.cross_kv_info()["format"] == 1 and eng(TINY_EN, "bf16", False).cross_kv_info()["format"] == 0


# --------------------------------------------------------------------------------------- the C sequence
def test_c_session(tmp_path):
    exe = str(tmp_path / "f8kv_session")
    libdir = os.path.join(ROOT, "spittle_amd")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-O1", os.path.join(ROOT, "tests", "native", "f8kv_session.c"),
                    "-I", os.path.join(ROOT, "include"), "-L", libdir, "-lspittle_hip", f"-Wl,-rpath,{libdir}", "-lm",
                    "-o", exe], check=True, capture_output=True, timeout=120)
    r = subprocess.run([exe, "synthetic:tiny.en"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "f8kv_session ok" in r.stdout
