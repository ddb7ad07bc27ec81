"""SPT_MODEL_QUANT_RESIDENT in the engine: a ggml file's quantised decoder matrices stay packed in HBM and
the decoder GEMVs dequantise them in registers.  The contract is bitwise: everything a
call returns with the flag equals what the same file returns without it.

Files are written by oracle.ggml.write_model from the oracle's weights (as tests/test_gpu_ggml.py does):
large-v3 geometry 2 + 2 layers in q5_0 (bf16 engine), medium geometry 2 + 2 in q4_1 (f16 engine), tiny.en
2 + 2 in q5_0 (bf16 engine)."""
import numpy as np
import pytest

from oracle import ggml as G
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SEED = 1234
MEDIUM = O.Dims(80, 1024, 16, 2, 2, 51865, 1500, 448)
FILES = {"large-q5_0-bf16": ("large-v3", G.Q5_0, "bf16"), "medium-q4_1-f16": (MEDIUM, G.Q4_1, "f16"),
         "tiny.en-q5_0-bf16": ("tiny.en", G.Q5_0, "bf16")}
MULTILINGUAL = ("large-q5_0-bf16", "medium-q4_1-f16")
FILE_BPW = {G.Q5_0: 22 / 32, G.Q4_1: 20 / 32}   # bytes per weight in the file


def _write(tmp, cfg, wtype, tag):
    dims = O.dims_for(cfg, 2, 2) if isinstance(cfg, str) else cfg
    base = O.Model(dims, SEED, O.W_F32)
    vocab = G.synth_vocab(O.special_tokens(dims.n_vocab)["eot"])
    path = str(tmp / f"ggml-{tag}.bin")
    G.write_model(path, dims, O.mel_filters(dims.n_mels), vocab, base.tensors(), wtype)
    base.close()
    return path, dims


def _engine(path, dtype, resident, max_batch=5, external=False):
    from spittle_amd import WhisperEngine, WhisperModelParams
    e = WhisperEngine(WhisperModelParams(dtype=dtype, max_batch=max_batch, seed=SEED, quant_resident=resident,
                                         external_weights=external))
    e.load_model(path)
    return e


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    """name -> (path, dims, wtype, dtype, engine without the flag, engine with it), built on first use"""
    tmp = tmp_path_factory.mktemp("qres")
    cache = {}

    def get(name):
        if name not in cache:
            cfg, wtype, dtype = FILES[name]
            path, dims = _write(tmp, cfg, wtype, name)
            cache[name] = (path, dims, wtype, dtype, _engine(path, dtype, False), _engine(path, dtype, True))
        return cache[name]

    yield get
    for v in cache.values():
        v[4].unload_model()
        v[5].unload_model()


def _params(**kw):
    from spittle_amd import WhisperInferenceParams
    kw.setdefault("language", "en")
    return WhisperInferenceParams(**kw)


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float32)).view(np.uint32)


def _same(a, b, what):
    assert a.tokens == b.tokens, what
    assert np.array_equal(_bits(a.top1), _bits(b.top1)), what
    assert np.array_equal(_bits(a.top2), _bits(b.top2)), what
    assert a.text == b.text and a.language == b.language and a.n_windows == b.n_windows, what
    assert a.n_fallbacks == b.n_fallbacks, what
    assert [(s.start, s.end, s.text, s.i0, s.n_tokens) for s in a.segments] == \
           [(s.start, s.end, s.text, s.i0, s.n_tokens) for s in b.segments], what


AUDIO_8S = 128000


@pytest.mark.parametrize("name", list(FILES))
def test_fast_path_is_bitwise(models, name):
    _, _, _, _, off, on = models(name)
    p = _params(no_timestamps=True, temperature_inc=0.0, ignore_eot=True, max_new_tokens=16)
    a, b = off.transcribe_samples(O.synth_audio(3), p), on.transcribe_samples(O.synth_audio(3), p)
    assert len(a.tokens) == 16
    _same(a, b, "B = 1")
    batch = [O.synth_audio(i) for i in range(4)]
    for x, y in zip(off.transcribe_batch(batch, p), on.transcribe_batch(batch, p)):
        _same(x, y, "B = 4")
    if name == "large-q5_0-bf16":
        # B = 5 (100 attention workgroups) takes the fused cross-Q + cross-attention launch, whose producers
        # run the quantised fetch: it stays the production path with the flag on
        batch = [O.synth_audio(i) for i in range(5)]
        for x, y in zip(off.transcribe_batch(batch, p), on.transcribe_batch(batch, p)):
            _same(x, y, "B = 5")
        assert on.xq_stats() == off.xq_stats() and on.xq_stats()["fused_launches"] == 15 * 2, on.xq_stats()
        assert on.xq_stats()["fallbacks"] == 0


@pytest.mark.parametrize("name", list(FILES))
def test_whisper_full_defaults_are_bitwise(models, name):
    """whisper_full at its defaults on 8 s: timestamps, temperature fallback with best_of 5."""
    _, _, _, _, off, on = models(name)
    x = O.synth_audio(5, AUDIO_8S)
    _same(off.transcribe_samples(x, _params()), on.transcribe_samples(x, _params()), "whisper_full")


@pytest.mark.parametrize("name", list(FILES))
def test_beam_is_bitwise(models, name):
    _, _, _, _, off, on = models(name)
    x = O.synth_audio(6, AUDIO_8S)
    p = _params(beam_size=3, temperature_inc=0.0)
    _same(off.transcribe_samples(x, p), on.transcribe_samples(x, p), "beam 3")


@pytest.mark.parametrize("name", MULTILINGUAL)
def test_language_auto_detect_is_bitwise(models, name):
    _, _, _, _, off, on = models(name)
    x = O.synth_audio(7, AUDIO_8S)
    p = _params(language=None, temperature_inc=0.0)
    _same(off.transcribe_samples(x, p), on.transcribe_samples(x, p), "auto-detect")


@pytest.mark.parametrize("name", list(FILES))
def test_initial_prompt_is_bitwise(models, name):
    """initial_prompt: the prompt rows go through the chunked prefill passes."""
    _, _, _, _, off, on = models(name)
    x = O.synth_audio(8, AUDIO_8S)
    p = _params(initial_prompt="Technical dictation. Common terms: Kubernetes, gRPC, MI355X. " * 3, temperature_inc=0.0)
    _same(off.transcribe_samples(x, p), on.transcribe_samples(x, p), "initial_prompt")


@pytest.mark.parametrize("name", list(FILES))
def test_checksums_and_residency(models, name):
    _, dims, wtype, _, off, on = models(name)
    for tid in (10, 5002, 5007, 5011, 5016, 5020, 5022, 5013):   # 5013: the cross K projection, not resident
        a, b = off.weight_checksum(tid), on.weight_checksum(tid)
        assert b[0] == pytest.approx(a[0], rel=1e-12) and b[1] == pytest.approx(a[1], rel=1e-9, abs=1e-9), tid
    r0, r = off.weight_residency(), on.weight_residency()
    assert r0 == {"resident_weights": 0, "resident_bytes": 0, "ggml_type": -1}
    want = dims.n_dec * 14 * dims.d * dims.d + dims.n_vocab * dims.d
    assert r["resident_weights"] == want and r["ggml_type"] == wtype
    print(f"{name}: resident bytes / file bytes = {r['resident_bytes'] / (want * FILE_BPW[wtype]):.4f}; "
          f"weight_bytes {off.info()['weight_bytes']} -> {on.info()['weight_bytes']}")
    assert r["resident_bytes"] <= 1.10 * want * FILE_BPW[wtype]
    assert off.info()["weight_bytes"] - on.info()["weight_bytes"] >= want * (2 - 1.10 * FILE_BPW[wtype])


def _unsupported_type_case(tmp_path, cfg, wtype, tag):
    path, _ = _write(tmp_path, cfg, wtype, tag)
    off, on = _engine(path, "bf16", False, 2), _engine(path, "bf16", True, 2)
    assert on.weight_residency() == {"resident_weights": 0, "resident_bytes": 0, "ggml_type": -1}
    assert on.info()["weight_bytes"] == off.info()["weight_bytes"]
    p = _params(no_timestamps=True, temperature_inc=0.0, ignore_eot=True, max_new_tokens=8)
    _same(off.transcribe_samples(O.synth_audio(2), p), on.transcribe_samples(O.synth_audio(2), p), tag)
    off.unload_model()
    on.unload_model()


def test_k_quant_file_loads_with_nothing_resident(tmp_path):
    """q5_K (the catalog's breeze-asr) has no resident layout: the flag keeps nothing and changes nothing."""
    _unsupported_type_case(tmp_path, O.Dims(80, 512, 8, 2, 2, 51865, 1500, 448), G.Q5_K, "base-q5_K")


def test_f16_file_loads_with_nothing_resident(tmp_path):
    _unsupported_type_case(tmp_path, "tiny.en", G.F16, "tiny.en-f16")


def test_f32_engine_with_the_flag_is_unsupported(models):
    from spittle_amd import _lib as L
    from spittle_amd.engine import TranscriptionError
    path = models("tiny.en-q5_0-bf16")[0]
    with pytest.raises(TranscriptionError) as ei:
        _engine(path, "f32", True, 2)
    assert ei.value.status == L.SPT_ERR_UNSUPPORTED
    with pytest.raises(TranscriptionError) as ei:
        _engine("synthetic:tiny.en", "f32", True, 2)
    assert ei.value.status == L.SPT_ERR_UNSUPPORTED
    e = _engine("synthetic:tiny.en", "bf16", True, 2)   # a synthetic model: loads as without the flag
    assert e.weight_residency()["resident_weights"] == 0
    e.unload_model()


def test_export_import_between_flag_on_contexts(models):
    import torch
    from spittle_amd import _lib as L
    from spittle_amd.dist import arena_tensor
    from spittle_amd.engine import TranscriptionError
    path, _, _, dtype, off, on = models("tiny.en-q5_0-bf16")
    dst = _engine(path, dtype, True, 5, external=True)
    n = on.info()["weight_bytes"]
    assert dst.info()["weight_bytes"] == n and n < off.info()["weight_bytes"]
    buf = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    on.export_weights(buf.data_ptr(), n)
    with pytest.raises(TranscriptionError) as ei:   # a flag-off arena's size is refused
        dst.import_weights(buf.data_ptr(), off.info()["weight_bytes"])
    assert ei.value.status == L.SPT_ERR_INVALID_ARG
    dst.import_weights(buf.data_ptr(), n)
    assert torch.equal(arena_tensor(dst, "cuda:0"), arena_tensor(on, "cuda:0"))
    p = _params(no_timestamps=True, temperature_inc=0.0, ignore_eot=True, max_new_tokens=16)
    _same(on.transcribe_samples(O.synth_audio(3), p), dst.transcribe_samples(O.synth_audio(3), p), "imported arena")
    dst.unload_model()
