"""CPU-only checks of the SenseVoice boundary: header / ctypes / Rust agreement, struct layouts against
gcc, defaults, the version words, the error paths that need no device, the pure-Python checkpoint
readers with a synthetic FunASR directory, and sv_host.h under AddressSanitizer + UBSan as a
stand-alone program (tests/native/sv_fuzz.cpp)."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from spittle_amd import _lib as L
from spittle_amd import sensevoice as S
from tests import sensevoice_torch as ST

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HEADER = os.path.join(ROOT, "include", "spittle_hip.h")
SV_FUNCS = ["spt_sensevoice_default_model_params", "spt_sensevoice_default_infer_params", "spt_sensevoice_create",
            "spt_sensevoice_destroy", "spt_sensevoice_last_error", "spt_sensevoice_info", "spt_sensevoice_tensor_numel",
            "spt_sensevoice_set_tensor", "spt_sensevoice_missing_tensors", "spt_sensevoice_set_cmvn",
            "spt_sensevoice_set_vocab", "spt_sensevoice_n_rows", "spt_sensevoice_transcribe",
            "spt_sensevoice_transcribe_batch", "spt_sensevoice_result_free", "spt_sensevoice_get_timings",
            "spt_sensevoice_debug_features", "spt_sensevoice_debug_encode", "spt_sensevoice_debug_frames"]
STRUCTS = {"spt_sv_model_params": L.SvModelParams, "spt_sv_infer_params": L.SvInferParams, "spt_sv_result": L.SvResult,
           "spt_sv_model_info": L.SvModelInfo, "spt_sv_timings": L.SvTimings}


def test_header_binding_and_rust_agree():
    hdr = open(HEADER).read()
    declared = set(re.findall(r"\b(spt_sensevoice_[a-z_]+)\s*\(", hdr))
    assert declared == set(SV_FUNCS)
    assert declared <= set(L.EXPORTS)
    lib = L.load()
    for f in SV_FUNCS:
        assert hasattr(lib, f), f
    rs = open(os.path.join(ROOT, "rust", "spittle-hip-sys", "src", "lib.rs")).read()
    assert set(re.findall(r"\bpub fn (spt_sensevoice_[a-z_]+)\s*\(", rs)) == declared
    for s in list(STRUCTS) + ["spt_sv_ctx"]:
        assert re.search(r"\bpub struct %s\b" % s, rs), s
        assert re.search(r"\b%s\b" % s, hdr), s
    # field names and order of every struct, header against Rust against ctypes
    for s, py in STRUCTS.items():
        body = re.search(r"pub struct %s \{(.*?)\n\}" % s, rs, re.S).group(1)
        assert re.findall(r"pub (\w+):", body) == [f[0] for f in py._fields_], s
    wrap = open(os.path.join(ROOT, "rust", "spittle-hip", "src", "lib.rs")).read()
    for name in ("pub struct HipSenseVoiceEngine", "pub enum HipSenseVoiceLanguage", "pub struct HipSenseVoiceInferenceParams",
                 "pub fn int8()", "pub fn from_code", "spt_sensevoice_transcribe", "spt_sensevoice_set_cmvn"):
        assert name in wrap, name
    for k, name in enumerate(("AUTO", "ZH", "EN", "YUE", "JA", "KO")):
        assert re.search(r"SPT_SV_LANG_%s = %d\b" % (name, k), hdr)
        assert "SPT_SV_LANG_%s: i32 = %d;" % (name, k) in rs
        assert getattr(L, "SPT_SV_LANG_" + name) == k


def test_abi_version_unchanged_and_version_words():
    hdr = open(HEADER).read()
    assert re.search(r"#define\s+SPT_ABI_VERSION\s+14\b", hdr)
    assert re.search(r"#define\s+SPT_HAS_SENSEVOICE\s+1\b", hdr)
    rs = open(os.path.join(ROOT, "rust", "spittle-hip-sys", "src", "lib.rs")).read()
    assert "SPT_ABI_VERSION: c_int = 14" in rs and "SPT_HAS_SENSEVOICE" in rs
    v = L.load().spt_version().decode()
    for word in ("ABI 14", "ABI 12", "moonshine", "sensevoice", "gfx950"):
        assert word in v, (word, v)


def test_struct_layouts_match_header(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void) {",
             "spt_sv_ctx* opaque = 0; (void)opaque;"]
    for cname, py in STRUCTS.items():
        lines.append(f'printf("{cname} size %zu\\n", sizeof({cname}));')
        for f in py._fields_:
            lines.append(f'printf("{cname} {f[0]} %zu\\n", offsetof({cname}, {f[0]}));')
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", str(src), "-o", str(exe)], check=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    seen = 0
    for line in filter(None, got):
        cname, field, val = line.split()
        py = STRUCTS[cname]
        want = C.sizeof(py) if field == "size" else getattr(py, field).offset
        assert int(val) == want, (cname, field, val, want)
        seen += 1
    assert seen == sum(len(s._fields_) + 1 for s in STRUCTS.values())
    bad = tmp_path / "bad.c"
    bad.write_text(f'#include "{HEADER}"\nint main(void) {{ return (int)sizeof(spt_sv_ctx); }}\n')
    assert subprocess.run(["gcc", str(bad), "-o", str(tmp_path / "bad")], capture_output=True).returncode != 0


def test_defaults():
    lib = L.load()
    mp = L.SvModelParams()
    lib.spt_sensevoice_default_model_params(C.byref(mp))
    assert (mp.dtype, mp.device, mp.max_batch, mp.max_samples, mp.seed) == (L.SPT_DTYPE_F16, 0, 8, 64 * 16000, 1234)
    assert mp.ln_eps == np.float32(1e-5) and (mp.sanm_shift, mp.lfr_m, mp.lfr_n, mp.blank_id, mp.n_prefix) == (0, 7, 6, 0, 4)
    assert list(mp.lang_rows) == [0, 3, 4, 7, 11, 12]
    assert (mp.event_row, mp.emo_row, mp.itn_row, mp.no_itn_row) == (1, 2, 14, 15)
    ip = L.SvInferParams(9, 9)
    lib.spt_sensevoice_default_infer_params(C.byref(ip))
    assert (ip.language, ip.use_itn) == (L.SPT_SV_LANG_AUTO, 0)
    p = S.SenseVoiceModelParams.int8()
    assert p.dtype == "f16" and p.lang_rows == tuple(ST.LANG_ROWS) and (p.lfr_m, p.lfr_n) == (7, 6)
    assert S.SenseVoiceInferenceParams().language is S.Language.Auto and not S.SenseVoiceInferenceParams().use_itn
    assert [m.value for m in (S.Language.Auto, S.Language.Chinese, S.Language.English, S.Language.Cantonese,
                              S.Language.Japanese, S.Language.Korean)] == list(range(6))
    for code, lang in (("zh", S.Language.Chinese), ("zh-Hans", S.Language.Chinese), ("zh-Hant", S.Language.Chinese),
                       ("en", S.Language.English), ("ja", S.Language.Japanese), ("ko", S.Language.Korean),
                       ("yue", S.Language.Cantonese), ("fr", S.Language.Auto), ("auto", S.Language.Auto)):
        assert S.Language.from_code(code) is lang
    e = S.SenseVoiceEngine()
    assert not e.is_loaded()
    with pytest.raises(S.TranscriptionError, match="not loaded"):
        e.transcribe_samples([0.0] * 1000, None)
    assert lib.spt_sensevoice_missing_tensors(None) == -1 and lib.spt_sensevoice_n_rows(None, 16000) == 0
    assert lib.spt_sensevoice_last_error(None) == b"null context"


def _create(spec, dtype=L.SPT_DTYPE_F16, **over):
    lib = L.load()
    mp = L.SvModelParams()
    lib.spt_sensevoice_default_model_params(C.byref(mp))
    mp.dtype = dtype
    for k, v in over.items():
        setattr(mp, k, v)
    ctx = C.c_void_p()
    err = C.create_string_buffer(256)
    st = lib.spt_sensevoice_create(spec, C.byref(mp), C.byref(ctx), err, 256)
    if ctx.value:
        lib.spt_sensevoice_destroy(ctx)
    return st, err.value.decode()


def test_errors_before_any_device_work():
    import torch
    for bad, msg in ((b"synthetic:sensevoice-huge", "unknown sensevoice model"), (b"sensevoice-small", "synthetic: or empty:"),
                     (b"synthetic:sensevoice-small:layers=3", "bad model spec option"),
                     (b"synthetic:sensevoice-small:depth=3", "bad model spec option"),
                     (b"empty:sensevoice-test-small:vocab=abc", "bad model spec option"),
                     (b"synthetic:moonshine-base", "unknown sensevoice model"), (b"synthetic:", "unknown sensevoice model")):
        st, err = _create(bad)
        assert st == L.SPT_ERR_LOAD and msg in err, (bad, st, err)
    assert _create(None)[0] == L.SPT_ERR_INVALID_ARG
    for dt in (L.SPT_DTYPE_F32, L.SPT_DTYPE_BF16, L.SPT_DTYPE_I8):
        st, err = _create(b"synthetic:sensevoice-small", dt)
        assert st == L.SPT_ERR_UNSUPPORTED and "SPT_DTYPE_F16" in err
    for over, msg in (({"max_batch": 0}, "max_batch"), ({"max_samples": 399}, "max_samples"), ({"max_samples": 4800001}, "max_samples"),
                      ({"lfr_m": 0}, "lfr_m"), ({"lfr_n": 17}, "lfr_m and lfr_n"), ({"sanm_shift": 6}, "sanm_shift"),
                      ({"blank_id": 25055}, "blank"), ({"n_prefix": 5}, "n_prefix"), ({"ln_eps": 0.0}, "ln_eps"),
                      ({"itn_row": 16}, "query row"), ({"emo_row": -1}, "query row")):
        st, err = _create(b"synthetic:sensevoice-small", **over)
        assert st == L.SPT_ERR_INVALID_ARG and msg in err, (over, st, err)
    if not torch.cuda.is_available():
        # every well-formed spec passes the grammar and then stops at the missing device
        for good in (b"synthetic:sensevoice-small", b"synthetic:sensevoice-test-small:seed=9", b"empty:sensevoice-test-small",
                     b"empty:sensevoice-small:layers=2,1:vocab=1024:seed=3"):
            st, err = _create(good)
            assert st == L.SPT_ERR_DEVICE, (good, st, err)


def test_am_mvn_and_token_readers(tmp_path):
    neg_mean, inv_std = ST.make_cmvn(ST.TEST_SMALL)
    fmt = lambda v: " ".join(repr(float(x)) for x in v)  # noqa: E731
    mvn = tmp_path / "am.mvn"
    mvn.write_text("<Nnet>\n<Splice> 560 560\n[ 0 ]\n<AddShift> 560 560\n<LearnRateCoef> 0 [ " + fmt(neg_mean) +
                   " ]\n<Rescale> 560 560\n<LearnRateCoef> 0 [ " + fmt(inv_std) + " ]\n</Nnet>\n")
    a, b = S.read_am_mvn(str(mvn))
    assert a.dtype == np.float32 and np.array_equal(a, neg_mean) and np.array_equal(b, inv_std)
    mvn.write_text("<Nnet>\n<AddShift> 2 2\n[ 1 2 ]\n</Nnet>\n")
    with pytest.raises(ValueError, match="<Rescale>"):
        S.read_am_mvn(str(mvn))
    mvn.write_text("<AddShift> [ 1 2 3 ]\n<Rescale> [ 1 2 ]\n")
    with pytest.raises(ValueError, match="3 values"):
        S.read_am_mvn(str(mvn))
    mvn.write_text("<AddShift> [ 1 x ]\n<Rescale> [ 1 2 ]\n")
    with pytest.raises(ValueError, match="not numeric"):
        S.read_am_mvn(str(mvn))
    # a SentencePiece ModelProto: field 1 = SentencePiece { 1: piece, 2: score (float), 3: type }
    pieces = ["<unk>", "<s>", "</s>", "▁hello", "<0xE6>", "<|en|>"]
    blob = b""
    for i, p in enumerate(pieces):
        raw = p.encode("utf-8")
        inner = b"\x0a" + bytes([len(raw)]) + raw + b"\x15" + struct.pack("<f", -float(i)) + b"\x18\x01"
        blob += b"\x0a" + bytes([len(inner)]) + inner
    blob += b"\x12\x04\x0a\x02hi"   # a trainer_spec-like field 2 that the reader skips
    sp = tmp_path / "spm.model"
    sp.write_bytes(blob)
    assert S.read_sentencepiece_pieces(str(sp)) == pieces
    sp.write_bytes(blob[:-3] + b"\xff\xff\xff\xff\xff\xff\xff\xff\xff\xff\xff\xff")
    with pytest.raises(ValueError, match="not a SentencePiece model"):
        S.read_sentencepiece_pieces(str(sp))
    tk = tmp_path / "tokens.txt"
    tk.write_text("<unk> 0\n<s> 1\n▁a b 3\n", encoding="utf-8")
    assert S.read_tokens_txt(str(tk)) == ["<unk>", "<s>", "", "▁a b"]
    tk.write_text("<unk>\n<s>\n▁x\n", encoding="utf-8")
    assert S.read_tokens_txt(str(tk)) == ["<unk>", "<s>", "▁x"]


def _write_checkpoint_dir(path, D, weights):
    import torch
    torch.save({k: torch.from_numpy(v) for k, v in weights.items()}, os.path.join(path, "model.pt"))
    neg_mean, inv_std = ST.make_cmvn(D)
    fmt = lambda v: " ".join(repr(float(x)) for x in v)  # noqa: E731
    with open(os.path.join(path, "am.mvn"), "w") as f:
        f.write("<Nnet>\n<AddShift> 560 560\n<LearnRateCoef> 0 [ " + fmt(neg_mean) + " ]\n<Rescale> 560 560\n"
                "<LearnRateCoef> 0 [ " + fmt(inv_std) + " ]\n</Nnet>\n")
    with open(os.path.join(path, "tokens.txt"), "w", encoding="utf-8") as f:
        f.write("\n".join(f"▁p{i}" for i in range(D.vocab)) + "\n")


def test_checkpoint_dir_round_trip(tmp_path):
    """a synthetic FunASR directory through load_checkpoint_dir: the geometry, layer counts and vocabulary
    are read off the tensors; without a device the load stops at engine creation with SPT_ERR_DEVICE,
    after every host-side reader has run; with one, the tensors all land and a call transcribes"""
    import torch
    D = ST.TEST_SMALL
    w = ST.make_weights(D)
    w["extra.not_in_the_engine"] = np.zeros(3, np.float32)   # ignored, as FunASR's non-encoder tensors would be
    _write_checkpoint_dir(str(tmp_path), D, w)
    seen = {}
    e = S.SenseVoiceEngine()
    real_create = e._create

    def spy(spec, params):
        seen["spec"] = spec
        return real_create(spec, params)

    e._create = spy
    if torch.cuda.is_available():
        e.load_model_with_params(str(tmp_path), S.SenseVoiceModelParams(max_batch=1, max_samples=16000))
        assert e.missing_tensors() == 0 and e.info()["n_vocab"] == 500
        r = e.transcribe_samples(ST.audio(16000, 0))
        assert r.text == " ".join(f"p{t}" for t in r.tokens)   # tokens.txt reached the detokeniser
        e.unload_model()
    else:
        with pytest.raises(S.TranscriptionError) as ei:
            e.load_model_with_params(str(tmp_path), S.SenseVoiceModelParams(max_batch=1, max_samples=16000))
        assert ei.value.status == L.SPT_ERR_DEVICE
    assert seen["spec"] == "empty:sensevoice-test-small:layers=2,1:vocab=500"
    # error paths of the directory reader
    with pytest.raises(S.TranscriptionError, match="neither a synthetic spec nor a FunASR checkpoint") as ei:
        S.SenseVoiceEngine().load_model_with_params(str(tmp_path / "nope"))
    assert ei.value.status == L.SPT_ERR_LOAD
    del w["ctc.ctc_lo.weight"]
    _write_checkpoint_dir(str(tmp_path), D, w)
    with pytest.raises(S.TranscriptionError, match="ctc.ctc_lo.weight"):
        S.SenseVoiceEngine().load_model_with_params(str(tmp_path))


@pytest.fixture(scope="module")
def sv_fuzz(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    out = str(tmp_path_factory.mktemp("asan_sv") / "sv_fuzz")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "native", "sv_fuzz.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    return out


def _run(exe, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, *args], capture_output=True, timeout=60, env=env)
    err = r.stderr.decode(errors="replace")
    assert r.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, (args, r.returncode, err[-2000:])
    return r.stdout


def test_host_code_under_sanitizers(sv_fuzz, tmp_path):
    assert _run(sv_fuzz, "selftest").startswith(b"selftest: 0 failures")
    out = _run(sv_fuzz, "spec", "synthetic:sensevoice-small").decode()
    assert out.startswith("parsed: synthetic d 512 heads 4 dh 128 ff 2048 layers 1+49+20 vocab 25055 in 560")
    out = _run(sv_fuzz, "spec", "empty:sensevoice-test-small:layers=3,2:vocab=2048:seed=77").decode()
    assert out.startswith("parsed: empty d 256 heads 2 dh 128 ff 512 layers 1+3+2 vocab 2048 in 560 seed 77")
    rng = np.random.default_rng(2)
    for k in range(40):  # random byte strings and mutated good specs
        raw = bytes(rng.integers(1, 256, int(rng.integers(1, 80)), dtype=np.uint8))
        if k % 2:
            g = bytearray(b"synthetic:sensevoice-small:layers=2,1:vocab=1024:seed=3")
            g[int(rng.integers(0, len(g)))] = int(rng.integers(1, 256))
            raw = bytes(g)
        out = _run(sv_fuzz, "spec", raw.decode("latin-1").encode("utf-8", "ignore").decode("utf-8"))
        assert out.startswith(b"parsed") or out.startswith(b"rejected"), (raw, out)
    # the tensor table is the restatement's
    names = dict(line.rsplit(" ", 1) for line in _run(sv_fuzz, "names", "empty:sensevoice-test-small").decode().splitlines())
    shapes = ST.tensor_shapes(ST.TEST_SMALL)
    assert {k: int(v) for k, v in names.items()} == {k: int(np.prod(v)) for k, v in shapes.items()}
    # LFR tables and length arithmetic against the restatement's
    for n in (399, 400, 1360, 57999, 58000):
        lines = _run(sv_fuzz, "lfr", str(n), "7", "6").decode().splitlines()
        T = ST.n_frames(n)
        assert lines[0] == f"frames {T} lfr {ST.n_lfr(T)} rows {ST.n_rows(n) if T else 0}"
        got = [[int(v) for v in ln.split(":")[1].split()] for ln in lines[1:]]
        assert got == (ST.lfr_index(T).tolist() if T else [])
    for args in (("-5", "7", "6"), ("1099511627776", "0", "0"), ("4800000", "16", "1")):
        _run(sv_fuzz, "lfr", *args)
    ids = rng.integers(0, 3, 40)
    out = _run(sv_fuzz, "collapse", "4", "0", *[str(i) for i in ids]).decode().split()[1:]
    _, tok, frame = ST.ctc_collapse(ids, 4, 0)
    assert out == [f"{t}@{f}" for t, f in zip(tok, frame)]


def test_detokeniser_cases(sv_fuzz, tmp_path):
    pieces = ["<unk>", "<s>", "</s>", "▁caf", "<0xC3>", "<0xA9>", "▁au", "<|zh|>", "▁lait", "<0xE6>", "<0x97>", "<0xA5>", "<|withitn|>"]

    def detok(ids, pcs=pieces):
        p = tmp_path / "d.txt"
        p.write_bytes((" ".join(str(i) for i in ids) + "\n").encode() + "\n".join(pcs).encode("utf-8") + b"\n")
        out = _run(sv_fuzz, "detok", str(p))
        assert out.startswith(b"text: ") and out.endswith(b"\n")
        return out[6:-1]

    assert detok([7, 12, 3, 4, 5, 6, 8, 2]).decode("utf-8") == "café au lait"   # tags dropped, bytes joined
    assert detok([9, 10, 11]).decode("utf-8") == "日"
    assert detok([0, 1, 2, 7, 12]) == b""
    assert detok([3]) == b"caf" and detok([6, 3]).decode() == "au caf"
    assert detok([3, 500, -1, 6]).decode() == "caf au"
    assert detok([]) == b""
