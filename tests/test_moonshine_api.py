"""CPU-only checks of the Moonshine boundary: header / ctypes / Rust agreement, struct layouts against
gcc, defaults, the model-spec grammar, the pure-Python safetensors reader, and the detokeniser and
spec parser under AddressSanitizer + UBSan as a stand-alone program (tests/native/ms_fuzz.cpp)."""
import ctypes as C
import json
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from spittle_amd import _lib as L
from spittle_amd import moonshine as M

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HEADER = os.path.join(ROOT, "include", "spittle_hip.h")
MS_FUNCS = ["spt_moonshine_default_model_params", "spt_moonshine_default_infer_params", "spt_moonshine_create",
            "spt_moonshine_destroy", "spt_moonshine_last_error", "spt_moonshine_info", "spt_moonshine_tensor_numel",
            "spt_moonshine_set_tensor", "spt_moonshine_missing_tensors", "spt_moonshine_set_vocab",
            "spt_moonshine_transcribe", "spt_moonshine_transcribe_batch", "spt_moonshine_result_free",
            "spt_moonshine_get_timings", "spt_moonshine_debug_stem", "spt_moonshine_debug_encode",
            "spt_moonshine_debug_logits"]
STRUCTS = {"spt_ms_model_params": L.MsModelParams, "spt_ms_infer_params": L.MsInferParams, "spt_ms_result": L.MsResult,
           "spt_ms_model_info": L.MsModelInfo, "spt_ms_timings": L.MsTimings}


def test_header_binding_and_rust_agree():
    hdr = open(HEADER).read()
    declared = set(re.findall(r"\b(spt_moonshine_[a-z_]+)\s*\(", hdr))
    assert declared == set(MS_FUNCS)
    assert declared <= set(L.EXPORTS)
    lib = L.load()
    for f in MS_FUNCS:
        assert hasattr(lib, f), f
    rs = open(os.path.join(ROOT, "rust", "spittle-hip-sys", "src", "lib.rs")).read()
    assert set(re.findall(r"\bpub fn (spt_moonshine_[a-z_]+)\s*\(", rs)) == declared
    for s in list(STRUCTS) + ["spt_ms_ctx"]:
        assert re.search(r"\bpub struct %s\b" % s, rs), s
        assert re.search(r"\b%s\b" % s, hdr), s
    wrap = open(os.path.join(ROOT, "rust", "spittle-hip", "src", "lib.rs")).read()
    for name in ("pub struct HipMoonshineEngine", "pub fn load_model_with_params", "pub fn transcribe_samples",
                 "pub fn unload_model"):
        assert name in wrap, name


def test_abi_version_unchanged_and_feature_macro():
    hdr = open(HEADER).read()
    assert re.search(r"#define\s+SPT_ABI_VERSION\s+14\b", hdr)
    assert re.search(r"#define\s+SPT_HAS_MOONSHINE\s+1\b", hdr)
    rs = open(os.path.join(ROOT, "rust", "spittle-hip-sys", "src", "lib.rs")).read()
    assert "SPT_ABI_VERSION: c_int = 14" in rs and "SPT_HAS_MOONSHINE" in rs
    v = L.load().spt_version().decode()
    assert "ABI 14" in v and "moonshine" in v and "gfx950" in v


def test_struct_layouts_match_header(tmp_path):
    """the opaque context is the sixth struct: it must stay incomplete in the header"""
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void) {",
             "spt_ms_ctx* opaque = 0; (void)opaque;"]
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
    bad.write_text(f'#include "{HEADER}"\nint main(void) {{ return (int)sizeof(spt_ms_ctx); }}\n')
    assert subprocess.run(["gcc", str(bad), "-o", str(tmp_path / "bad")], capture_output=True).returncode != 0


def test_defaults():
    lib = L.load()
    mp = L.MsModelParams()
    lib.spt_moonshine_default_model_params(C.byref(mp))
    assert (mp.dtype, mp.device, mp.max_batch, mp.max_samples, mp.seed) == (L.SPT_DTYPE_F16, 0, 8, 64 * 16000, 1234)
    ip = L.MsInferParams()
    lib.spt_moonshine_default_infer_params(C.byref(ip))
    assert ip.tokens_per_second == 6.5 and ip.max_tokens == 0
    p = M.MoonshineModelParams.variant(M.ModelVariant.Base)
    assert p.model_variant is M.ModelVariant.Base and p.dtype == "f16"
    assert M.MoonshineModelParams.variant("tiny").model_variant is M.ModelVariant.Tiny
    assert M.MoonshineInferenceParams().tokens_per_second == 6.5
    e = M.MoonshineEngine()
    assert not e.is_loaded()
    with pytest.raises(M.TranscriptionError, match="not loaded"):
        e.transcribe_samples([0.0] * 1000, None)


def _create(spec, dtype=L.SPT_DTYPE_F16):
    lib = L.load()
    mp = L.MsModelParams()
    lib.spt_moonshine_default_model_params(C.byref(mp))
    mp.dtype = dtype
    ctx = C.c_void_p()
    err = C.create_string_buffer(256)
    st = lib.spt_moonshine_create(spec, C.byref(mp), C.byref(ctx), err, 256)
    if ctx.value:
        lib.spt_moonshine_destroy(ctx)
    return st, err.value.decode()


def test_spec_grammar_is_checked_before_any_device_work():
    import torch
    for bad, msg in ((b"synthetic:moonshine-huge", "unknown moonshine model"), (b"moonshine-base", "synthetic: or empty:"),
                     (b"synthetic:moonshine-base:layers=0", "bad model spec option"),
                     (b"synthetic:moonshine-base:depth=3", "bad model spec option"),
                     (b"empty:moonshine-tiny:vocab=abc", "bad model spec option"),
                     (b"synthetic:moonshine-test-small:eos=5000", "eos outside the vocabulary"), (b"synthetic:", "unknown moonshine model")):
        st, err = _create(bad)
        assert st == L.SPT_ERR_LOAD and msg in err, (bad, st, err)
    assert _create(None)[0] == L.SPT_ERR_INVALID_ARG
    for dt in (L.SPT_DTYPE_F32, L.SPT_DTYPE_BF16, L.SPT_DTYPE_I8):
        st, err = _create(b"synthetic:moonshine-base", dt)
        assert st == L.SPT_ERR_UNSUPPORTED and "SPT_DTYPE_F16" in err
    if not torch.cuda.is_available():
        # every well-formed spec passes the grammar and then stops at the missing device
        for good in (b"synthetic:moonshine-base", b"synthetic:moonshine-tiny:seed=9", b"empty:moonshine-test-small",
                     b"empty:moonshine-base:layers=2:vocab=1024:eos=7:seed=3"):
            st, err = _create(good)
            assert st == L.SPT_ERR_DEVICE, (good, st, err)


def test_safetensors_reader_round_trip(tmp_path):
    rng = np.random.default_rng(5)
    a = rng.standard_normal((3, 5)).astype(np.float32)
    b = rng.standard_normal(7).astype(np.float16)
    c = rng.standard_normal((2, 2, 3)).astype(np.float32)
    c_bf = (c.view(np.uint32) >> 16).astype(np.uint16)  # truncated bf16
    blobs, header, off = [], {"__metadata__": {"format": "pt"}}, 0
    for name, dt, arr in (("model.a", "F32", a), ("model.b", "F16", b), ("model.c", "BF16", c_bf)):
        raw = arr.tobytes()
        header[name] = {"dtype": dt, "shape": list(c.shape if dt == "BF16" else arr.shape), "data_offsets": [off, off + len(raw)]}
        blobs.append(raw)
        off += len(raw)
    hj = json.dumps(header).encode()
    path = tmp_path / "model.safetensors"
    path.write_bytes(struct.pack("<Q", len(hj)) + hj + b"".join(blobs))
    got = M.read_safetensors(str(path))
    assert set(got) == {"model.a", "model.b", "model.c"}
    assert got["model.a"].dtype == np.float32 and np.array_equal(got["model.a"], a)
    assert np.array_equal(got["model.b"], b.astype(np.float32))
    assert np.array_equal(got["model.c"], (c_bf.astype(np.uint32) << 16).view(np.float32).reshape(c.shape))
    path.write_bytes(struct.pack("<Q", 1 << 40) + hj)
    with pytest.raises(ValueError, match="past the end"):
        M.read_safetensors(str(path))
    header["model.a"]["data_offsets"] = [0, 10 ** 6]
    hj = json.dumps(header).encode()
    path.write_bytes(struct.pack("<Q", len(hj)) + hj + b"".join(blobs))
    with pytest.raises(ValueError, match="outside the file"):
        M.read_safetensors(str(path))
    tok = tmp_path / "tokenizer.json"
    tok.write_text(json.dumps({"model": {"vocab": {"<unk>": 0, "<s>": 1, "</s>": 2, "▁a": 3}},
                               "added_tokens": [{"id": 5, "content": "<<ST_0>>"}]}), encoding="utf-8")
    assert M.read_tokenizer_pieces(str(tok)) == ["<unk>", "<s>", "</s>", "▁a", "", "<<ST_0>>"]


@pytest.fixture(scope="module")
def ms_fuzz(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    out = str(tmp_path_factory.mktemp("asan_ms") / "ms_fuzz")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "native", "ms_fuzz.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    return out


def _run(exe, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, *args], capture_output=True, timeout=60, env=env)
    err = r.stderr.decode(errors="replace")
    assert r.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, (args, r.returncode, err[-2000:])
    return r.stdout


def test_host_parsers_under_sanitizers(ms_fuzz, tmp_path):
    assert _run(ms_fuzz, "selftest").startswith(b"selftest: 0 failures")
    out = _run(ms_fuzz, "spec", "synthetic:moonshine-base").decode()
    assert out.startswith("parsed: synthetic d 416 heads 8 dh 52 rot 46 ff 1664 layers 8+8 vocab 32768 eos 2")
    out = _run(ms_fuzz, "spec", "empty:moonshine-tiny:layers=3:vocab=2048:eos=9:seed=77").decode()
    assert out.startswith("parsed: empty d 288 heads 8 dh 36 rot 32 ff 1152 layers 3+3 vocab 2048 eos 9 seed 77")
    out = _run(ms_fuzz, "spec", "synthetic:moonshine-test-small").decode()
    assert "d 416" in out and "layers 2+2 vocab 1024" in out
    rng = np.random.default_rng(2)
    for k in range(40):  # random byte strings and mutated good specs
        raw = bytes(rng.integers(1, 256, int(rng.integers(1, 80)), dtype=np.uint8))
        if k % 2:
            g = bytearray(b"synthetic:moonshine-base:layers=2:vocab=1024:eos=5:seed=3")
            g[int(rng.integers(0, len(g)))] = int(rng.integers(1, 256))
            raw = bytes(g)
        out = _run(ms_fuzz, "spec", raw.decode("latin-1").encode("utf-8", "ignore").decode("utf-8"))
        assert out.startswith(b"parsed") or out.startswith(b"rejected"), (raw, out)


def test_detokeniser_cases(ms_fuzz, tmp_path):
    pieces = ["<unk>", "<s>", "</s>", "▁caf", "<0xC3>", "<0xA9>", "▁au", "<<ST_1>>", "▁lait", "<0xE6>", "<0x97>", "<0xA5>"]

    def detok(ids, pcs=pieces):
        p = tmp_path / "d.txt"
        p.write_bytes((" ".join(str(i) for i in ids) + "\n").encode() + "\n".join(pcs).encode("utf-8") + b"\n")
        out = _run(ms_fuzz, "detok", str(p))
        assert out.startswith(b"text: ") and out.endswith(b"\n")
        return out[6:-1]

    assert detok([1, 3, 4, 5, 6, 7, 8, 2]).decode("utf-8") == "café au lait"   # byte fallback -> one 2-byte character
    assert detok([9, 10, 11]).decode("utf-8") == "日"                           # a 3-byte character
    assert detok([0, 1, 2, 7]) == b""                                           # only specials
    assert detok([3]) == b"caf" and detok([6, 3]).decode() == "au caf"           # only the leading space goes
    assert detok([4]) == b"\xc3"                                                # a lone byte piece stays a byte
    assert detok([3, 500, -1, 6]).decode() == "caf au"                           # ids outside the vocabulary skipped
    assert detok([]) == b""
