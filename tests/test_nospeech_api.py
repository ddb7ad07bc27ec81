"""CPU-only checks of the no-speech additions to the C ABI (SPT_HAS_NO_SPEECH): the header, the Python
binding and the Rust sys crate agree on the renamed field, the flag and spt_window_info; the ABI
version did not move; the defaults leave the feature off; bad values and bad hook arguments are refused
before any device work."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from spittle_amd import _lib as L
from spittle_amd import nospeech_debug as D
from spittle_amd.engine import TranscriptionError, WhisperInferenceParams, _infer_params

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HEADER = os.path.join(ROOT, "include", "spittle_hip.h")
NEW = ("spt_get_window_info", "spt_debug_no_speech")


def test_symbols_flag_and_version_everywhere():
    hdr = open(HEADER).read()
    rs = open(os.path.join(ROOT, "rust", "spittle-hip-sys", "src", "lib.rs")).read()
    lib = L.load()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in L.EXPORTS and hasattr(lib, name), name
        assert len(re.findall(r"\bpub fn %s\s*\(" % name, rs)) == 1, name
    assert re.search(r"^#define SPT_HAS_NO_SPEECH 1$", hdr, re.M) and "SPT_HAS_NO_SPEECH: c_int = 1" in rs
    assert re.search(r"^#define SPT_NO_SPEECH_PROB 16u\b", hdr, re.M) and "SPT_NO_SPEECH_PROB: u32 = 16" in rs
    assert L.SPT_NO_SPEECH_PROB == 16
    assert L.SPT_NO_SPEECH_PROB not in (L.SPT_SUPPRESS_BLANK, L.SPT_NO_TIMESTAMPS, L.SPT_IGNORE_EOT, L.SPT_SUPPRESS_NST)
    assert re.search(r"^#define SPT_ABI_VERSION 14$", hdr, re.M) and "SPT_ABI_VERSION: c_int = 14" in rs
    v = lib.spt_version().decode()
    assert "ABI 14" in v and "nospeech" in v


def test_field_and_struct_layouts(tmp_path):
    """no_speech_thold is a float where reserved0 was (offset and struct size unchanged: between
    max_initial_ts and seed), and spt_window_info's mirror has gcc's size and offsets"""
    structs = {"spt_infer_params": L.InferParams, "spt_window_info": L.WindowInfo}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"',
             "_Static_assert(sizeof(((spt_infer_params*)0)->no_speech_thold) == 4, \"4 bytes\");",
             "_Static_assert(_Generic(((spt_infer_params*)0)->no_speech_thold, float: 1, default: 0), \"a float\");",
             "int main(void) {"]
    for cname, py in structs.items():
        lines.append(f'printf("{cname} size %zu\\n", sizeof({cname}));')
        for f in py._fields_:
            lines.append(f'printf("{cname} {f[0]} %zu\\n", offsetof({cname}, {f[0]}));')
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c11", str(src), "-o", str(tmp_path / "layout")], check=True)
    got = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.split("\n")
    seen = {}
    for line in filter(None, got):
        cname, field, val = line.split()
        py = structs[cname]
        assert int(val) == (C.sizeof(py) if field == "size" else getattr(py, field).offset), line
        seen[(cname, field)] = int(val)
    # the slot reserved0 held: the 4 bytes after max_initial_ts, before the 8-aligned seed
    assert seen[("spt_infer_params", "no_speech_thold")] == seen[("spt_infer_params", "max_initial_ts")] + 4 == 88
    assert seen[("spt_infer_params", "seed")] == 96 and seen[("spt_infer_params", "size")] == 104
    assert dict(L.InferParams._fields_)["no_speech_thold"] is C.c_float
    assert seen[("spt_window_info", "size")] == 40
    rs = open(os.path.join(ROOT, "rust", "spittle-hip-sys", "src", "lib.rs")).read()
    body = re.search(r"pub struct spt_infer_params \{(.*?)\n\}", rs, re.S).group(1)
    fields = re.findall(r"pub (\w+): ([^,]+),", body)
    assert fields[[f for f, _ in fields].index("max_initial_ts") + 1] == ("no_speech_thold", "f32")
    assert "reserved0" not in body
    wbody = re.search(r"pub struct spt_window_info \{(.*?)\n\}", rs, re.S).group(1)
    assert re.findall(r"pub (\w+): (\w+),", wbody) == \
        [(n, "f32" if t is C.c_float else "i32") for n, t in L.WindowInfo._fields_]


def test_defaults_leave_it_off():
    ip = L.InferParams()
    L.load().spt_default_infer_params(C.byref(ip))
    assert ip.no_speech_thold == 0.0 and not (ip.flags & L.SPT_NO_SPEECH_PROB)
    assert bytes(C.string_at(C.addressof(ip) + L.InferParams.no_speech_thold.offset, 4)) == b"\0\0\0\0"
    p = WhisperInferenceParams()
    assert p.no_speech_thold == 0.0 and p.no_speech_prob is False
    keep = []
    ip = _infer_params(p, keep)
    assert ip.no_speech_thold == 0.0 and not (ip.flags & L.SPT_NO_SPEECH_PROB)
    ip = _infer_params(WhisperInferenceParams(no_speech_thold=0.6, no_speech_prob=True), keep)
    assert ip.no_speech_thold == pytest.approx(0.6) and ip.flags & L.SPT_NO_SPEECH_PROB


def test_invalid_thresholds_are_refused_before_any_device_work():
    for bad in (-0.1, -1.0, float("nan"), -math.inf):
        with pytest.raises(TranscriptionError) as e:
            _infer_params(WhisperInferenceParams(no_speech_thold=bad), [])
        assert e.value.status == L.SPT_ERR_INVALID_ARG
    lib = L.load()
    n = C.c_int32(-1)
    assert lib.spt_get_window_info(None, None, 0, C.byref(n)) == L.SPT_ERR_INVALID_ARG


def test_hook_refuses_bad_arguments_without_a_device():
    ok = np.zeros((1, 32), np.float32)
    bad = [dict(logits=np.zeros((1, 53249), np.float32), nosp=0),           # V 53249
           dict(logits=ok, nosp=32), dict(logits=ok, nosp=-1),              # nosp out of range
           dict(logits=ok, nosp=0, B=0),                                    # B 0
           dict(logits=None, nosp=0, n_vocab=32, ldl=32),                   # null logits
           dict(logits=ok, nosp=0, n_vocab=32, ldl=31)]                     # ldl < V
    for kw in bad:
        with pytest.raises(TranscriptionError) as e:
            D.no_speech(kw.pop("logits"), kw.pop("nosp"), **kw)
        assert e.value.status == L.SPT_ERR_INVALID_ARG, kw
    lib = L.load()
    err = C.create_string_buffer(256)
    fp = C.POINTER(C.c_float)
    st = lib.spt_debug_no_speech(0, ok.ctypes.data_as(fp), 1, 32, 32, 0, None, err, 256)   # null prob
    assert st == L.SPT_ERR_INVALID_ARG and b"null" in err.value
