"""CPU-only checks of the block prefill's additions to the C ABI (SPT_HAS_BLOCK_PREFILL): the
header, the Python binding and the Rust sys crate agree on the flag, the announcement and the new symbols;
the ABI version did not move and spt_infer_params kept its layout; the defaults leave the flag clear; both
attention hooks refuse bad arguments before any device work and a valid call without a device is
SPT_ERR_DEVICE; the host-only arithmetic (workspace rows, slices, the refusals) runs clean under
AddressSanitizer + UndefinedBehaviorSanitizer in a stand-alone program."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from spittle_amd import _lib as L
from spittle_amd import prefill_debug as D
from spittle_amd.engine import TranscriptionError, WhisperEngine, WhisperInferenceParams, _infer_params

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HEADER = os.path.join(ROOT, "include", "spittle_hip.h")
NEW = ("spt_get_prefill_stats", "spt_debug_attn_prefill_self", "spt_debug_attn_prefill_cross")


def test_symbols_flag_and_version_everywhere():
    hdr = open(HEADER).read()
    rs = open(os.path.join(ROOT, "rust", "spittle-hip-sys", "src", "lib.rs")).read()
    hi = open(os.path.join(ROOT, "rust", "spittle-hip", "src", "lib.rs")).read()
    lib = L.load()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in L.EXPORTS and hasattr(lib, name), name
        assert len(re.findall(r"\bpub fn %s\s*\(" % name, rs)) == 1, name
    assert re.search(r"^#define SPT_HAS_BLOCK_PREFILL 1$", hdr, re.M) and "SPT_HAS_BLOCK_PREFILL: c_int = 1" in rs
    assert re.search(r"^#define SPT_BLOCK_PREFILL +32u\b", hdr, re.M) and "SPT_BLOCK_PREFILL: u32 = 32" in rs
    assert L.SPT_BLOCK_PREFILL == 32 and L.SPT_HAS_BLOCK_PREFILL == 1
    others = (L.SPT_SUPPRESS_BLANK, L.SPT_NO_TIMESTAMPS, L.SPT_IGNORE_EOT, L.SPT_SUPPRESS_NST, L.SPT_NO_SPEECH_PROB)
    assert len(set(others)) == 5 and all(L.SPT_BLOCK_PREFILL & f == 0 for f in others)
    flags = dict(re.findall(r"^#define (SPT_(?:SUPPRESS_BLANK|NO_TIMESTAMPS|IGNORE_EOT|SUPPRESS_NST|NO_SPEECH_PROB|BLOCK_PREFILL)) +(\d+)u",
                            hdr, re.M))
    assert len(flags) == 6 and len(set(flags.values())) == 6, flags
    assert re.search(r"^#define SPT_ABI_VERSION 14$", hdr, re.M) and "SPT_ABI_VERSION: c_int = 14" in rs
    v = lib.spt_version().decode()
    assert "ABI 14" in v and "blockprefill" in v
    # the high-level crate carries the parameter and the statistics
    assert "pub fn set_block_prefill(&mut self, on: bool)" in hi and "pub fn prefill_stats(&self)" in hi
    assert "sys::SPT_BLOCK_PREFILL" in hi and "sys::spt_get_prefill_stats" in hi
    # spt_call_stats says what a block pass counts as
    assert re.search(r"decoder_passes;.*block pass", hdr, re.S)


def test_infer_params_keeps_its_layout(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void) {",
             'printf("size %zu\\n", sizeof(spt_infer_params));']
    for f in L.InferParams._fields_:
        lines.append(f'printf("{f[0]} %zu\\n", offsetof(spt_infer_params, {f[0]}));')
    lines.append('printf("stats %zu\\n", sizeof(spt_call_stats));')
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c11", str(src), "-o", str(tmp_path / "layout")], check=True)
    got = dict(l.split() for l in subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True,
                                                 text=True).stdout.splitlines() if l)
    assert int(got["size"]) == C.sizeof(L.InferParams) == 104
    for f in L.InferParams._fields_:
        assert int(got[f[0]]) == getattr(L.InferParams, f[0]).offset, f[0]
    assert int(got["flags"]) == 24 and int(got["seed"]) == 96
    assert int(got["stats"]) == C.sizeof(L.CallStats)


def test_defaults_leave_the_flag_clear():
    ip = L.InferParams()
    L.load().spt_default_infer_params(C.byref(ip))
    assert not (ip.flags & L.SPT_BLOCK_PREFILL)
    p = WhisperInferenceParams()
    assert p.block_prefill is False
    assert not (_infer_params(p, []).flags & L.SPT_BLOCK_PREFILL)
    ip = _infer_params(WhisperInferenceParams(block_prefill=True), [])
    assert ip.flags & L.SPT_BLOCK_PREFILL and ip.flags & L.SPT_SUPPRESS_BLANK
    assert callable(WhisperEngine.prefill_stats)
    lib = L.load()
    a = C.c_int32(-1)
    assert lib.spt_get_prefill_stats(None, C.byref(a), None, None) == L.SPT_ERR_INVALID_ARG


def _self_ok():
    return dict(qkv=np.zeros((2 * 5, 3 * 2 * 64), np.float32), cache=np.zeros((2, 2, 2, 16, 64), np.float32), P=5)


def _cross_ok():
    return dict(q=np.zeros((2 * 5, 2 * 64), np.float32), k=np.zeros((3, 2, 33, 64), np.float32),
                v=np.zeros((3, 2, 33, 64), np.float32), P=5, b0=1)


def _refused(fn, kw, word=None):
    with pytest.raises(TranscriptionError) as e:
        fn(**kw)
    assert e.value.status == L.SPT_ERR_INVALID_ARG, (kw.keys(), e.value)
    assert str(e.value), "a refusal carries a message"
    if word:
        assert word in str(e.value), (word, str(e.value))


def test_self_hook_refuses_bad_arguments_without_a_device():
    for P in (0, -1, 17):                                    # P < 1, P > ctx
        _refused(D.self_attn, dict(_self_ok(), P=P, B=2))
    _refused(D.self_attn, dict(_self_ok(), H=0), "head")      # a head count < 1
    _refused(D.self_attn, dict(_self_ok(), H=-2), "head")
    _refused(D.self_attn, dict(_self_ok(), qkv=None), "null")
    _refused(D.self_attn, dict(_self_ok(), cache=None, B=2, H=2, ctx=16), "null")
    for dt in (3, 4, -1):                                    # a dtype outside f32 / bf16 / f16
        _refused(D.self_attn, dict(_self_ok(), dtype=dt), "dtype")
    lib = L.load()
    err = C.create_string_buffer(256)
    fp = C.POINTER(C.c_float)
    ok = _self_ok()
    st = lib.spt_debug_attn_prefill_self(0, 0, ok["qkv"].ctypes.data_as(fp), ok["cache"].ctypes.data_as(fp), 2, 2, 16, 5,
                                         None, err, 256)     # null out
    assert st == L.SPT_ERR_INVALID_ARG and b"null" in err.value


def test_cross_hook_refuses_bad_arguments_without_a_device():
    for P in (0, -1, 449):
        _refused(D.cross, dict(_cross_ok(), P=P, B=2))
    _refused(D.cross, dict(_cross_ok(), P=17, ctx=16, B=2))   # P > ctx
    _refused(D.cross, dict(_cross_ok(), H=0, B=2), "head")
    for name in ("q", "k", "v"):
        _refused(D.cross, dict(_cross_ok(), **{name: None}, B=2, B_layout=3, H=2, T_enc=33), "null")
    _refused(D.cross, dict(_cross_ok(), out=False), "null")
    _refused(D.cross, dict(_cross_ok(), T_enc=0), "T_enc")
    _refused(D.cross, dict(_cross_ok(), T_enc=-5), "T_enc")
    _refused(D.cross, dict(_cross_ok(), b0=2), "B_layout")    # b0 + B / share > B_layout
    _refused(D.cross, dict(_cross_ok(), b0=-1), "B_layout")
    q10 = np.zeros((10 * 5, 2 * 64), np.float32)
    _refused(D.cross, dict(_cross_ok(), q=q10, b0=2, share=5, kvrow=[0] * 10), "B_layout")
    _refused(D.cross, dict(_cross_ok(), q=q10, b0=0, share=5, kvrow=[2] * 5 + [3] * 5), "window map")
    _refused(D.cross, dict(_cross_ok(), q=q10, b0=0, share=5, kvrow=[2] * 5 + [-1] * 5), "window map")
    _refused(D.cross, dict(_cross_ok(), q=q10, b0=0, share=5), "map")   # shared windows need the map
    for dt in (3, -1):
        _refused(D.cross, dict(_cross_ok(), dtype=dt), "dtype")


def test_valid_calls_without_a_device_are_device_errors():
    """Nothing is refused, so the call goes on to look for a device: without one it is SPT_ERR_DEVICE (with
    one it runs: all-zero scores average the all-zero V)."""
    for fn, kw in ((D.self_attn, _self_ok()), (D.cross, _cross_ok())):
        try:
            got = fn(**kw)
        except TranscriptionError as e:
            assert e.status == L.SPT_ERR_DEVICE, e
            continue
        out = got[0] if isinstance(got, tuple) else got
        assert np.array_equal(out, np.zeros_like(out))


def test_host_arithmetic_under_sanitizers(tmp_path):
    """tests/native/prefill_san.cpp: prefill_host.h alone (no HIP), built with ASan + UBSan, run once."""
    assert shutil.which("g++"), "g++ builds the stand-alone sanitizer program"
    exe = str(tmp_path / "prefill_san")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "native", "prefill_san.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr[-2000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
