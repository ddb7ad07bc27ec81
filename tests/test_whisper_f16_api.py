"""The boundary of the Whisper fp16 mode (ABI 14) as far as it can be checked without a device: the
Python dtype mapping, the version string, and the ABI number in the header and the Rust sys crate
(read as text, as tests/test_capi.py reads them: there is no cargo in the test image)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_python_dtype_mapping():
    from spittle_amd import _lib as L
    from spittle_amd.engine import WhisperModelParams, dtype_code
    assert dtype_code("f16") == L.SPT_DTYPE_F16 == 2
    assert dtype_code("bf16") == L.SPT_DTYPE_BF16 == 1
    assert dtype_code("f32") == L.SPT_DTYPE_F32 == 0
    assert dtype_code(WhisperModelParams().dtype) == L.SPT_DTYPE_BF16  # the default is unchanged
    assert dtype_code(WhisperModelParams(dtype="f16").dtype) == L.SPT_DTYPE_F16
    with pytest.raises(ValueError, match="i8"):
        dtype_code("i8")  # the Parakeet int8 mode is not a Whisper engine dtype


def test_version_string_names_abi_14():
    from spittle_amd import _lib as L
    v = L.load().spt_version().decode()
    assert "ABI 14" in v and "ABI 12" in v, v


def test_abi_version_agrees_between_header_and_rust():
    hdr = open(os.path.join(ROOT, "include", "spittle_hip.h")).read()
    rs = open(os.path.join(ROOT, "rust", "spittle-hip-sys", "src", "lib.rs")).read()
    h = re.findall(r"^#define SPT_ABI_VERSION (\d+)$", hdr, re.M)
    r = re.findall(r"^pub const SPT_ABI_VERSION: c_int = (\d+);$", rs, re.M)
    assert h == ["14"] and r == ["14"], (h, r)
    # the dtype codes of the two sides
    for name, code in (("SPT_DTYPE_F32", 0), ("SPT_DTYPE_BF16", 1), ("SPT_DTYPE_F16", 2), ("SPT_DTYPE_I8", 3)):
        assert re.search(rf"\b{name} = {code}\b", hdr), name
        assert re.search(rf"^pub const {name}: spt_dtype = {code};$", rs, re.M), name
    # the safe crate asks for the f16 engine through the sys constant
    safe = open(os.path.join(ROOT, "rust", "spittle-hip", "src", "lib.rs")).read()
    assert "sys::SPT_DTYPE_F16" in safe and "pub fn load_model_f16" in safe
