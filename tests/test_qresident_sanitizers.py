"""The host packer of SPT_MODEL_QUANT_RESIDENT (spittle_amd/csrc/ggml_qpack.h: the file's blocks re-laid into
the resident records at load) built stand-alone with AddressSanitizer + UndefinedBehaviorSanitizer (g++,
no device code, no preload; tests/native/qpack_fuzz.cpp, the way tests/test_host_sanitizers.py builds its
programs) and run on valid tensors, truncated ones, random bytes and refused shapes.  Every run must pack
losslessly or reject cleanly: exit 0, no sanitizer report."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import qgemv_ref as Q

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    out = str(tmp_path_factory.mktemp("asan") / "qpack_fuzz")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__",
           os.path.join(ROOT, "tests", "native", "qpack_fuzz.cpp"), "-o", out]
    subprocess.run(cmd, check=True, capture_output=True, timeout=300)
    return out


def _run(harness, tmp_path, t, N, K, data: bytes, tag: str):
    p = tmp_path / f"{tag}.bin"
    p.write_bytes(data)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([harness, str(t), str(N), str(K), str(p)], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, \
        (tag, r.returncode, r.stdout, r.stderr[-2000:])
    return r.stdout


def _tensor(t, N, K, seed=0):
    rng = np.random.default_rng(seed)
    nb = N * K // 32
    codes = rng.integers(0, 32 if Q.Q5[t] else 16, (nb, 32))
    return Q.make_blocks(t, codes, rng.standard_normal(nb) * 0.02, rng.standard_normal(nb) * 0.1)


@pytest.mark.parametrize("t", [Q.Q5_0, Q.Q4_1, Q.Q5_1], ids=["q5_0", "q4_1", "q5_1"])
def test_valid_and_truncated_tensors(harness, tmp_path, t):
    N, K = 7, 384
    data = _tensor(t, N, K)
    assert _run(harness, tmp_path, t, N, K, data, "valid").startswith(f"packed: {N} x {K} lossless")
    assert _run(harness, tmp_path, t, N, K, data + b"\x5a" * 13, "longer").startswith("packed")
    bb = Q.BLOCK_BYTES[t]
    for cut in (0, 1, bb - 1, bb, 4 * bb - 1, len(data) // 2, len(data) - bb, len(data) - 1):
        assert _run(harness, tmp_path, t, N, K, data[:cut], f"cut{cut}").startswith("rejected"), cut
    # random bytes are valid blocks of some tensor (NaN and infinite scales included)
    junk = np.random.default_rng(5).integers(0, 256, len(data), dtype=np.uint8).tobytes()
    assert _run(harness, tmp_path, t, N, K, junk, "junk").startswith("packed")


def test_refused_shapes_and_types(harness, tmp_path):
    data = _tensor(Q.Q5_0, 4, 128)
    for t, N, K in ((Q.Q5_0, 4, 96), (Q.Q5_0, 4, 100), (Q.Q5_0, -1, 128), (Q.Q5_0, 4, -128), (2, 4, 128), (8, 4, 128),
                    (13, 4, 256), (99, 4, 128), (Q.Q5_0, 1 << 40, 128), (Q.Q5_0, 5, 128)):
        assert _run(harness, tmp_path, t, N, K, data, f"t{t}-{N}-{K}").startswith("rejected"), (t, N, K)
    assert _run(harness, tmp_path, Q.Q5_0, 0, 128, b"", "empty").startswith("rejected")   # no records to lay out
