"""CPU-only checks of the token-alignment additions to the C ABI: the new symbols are in the header,
the Python binding and the Rust sys crate, the ABI version did not move, the hooks refuse bad shapes
before looking for a device, and the host-only word grouping does what DESIGN 4.5 says."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from spittle_amd import _lib as L
from spittle_amd import align_debug as D
from spittle_amd.engine import TranscriptionError

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW = ("spt_debug_align_qk", "spt_debug_align_norm", "spt_debug_align_dtw", "spt_debug_align_words",
       "spt_set_alignment_heads", "spt_transcribe_aligned", "spt_transcribe_aligned_batch", "spt_alignment_free",
       "spt_debug_align_last", "spt_debug_align_stats")


def test_symbols_everywhere():
    hdr = open(os.path.join(ROOT, "include", "spittle_hip.h")).read()
    rs = open(os.path.join(ROOT, "rust", "spittle-hip-sys", "src", "lib.rs")).read()
    lib = L.load()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in L.EXPORTS and hasattr(lib, name), name
        assert len(re.findall(r"\bpub fn %s\s*\(" % name, rs)) == 1, name
    assert re.search(r"^#define SPT_HAS_ALIGN_KERNELS 1$", hdr, re.M) and "SPT_HAS_ALIGN_KERNELS: c_int = 1" in rs
    assert re.search(r"^#define SPT_HAS_TOKEN_TIMESTAMPS 1$", hdr, re.M) and "SPT_HAS_TOKEN_TIMESTAMPS: c_int = 1" in rs
    assert re.search(r"^#define SPT_ABI_VERSION 14$", hdr, re.M) and "SPT_ABI_VERSION: c_int = 14" in rs


def test_alignment_struct_layouts(tmp_path):
    """The ctypes mirrors of the alignment structs have the header's sizes and offsets."""
    import subprocess
    structs = {"spt_token_time": L.TokenTime, "spt_word": L.Word, "spt_alignment": L.Alignment}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % os.path.join(ROOT, "include", "spittle_hip.h"),
             "int main(void) {"]
    for cname, py in structs.items():
        lines.append(f'printf("{cname} size %zu\\n", sizeof({cname}));')
        for f in py._fields_:
            lines.append(f'printf("{cname} {f[0]} %zu\\n", offsetof({cname}, {f[0]}));')
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", str(src), "-o", str(tmp_path / "layout")], check=True)
    got = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.split("\n")
    for line in filter(None, got):
        cname, field, val = line.split()
        py = structs[cname]
        assert int(val) == (C.sizeof(py) if field == "size" else getattr(py, field).offset), line


def test_aligned_calls_need_a_context():
    lib = L.load()
    out, al = C.POINTER(L.Result)(), C.POINTER(L.Alignment)()
    assert lib.spt_transcribe_aligned(None, None, 0, None, C.byref(out), C.byref(al)) == L.SPT_ERR_INVALID_ARG
    assert lib.spt_set_alignment_heads(None, None, 0) == L.SPT_ERR_INVALID_ARG
    lib.spt_alignment_free(None)  # as free(NULL)


def test_words_leading_spaces():
    pieces = [b" Hello", b" wor", b"ld", b",", b" again"]
    t0, t1 = [100, 120, 130, 140, 150], [120, 130, 140, 150, 190]
    w = D.words(pieces, t0, t1, [0.5, 1.0, 0.5, 0.25, 1.0])
    assert [x[:4] for x in w] == [(0, 1, 100, 120), (1, 3, 120, 150), (4, 1, 150, 190)]
    assert [x[4] for x in w] == [0.5, pytest.approx((1.0 + 0.5 + 0.25) / 3), 1.0]


def test_words_first_token_without_space_and_single_token():
    assert [x[:4] for x in D.words([b"Hi", b" there"], [0, 10], [10, 30])] == [(0, 1, 0, 10), (1, 1, 10, 30)]
    assert [x[:4] for x in D.words([b" one"], [7], [9])] == [(0, 1, 7, 9)]
    assert D.words([], [], []) == []


def test_words_split_utf8_character():
    """' caf' + the first byte of e-acute, then its second byte: the token that stops inside the
    character joins the next one even though that one begins with a space."""
    e = "é".encode()
    euro = "€".encode()  # three bytes
    w = D.words([b" caf" + e[:1], e[1:], b" " + euro[:2], b" x", b" y"], [0, 4, 8, 12, 16], [4, 8, 12, 16, 20])
    #            word 0 ........  joins   word 1: ends inside the euro sign, so " x" joins it;  " y" starts word 2
    assert [x[:4] for x in w] == [(0, 2, 0, 8), (2, 2, 8, 16), (4, 1, 16, 20)]


def test_hooks_refuse_bad_shapes_without_a_device():
    q = np.zeros((1, 2 * 64), np.float32)
    k = np.zeros((1, 2, 40, 64), np.float32)
    bad = [dict(Tq=5), dict(pos0=-1), dict(N_cap=0), dict(M_cap=41), dict(kvrow=[1])]
    for kw in bad:
        with pytest.raises(TranscriptionError) as e:
            D.qk(np.zeros((kw.get("Tq", 1), 2 * 64), np.float32), k, [0], 4, **kw)
        assert e.value.status == L.SPT_ERR_INVALID_ARG, kw
    for heads, M in (([2], 4), ([-1], 4), ([0], 41)):
        with pytest.raises(TranscriptionError) as e:
            D.qk(q, k, heads, M)
        assert e.value.status == L.SPT_ERR_INVALID_ARG
    with pytest.raises(TranscriptionError) as e:
        D.norm(np.zeros((1, 1, 4, 8), np.float32), N=5)
    assert e.value.status == L.SPT_ERR_INVALID_ARG
    with pytest.raises(TranscriptionError) as e:
        D.dtw(np.zeros((1, 257, 8), np.float32))
    assert e.value.status == L.SPT_ERR_INVALID_ARG
    with pytest.raises(TranscriptionError) as e:  # 256 rows x 32768 keys at 2 bits: beyond the LDS
        D.dtw(np.zeros((1, 256, 32768), np.float32))
    assert e.value.status == L.SPT_ERR_INVALID_ARG
