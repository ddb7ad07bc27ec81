"""CPU checks of the fp8 cross K/V cache (SPT_MODEL_CROSS_KV_F8): the numpy e4m3 code against
torch.float8_e4m3fn, the numpy row quantiser against the C++ host quantiser (kv_f8.h, returned by
spt_debug_attn_cross_quant before it looks for a device), the hook's refusals, the additions to the ABI, and
the sensitivity of every cross case to its named faults once K and V are quantised."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from spittle_amd import _lib as L
from spittle_amd import f8kv_debug as FD
from tests import attn_cases as AC
from tests import attn_ref as R
from tests import f8kv_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENS = 100.0


def test_decode_matches_torch_for_all_codes():
    codes = np.arange(256, dtype=np.uint8)
    t = torch.from_numpy(codes.copy()).view(torch.float8_e4m3fn).to(torch.float32).numpy()
    mine = F.e4m3_decode(codes)
    assert np.array_equal(np.isnan(t), np.isnan(mine)) and np.isnan(mine).sum() == 2
    ok = ~np.isnan(t)
    assert np.array_equal(t[ok].view(np.uint32), mine[ok].view(np.uint32))
    # every finite code encodes to itself
    assert np.array_equal(F.e4m3_encode(mine[ok]), codes[ok])


def test_encode_matches_torch_on_a_sweep():
    rng = np.random.default_rng(1)
    fin = F.e4m3_decode(np.arange(256, dtype=np.uint8))
    fin = np.sort(fin[np.isfinite(fin)])
    ties = ((fin[:-1].astype(np.float64) + fin[1:]) / 2).astype(np.float32)  # exact: 4 extra bits at most
    near = np.concatenate([np.nextafter(ties, np.float32(np.inf)), np.nextafter(ties, np.float32(-np.inf))])
    x = np.concatenate([fin, ties, near, rng.uniform(-448, 448, 20000).astype(np.float32),
                        (rng.standard_normal(20000) * 2.0 ** rng.integers(-12, 8, 20000)).astype(np.float32),
                        np.float32([0.0, -0.0, 448.0, -448.0, 2.0 ** -9, 2.0 ** -10, 3 * 2.0 ** -10, 2.0 ** -6,
                                    448.0 * (1 + 2.0 ** -22), 1e-30, -1e-30])])
    x = x[np.abs(x) <= np.float32(448.0 * (1 + 2.0 ** -22))]
    want = torch.from_numpy(x.copy()).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    assert np.array_equal(F.e4m3_encode(x), want)


def _host(k, v, dtype):
    """The hook without a device (or with one: the device quantiser's arrays must be the same bits)."""
    H = k.shape[1]
    q = np.zeros((1, H * 64), np.float32)
    return FD.cross_f8(q, k, v, dtype=dtype, allow_no_device=True)


def _rows_for_the_quantiser(dtype):
    rng = np.random.default_rng(7)
    T = 40
    x = (rng.standard_normal((1, 2, T, 64)) * 2.0 ** rng.integers(-6, 6, (1, 2, T, 1))).astype(np.float32)
    x[0, 0, 0] = 0.0                                    # an all-zero row
    x[0, 0, 1] = 0.0
    x[0, 0, 1, 5] = -0.0
    x[0, 0, 2] = 0.0
    x[0, 0, 2, 17] = -3.0                               # a row with one element
    tiny = 2.0 ** -130 if dtype == "bf16" else 2.0 ** -24  # a subnormal of the dtype
    x[0, 0, 3] = 0.0
    x[0, 0, 3, :4] = [tiny, -2 * tiny, 3 * tiny, tiny]
    # rows where y lands exactly on ties: amax 448 (inv = 1), elements halfway between neighbouring codes
    fin = np.sort(F.e4m3_decode(np.arange(128, dtype=np.uint8))[:127])
    ties = ((fin[:-1].astype(np.float64) + fin[1:]) / 2).astype(np.float32)
    ties = ties[ties == R.round_dtype(ties, dtype)][:63]
    x[0, 1, 0] = 0.0
    x[0, 1, 0, :len(ties)] = ties
    x[0, 1, 0, 63] = 448.0
    x[0, 1, 1] = -x[0, 1, 0]
    x[0, 1, 2] = 0.0
    x[0, 1, 2, :2] = [1e-30, -2e-30] if dtype == "bf16" else [6e-5, -6.1e-5]
    return x


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_row_quantiser_matches_the_host_quantiser(dtype):
    k = _rows_for_the_quantiser(dtype)
    v = np.ascontiguousarray(k[:, ::-1])
    r = _host(k, v, dtype)
    assert r.status in (L.SPT_OK, L.SPT_ERR_DEVICE)
    for x, got, got_s in ((k, r.kq, r.k_scale), (v, r.vq, r.v_scale)):
        codes, scale = F.quant_rows(R.round_dtype(x, dtype))
        assert np.array_equal(scale.view(np.uint32), got_s.view(np.uint32))
        want = F.dequant(codes, scale)
        assert np.array_equal(want.view(np.uint32), got.view(np.uint32))
        # the codes themselves: f32(code) * scale / scale is within an ulp of f32(code)
        live = scale > 2.0 ** -100
        back = F.e4m3_encode((got / scale[..., None]).astype(np.float32))
        assert np.array_equal(back[live] & 0x7F, codes[live] & 0x7F)
    zc, zs = F.quant_rows(R.round_dtype(k, dtype)[0, 0, :2])
    assert not zc.any() and (zs == 1.0).all()


def _status(**kw):
    a = dict(device=0, dtype=L.SPT_DTYPE_BF16, mode=0, B=2, B_layout=3, b0=1, H=2, T_enc=33, Tq=1, kvrow=None, share=1,
             null=(), pad=0.0)
    a.update(kw)
    # (a shape refused for its size is refused before any buffer is read: those calls get small ones)
    BL, H, T = min(max(a["B_layout"], 1), 8), min(max(a["H"], 1), 8), min(max(a["T_enc"], 1), 64)
    bufs = dict(q=np.zeros((max(a["B"], 1) * 4, H * 64), np.float32), k=np.zeros((BL, H, T, 64), np.float32),
                v=np.zeros((BL, H, T, 64), np.float32), kq=np.zeros((BL, H, T, 64), np.float32),
                vq=np.zeros((BL, H, T, 64), np.float32), ks=np.zeros((BL, H, T), np.float32),
                vs=np.zeros((BL, H, T), np.float32), out=np.zeros((max(a["B"], 1) * 4, H * 64), np.float32),
                part=np.zeros((max(a["B"], 1) * 4, H, 8, 66), np.float32))
    p = {n: (None if n in a["null"] else x.ctypes.data_as(C.POINTER(C.c_float))) for n, x in bufs.items()}
    km = None if a["kvrow"] is None else np.asarray(a["kvrow"], np.int32)
    err = C.create_string_buffer(512)
    st = L.load().spt_debug_attn_cross_quant(a["device"], a["dtype"], a["mode"], p["q"], p["k"], p["v"], a["pad"], a["B"],
                                         a["B_layout"], a["b0"], a["H"], a["T_enc"], a["Tq"],
                                         None if km is None else km.ctypes.data_as(C.POINTER(C.c_int32)), a["share"],
                                         p["kq"], p["vq"], p["ks"], p["vs"], p["out"], p["part"], err, 512)
    return st, err.value.decode()


def test_hook_refusals_come_before_any_launch():
    assert _status()[0] in (L.SPT_OK, L.SPT_ERR_DEVICE)
    assert _status(dtype=L.SPT_DTYPE_F16, mode=4)[0] in (L.SPT_OK, L.SPT_ERR_DEVICE)
    assert _status(dtype=L.SPT_DTYPE_F32)[0] == L.SPT_ERR_UNSUPPORTED
    bad = [dict(dtype=3), dict(dtype=-1), dict(mode=-1), dict(mode=5), dict(B=0), dict(B=1025), dict(H=0), dict(B_layout=0),
           dict(T_enc=0), dict(Tq=0), dict(Tq=5), dict(share=0), dict(share=9), dict(share=2, B=3, kvrow=[0, 0, 0]),
           dict(share=2, B=2), dict(mode=2, Tq=2), dict(mode=4, Tq=3), dict(b0=-1), dict(b0=2), dict(B=4, B_layout=3, b0=0),
           dict(kvrow=[0, 2]), dict(kvrow=[-1, 0]), dict(null=("q",)), dict(null=("k",)), dict(null=("v",)),
           dict(null=("kq",)), dict(null=("vq",)), dict(null=("ks",)), dict(null=("vs",)), dict(null=("out",)),
           dict(mode=1, null=("part",)), dict(mode=3, null=("out",)), dict(B_layout=4096, H=64, T_enc=1500, b0=0),
           dict(B_layout=1100, H=20, T_enc=1500, b0=0)]
    for kw in bad:
        st, msg = _status(**kw)
        assert st == L.SPT_ERR_INVALID_ARG and msg, (kw, st, msg)
    # a mode's unused output may be null
    assert _status(mode=1, null=("out",))[0] in (L.SPT_OK, L.SPT_ERR_DEVICE)
    assert _status(mode=0, null=("part",))[0] in (L.SPT_OK, L.SPT_ERR_DEVICE)
    assert _status(device=10 ** 6)[0] in (L.SPT_ERR_INVALID_ARG, L.SPT_ERR_DEVICE)


def test_abi_additions():
    hdr = open(os.path.join(ROOT, "include", "spittle_hip.h")).read()
    rs = open(os.path.join(ROOT, "rust", "spittle-hip-sys", "src", "lib.rs")).read()
    hi = open(os.path.join(ROOT, "rust", "spittle-hip", "src", "lib.rs")).read()
    assert re.search(r"^#define SPT_MODEL_CROSS_KV_F8 4u", hdr, re.M) and "SPT_MODEL_CROSS_KV_F8: u32 = 4" in rs
    assert re.search(r"^#define SPT_HAS_CROSS_KV_F8 1$", hdr, re.M) and "SPT_HAS_CROSS_KV_F8: c_int = 1" in rs
    assert re.search(r"^#define SPT_ABI_VERSION 14$", hdr, re.M) and "SPT_ABI_VERSION: c_int = 14" in rs
    assert L.SPT_MODEL_CROSS_KV_F8 == 4 and L.SPT_HAS_CROSS_KV_F8 == 1
    for fn in ("spt_get_cross_kv_info", "spt_debug_cross_kv", "spt_debug_attn_cross_quant"):
        assert fn in L.EXPORTS and re.search(r"\b%s\(" % fn, hdr) and ("pub fn %s(" % fn) in rs
        assert hasattr(L.load(), fn)
    assert "load_model_cross_kv_f8" in hi and "fn cross_kv_info" in hi and "sys::SPT_MODEL_CROSS_KV_F8" in hi
    assert "crosskvf8" in L.load().spt_version().decode()
    lib = L.load()
    assert lib.spt_get_cross_kv_info(None, None, None, None) == L.SPT_ERR_INVALID_ARG
    assert lib.spt_debug_cross_kv(None, 0, 0, None, None) == L.SPT_ERR_INVALID_ARG
    # the f32 engine refuses the flag before it looks for a device
    mp = L.ModelParams()
    lib.spt_default_model_params(C.byref(mp))
    mp.dtype, mp.flags = L.SPT_DTYPE_F32, L.SPT_MODEL_CROSS_KV_F8
    ctx, err = C.c_void_p(), C.create_string_buffer(256)
    assert lib.spt_ctx_create(b"synthetic:tiny.en", C.byref(mp), C.byref(ctx), err, 256) == L.SPT_ERR_UNSUPPORTED
    assert b"CROSS_KV_F8" in err.value and not ctx


def test_record_layout():
    """4352-byte records, 0.531 of the 16-bit block, every part on the 16-byte grid (kv_f8.h)."""
    h = open(os.path.join(ROOT, "spittle_amd", "csrc", "kv_f8.h")).read()
    rec = int(re.search(r"kRecBytes = (\d+)", h).group(1))
    assert rec == 2 * 32 * 64 + 2 * 32 * 4 and rec % 16 == 0 and rec / 8192 <= 0.54
    assert int(re.search(r"kRecV = (\d+)", h).group(1)) == 2048 and int(re.search(r"kRecScale = (\d+)", h).group(1)) == 4096


def _sensitive(ref, bad, tol, rows, what):
    assert rows.any(), f"{what}: the fault targets no row"
    worst = (AC.diff(bad, ref) / tol).max(-1)
    assert (worst[rows] >= SENS).all(), f"{what}: moved only {worst[rows].min():.1f} tolerances"


@pytest.mark.parametrize("c", F.CASES, ids=lambda c: c["id"])
def test_cases_stay_sensitive_once_quantised(c):
    q, k, v, peak = F.inputs(c["id"])
    assert set(peak.ravel()) == set(AC.cross_peaks(c["T"]))
    for dtype in ("bf16", "f16"):
        kq, vq, ks, vs, kc, vc = F.quantised(c["id"], dtype)
        kr = R.round_dtype(k, dtype)
        # the code dimensions land on representable values: the quantised scores keep the built margins
        nbits = max(1, int(c["T"] - 1).bit_length())
        assert np.array_equal(kq[..., 1:1 + nbits], kr[..., 1:1 + nbits])
        if c["T"] > 1:
            assert (ks[:, :, 1] == 4 * ks[:, :, 0]).all() and (vs[:, :, 1] > 2 * vs[:, :, 0]).all()
        ref, tol, _ = F.ref(c["id"], dtype)
        assert np.isfinite(ref).all()
        for f in F.faults_of(c):
            bad, _, rows = F.ref(c["id"], dtype, f)
            if rows.any():
                _sensitive(ref, bad, tol, rows, f"{c['id']} {dtype} {f}")


def test_c_session_compiles_and_links(tmp_path):
    """tests/native/f8kv_session.c as C11 with -Wall -Wextra -Werror against the library; --link-only stops after
    the refusals that need no device (tests/test_gpu_f8kv.py runs the whole session)."""
    exe = str(tmp_path / "f8kv_session")
    libdir = os.path.join(ROOT, "spittle_amd")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-O1", os.path.join(ROOT, "tests", "native", "f8kv_session.c"),
                    "-I", os.path.join(ROOT, "include"), "-L", libdir, "-lspittle_hip", f"-Wl,-rpath,{libdir}", "-lm",
                    "-o", exe], check=True, capture_output=True, timeout=120)
    r = subprocess.run([exe, "synthetic:tiny.en", "--link-only"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "f8kv_session linked" in r.stdout and "crosskvf8" in r.stdout
