"""numpy model of the fp8 cross K/V cache (spittle_amd/csrc/kv_f8.h) and the float64 reference
of its cross-attention, for tests/test_f8kv_ref.py (CPU), tests/test_gpu_f8kv_attn.py and
tests/test_gpu_f8kv.py.

The quantiser is stated in np.float32 operations, each one rounding: amax, scale = amax / 448,
inv = 448 / amax, y = x * inv, the e4m3fn code of y (round to nearest even, subnormals kept).  The
attention reference is tests/attn_ref.py's softmax(q . k / 8) v on the DEQUANTISED rows f32(code) * scale:
the quantisation is part of the input, not of the error the kernels are allowed.

The cases are those of tests/attn_cases.py (every T_enc, every peak position, every window map) with two
changes that keep every score: odd keys carry 8 A0 in dimension 60 of K (no cross query has a component
there), so the K scales of neighbouring keys differ by 4 and the code dimensions still land on
e4m3-representable values (448 and 112); odd keys' V rows are multiplied by 4, so the V scales do too."""
from __future__ import annotations

import functools

import numpy as np

from tests import attn_cases as AC
from tests import attn_ref as R

F8_MAX = np.float32(448.0)
TINY = np.float32(2.0 ** -64)
UP = np.float32(2.0 ** 64)
PAD_CODE = 0x38  # 1.0: what the debug hook puts in the rows that pad the last block


def _decode_table() -> np.ndarray:
    t = np.zeros(256, np.float32)
    for c in range(256):
        e, m = (c >> 3) & 15, c & 7
        if e == 15 and m == 7:
            a = np.nan
        elif e == 0:
            a = m * 2.0 ** -9
        else:
            a = (1.0 + m / 8.0) * 2.0 ** (e - 7)
        t[c] = -a if c & 0x80 else a
    return t


DECODE = _decode_table()


def e4m3_decode(code) -> np.ndarray:
    return DECODE[np.asarray(code, np.uint8)]


def e4m3_encode(y) -> np.ndarray:
    """f32 -> e4m3fn codes: round to nearest even, subnormals kept; NaN and everything that rounds above
    448 give 0x7F (the row quantiser never produces either)."""
    y = np.ascontiguousarray(y, np.float32)
    u = y.view(np.uint32)
    sign = ((u >> 24) & 0x80).astype(np.uint8)
    a = u & np.uint32(0x7FFFFFFF)
    mag = a.view(np.float32)
    sub = np.rint(mag.astype(np.float64) * 512.0)  # units of 2^-9 (exact product; rint is nearest even)
    r = (a.astype(np.uint64) + 0x7FFFF + ((a >> 20) & 1)) >> 20
    norm = np.where(r > ((135 << 3) | 6), 0x7F, r.astype(np.int64) - (120 << 3))
    with np.errstate(invalid="ignore"):
        code = np.where(mag < np.float32(2.0 ** -6), np.where(np.isnan(sub), 0, sub).astype(np.int64), norm)
    code = np.where(a > 0x7F800000, 0x7F, code)
    return (code.astype(np.uint8) | sign).astype(np.uint8)


def quant_rows(x):
    """x [..., n] f32 (what the 16-bit cache holds, widened) -> (codes uint8 [..., n], scale f32 [...])."""
    x = np.ascontiguousarray(x, np.float32)
    amax = np.abs(x).max(-1)
    zero = amax == 0
    up = np.where(amax < TINY, UP, np.float32(1.0)).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv = (F8_MAX / (amax * up)).astype(np.float32)
        scale = np.where(zero, np.float32(1.0), (amax / F8_MAX).astype(np.float32)).astype(np.float32)
        y = ((x * up[..., None]).astype(np.float32) * inv[..., None]).astype(np.float32)
    codes = np.where(zero[..., None], np.uint8(0), e4m3_encode(np.where(zero[..., None], np.float32(0), y)))
    return codes.astype(np.uint8), scale


def dequant(codes, scale) -> np.ndarray:
    return (e4m3_decode(codes) * np.asarray(scale, np.float32)[..., None]).astype(np.float32)


def quant_dequant(x, dtype) -> np.ndarray:
    """Rows rounded to dtype, quantised and dequantised: what a flagged context's cache reads back as."""
    c, s = quant_rows(R.round_dtype(x, dtype))
    return dequant(c, s)


# ------------------------------------------------------------------------------------------- cases
CASES = AC.CROSS_CASES
BY_ID = AC.CROSS_BY_ID
MODES = ("8wave", "vw_merge", "vw_pq_merge")


@functools.lru_cache(maxsize=None)
def inputs(cid):
    """attn_cases.cross_inputs with neighbouring keys' scales 4 apart (module docstring)."""
    q, k, v, peak = AC.cross_inputs(cid)
    k, v = k.copy(), v.copy()
    assert not q[..., 60].any() and not k[..., 60].any()
    odd = np.arange(k.shape[2]) % 2 == 1
    k[:, :, odd, 60] = 8.0 * AC.A0
    v[:, :, odd, :] *= 4.0
    return q, k, v, peak


@functools.lru_cache(maxsize=None)
def quantised(cid, dtype):
    """-> (kq, vq [B_layout][H][T][64] f32 dequantised, k_scale, v_scale [B_layout][H][T], k codes, v codes)."""
    _, k, v, _ = inputs(cid)
    kc, ks = quant_rows(R.round_dtype(k, dtype))
    vc, vs = quant_rows(R.round_dtype(v, dtype))
    return dequant(kc, ks), dequant(vc, vs), ks, vs, kc, vc


# roundings on a score: q * kLog2Scale, 16 fmaf over the lane's codes, 2 shuffle adds, the scale (the
# decoder kernels' 12 = 1 + 8 + 3 with this kernel's 16 elements per lane, plus one for scale_k)
CHAIN = 1 + 16 + 2 + 1


def tol_of(qr, kw, vw, ref, dtype) -> np.ndarray:
    """attn_cases.dec_tol with this kernel's operation counts: 4 x (the f32 linear bound with CHAIN roundings
    per score, plus one rounding per V term for p * scale_v) x max |v|, plus half an ulp of the 16-bit output."""
    rel = R.rel_bound_f32(qr, kw, None, chain=CHAIN) + 2.0 ** -24
    return 4.0 * rel[..., None] * R.vmax_visible(vw, None)[..., None] + R.half_ulp(ref, dtype)


FAULTS = ("drop_last", "admit_pad", "neighbour_block", "wrong_window", "unweighted", "neighbour_scale")


def faults_of(c):
    f = AC.cross_faults(c) + ["unweighted"]
    if c["T"] > 1:
        f.append("neighbour_scale")
    return f


def ref(cid, dtype, fault=None):
    """-> (out [B][H][Tq][64] float64, tol, rows [B][H][Tq] the fault targets), on the dequantised K/V.
    unweighted: the 8 waves' partials (blocks w, w + 8, ..) merged without their weights.
    neighbour_scale: key j dequantised with the scale of key j ^ 1 (K and V)."""
    c = BY_ID[cid]
    q, _, _, peak = inputs(cid)
    kq, vq, ks, vs, kc, vc = quantised(cid, dtype)
    T, B = c["T"], c["B"]
    qr = R.round_dtype(q, dtype)
    win = [AC.cross_window(c, b) for b in range(B)]
    true_win = list(win)
    if fault == "wrong_window":
        win = [c["b0"] + b // c["share"] for b in range(B)]
    if fault == "neighbour_scale":
        j = np.minimum(np.arange(T) ^ 1, T - 1)
        kq, vq = dequant(kc, ks[:, :, j]), dequant(vc, vs[:, :, j])
    kw, vw = kq[win], vq[win]
    rows = np.ones(peak.shape, bool)
    out = R.attend(qr, kw, vw)
    tol = tol_of(qr, kq[true_win], vq[true_win], R.attend(qr, kq[true_win], vq[true_win]), dtype) if fault else None
    if fault is None:
        tol = tol_of(qr, kw, vw, out, dtype)
    elif fault == "wrong_window":
        rows = np.broadcast_to((np.array(win) != true_win)[:, None, None], peak.shape)
    elif fault == "neighbour_scale":
        pass
    elif fault == "drop_last":
        out = R.attend(qr, kw, vw, (np.arange(T) < T - 1)[None, :])
        rows = peak == T - 1
    elif fault == "admit_pad":
        n = -T % 32
        pad = np.full(kw.shape[:2] + (n, 64), AC.PAD, np.float64)
        out = R.attend(qr, np.concatenate([kw, pad], 2), np.concatenate([vw, pad], 2))
    elif fault == "neighbour_block":
        out = np.array(out)
        nblk = -(-T // 32)
        for idx in np.ndindex(peak.shape if nblk > 1 else (0, 0, 0)):
            b, h, t = idx
            blk = peak[idx] // 32
            other = blk + 1 if blk + 1 < nblk else blk - 1
            jj = np.arange(T)
            src = np.where(jj // 32 == blk, np.minimum(jj + 32 * (other - blk), T - 1), jj)
            out[b, h, t] = R.attend(qr[b, h, t:t + 1], kw[b, h][src], vw[b, h][src])[0]
        rows = np.broadcast_to(nblk > 1, peak.shape)
    elif fault == "unweighted":
        s = R.scores(qr, kw)
        parts = [R.partial(s, vw, AC.wave_keys(T, w)[None, :]) for w in range(8)]
        out = R.merge(parts, weighted=False)
        rows = np.broadcast_to(T > 32, peak.shape)
    else:
        raise ValueError(fault)
    return out, tol, rows
