"""CPU checks of tests/pk_ref.py and tests/pk_cases.py: the float64 reference of the Parakeet
kernels against independent formulations in torch float64 (NeMo's rel_shift, conv2d, LSTMCell, ..), and its greedy
TDT loop against oracle.parakeet.Model.decode; every refusal of the spt_debug_pk_* hooks (made on the host before
any launch); each case's
preconditions; and each case's sensitivity: the reference recomputed with a named fault differs from the
true one by at least 100 bars, or in an exact value."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from spittle_amd import _lib as L
from spittle_amd import pk_debug as D
from spittle_amd.engine import TranscriptionError
from tests import pk_cases as K
from tests import pk_ref as R

t64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64))  # noqa: E731
z = lambda *s: np.zeros(s, np.float32)  # noqa: E731


def _close(a, b, what, tol=1e-12):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, what
    assert np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)), initial=0.0) <= tol, what


# ------------------------------------------------------------------------------------- the reference
def _nemo_rel_shift(x):
    """NeMo RelPositionMultiHeadAttention.rel_shift: pad a zero column on the left, view the matrix with the
    last two sizes swapped, drop the first row, view back.  x [b][h][T][2T - 1]."""
    b, h, qlen, pos_len = x.shape
    x = F.pad(x, pad=(1, 0))
    x = x.view(b, h, -1, qlen)
    return x[:, :, 1:].view(b, h, qlen, pos_len)


@pytest.mark.parametrize("T,dk", [(1, 8), (2, 16), (7, 8), (33, 64)])
def test_rel_attn_index_form_is_nemo_rel_shift(T, dk):
    """bd[i][j] = (q_i + v) . p[T - 1 - i + j] is rel_shift(matrix_bd)[:, :, :, :T] on the full [T][2T - 1] matrix;
    the whole attention is NeMo's softmax((ac + bd) / sqrt(dk)) v."""
    rng = np.random.default_rng(T)
    Hh, d = 2, 2 * dk
    qkv = rng.normal(0, 1, (T, 3 * d))
    p = rng.normal(0, 1, (2 * T - 1, d))
    pu, pv = rng.normal(0, 1, (Hh, dk)), rng.normal(0, 1, (Hh, dk))
    lens = np.array([[0, 0, 0, T]])
    got = R.rel_attn(qkv, p, pu, pv, lens, B=1, Tp=T, H=Hh, dk=dk, ldp=d)
    heads = lambda m: t64(m).view(-1, Hh, dk).transpose(0, 1)[None]  # noqa: E731  [1][H][rows][dk]
    q, k, v = (heads(qkv[:, n * d:(n + 1) * d]) for n in range(3))
    ac = (q + t64(pu)[None, :, None, :]) @ k.transpose(-1, -2)
    bd = _nemo_rel_shift((q + t64(pv)[None, :, None, :]) @ heads(p).transpose(-1, -2))[..., :T]
    o = torch.softmax((ac + bd) / math.sqrt(dk), -1) @ v
    _close(got, o[0].transpose(0, 1).reshape(T, d).numpy(), "rel_attn")


def test_rel_attn_masks_and_strides():
    """Keys >= T3 take no part, rows >= T3 are zero, and the table is read through ldp / p_off / p_bstride."""
    rng = np.random.default_rng(5)
    B, Tp, Hh, dk = 2, 9, 2, 8
    d = Hh * dk
    qkv = rng.normal(0, 1, (B * Tp, 3 * d))
    tab = rng.normal(0, 1, (B, 2 * Tp - 1, 3 * d))
    pu, pv = rng.normal(0, 1, (Hh, dk)), rng.normal(0, 1, (Hh, dk))
    lens = np.array([[0, 0, 0, 5], [0, 0, 0, 9]])
    got = R.rel_attn(qkv, tab.reshape(-1), pu, pv, lens, B=B, Tp=Tp, H=Hh, dk=dk, ldp=3 * d, p_off=d,
                     p_bstride=(2 * Tp - 1) * 3 * d)
    for b, T3 in enumerate((5, 9)):
        # the same utterance alone, unpadded: its own rows of the table are those around the centre
        own = tab[b, Tp - T3:Tp - 1 + T3, d:2 * d]
        alone = R.rel_attn(qkv[b * Tp:b * Tp + T3], own, pu, pv, np.array([[0, 0, 0, T3]]), B=1, Tp=T3, H=Hh, dk=dk, ldp=d)
        _close(got[b * Tp:b * Tp + T3], alone, "padded == alone")
        assert not got[b * Tp + T3:(b + 1) * Tp].any()


def test_mfma_operand_rounding_is_f16():
    q, u = np.float32([0.333251953125, 1000.0]), np.float32([1e-4, 0.3])
    want = (torch.tensor(q) + torch.tensor(u)).to(torch.float16).double().numpy()
    assert (R.f16_add(q, u) == want).all()


@pytest.mark.parametrize("T,Fd,C", [(1, 9, 3), (4, 16, 2), (9, 9, 4), (5, 16, 3)])
def test_subsampling_is_conv2d(T, Fd, C):
    rng = np.random.default_rng(T * Fd)
    lens = np.array([[T, T, T, 0], [max(T - 2, 0)] * 3 + [0]])
    w, bias = rng.normal(0, 1, (C, 9)), rng.normal(0, 1, C)
    mel = rng.normal(0, 1, (2, T, Fd))
    x = rng.normal(0, 1, (2, T, Fd, C))
    for b in range(2):  # the convolution sees zeros past the valid frames
        n = lens[b, 0]
        m1, x1 = mel[b:b + 1].copy(), x[b:b + 1].copy()
        m1[:, n:], x1[:, n:] = 0, 0
        y0 = F.relu(F.conv2d(t64(m1)[:, None], t64(w).view(C, 1, 3, 3), t64(bias), stride=2, padding=1))
        _close(R.conv0(mel, lens, w, bias)[b], y0[0].permute(1, 2, 0).numpy(), "conv0")
        for stage in (1, 2):
            yd = F.conv2d(t64(x1).permute(0, 3, 1, 2), t64(w).view(C, 1, 3, 3), t64(bias), stride=2, padding=1, groups=C)
            _close(R.dwconv(x, lens, stage, w, bias)[b], yd[0].permute(1, 2, 0).numpy(), "dwconv")


@pytest.mark.parametrize("Tp,T3", [(1, 1), (5, 5), (11, 4), (17, 17), (21, 13)])
def test_conv_module_is_glu_conv1d_batchnorm_silu(Tp, T3):
    rng = np.random.default_rng(Tp)
    d = 8
    a = rng.normal(0, 1, (Tp, 2 * d))
    w, bias = rng.normal(0, 1, (d, 9)), rng.normal(0, 1, d)
    g, b, m, v = rng.normal(0, 1, d), rng.normal(0, 1, d), rng.normal(0, 1, d), rng.uniform(0.1, 2, d)
    got = R.conv_module(a, np.array([[0, 0, 0, T3]]), w, bias, g, b, m, v, Tp)
    x = F.glu(t64(a[:T3]), dim=-1).t()[None]                                  # [1][d][T3]
    y = F.conv1d(x, t64(w).view(d, 1, 9), t64(bias), padding=4, groups=d)
    y = F.silu(F.batch_norm(y, t64(m), t64(v), t64(g), t64(b), training=False, eps=1e-5))
    _close(got[:T3], y[0].t().numpy(), "conv module")
    assert not got[T3:].any()


@pytest.mark.parametrize("Tp,d", K.RELPOS_CASES)
def test_relpos_is_the_sinusoid_table(Tp, d):
    pe = R.relpos(Tp, d)
    for r in (0, Tp - 1, 2 * Tp - 2):
        for k in (0, 1, d // 2 - 1):
            ang = (Tp - 1 - r) / (10000.0 ** (2 * k / d))
            assert abs(pe[r, 2 * k] - math.sin(ang)) < 1e-12 * max(1, Tp) and abs(pe[r, 2 * k + 1] - math.cos(ang)) < 1e-12 * max(1, Tp)
    assert (pe[Tp - 1] == np.tile([0.0, 1.0], d // 2)).all()


# ------------------------------------------------------------------- preconditions of the cases
def _attn_ref(cid, dk, dtype, mfma, fault=None, parts=True):
    x = K.attn_inputs(cid, dk)
    kw = {k: x[k] for k in ("B", "Tp", "H", "dk", "ldp", "p_off", "p_bstride")}
    return R.rel_attn(R.round_dtype(x["qkv"], dtype), R.round_dtype(x["p"], dtype), x["pu"], x["pv"], x["lens"], mfma=mfma,
                      fault=fault, parts=parts, **kw)


ATTN_KEYS = [(c["id"], kern, dt, dk) for c in K.ATTN_CASES for kern, dt, dk in K.attn_kernels(c)]
# the CPU checks walk one kernel of each arithmetic and head dim (the 16-bit VALU runs differ in input rounding only)
ATTN_CPU = [k for k in ATTN_KEYS if (k[1], k[2]) in (("valu", "f32"), ("mfma", "f16")) or k[3] == 72]


@pytest.mark.parametrize("cid,kern,dtype,dk", ATTN_CPU)
def test_attn_case_preconditions(cid, kern, dtype, dk):
    c, x = K.attn_case(cid), K.attn_inputs(cid, dk)
    r = _attn_ref(cid, dk, dtype, kern == "mfma")
    assert r["smax"].max() < 60.0                       # exp() of a score difference stays a normal f32
    assert np.abs(R.round_dtype(x["qkv"], "f16")).max() <= 1e4 and np.isfinite(x["p"]).all()
    qu = np.abs(x["qkv"].reshape(x["B"], x["Tp"], 3, K.H, dk)[:, :, 0] + x["pu"]).max()
    assert qu < 16.0                                    # the MFMA operands after the add: far inside f16
    assert (x["pu"] != 0).all() and (x["pv"] != 0).all() and (x["pu"][0] != x["pu"][1]).any() and (x["pu"] != x["pv"]).all()
    for b in range(x["B"]):
        T3 = int(x["lens"][b, 3])
        assert (r["out"].reshape(x["B"], x["Tp"], -1)[b, T3:] == 0).all()
        if c["family"] in ("bd", "ac", "mix"):
            for h in range(K.H):
                assert (r["arg"][b, :T3, h] == x["peak"][b, h, :T3]).all(), (b, h)
                if T3 > 1:
                    assert r["gap"][b, :T3, h].min() > 4.0, r["gap"][b, :T3, h].min()
    if c["family"] == "equal":
        d = K.H * dk
        v = R.round_dtype(x["qkv"], dtype).reshape(x["B"], x["Tp"], 3 * d)[:, :33, 2 * d:].astype(np.float64)
        _close(r["out"].reshape(x["B"], x["Tp"], d)[:, :33], np.broadcast_to(v.mean(1, keepdims=True), (x["B"], 33, d)), "mean of V")
        assert r["gap"].max() == 0.0


@pytest.mark.parametrize("T3", [1, 31, 32, 33, 63, 64, 65, 97])
def test_peaks_cover_the_edges(T3):
    """Over the heads of a case: every key beside a 32-key tile edge, key 0 and key T3 - 1 is the peak of a query
    at the end of a 32-query tile, and the two extreme relative positions occur."""
    pk = [K.peaks(g, T3) for g in range(4)]
    ends = [q for q in K.EDGES + (T3 - 1,) if q < T3]
    hit = {int(p[q]) for p in pk for q in ends}
    want = {k for k in K.EDGES + (T3 - 1,) if k < T3}
    assert hit == want, (hit, want)
    assert pk[0][0] == T3 - 1 and pk[0][T3 - 1] == 0 and all(((p >= 0) & (p < T3)).all() for p in pk)


def test_attn_shapes_cover_the_issue():
    t3 = {t for c in K.ATTN_CASES for t in c["lens"]}
    assert {0, 1, 31, 32, 33, 63, 64, 65, 97} <= t3
    assert any(c["Tp"] == max(c["lens"]) for c in K.ATTN_CASES) and any(c["Tp"] == max(c["lens"]) + 40 for c in K.ATTN_CASES)
    assert any(c["lens"] == (97, 33, 1, 0) for c in K.ATTN_CASES)
    kern = {k for c in K.ATTN_CASES for k in K.attn_kernels(c)}
    assert {("mfma", "f16", 64), ("mfma", "f16", 128)} <= kern and {d for _, _, d in kern} >= {40, 72}
    x = K.attn_inputs("ragged-Tp137-bstride", 64)
    assert x["p_bstride"] and x["ldp"] == 3 * K.H * 64 and x["p_off"] == K.H * 64
    t = x["p"].reshape(x["B"], -1)
    assert (t[0] != t[1]).any()


# --------------------------------------------------------------------------------- sensitivity
def _worst(a, b, bar):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.nanmax(np.abs(a - b) / bar)


@pytest.mark.parametrize("cid,kern,dtype,dk", ATTN_KEYS)
def test_attn_case_sensitivity(cid, kern, dtype, dk):
    c = K.attn_case(cid)
    mfma = kern == "mfma"
    r = _attn_ref(cid, dk, dtype, mfma)
    bar = R.rel_attn_bar(r["out"], r["amax"], r["vmax"], r["nvis"], dk=dk, dtype=dtype, mfma=mfma)
    assert c["faults"]
    for f in c["faults"]:
        tmax = max(c["lens"])
        if tmax == 0 and f != "lens_col":
            continue  # no frame: every row is zero whatever the keys
        if tmax == 1 and f not in ("lens_col", "admit_one", "read_pad"):
            continue  # one key: its probability is 1 whatever its score
        if f in ("admit_one", "read_pad") and c["Tp"] == max(c["lens"]) and len(set(c["lens"])) == 1:
            continue  # no padded key in the launch
        bad = _attn_ref(cid, dk, dtype, mfma, fault=f, parts=False)
        assert _worst(bad, r["out"], bar) >= 100.0, (f, _worst(bad, r["out"], bar))


@pytest.mark.parametrize("family", K.CM_FAMILIES)
@pytest.mark.parametrize("cid", [c["id"] for c in K.CM_CASES])
def test_conv_module_case_sensitivity(cid, family):
    x = K.cm_inputs(cid, family)
    ref, zz, mag = R.conv_module(x["a"], x["lens"], x["dw_w"], x["dw_b"], *x["bn"], x["Tp"], parts=True)
    assert np.abs(x["dw_w"]).min() >= 0.25
    for dt in K.DT:
        bar = R.conv_module_bar(R.round_dtype(x["a"], dt), zz, mag, x["bn"], dt)
        assert (bar < 0.05 * np.maximum(1.0, np.abs(ref))).all()  # f32: about 1e-5
        for f in K.CM_FAULTS:
            if f == "tp_valid" and all(t == x["Tp"] for t in x["lens"][:, 3]):
                continue  # no padded frame
            bad = R.conv_module(x["a"], x["lens"], x["dw_w"], x["dw_b"], *x["bn"], x["Tp"], fault=f)
            assert _worst(bad, ref, bar) >= 100.0, (dt, f)


@pytest.mark.parametrize("mode", K.SUB_MODES)
@pytest.mark.parametrize("cid", [c["id"] for c in K.SUB_CASES])
def test_subsampling_case_is_exact_and_sensitive(cid, mode):
    x = K.sub_inputs(cid, mode)
    ref = _sub_ref(x, mode)
    assert (ref == np.round(ref)).all() and np.abs(ref).max() < 64        # exact in f32, bf16 and f16
    for dt in K.DT:
        assert (R.round_dtype(ref, dt) == ref).all() and (R.round_dtype(x["x"], dt) == x["x"]).all()
    assert (_sub_ref(x, mode, col=(x["col"] + 1) % 3) != ref).any()        # the wrong lens column
    assert (_sub_ref(x, mode, shift=1) != ref).any()                        # a tap shifted by one


def _sub_ref(x, mode, col=None, shift=0):
    col = x["col"] if col is None else col
    if mode == "conv0":
        return R.conv0(x["x"], x["lens"], x["w"], x["bias"], col=col, shift=shift)
    return R.dwconv(x["x"], x["lens"], col, x["w"], x["bias"], shift=shift)


def test_sub_cases_cover_the_issue():
    cs = K.SUB_CASES
    assert {c["F"] for c in cs} == {9, 16} and {c["C"] for c in cs} == {64, 1024} and {c["Tp"] for c in cs} >= {1, 2, 3, 4, 5, 9}
    assert any(max(c["lens"]) > c["Tp"] for c in cs)
    assert {c["d"] for c in K.CM_CASES} == {256, 1024, 1028}
    assert {t for c in K.CM_CASES for t in c["lens"]} >= {1, 4, 5, 8, 9, 12, 13, 17}
    assert any(c["Tp"] % 8 and c["Tp"] > max(c["lens"]) for c in K.CM_CASES)


# ----------------------------------------------------------------------------------- refusals
def _rejects(word, fn, *a, **kw):
    with pytest.raises(TranscriptionError) as e:
        fn(*a, **kw)
    assert e.value.status == L.SPT_ERR_INVALID_ARG and word in e.value.message, e.value.message


def _ok_attn(**over):
    B, Tp, Hh, dk = 2, 5, 2, 64
    kw = dict(dtype="f16", B=B, Tp=Tp, H=Hh, dk=dk, ldp=128, lens=np.array([[0, 0, 0, 5], [0, 0, 0, 3]], np.int32))
    kw.update(over)
    d = kw["H"] * kw["dk"]
    kw.setdefault("qkv", z(kw["B"] * kw["Tp"] * 3 * max(d, 1)))
    kw.setdefault("p", z(max((2 * kw["Tp"] - 1) * kw["ldp"] + kw.get("p_off", 0), 1)))
    kw.setdefault("pu", z(max(d, 1)))
    kw.setdefault("pv", z(max(d, 1)))
    args = [kw.pop(n) for n in ("qkv", "p", "pu", "pv", "lens")]
    return D.rel_attn(*args, **kw)


def test_rel_attn_refusals():
    _rejects("lens[b][3] above Tp", _ok_attn, lens=np.array([[0, 0, 0, 6], [0, 0, 0, 3]], np.int32))
    _rejects("negative entry", _ok_attn, lens=np.array([[0, 0, 0, 5], [0, 0, 0, -1]], np.int32))
    _rejects("negative entry", _ok_attn, lens=np.array([[0, -2, 0, 5], [0, 0, 0, 1]], np.int32))
    for v in ("mfma",):
        _rejects("MFMA kernel is f16", _ok_attn, variant=v, dtype="f32")
        _rejects("MFMA kernel is f16", _ok_attn, variant=v, dtype="bf16")
        _rejects("MFMA kernel is f16", _ok_attn, variant=v, dk=72, ldp=144)
        _rejects("MFMA kernel is f16", _ok_attn, variant=v, dk=256, ldp=512)
    _rejects("variant 0..2", _ok_attn, variant=3)
    _rejects("multiple of 8", _ok_attn, dk=60, ldp=120)
    _rejects("multiple of 8", _ok_attn, dk=0)
    _rejects("multiple of 8", _ok_attn, dk=264, ldp=528)
    _rejects("16-byte grid", _ok_attn, ldp=132)                              # f16: 8 elements
    _rejects("16-byte grid", _ok_attn, ldp=256, p_off=4)
    _rejects("16-byte grid", _ok_attn, dtype="f32", ldp=130)                 # f32: 4 elements
    _rejects("16-byte grid", _ok_attn, dtype="f32", ldp=256, p_off=2)
    _rejects("16-byte grid", _ok_attn, dtype="f32", p_bstride=9 * 128 + 2, p=z(2 * 9 * 128 + 2))
    _rejects("f32 only", _ok_attn, p_bstride=9 * 128, p=z(2 * 9 * 128))
    _rejects("f32 only", _ok_attn, dtype="bf16", p_bstride=9 * 128, p=z(2 * 9 * 128))
    _rejects("ldp below d", _ok_attn, ldp=64)
    _rejects("beyond p_count", _ok_attn, p=z(9 * 128 - 1))
    _rejects("beyond p_count", _ok_attn, ldp=256, p_off=128, p=z(9 * 256 - 1))
    _rejects("beyond p_count", _ok_attn, dtype="f32", p_bstride=9 * 128, p=z(2 * 9 * 128 - 1))
    _rejects("out_count below", _ok_attn, out_count=2 * 5 * 128 - 1)
    _rejects("too many frames", _ok_attn, Tp=16384, qkv=z(1), p=z(1), lens=np.zeros((2, 4), np.int32))
    _rejects("B, H in 1..65535", _ok_attn, B=0, lens=np.zeros((1, 4), np.int32))
    _rejects("B, H in 1..65535", _ok_attn, Tp=0, p=z(1))
    _rejects("dtype is", _ok_attn, dtype=7)
    _rejects("negative offset", _ok_attn, p_off=-8, p=z(9 * 128))
    _rejects("null", _ok_attn, pu=None)


def _ok_conv(mode="conv_module", **over):
    kw = dict(dtype="f16", B=2, Tp=5, C_=8, F=9, lens=np.array([[5, 5, 5, 5], [3, 3, 3, 3]], np.int32))
    kw.update(over)
    C_ = max(kw["C_"], 1)
    kw.setdefault("x", z(kw["B"] * max(kw["Tp"], 1) * max(kw["F"], 2) * 2 * C_))
    kw.setdefault("w", z(C_ * 9))
    kw.setdefault("bias", z(C_))
    if mode == "conv_module":
        kw.setdefault("bn", (z(C_),) * 4)
    args = [kw.pop(n) for n in ("x", "lens", "w", "bias")]
    return D.conv(mode, *args, **kw)


def test_conv_refusals():
    _rejects("multiple of 4", _ok_conv, C_=6)
    _rejects("multiple of 4", _ok_conv, C_=0)
    _rejects("lens[b][3] above Tp", _ok_conv, lens=np.array([[5, 5, 5, 6], [3, 3, 3, 3]], np.int32))
    _rejects("negative entry", _ok_conv, lens=np.array([[5, 5, 5, 5], [3, 3, -1, 3]], np.int32))
    _rejects("null BatchNorm", _ok_conv, bn=(z(8), None, z(8), z(8)))
    _rejects("y_count below", _ok_conv, y_count=2 * 5 * 8 - 1)
    _rejects("mode 0..3", _ok_conv, 4)
    _rejects("dtype is", _ok_conv, dtype=5)
    _rejects("Tp >= 1", _ok_conv, Tp=0)
    _rejects("Tp >= 1", _ok_conv, B=0)
    for m in ("conv0", "dwconv1", "dwconv2"):
        _rejects("1..1024 channels", _ok_conv, m, C_=1025, x=z(1))
        _rejects("1..1024 channels", _ok_conv, m, C_=0)
        _rejects("F >= 1", _ok_conv, m, F=0)
        _rejects("y_count below", _ok_conv, m, y_count=2 * 3 * 5 * 8 - 1)
        _rejects("negative entry", _ok_conv, m, lens=np.array([[5, 5, 5, 5], [-3, 3, 3, 3]], np.int32))
    _rejects("64 KiB", _ok_conv, "conv0", F=6000, x=z(2 * 5 * 6000))
    _rejects("null", _ok_conv, w=None)


def test_relpos_refusals():
    _rejects("even d", D.relpos, 4, 7, dtype="f32")
    _rejects("even d", D.relpos, 4, 0, dtype="f32")
    _rejects("even d", D.relpos, 0, 8, dtype="f32")
    _rejects("pe_count below", D.relpos, 4, 8, dtype="f16", pe_count=7 * 8 - 1)
    _rejects("2^26", D.relpos, 1 << 20, 256, dtype="f16", pe_count=8)
    _rejects("dtype is", D.relpos, 4, 8, dtype=3)


def test_hooks_without_gpu_report_device_error():
    """A valid call on a machine without a GPU is SPT_ERR_DEVICE; with one it runs."""
    calls = [lambda: _ok_attn()[1], lambda: _ok_attn(variant="valu", dtype="f32", p_bstride=9 * 128, p=z(2 * 9 * 128))[1],
             lambda: _ok_conv()[1], lambda: _ok_conv("conv0")[1], lambda: _ok_conv("dwconv2")[1],
             lambda: D.relpos(4, 8, dtype="bf16")[1], lambda: _ok_tdt()["fecur"]]
    for call in calls:
        if torch.cuda.is_available():
            assert np.isfinite(call()).all()
            continue
        with pytest.raises(TranscriptionError) as e:
            call()
        assert e.value.status == L.SPT_ERR_DEVICE and e.value.message


def test_exported_and_declared():
    import ctypes as C
    for fn in ("spt_debug_pk_conv", "spt_debug_pk_relpos", "spt_debug_pk_rel_attn", "spt_debug_pk_tdt", "spt_debug_pk_dec_stage",
               "spt_debug_pk_tdt_steps"):
        assert fn in L.EXPORTS and getattr(L.load(), fn).restype is C.c_int


# ------------------------------------------------------------------------------ TDT bookkeeping
def _tdt_ref(cid, fault=None):
    x = K.tdt_inputs(cid)
    return R.tdt_run(x["part"], x["dur"], x["lens"], x["emb"], x["fe"], V=x["V"], max_symbols=x["max_symbols"], cap=x["cap"],
                     T3p=x["T3p"], fault=fault)


def _tdt_same(a, b):
    return all((np.ascontiguousarray(a[k]).view(np.uint32) == np.ascontiguousarray(b[k]).view(np.uint32)).all() for k in a)


def test_merge_top2_against_a_sort():
    """The merge of per-tile top-2 partials is the top-2 of the logits the tiles were cut from."""
    from spittle_amd.pk_debug import pack_part
    rng = np.random.default_rng(9)
    for nt in (1, 2, 5, 40):
        logits = rng.integers(-5, 6, 64 * nt).astype(np.float32)
        tiles = logits.reshape(nt, 64)
        order = np.argsort(-tiles, 1, kind="stable")             # first index on ties
        v1 = np.take_along_axis(tiles, order[:, :1], 1)[:, 0]
        v2 = np.take_along_axis(tiles, order[:, 1:2], 1)[:, 0]
        got = R.merge_top2(pack_part(v1, (order[:, 0] + 64 * np.arange(nt)).astype(np.int32), v2))
        best = int(np.argmax(logits))                              # first maximum
        assert got == (logits[best], best, np.delete(logits, best).max())


@pytest.mark.parametrize("cid", [c["id"] for c in K.TDT_CASES])
def test_tdt_case_preconditions_and_sensitivity(cid):
    x, r = K.tdt_inputs(cid), _tdt_ref(cid)
    st = {n: r["state"][..., i] for i, n in enumerate(R.STATE_FIELDS)}
    part = x["part"]
    v1, i1 = part[..., 0], part[..., 1].copy().view(np.int32)
    assert np.isneginf(v1).any() or part.shape[2] == 1           # a tile that holds no token
    assert (np.isneginf(v1) == (i1 == 0x7FFFFFFF)).all() and ((i1 <= x["V"]) | np.isneginf(v1)).all()
    top = v1.max(-1, keepdims=True)
    assert ((v1 == top).sum(-1) > 1).any() or part.shape[2] == 1  # the best value in two tiles
    assert (st["done"][0] == (x["lens"][:, 3] == 0)).all() and st["done"][0].any()   # T3 = 0: done from the init
    assert (st["done"][-1] == 1).all()                            # every row ends inside the steps
    live = st["done"][:-1] == 0                                   # rows a step works on
    tok_step = live & (st["upd"][1:] == 1)
    blank_step = live & (st["upd"][1:] == 0)
    moved = st["t"][1:] - st["t"][:-1]
    dmax = x["dur"].argmax(-1)
    assert (tok_step & (dmax == 0)).any() and (blank_step & (dmax == 0) & (moved == 1)).any()   # duration 0, both kinds
    assert (tok_step & (dmax == 0) & (moved == 1)).any()         # at_t reaches max_symbols: the frame is forced on
    assert (tok_step & (moved == 0)).any() == (x["max_symbols"] > 1)
    assert (st["n_out"][-1] > x["cap"]).any()                     # the counter passes cap
    assert (st["t"][-1] > x["T3p"] - 1).any()                     # the frame clamp binds
    assert (r["out_tok"][:, -1] == -1).all()                      # the guard
    for s in range(1, st["t"].shape[0]):                          # a done row is frozen
        was = st["done"][s - 1] == 1
        assert (r["state"][s][was] == r["state"][s - 1][was]).all()
    for f in K.TDT_FAULTS:
        if f != "dur_ge" and part.shape[2] == 1:
            continue  # one tile: nothing to merge
        assert not _tdt_same(_tdt_ref(cid, f), r), f


def _ok_tdt(**over):
    from spittle_amd.pk_debug import pack_part
    kw = dict(V=10, max_symbols=2, cap=2, T3p=3)
    part = pack_part(np.zeros((2, 2, 3), np.float32), np.full((2, 2, 3), 4, np.int32), np.zeros((2, 2, 3), np.float32))
    a = dict(part=part, dur=z(2, 2, 5), lens=np.array([[0, 0, 0, 3], [0, 0, 0, 0]], np.int32), emb=z(11, 8), fe=z(2 * 3, 8))
    for k in list(over):
        if k in a:
            a[k] = over.pop(k)
    kw.update(over)
    return D.tdt(a["part"], a["dur"], a["lens"], a["emb"], a["fe"], **kw)


def test_tdt_refusals():
    from spittle_amd.pk_debug import pack_part
    ok = lambda v, i: pack_part(np.full((2, 2, 3), v, np.float32), np.full((2, 2, 3), i, np.int32), z(2, 2, 3))  # noqa: E731
    _rejects("index outside 0 .. V", _ok_tdt, part=ok(0.0, 11))
    _rejects("index outside 0 .. V", _ok_tdt, part=ok(0.0, -1))
    _rejects("no best above -inf", _ok_tdt, part=ok(-np.inf, 0x7FFFFFFF))
    _rejects("best is NaN", _ok_tdt, part=ok(np.nan, 4))
    _rejects("lens[b][3] above Tp", _ok_tdt, lens=np.array([[0, 0, 0, 4], [0, 0, 0, 0]], np.int32))
    _rejects("negative entry", _ok_tdt, lens=np.array([[0, 0, 0, 3], [0, 0, 0, -1]], np.int32))
    _rejects("n_dur", _ok_tdt, n_dur=0)
    _rejects("n_dur", _ok_tdt, n_tiles=0)
    _rejects("n_dur", _ok_tdt, cap=-1)
    _rejects("n_dur", _ok_tdt, B=0)
    _rejects("n_dur", _ok_tdt, P=0)
    _rejects("n_steps 1..4096", _ok_tdt, n_steps=0)
    _rejects("max_symbols >= 1", _ok_tdt, max_symbols=0)
    _rejects("max_symbols >= 1", _ok_tdt, T3p=0)
    assert "spt_debug_pk_tdt" in L.EXPORTS


# ------------------------------------------------------------------------------- the decode stages
def test_lstm_cell_is_torch_lstmcell():
    """Gate order i, f, g, o; rows with upd = 0 keep their state."""
    rng = np.random.default_rng(3)
    P, B = 12, 5
    cell = torch.nn.LSTMCell(P, P).double()
    x, h, c = (rng.normal(0, 1, (B, P)) for _ in range(3))
    with torch.no_grad():
        th, tc = cell(t64(x), (t64(h), t64(c)))
    W = [p.detach().numpy() for p in (cell.weight_ih, cell.weight_hh, cell.bias_ih, cell.bias_hh)]
    upd = np.array([1, 0, 2, 1, 0])
    gh, gc = R.lstm_cell(x, h, c, *W, upd)
    on = upd != 0
    _close(gh[on], th.numpy()[on], "h")
    _close(gc[on], tc.numpy()[on], "c")
    assert (gh[~on] == h[~on]).all() and (gc[~on] == c[~on]).all()


def test_joint_is_relu_linear_and_tile_top2_is_a_sort():
    rng = np.random.default_rng(4)
    P, B, V = 16, 3, 70
    N = V + 1 + K.N_DUR
    fe, gp = (rng.normal(0, 1, (B, P)).astype(np.float32) for _ in range(2))
    W, b = rng.normal(0, 1, (N, P)), rng.normal(0, 1, N)
    logits, x = R.joint(fe, gp, W, b, V, K.N_DUR)
    want = F.linear(F.relu(torch.from_numpy(fe + gp).double()), t64(W), t64(b)).numpy()
    _close(logits, want, "joint")
    for r in range(B):
        lg = np.round(logits[r] * 2)                               # coarse: ties occur
        v1, i1, v2 = R.tile_top2(lg, V)
        from spittle_amd.pk_debug import pack_part
        got = R.merge_top2(pack_part(v1, np.minimum(i1, 0x7FFFFFFF).astype(np.int32), v2))
        tok = lg[:V + 1]
        best = int(np.argmax(tok))
        assert got == (np.float32(tok[best]), best, np.float32(np.delete(tok, best).max()))
        assert np.isneginf(v1[(N + 63) // 64 - 1]) == (64 * ((N + 63) // 64 - 1) > V)


@pytest.mark.parametrize("V", K.JOINT_V)
def test_joint_bias_cases(V):
    """The six crafted logit patterns give the stated token, best and runner-up through tile_top2 + merge_top2, and
    where the vocabulary allows it the runner-up comes from another tile than the best."""
    from spittle_amd.pk_debug import pack_part
    cross = 0
    for pat in range(6):
        b, want = K.joint_bias_case(V, pat)
        v1, i1, v2 = R.tile_top2(b, V)
        got = R.merge_top2(pack_part(v1, np.minimum(i1, 0x7FFFFFFF).astype(np.int32), v2))
        assert (got[1], float(got[0]), float(got[2])) == want, (pat, got, want)
        win = got[1] // 64
        cross += v2[win] < got[2]
        assert not _same3(R.tile_top2(b, V, "blank_out"), (v1, i1, v2)) or pat < 4
    assert cross >= 1 or V < 64
    N = V + 1 + K.N_DUR
    assert {61: N > 64 > V, 63: N > 64 and V < 64, 64: V == 64, 1024: True}[V]


def _same3(a, b):
    return all((np.asarray(x) == np.asarray(y)).all() for x, y in zip(a, b))


@pytest.mark.parametrize("P,B", [(128, 9), (640, 17)])
def test_dec_stage_sensitivity(P, B):
    """gate order permuted, a unit's rows taken from its neighbour, upd ignored: >= 100 bars; n < V for n <= V: an
    exact value."""
    x = K.lstm_inputs(P, B)
    a = (x["x"], x["h"], x["c"], x["W_ih"], x["W_hh"], x["b_ih"], x["b_hh"], x["upd"])
    h, c, g, mag = R.lstm_cell(*a, parts=True)
    bh, bc = R.lstm_bar(x["c"], g, mag)
    assert bh.max() < 2e-2 and (g > 10).any() and (g < -10).any()     # both saturations are reached
    for f in K.DEC_FAULTS["lstm"]:
        fh, fc = R.lstm_cell(*a, fault=f)
        assert max(np.max(np.abs(fh - h) / bh), np.max(np.abs(fc - c) / bc)) >= 100.0, f
    p = K.pred_inputs(P, B, True)
    assert (R.pred_proj(p["x"], p["W"], p["b"], p["gp"], p["upd"], "upd_ignored") != R.pred_proj(p["x"], p["W"], p["b"], p["gp"], p["upd"])).any()
    assert (p["upd"] == 0).any() and (p["upd"] != 0).any()


def _ok_dec(mode="lstm", **over):
    P, B = over.pop("P", 128), over.pop("B", 2)
    kw = dict(B=B, P=P, state=D.state_rows(np.ones(max(B, 1))))
    Pn = max(P, 1)
    if mode == "lstm":
        kw.update(W=z(4 * Pn, Pn), W2=z(4 * Pn, Pn), b0=z(4 * Pn), b1=z(4 * Pn), xin=z(max(B, 1), Pn), h_in=z(max(B, 1), Pn), c_in=z(max(B, 1), Pn))
    elif mode == "pred":
        kw.update(W=z(Pn, Pn), b0=z(Pn), xin=z(max(B, 1), Pn), gp=z(max(B, 1), Pn))
    else:
        V, nd = over.get("V", 61), over.get("n_dur", 5)
        kw.update(W=z(max(V + 1 + nd, 1), Pn), b0=z(max(V + 1 + nd, 1)), fe=z(max(B, 1), Pn), gp=z(max(B, 1), Pn), V=V, n_dur=nd)
    kw.update(over)
    return D.dec_stage(mode, kw.pop("W"), kw.pop("b0"), kw.pop("state"), **kw)


def test_dec_stage_refusals():
    # what each stage's register and LDS budget admits: 64 | P (LSTM), 128 | P (prediction), 32 | P (joint), P <= 640
    for m, bad in (("lstm", (0, 96, 704, 1280)), ("pred", (0, 64, 192, 704, 1280)), ("joint", (0, 48, 672, 1280))):
        for P in bad:
            _rejects("bad shape", _ok_dec, m, P=P)
        _rejects("bad shape", _ok_dec, m, B=0)
        _rejects("bad shape", _ok_dec, m, B=65)
        _rejects("null", _ok_dec, m, state=None)
    _rejects("mode 0..2", _ok_dec, 3)
    _rejects("needs W2", _ok_dec, "lstm", W2=None)
    _rejects("needs W2", _ok_dec, "lstm", c_in=None)
    _rejects("needs xin and gp", _ok_dec, "pred", gp=None)
    _rejects("needs fe, gp", _ok_dec, "joint", fe=None)
    _rejects("n_dur", _ok_dec, "joint", n_dur=0)
    _rejects("n_dur", _ok_dec, "joint", V=-1)
    _rejects("n_dur", _ok_dec, "joint", n_dur=65)


def test_dec_stage_without_gpu_reports_device_error():
    for m in ("lstm", "pred", "joint"):
        if torch.cuda.is_available():
            assert _ok_dec(m)["status"] == L.SPT_OK
            continue
        with pytest.raises(TranscriptionError) as e:
            _ok_dec(m)
        assert e.value.status == L.SPT_ERR_DEVICE and e.value.message


# ------------------------------------------------------------------------------------ the whole step
def _steps_ref():
    x, S = K.steps_inputs(), K.STEPS
    return R.tdt_steps(**x, V=S["V"], n_dur=K.N_DUR, max_symbols=S["max_symbols"], cap=S["cap"], T3p=S["T3p"], n_steps=S["n_steps"])


def test_whole_step_case_is_wide_and_varied():
    """Every token and duration decision of the 14 steps leads its runner-up by >= 100 bars of a joint logit, so an
    f32 kernel must take the same decisions; blanks occur, several tokens occur, a counter passes cap, every row ends."""
    r, S = _steps_ref(), K.STEPS
    assert S["n_steps"] >= 12 and (S["P"], S["B"], S["V"]) == (128, 9, 61)
    assert r["gap"] >= 100 * r["bar"], (r["gap"], r["bar"])
    st = r["state"]
    assert ((st[1:, :, 4] == 0) & (st[:-1, :, 3] == 0)).sum() >= 3          # steps that chose the blank
    assert len(set(r["out_tok"][r["out_tok"] >= 0].tolist())) >= 3
    assert (st[-1, :, 2] > S["cap"]).any() and (st[-1, :, 3] == 1).all() and st[0, 1, 3] == 1


def test_greedy_loop_is_the_oracles_decode():
    """pk_ref's step (LSTM cell, prediction projection, joint, first maxima) and TDT rule, run on the oracle model's
    own tensors and one encoder output, give the tokens, frames and best logits of oracle.parakeet.Model.decode at
    max_symbols 1, 2 and 10: the rules are pinned to the oracle, which test_parakeet_oracle_golden.py pins to the HF
    fixtures."""
    from oracle import parakeet as PO
    d = PO.dims_for("test-small")
    om = PO.Model(d, seed=21)
    P, V, nd = d.pred, d.n_vocab, d.n_dur
    N = V + 1 + nd
    rng = np.random.default_rng(2)
    enc = rng.normal(0, 1, (23, d.d)).astype(np.float32)
    T = lambda tid, *s: om.tensor(tid).reshape(s)  # noqa: E731
    emb = T(90000, V + 1, P)
    lstm = tuple((T(90001 + 4 * j, 4 * P, P), T(90002 + 4 * j, 4 * P, P), T(90003 + 4 * j, 4 * P), T(90004 + 4 * j, 4 * P))
                 for j in range(2))
    fe = enc.astype(np.float64) @ T(90009, P, d.d).astype(np.float64).T + T(90010, P)
    T3 = enc.shape[0]
    for ms in (1, 2, 10):
        tok, frm, t1, t2 = om.decode(enc, ms)
        r = R.tdt_steps(lstm, T(90011, P, P), T(90012, P), T(90013, N, P), T(90014, N), emb, fe, np.array([[0, 0, 0, T3]]), V=V,
                        n_dur=nd, max_symbols=ms, cap=len(tok) + 4, T3p=T3, n_steps=T3 * (ms + 1) + 2)
        assert r["state"][-1, 0, 3] == 1 and r["state"][-1, 0, 2] == len(tok)
        n = len(tok)
        assert (r["out_tok"][:n] == tok).all() and (r["out_frame"][:n] == frm).all() and (r["out_tok"][n:] == -1).all()
        assert np.abs(r["out_t1"][:n] - t1).max() < 1e-3 and np.abs(r["out_t2"][:n] - t2).max() < 1e-3


def test_tdt_steps_refusals():
    x, S = K.steps_inputs(), K.STEPS
    kw = dict(V=S["V"], n_dur=K.N_DUR, max_symbols=S["max_symbols"], cap=S["cap"], T3p=S["T3p"], n_steps=2)
    ok = lambda **o: D.tdt_steps(**{**x, **kw, **o})  # noqa: E731
    _rejects("n_steps 1..4096", ok, n_steps=0)
    _rejects("bad shape", ok, P=192)
    _rejects("bad shape", ok, B=65)
    _rejects("bad shape", ok, n_dur=0)
    _rejects("max_symbols >= 1", ok, max_symbols=0)
    _rejects("max_symbols >= 1", ok, T3p=0)
    _rejects("max_symbols >= 1", ok, cap=-1)
    _rejects("lens[b][3] above Tp", ok, T3p=5)
    _rejects("null", ok, pred_b=None)
    if not torch.cuda.is_available():
        with pytest.raises(TranscriptionError) as e:
            ok()
        assert e.value.status == L.SPT_ERR_DEVICE
