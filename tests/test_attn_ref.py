"""CPU checks of the attention reference (tests/attn_ref.py) and of the crafted cases
(tests/attn_cases.py), before tests/test_gpu_attn.py holds the kernels to them: the plain
path against torch's scaled_dot_product_attention in float64, the merge identity, every case's score
range and sensitivity to the fault it names, and the spt_debug_attn_* hooks' argument checks."""
import numpy as np
import pytest
import torch

from tests import attn_cases as K
from tests import attn_ref as R

SENS = 100.0  # a named fault must move a targeted row by at least this many tolerances


def test_round_dtype_matches_torch():
    x = np.random.default_rng(0).normal(0, 3, 4096).astype(np.float32)
    x[:4] = [0.0, 1.00390625, 1.01171875, -65504.0]  # bf16 ties: to even, both ways
    t = torch.from_numpy(x)
    assert np.array_equal(R.round_dtype(x, "bf16"), t.to(torch.bfloat16).float().numpy())
    assert np.array_equal(R.round_dtype(x, "f16"), t.to(torch.float16).float().numpy())
    assert np.array_equal(R.round_dtype(x, "f32"), x)
    assert R.half_ulp(1.5, "bf16") == 2.0 ** -8 and R.half_ulp(0.75, "f16") == 2.0 ** -12 and R.half_ulp(3.0, "f32") == 0


def test_plain_path_matches_torch_sdpa_float64():
    rng = np.random.default_rng(1)
    q, k, v = (rng.normal(0, 1.5, (2, 2, n, 64)) for n in (5, 37, 37))
    want = torch.nn.functional.scaled_dot_product_attention(*(torch.from_numpy(x) for x in (q, k, v))).numpy()
    assert np.abs(R.attend(q, k, v) - want).max() < 1e-12
    # causal: query t of 5 at position 32 + t
    vis = R.causal(32, 5, 37)
    got = R.attend(q, k, v, vis)
    want = torch.nn.functional.scaled_dot_product_attention(*(torch.from_numpy(x) for x in (q, k, v)),
                                                            attn_mask=torch.from_numpy(vis)).numpy()
    assert np.abs(got - want).max() < 1e-12
    # a pre-scaled q gives the same scores in log2 units
    assert np.abs(R.attend(q * R.C64, k, v, None, prescaled=True) - R.attend(q, k, v)).max() < 1e-12


def test_merge_identity_any_split_gives_the_unsplit_result():
    rng = np.random.default_rng(2)
    q, k, v = (rng.normal(0, 2.0, (3, 2, n, 64)) for n in (4, 100, 100))
    k[..., 40:60, :] *= 4.0  # a chunk that dominates
    s = R.scores(q, k)
    whole = R.attend(q, k, v)
    for cuts in ((0, 100), (0, 1, 100), (0, 32, 64, 96, 100), (0, 50, 50, 100), (0, 0, 7, 100, 100)):
        parts = [R.partial(s[..., a:e], v[..., a:e, :]) for a, e in zip(cuts[:-1], cuts[1:])]
        assert np.abs(R.merge(parts) - whole).max() < 1e-12, cuts
    empty = R.partial(s[..., 0:0], v[..., 0:0, :])
    assert np.all(empty[1] == -np.inf) and np.all(empty[2] == 0) and np.all(empty[0] == 0)
    # waves: interleaved blocks, as the 8 waves of the decoder kernels take them
    parts = [R.partial(s, v, K.wave_keys(100, w)[None, :]) for w in range(8)]
    assert np.abs(R.merge(parts) - whole).max() < 1e-12
    assert np.abs(R.merge(parts, weighted=False) - whole).max() > 1e-3


def _sensitive(ref, bad, tol, rows, what):
    assert rows.any(), f"{what}: the fault targets no row"
    worst = (K.diff(bad, ref) / tol).max(-1)  # the most moved element of each row
    assert (worst[rows] >= SENS).all(), f"{what}: moved only {worst[rows].min():.1f} tolerances"


@pytest.mark.parametrize("c", K.ENC_CASES, ids=lambda c: c["id"])
def test_encoder_cases_are_in_range_and_sensitive(c):
    q, k, v, _ = K.enc_inputs(c["id"])
    for dtype, sum4 in (("f32", True), ("bf16", True), ("bf16", False), ("f16", True)):
        qr, kr = R.round_dtype(q, dtype), R.round_dtype(k, dtype)
        assert np.abs(R.scores(qr, kr)).max() <= 64.0
        ref, tol, _ = K.enc_ref(c["id"], dtype, sum4)
        assert np.isfinite(ref).all() and np.abs(v).max() <= 1.0
        for f in c["faults"]:
            bad, _, rows = K.enc_ref(c["id"], dtype, sum4, f)
            _sensitive(ref, bad, tol, rows, f"{c['id']} {dtype} {f}")
    if c["kind"] == "equal":
        assert np.abs(K.enc_ref(c["id"], "f32")[0] - v.astype(np.float64).mean(2, keepdims=True)).max() < 1e-12


def test_encoder_ladders_sit_on_both_sides_of_the_rebase_threshold():
    """The SUM = 4 kernel re-bases a query when a lane's 32-key sum of 2^(s - m) leaves 4096.  Traced here
    in float64 per query (the kernel re-bases a whole wave when any of its lanes does)."""
    def trace(cid):
        q, k, _, _ = K.enc_inputs(cid)
        s = R.scores(R.scale_q(R.round_dtype(q, "bf16"), "bf16"), R.round_dtype(k, "bf16"), True)[0, 0]
        T = s.shape[-1]
        half = (np.arange(T) % 8) >= 4
        m = s[:, :64].max(-1)
        hits = []
        for t0 in range(64, T, 64):
            blk = s[:, t0:t0 + 64] - m[:, None]
            lt = np.maximum(np.exp2(blk[:, ~half[t0:t0 + 64]]).sum(-1), np.exp2(blk[:, half[t0:t0 + 64]]).sum(-1))
            re = lt > 4096.0
            m = np.where(re, m + np.maximum(blk.max(-1), 0.0), m)
            hits.append(re)
        return np.array(hits)  # [tile - 1][query]
    # (the last tile of T = 257 holds one key: only the whole tiles are counted)
    lo = trace("ladder+11.5")
    assert not lo[0].any() and lo[1].all() and not lo[2].any()
    assert trace("ladder+12.5")[:3].all()
    st = trace("stairs5.9")
    assert not st[0].any() and not st[1].any() and st[2].all() and not st[3].any()
    assert not trace("tile+6.5").any()
    assert trace("tile+7.5")[1].all() and trace("tile+7.5").sum(0).max() == 1
    assert not trace("descend20").any()
    assert trace("-60+60").all()
    mx = trace("mixed+-12.5")
    assert mx[:3, 0::2].all() and not mx[:, 1::2].any()


@pytest.mark.parametrize("c", K.SELF_CASES, ids=lambda c: c["id"])
def test_self_cases_are_in_range_and_sensitive(c):
    q, k, v, peak = K.self_inputs(c["id"])
    vis = R.causal(c["pos0"], c["Tq"], c["ctx"])
    for dtype in K.DT:
        s = R.scores(R.round_dtype(q, dtype), R.round_dtype(k, dtype))
        assert np.abs(np.where(vis, s, 0.0)).max() <= 64.0
        # every poisoned key would win: it beats the row's best visible score
        best = np.where(vis, s, -np.inf).max(-1, keepdims=True)
        assert (np.where(vis, np.inf, s) > best + 8.0).all()
        ref, tol, _ = K.self_ref(c["id"], dtype)
        assert np.isfinite(ref).all()
        for f in K.SELF_FAULTS:
            bad, _, rows = K.self_ref(c["id"], dtype, f)
            if rows.any():
                _sensitive(ref, bad, tol, rows, f"{c['id']} {dtype} {f}")
    assert np.abs(v[:, :, c["pos0"] + c["Tq"]:]).min(initial=5e3) >= 5e3


@pytest.mark.parametrize("c", K.CROSS_CASES, ids=lambda c: c["id"])
def test_cross_cases_are_in_range_and_sensitive(c):
    q, k, v, peak = K.cross_inputs(c["id"])
    assert set(peak.ravel()) == set(K.cross_peaks(c["T"]))  # every listed peak key is some row's
    for dtype in K.DT:
        qr = R.round_dtype(q, dtype)
        assert qr.sum(-1).min() >= 16.0  # a padded key (pad_value in all 64 elements) scores >= 92 log2 units
        win = [K.cross_window(c, b) for b in range(c["B"])]
        assert np.abs(R.scores(qr, R.round_dtype(k, dtype)[win])).max() <= 64.0
        ref, tol, _, _ = K.cross_ref(c["id"], dtype)
        assert np.isfinite(ref).all()
        for f in K.cross_faults(c):
            bad, _, rows, _ = K.cross_ref(c["id"], dtype, f)
            if rows.any():
                _sensitive(ref, bad, tol, rows, f"{c['id']} {dtype} {f}")
        if c["share"] == 1:
            for S in (2, 3, 4):
                _, _, _, parts = K.cross_ref(c["id"], dtype, None, S)
                assert np.abs(R.merge(parts) - ref).max() < 1e-9
                bad, _, rows, _ = K.cross_ref(c["id"], dtype, "unweighted", S)
                if rows.any():
                    _sensitive(ref, bad, tol, rows, f"{c['id']} {dtype} unweighted S={S}")


def test_every_listed_peak_and_edge_is_a_case():
    assert K.cross_peaks(1500) == [0, 1499, 31, 32, 255, 256, 767, 768, 511, 512, 1023, 1024, 383, 384, 1151, 1152,
                                   751, 752]  # 752: the f32 prompt kernels' S = 2 edge (94 blocks of 16 keys)
    assert {1247, 1248, 399, 400, 1199, 1200}.issubset(K.cross_peaks(1600))
    for c in K.CROSS_CASES:  # both sides of every chunk edge of both block sizes is some row's peak
        _, _, _, peak = K.cross_inputs(c["id"])
        for kb in (32, 16):
            for S in (2, 3, 4):
                for a, _ in K.chunk_edges(c["T"], S, kb)[1:]:
                    assert a >= c["T"] or {a - 1, a}.issubset(set(peak.ravel())), (c["id"], kb, S, a)
    assert K.chunk_edges(32, 4) == [(0, 32), (32, 32), (32, 32), (32, 32)]  # the empty chunks
    assert K.chunk_edges(1500, 3) == [(0, 512), (512, 1024), (1024, 1500)]
    for T in K.ENC_T:
        if T >= 64:  # (7 i + 3) mod T reaches every position of a 64-key tile
            _, _, _, peak = K.enc_inputs(f"peaks-T{T}")
            assert set(peak[0, 0] % 64) == set(range(64))
            assert {0, T - 1, 63}.issubset(set(peak[0, 1])) and (T <= 64 or 64 in peak[0, 1])


def test_hook_rejects_bad_arguments_on_the_host():
    """spt_debug_attn_*: every shape a launcher would throw on, or that would read outside a buffer, comes
    back as SPT_ERR_INVALID_ARG with a message before any device is touched."""
    from spittle_amd import _lib as L
    from spittle_amd import attn_debug as D
    from spittle_amd.engine import TranscriptionError

    def rejects(word, fn, *a, **kw):
        with pytest.raises(TranscriptionError) as e:
            fn(*a, **kw)
        assert e.value.status == L.SPT_ERR_INVALID_ARG and word in e.value.message, e.value.message

    z = np.zeros
    rejects("null", D.enc, None, 1, 4, 2)
    rejects("T, H >= 1", D.enc, z((0, 384)), 1, 0, 2)
    cache = z((2, 1, 2, 8, 64), np.float32)
    rejects("negative pos0", D.self_attn, z((1, 128)), cache, -1, 1)
    rejects("beyond the cache", D.self_attn, z((2, 128)), cache, 7, 2)
    rejects("1..4 queries", D.self_attn, z((5, 128)), cache, 0, 5)
    kv = z((3, 2, 40, 64), np.float32)
    q1 = z((2, 128), np.float32)
    rejects("T_enc below 1", D.cross, q1, z((3, 2, 0, 64)), z((3, 2, 0, 64)))
    rejects("beyond B_layout", D.cross, q1, kv, kv, b0=2)
    rejects("beyond B_layout", D.cross, q1, kv, kv, b0=-1)
    rejects("window map entry", D.cross, q1, kv, kv, kvrow=[0, 3])
    rejects("window map entry", D.cross, q1, kv, kv, kvrow=[-1, 0])
    rejects("window map entry", D.cross, q1, kv, kv, kvrow=[2, 2], b0=1, share=2)
    rejects("need the window map", D.cross, q1, kv, kv, share=2)
    rejects("dividing B", D.cross, z((3, 128)), kv, kv, share=2, kvrow=[0, 0, 0])
    rejects("1..4 key chunks", D.cross, q1, kv, kv, splits=5)
    rejects("8-wave kernel's", D.cross, q1, kv, kv, splits=2, mode="vw")
    rejects("one query chunk", D.cross, z((8, 128)), kv, kv, splits=2, share=8, kvrow=[0] * 8)
    rejects("1..4 queries", D.cross, z((10, 128)), kv, kv, Tq=5, B=2)
    rejects("per_query", D.cross, z((4, 128)), kv, kv, Tq=2, mode="vw_pq")
    rejects("mode 0..4", D.cross, q1, kv, kv, mode=7)
    lib = L.load()
    import ctypes as C
    err = C.create_string_buffer(64)
    assert lib.spt_debug_attn_enc(0, 3, D._ptr(z(384, np.float32)), 1, 1, 2, D._ptr(z(128, np.float32)), err, 64) == \
        L.SPT_ERR_INVALID_ARG and b"dtype" in err.value


def test_hook_without_gpu_reports_device_error():
    """A valid call on a machine without a GPU is SPT_ERR_DEVICE; with one it runs."""
    from spittle_amd import _lib as L
    from spittle_amd import attn_debug as D
    from spittle_amd.engine import TranscriptionError
    q, k, v, _ = K.enc_inputs("equal")
    call = lambda: D.enc(K.enc_pack(q, k, v), q.shape[0], q.shape[2], K.H)  # noqa: E731
    if torch.cuda.is_available():
        assert np.isfinite(call()).all()
        return
    with pytest.raises(TranscriptionError) as e:
        call()
    assert e.value.status == L.SPT_ERR_DEVICE and e.value.message
