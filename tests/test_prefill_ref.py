"""The float64 reference of the block prefill's attention kernels and the sensitivity of every
crafted case of tests/prefill_cases.py, on the CPU: attn_ref.attend with attn_ref.causal(0, P, P) (self)
or no mask (cross).  Each fault a case is built for -- the key one past the causal limit admitted, the
newest key dropped, a padded key admitted, the wrong window, a 64-key tile merged without its weight, an
unclamped f16 store -- moves the reference by at least 100 tolerances on an element of every row it
targets, so a kernel that commits it cannot pass tests/test_gpu_prefill_attn.py."""
import numpy as np
import pytest

from tests import attn_cases as K
from tests import attn_ref as R
from tests import prefill_cases as PC


def _moves(ref, bad, tol, rows, what):
    assert rows.any(), f"{what}: targets no row"
    d = (K.diff(ref, bad) / tol).max(-1)
    assert np.all(d[rows] >= 100.0), f"{what}: {d[rows].min():.1f} tolerances on some row"


def test_reference_is_attend_with_the_causal_mask():
    c = PC.SELF_BY_ID["P33"]
    q, k, v, _ = PC.self_inputs(c["id"])
    ref, tol, _ = PC.self_ref(c["id"], "f32")
    s = (q.astype(np.float64) @ np.swapaxes(k.astype(np.float64), -1, -2)) / 8.0
    s = np.where(np.tril(np.ones((33, 33), bool)), s, -np.inf)
    p = np.exp(s - s.max(-1, keepdims=True))
    want = (p / p.sum(-1, keepdims=True)) @ v.astype(np.float64)
    assert np.abs(ref - want).max() < 1e-12
    assert np.isfinite(ref).all() and np.all(tol > 0)


def test_visible_scores_stay_within_64_log2_units_and_poison_is_100():
    for c in PC.SELF_CASES:
        if c["big"]:
            continue
        q, k, v, peak = PC.self_inputs(c["id"])
        P = c["P"]
        s = R.scores(q, k)
        vis = R.causal(0, P, P)
        assert np.abs(np.where(vis, s, 0.0)).max() <= 64.0, c["id"]
        t = np.arange(P)
        for b in range(c["B"]):
            for h in range(PC.H):
                tgt = t // 32 == PC.self_target(P, b, h, c["shift"])
                hidden = s[b, h][tgt][:, :] [~vis[tgt]]
                if hidden.size:
                    assert hidden.min() >= 100.0 - 64.0 and hidden.max() >= 100.0 - 1.0, c["id"]
                # the peak key is the row's best visible key
                best = np.where(vis, s[b, h], -np.inf).argmax(-1)
                assert np.array_equal(best, peak[b, h]), c["id"]
    for c in PC.CROSS_CASES:
        q, k, v, peak = PC.cross_inputs(c["id"])
        kw = k[[PC.cross_window(c, b) for b in range(c["B"])]]
        s = R.scores(q, kw)
        assert np.abs(s).max() <= 64.0, c["id"]
        assert np.array_equal(s.argmax(-1), peak), c["id"]
        assert (q.sum(-1) * K.PAD * R.C64).min() >= 64.0, c["id"]  # a padded key would win every row


# the 7e4 entries are the f16 clamp's case
SELF_RUNS = [(c, dt) for c in PC.SELF_CASES for dt in PC.DT if dt == "f16" or not c["big"]]


@pytest.mark.parametrize("c,dtype", SELF_RUNS, ids=lambda x: x["id"] if isinstance(x, dict) else x)
def test_self_case_is_sensitive(c, dtype):
    ref, tol, _ = PC.self_ref(c["id"], dtype)
    assert np.isfinite(ref).all()
    for f in PC.self_faults(c, dtype):
        bad, _, rows = PC.self_ref(c["id"], dtype, f)
        if f == "unweighted" and not rows.any():
            continue
        _moves(ref, bad, tol, rows, f"{c['id']} {dtype} {f}")


@pytest.mark.parametrize("dtype", PC.DT)
@pytest.mark.parametrize("c", PC.CROSS_CASES, ids=lambda c: c["id"])
def test_cross_case_is_sensitive(c, dtype):
    ref, tol, _ = PC.cross_ref(c["id"], dtype)
    assert np.isfinite(ref).all()
    for f in PC.cross_faults(c):
        bad, _, rows = PC.cross_ref(c["id"], dtype, f)
        if f == "drop_last" and not rows.any():
            continue  # too few rows for the peak list to reach key T - 1 (P = 1 at the long windows does)
        _moves(ref, bad, tol, rows, f"{c['id']} {dtype} {f}")


def test_every_fault_is_targeted_somewhere():
    hit = set()
    for c in PC.SELF_CASES:
        for dt in PC.DT:
            for f in PC.self_faults(c, dt):
                if PC.self_ref(c["id"], dt, f)[2].any():
                    hit.add(("self", f))
    for c in PC.CROSS_CASES:
        for f in PC.cross_faults(c):
            if PC.cross_ref(c["id"], "f32", f)[2].any():
                hit.add(("cross", f))
    assert hit >= {("self", f) for f in PC.SELF_FAULTS} | {("cross", f) for f in ("drop_last", "admit_pad", "wrong_window", "unweighted")}


def test_clamped_store_is_what_the_reference_reads():
    q, k, v, _ = PC.self_inputs("P33-7e4")
    with np.errstate(over="ignore"):
        kr, vr = PC.stored(k, "f16"), PC.stored(v, "f16")
        assert np.isinf(R.round_dtype(k, "f16")).any() and np.isinf(R.round_dtype(v, "f16")).any()
    assert np.abs(kr).max() == 65504.0 and np.abs(vr).max() == 65504.0


def test_every_block_of_the_longest_prefixes_carries_the_poison():
    for P in (225, 448):
        blocks = {PC.self_target(P, b, h, c["shift"]) for c in PC.SELF_CASES if c["P"] == P and not c["big"]
                  for b in range(c["B"]) for h in range(PC.H)}
        assert blocks == set(range(-(-P // 32))), (P, sorted(blocks))
