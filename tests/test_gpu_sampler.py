"""The sampler kernels (spittle_amd/csrc/k_sample.hip) alone against the float64 reference of
tests/sampler_ref.py, through the context-free hooks spt_debug_sample_* (no engine, no model).

Every row is crafted (tests/sampler_cases.py): base logits are a seeded normal x 2 with chosen
entries overwritten so that every argmax, every candidate rank and the timestamp-rule comparison
has a gap of at least 1e-2 (asserted on the reference).  Tokens, timestamp ids, states and
candidate ids are therefore compared exactly, at every step.

Log-probabilities: logits are identical on both sides, so the error is the f32 log-sum-exp (about
2.5e-6 from the sums, 2e-6 from logf) and one subtraction at |values| <= 30 (4e-6): PLOG_TOL = 5e-5.
The sampling CDF: each f32 prefix is a sum of positive terms through <= 52 serial adds, 10 scan
levels, expf and the f32 val - M2, about 70 * 2^-24 = 4e-6 of the prefix: DELTA = 1e-5 (the f32
emulation of those sums on these rows deviates by 9.5e-7 at most,
test_sampler_ref.py::test_emulated_f32_cdf_stays_inside_delta).
"""
import dataclasses

import numpy as np
import pytest

from oracle import whisper_full as W
from spittle_amd import _lib as L
from spittle_amd import sampler_debug as D
from spittle_amd.engine import TranscriptionError
from tests import sampler_cases as K
from tests import sampler_ref as R

pytestmark = pytest.mark.gpu

VS = (51864, 51865, 51866)
PLOG_TOL = 5e-5   # largest |device - reference| seen over this file: 1.4e-6
DELTA = 1e-5
FAR = 10 ** 6     # an audio end no script reaches
# The two beam paths sum the row's exponentials in different orders (one workgroup: 52 strided terms
# per thread; chunked: 13 per thread against the chunk's maximum, rescaled and added in chunk order),
# so their log-sum-exp can differ in the last bits: each is within 2.5e-6 of the exact one, and the
# candidate's subtraction rounds by at most 2e-6 at |values| <= 32 on each side.  Seen: 1.9e-6 (one
# ulp of the log-sum-exp) on the maxima, pairing, max_initial and has_ts rows; 0 on the beam cases.
PATHS_TOL = 1e-5
_seen = {"plog": 0.0, "paths": 0.0}


def _words(V, smask):
    return D.suppress_words(smask)


def _dprm(prm):
    return D.SampleParams(**dataclasses.asdict(prm))


def run_tokens(V, lg, prm, smask=None, *, seek=0, seek_end=FAR, state=None, done=None, forced=None, out_cap=None,
               step=0, history=None, pos0=0, Tq=1, dtype="f32", n_vocab=None):
    """The hook and the reference driver on the same inputs -> (device outputs, reference)."""
    sp, sm = K.vocab(V)
    sm = sm if smask is None else smask
    emb, pos = K.tables(V)
    dev = D.sample_tokens(lg, _words(V, sm), _dprm(prm), eot=sp["eot"], beg=sp["beg"], blank=K.BLANK, seek=seek,
                          seek_end=seek_end, emb=emb, pos=pos, n_vocab=n_vocab, state=state, done=done,
                          forced=forced, out_cap=out_cap, pos0=pos0, step=step, Tq=Tq, dtype=dtype, history=history)
    ref = R.replay(lg, prm, sp, sm, K.BLANK, seek, seek_end, n_vocab=n_vocab, state=state, done=done, forced=forced,
                   out_cap=out_cap, step=step, history=history)
    return dev, ref


def check_plog(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    fin = np.isfinite(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~fin & ~np.isnan(want)],
                                                                            want[~fin & ~np.isnan(want)])
    if fin.any():
        err = float(np.abs(got[fin] - want[fin]).max())
        _seen["plog"] = max(_seen["plog"], err)
        print(f"plog: largest |device - reference| {err:.3e} (this file so far {_seen['plog']:.3e})")
        assert err <= PLOG_TOL, err


def check_tokens(dev, ref):
    """Exact records, states and next tokens; plog within PLOG_TOL."""
    for key in ("out_tok", "state", "done", "next_tok"):
        assert np.array_equal(dev[key], ref[key]), (key, dev[key], ref[key])
    assert np.array_equal(dev["out_tid"].astype(np.int64), ref["out_tid"].astype(np.int64))
    assert np.array_equal(dev["out_tid"], np.floor(dev["out_tid"]))
    check_plog(dev["out_plog"], ref["out_plog"])
    assert dev["step"] == ref["step"] and dev["arrive"] == 0


def check_beam(V, lg, prm, rows4, step, k, smask=None, ties=False, bitwise=False):
    """Both beam paths against W.topk, and against each other: ids bit for bit; cand_lp bit for bit
    on the beam cases (bitwise), elsewhere within PATHS_TOL -> reference ids [B][8]."""
    sp, sm = K.vocab(V)
    sm = sm if smask is None else smask
    kw = dict(eot=sp["eot"], beg=sp["beg"], blank=K.BLANK, row=rows4, step=step, k=k)
    out = [D.sample_beam(lg, _words(V, sm), _dprm(prm), chunked=c, **kw) for c in (1, 0)]
    ids = np.full((len(lg), 8), -9, np.int64)
    lps = np.zeros((len(lg), 8))
    tid = np.zeros(len(lg), np.int64)
    for b in range(len(lg)):
        i, lp, tid[b] = R.beam(lg[b], rows4[b], step, k, prm, sp, sm, K.BLANK)
        ids[b, :k], lps[b, :k] = i[:k], lp[:k]
        gaps = -np.diff(lp[:k][np.isfinite(lp[:k])])
        assert ties or gaps.size == 0 or gaps.min() >= 1e-2, (b, gaps)
    for o in out:
        assert np.array_equal(o["cand_id"], ids), (o["cand_id"], ids)   # ids, order, the -1 tail, nothing past k
        assert np.array_equal(o["tid"], tid), (o["tid"], tid)
        check_plog(o["cand_lp"], lps)
    assert np.array_equal(out[0]["cand_id"], out[1]["cand_id"])
    a, b = out[0]["cand_lp"], out[1]["cand_lp"]
    fin = np.isfinite(a)
    assert np.array_equal(fin, np.isfinite(b)) and np.array_equal(a[~fin], b[~fin])
    diff = float(np.abs(a[fin].astype(np.float64) - b[fin]).max()) if fin.any() else 0.0
    _seen["paths"] = max(_seen["paths"], diff)
    print(f"beam paths: largest |chunked - one workgroup| {diff:.3e} (this file so far {_seen['paths']:.3e})")
    if bitwise:
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert diff <= PATHS_TOL
    return ids


def check_rows(V, prm, step, rows, k=5, ties=False, smask=None):
    """One step of up to 8 crafted rows on all three paths: the token path at temperature 0 and both
    beam kernels.  rows: dict(lg, last, pen, has_ts, sd, expect).  -> the tokens chosen."""
    B = len(rows)
    assert B <= 8
    lg = np.stack([r["lg"] for r in rows]).astype(np.float32)
    r4 = np.array([[r.get("last", K.TEXT), r.get("pen", K.TEXT), r.get("has_ts", 0), r.get("sd", 0)] for r in rows])
    hist = np.full((B, step + 1), -9, np.int64)
    if step > 0:
        hist[:, step - 1] = r4[:, 0]
    if step > 1:
        hist[:, step - 2] = r4[:, 1]
    state = np.stack([r4[:, 2], r4[:, 3], np.full(B, step), np.zeros(B, np.int64)], axis=1)
    dev, ref = run_tokens(V, lg[None], prm, smask, state=state, step=step, history=hist, pos0=step)
    assert ties or ref["min_margin"] >= 1e-2, ref["min_margin"]
    check_tokens(dev, ref)
    toks = ref["out_tok"][:, step]
    for b, r in enumerate(rows):
        if "expect" in r:
            assert toks[b] == r["expect"], (b, toks[b], r["expect"])
    ids = check_beam(V, lg, prm, r4, step, k, smask, ties)
    assert np.array_equal(ids[:, 0], toks)
    return toks


OPEN = R.Prm(suppress_blank=False, max_initial=-1)   # step 0 with no step-0 rule


# ---- maxima and ties ----------------------------------------------------------------------------
def _positions(V):
    sp, _ = K.vocab(V)
    cs = K.chunk_size(V)
    p = [0, V - 1, sp["beg"] - 1, sp["beg"], sp["eot"], cs + 255, cs + 256, K.TW - 1, K.TW]
    for c in (1, 8, 15):
        p += [c * cs - 1, c * cs]
    return [t for t in p if 0 <= t < V]


@pytest.mark.parametrize("V", VS + (1000,))
def test_maximum_at_every_edge(V):
    """The row maximum at id 0, V - 1, both sides of chunk edges 1, 8 and 15, of a thread-stride edge
    of the chunk kernels (n0 + 255 / 256) and of the one-workgroup kernel (1023 / 1024), beg - 1 / beg
    and [eot]: it wins unless the static mask holds it, then the first runner-up does."""
    sp, smask = K.vocab(V)
    assert K.chunk_size(V) % 32 != 0
    lad, tsl = K.text_ladder(V), [sp["beg"] + 40 + 5 * j for j in range(9)]
    pos = _positions(V)
    assert not set(pos) & set(lad + tsl)
    for i in range(0, len(pos), 8):
        rows = [dict(lg=K.crafted(10 + t % 97, V, [(t, K.TOP)], lad, tsl), expect=lad[0] if smask[t] else t)
                for t in pos[i:i + 8]]
        check_rows(V, OPEN, 0, rows)


@pytest.mark.parametrize("V", VS)
def test_ties(V):
    """Two equal maxima in different chunks: the lower id, first in the candidates too.  Equal text
    and timestamp maxima (the only timestamp, so the mass rule's two sides are equal and it does not
    fire): the text id, as np.argmax."""
    sp, _ = K.vocab(V)
    beg, lad = sp["beg"], K.text_ladder(V)
    a = K.crafted(20, V, [(30000, K.TOP), (1000, K.TOP)], lad)
    b = K.crafted(21, V, [(1000 + 9 * K.chunk_size(V), K.TOP), (1000 + K.chunk_size(V), K.TOP)], lad)
    c = K.crafted(22, V, [(500, K.TOP), (beg + 10, K.TOP)], lad)
    c[beg:beg + 10] = c[beg + 11:] = -np.inf
    toks = check_rows(V, OPEN, 0, [dict(lg=a, expect=1000), dict(lg=b, expect=1000 + K.chunk_size(V)),
                                   dict(lg=c, expect=500)], ties=True)
    assert toks.tolist() == [1000, 1000 + K.chunk_size(V), 500]


@pytest.mark.parametrize("V", VS)
def test_suppress_bits_at_word_and_chunk_edges(V):
    """Suppress bits on the would-be maximum in the last bit of a word, the first bit of the next
    word and in the words that straddle chunk edges 1 and 2 (both sides); the unsuppressed
    neighbours in the same words still win."""
    sp, _ = K.vocab(V)
    cs = K.chunk_size(V)
    w = cs // 32 * 32              # first id of the word that straddles chunk edge 1
    assert w < cs < w + 32 and (2 * cs) % 32 != 0
    extra = [w - 1, w + 32, cs - 1, 2 * cs]
    smask = W.static_mask(V, sp, extra=extra)
    lad = K.text_ladder(V)
    two = lambda a, b_: K.crafted(30 + a % 89, V, [(a, K.TOP), (b_, K.TOP - 1)], lad)
    rows = [dict(lg=two(w - 1, w - 2), expect=w - 2),         # last bit of a word set
            dict(lg=two(w + 32, w + 31), expect=w + 31),      # first bit of the next word set
            dict(lg=two(cs - 1, cs), expect=cs),              # the straddling word, chunk 0's side set
            dict(lg=two(2 * cs, 2 * cs - 1), expect=2 * cs - 1),   # chunk 2's first id set
            dict(lg=two(w, w - 1), expect=w),                 # neighbours of set bits win
            dict(lg=two(cs, cs - 1), expect=cs),
            dict(lg=two(2 * cs + 1, 2 * cs), expect=2 * cs + 1)]
    check_rows(V, OPEN, 0, rows, smask=smask)


def test_minus_inf_entries_and_row_padding():
    """-inf logits in the row (a whole chunk, the row's two ends, every other id of a stretch) are
    not survivors; logits beyond n_vocab in a padded row (ldl > n_vocab) are never read."""
    V = 51865
    sp, _ = K.vocab(V)
    lad, cs = K.text_ladder(V), K.chunk_size(V)
    a = K.crafted(40, V, [(7 * cs + 5, K.TOP)], lad)
    a[5 * cs:6 * cs] = a[0] = a[V - 1] = -np.inf
    a[20000:21000:2] = -np.inf
    b = K.crafted(41, V, [(0, K.TOP)], lad)
    b[1:3000] = -np.inf
    check_rows(V, OPEN, 0, [dict(lg=a, expect=7 * cs + 5), dict(lg=b, expect=0)])
    pad = np.concatenate([np.stack([a, b]), np.full((2, 7), 100.0, np.float32)], axis=1)[None]
    dev, ref = run_tokens(V, pad, OPEN, n_vocab=V)
    check_tokens(dev, ref)
    assert ref["out_tok"][:, 0].tolist() == [7 * cs + 5, 0]


# ---- each mask rule, on and off -----------------------------------------------------------------
@pytest.mark.parametrize("V", (51864, 51866, 1000))
def test_step0_blank_rule(V):
    sp, _ = K.vocab(V)
    eot, lad = sp["eot"], K.text_ladder(V)
    rows = lambda: [dict(lg=K.crafted(50, V, [(eot, K.TOP)], lad)), dict(lg=K.crafted(51, V, [(K.BLANK, K.TOP)], lad))]
    on = R.Prm(suppress_blank=True, max_initial=-1)
    assert check_rows(V, on, 0, rows()).tolist() == [lad[0], lad[0]]          # masked at step 0
    assert check_rows(V, on, 1, rows()).tolist() == [eot, K.BLANK]            # ... and only there
    assert check_rows(V, OPEN, 0, rows()).tolist() == [eot, K.BLANK]          # ... and only when asked


@pytest.mark.parametrize("V", (51865, 1000))
def test_timestamp_pairing_rules(V):
    sp, _ = K.vocab(V)
    beg, eot, lad = sp["beg"], sp["eot"], K.text_ladder(V)
    tsl = [beg + 30 + 4 * j for j in range(9)]   # runners-up among the timestamps
    ts_top = lambda seed: K.crafted(seed, V, [(beg + 20, K.TOP)], lad, tsl)
    # no_ts: every timestamp masked
    assert check_rows(V, R.Prm(no_ts=True), 2, [dict(lg=ts_top(60))]).tolist() == [lad[0]]
    # after two timestamps no timestamp; step 1 counts the missing penultimate as one
    assert check_rows(V, R.Prm(), 2, [dict(lg=ts_top(61), last=beg + 5, pen=beg + 4, has_ts=1, sd=10),
                                      dict(lg=ts_top(62), last=K.TEXT, pen=beg + 4, has_ts=1, sd=8),      # off
                                      dict(lg=ts_top(63), last=K.TEXT, pen=K.TEXT)]).tolist() == [lad[0], beg + 20, beg + 20]
    assert check_rows(V, R.Prm(), 1, [dict(lg=ts_top(64), last=beg + 5, has_ts=1, sd=10),
                                      dict(lg=ts_top(65), last=K.TEXT)]).tolist() == [lad[0], beg + 20]
    # after a lone timestamp only a timestamp or [eot]
    txt = K.crafted(66, V, [(K.TEXT, K.TOP)], tsl)
    txt_eot = K.crafted(67, V, [(K.TEXT, K.TOP), (eot, K.TOP - 1)], tsl)
    assert check_rows(V, R.Prm(), 2, [dict(lg=txt, last=beg + 5, pen=K.TEXT, has_ts=1, sd=10),
                                      dict(lg=txt_eot, last=beg + 5, pen=K.TEXT, has_ts=1, sd=10),
                                      dict(lg=txt, last=K.TEXT, pen=beg + 5, has_ts=1, sd=10)]).tolist() == \
        [tsl[0], eot, K.TEXT]


@pytest.mark.parametrize("V", (51864, 51865, 1000))
@pytest.mark.parametrize("mi", (-1, 0, 50))
def test_max_initial_edge(V, mi):
    """The best timestamp at beg + max_initial is allowed at step 0, the one after it masked; the rule
    is off at step 1 and when max_initial < 0."""
    sp, _ = K.vocab(V)
    beg, lad = sp["beg"], K.text_ladder(V)
    tsl = [beg + 1 + 5 * j for j in range(9)]   # below beg + 50: candidates beside the winner when the rule fires
    at = lambda t, seed: dict(lg=K.crafted(seed, V, [(t, K.TOP)], lad, tsl))
    prm = R.Prm(max_initial=mi)
    if mi < 0:
        assert check_rows(V, prm, 0, [at(beg, 70), at(V - 1, 71)]).tolist() == [beg, V - 1]
    else:
        assert check_rows(V, prm, 0, [at(beg + mi, 72), at(beg + mi + 1, 73), at(V - 1, 74)]).tolist() == \
            [beg + mi, lad[0], lad[0]]
        assert check_rows(V, prm, 1, [at(beg + mi + 1, 75)]).tolist() == [beg + mi + 1]


@pytest.mark.parametrize("V", (51865, 51866))
@pytest.mark.parametrize("sd", (0, 1, 2, 101, 2998))
def test_has_ts_edge(V, sd):
    """With has_ts the best timestamp at beg + seek_delta // 2 - 1 is masked (for seek_delta < 2 that
    id is the suppressed text token below beg) and the one at beg + seek_delta // 2 is allowed; without
    has_ts the same seek_delta masks nothing."""
    sp, _ = K.vocab(V)
    beg, lad = sp["beg"], K.text_ladder(V)
    lo = beg + sd // 2
    tsl = [beg + 1400 + 10 * j for j in range(9)]   # above every limit but the last one's
    at = lambda t, seed, **kw: dict(lg=K.crafted(seed, V, [(t, K.TOP)], lad, tsl), **kw)
    got = check_rows(V, R.Prm(), 2, [at(lo - 1, 80, has_ts=1, sd=sd), at(lo, 81, has_ts=1, sd=sd),
                                     at(max(lo - 1, beg), 82, has_ts=0, sd=sd)])
    assert got.tolist() == [lad[0], lo, max(lo - 1, beg)]


# ---- the timestamp-mass rule --------------------------------------------------------------------
def _mass_row(V, seed, gap):
    """Text maximum 12 at id 300; 400 timestamps 0.02 apart, each below it, whose log-sum-exp over all
    timestamps is 12 + gap."""
    sp, _ = K.vocab(V)
    beg = sp["beg"]
    r = K.crafted(seed, V, [(300, 12.0)])
    r[beg:] -= 20
    ts = np.arange(beg + 700, beg + 1100)
    r[ts] = -0.02 * np.arange(400)
    for _ in range(4):
        v = r[beg:].astype(np.float64)
        r[ts] += np.float32(12.0 + gap - (np.log(np.exp(v - v.max()).sum()) + v.max()))
    assert r[ts].max() < 12.0 - 1
    return r, int(ts[0])


@pytest.mark.parametrize("V", VS)
def test_timestamp_mass_rule(V):
    sp, _ = K.vocab(V)
    beg = sp["beg"]
    over, t0 = _mass_row(V, 90, +0.02)
    under, _ = _mass_row(V, 91, -0.02)
    prm = R.Prm(max_initial=-1)
    # the rule fires on mass alone: the best timestamp, plog before the text mask (checked against W.pick)
    assert check_rows(V, prm, 0, [dict(lg=over), dict(lg=under)]).tolist() == [t0, 300]
    # every timestamp masked (a pair was just closed): no rule, tid = 0
    dev, ref = run_tokens(V, over[None, None], R.Prm(), step=2, history=[[beg + 1, beg + 2, -9]],
                          state=[[1, 4, 2, 0]])
    check_tokens(dev, ref)
    assert dev["out_tok"][0, 2] == 300 and dev["out_tid"][0, 2] == 0


# ---- bookkeeping --------------------------------------------------------------------------------
@pytest.mark.parametrize("V", (51864, 51865))
def test_bookkeeping_scripts(V):
    """The scripted sequences (every branch of W.bookkeep, pinned by
    test_sampler_ref.py::test_driver_reaches_every_branch): states, records of rows that have
    finished (-1 / -inf / -1), a row where nothing survives (-2 / NaN / status 2), steps at or past
    out_cap (nothing written, [eot] fed), forced tokens (fed, not recorded)."""
    sp, _ = K.vocab(V)
    reached = set()
    for g in K.bookkeeping_groups(V):
        lg = K.script_logits(V, g["scripts"], g["S"])
        dev, ref = run_tokens(V, lg, g["prm"], seek=g["seek"], seek_end=g["seek_end"], state=g["state"],
                              forced=g["forced"], out_cap=g["out_cap"], done=g.get("done"))
        assert ref["min_margin"] >= 1e-2
        check_tokens(dev, ref)
        reached |= ref["reached"]
        if g["name"] == "out_cap":
            assert dev["out_tok"].shape == (3, 2) and dev["step"] == 4 and dev["next_tok"].tolist() == [sp["eot"]] * 3
            assert dev["out_tok"][2].tolist() == [-1, -1]   # the row that arrived done
    assert reached == K.REACHED


# ---- step state and embedding -------------------------------------------------------------------
@pytest.mark.parametrize("dtype,B", [("f32", 1), ("bf16", 1), ("f16", 1), ("f32", 5), ("bf16", 5), ("f16", 5),
                                     ("bf16", 64)])
def test_step_state_and_embedding(dtype, B):
    """x = round_dtype(emb[next_tok]) + pos[min(pos0 + Tq, ctx - 1)] bit for bit, below and at the
    clamp; after S steps pos0 += S Tq, step += S, epoch += S and the arrival counter is back at 0."""
    V = 51865
    emb, pos = K.tables(V)
    S = 2 if B == 64 else 3
    scripts = [[2000 + 37 * b + s for s in range(S)] for b in range(B)]
    lg = K.script_logits(V, scripts, S, seed=200 + B)
    for pos0, Tq in ((3, 1), (13 - (S - 2), 1), (12, 2)):
        dev, ref = run_tokens(V, lg, R.Prm(), pos0=pos0, Tq=Tq, dtype=dtype)
        check_tokens(dev, ref)
        last = pos0 + (S - 1) * Tq
        assert (last + Tq < K.CTX - 1) == (pos0 == 3)
        want = R.embed(ref["next_tok"], emb, pos, last, Tq, dtype)
        assert np.array_equal(dev["x"].view(np.uint32), want.view(np.uint32))
        assert (dev["pos0"], dev["step"], dev["epoch"], dev["arrive"]) == (pos0 + S * Tq, S, S, 0)
    assert dev["next_tok"].tolist() == [sc[-1] for sc in scripts]


# ---- temperature sampling -----------------------------------------------------------------------
def _temperature_run(V, T, seed):
    sp, smask = K.vocab(V)
    emb, pos = K.tables(V)
    lg = K.temperature_logits(V, T, seed)
    prm = R.Prm(temperature=T, max_initial=-1, seed=seed)
    dev = D.sample_tokens(lg, _words(V, smask), _dprm(prm), eot=sp["eot"], beg=sp["beg"], blank=K.BLANK, seek=0,
                          seek_end=FAR, emb=emb, pos=pos)
    return lg, prm, dev


@pytest.mark.parametrize("seed", K.SEEDS)
@pytest.mark.parametrize("T", K.TEMPS)
def test_temperature_sampling(T, seed):
    """Every one of the 32 draws of a run (192 over the parameters) lies in the reference draw set (so
    it is never a masked token, nor text when the rule fired) and in the reference CDF interval of
    u01(seed, row, step) widened by DELTA; plog = val[tok] - lse and tid as the reference has them.
    The reference follows the device's own token history, so no draw is excluded."""
    V = 51865 if seed == 7 else 51866
    sp, smask = K.vocab(V)
    lg, prm, dev = _temperature_run(V, T, seed)
    fired = 0
    for b in range(K.T_B):
        w, toks = W.Window(seek_delta=0), []
        for s in range(K.T_S):
            u = R.u01(seed, b, s)
            r = R.sample(lg[s, b], u, s, toks, w, prm, sp, smask, K.BLANK)
            tok = int(dev["out_tok"][b, s])
            assert tok in r["ids"], (b, s, tok, r["tok"])
            j = int(np.searchsorted(r["ids"], tok))
            assert r["lo"][j] - DELTA <= u < r["hi"][j] + DELTA, (b, s, tok, r["tok"], u, r["lo"][j], r["hi"][j])
            val = (lg[s, b] / np.float32(T)).astype(np.float64)
            keep = np.isfinite(val) & ~R.rule_mask(s, toks, w, prm, sp, smask, K.BLANK)
            lse = np.log(np.exp(val[keep] - val[keep].max()).sum()) + val[keep].max()
            if keep[sp["beg"]:].any() and keep[:sp["beg"]].any():   # the rule's comparison is never close
                v = val[sp["beg"]:][keep[sp["beg"]:]]
                assert abs(np.log(np.exp(v - v.max()).sum()) + v.max() - val[:sp["beg"]][keep[:sp["beg"]]].max()) >= 1e-2
            check_plog(dev["out_plog"][b, s], val[tok] - lse)
            ts = np.flatnonzero(keep[sp["beg"]:]) + sp["beg"]
            tid = tok if tok >= sp["beg"] else (int(ts[np.argmax(val[ts])]) if ts.size else 0)
            assert int(dev["out_tid"][b, s]) == tid
            if K.ROW_KINDS[b] == "one":
                assert r["ids"].size == 1 and tok == r["ids"][0]
            if r["rule"]:
                assert tok >= sp["beg"]
                fired += K.ROW_KINDS[b] == "rule"
            toks.append(tok)
            W.bookkeep(w, tok, s, 0, FAR, prm.w(), sp, prm.n_max)
            assert w.status == 0
        assert dev["state"][b].tolist() == [int(w.has_ts), w.seek_delta, w.result_len, 0]
    assert fired >= 2   # the rule rows do draw from timestamps only


def test_temperature_repeats_and_depends_on_seed():
    V, T = 51865, 0.6
    lg, prm, a = _temperature_run(V, T, 7)
    _, _, b = _temperature_run(V, T, 7)
    for key in ("out_tok", "out_plog", "out_tid", "state", "x"):
        assert np.array_equal(a[key].view(np.uint32), b[key].view(np.uint32)), key
    sp, smask = K.vocab(V)
    emb, pos = K.tables(V)
    c = D.sample_tokens(lg, _words(V, smask), _dprm(dataclasses.replace(prm, seed=8)), eot=sp["eot"], beg=sp["beg"],
                        blank=K.BLANK, seek=0, seek_end=FAR, emb=emb, pos=pos)
    flat = [i for i, k in enumerate(K.ROW_KINDS) if k == "flat"]
    assert not np.array_equal(a["out_tok"][flat], c["out_tok"][flat])


# ---- beam ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (1, 5, 8))
def test_beam_candidates(k):
    V = 51865
    sp, _ = K.vocab(V)
    beg, cs = sp["beg"], K.chunk_size(V)
    desc = lambda ids: [(t, K.TOP - j) for j, t in enumerate(ids)]
    one_chunk = K.crafted(300, V, desc([4 * cs + 3 + 300 * j for j in range(9)]))
    per_chunk = K.crafted(301, V, desc([c * cs + 11 * c + 5 for c in (9, 2, 14, 0, 7, 5, 12, 3, 10)]))
    tie = K.crafted(302, V, [(c * cs + 40, K.TOP) for c in (13, 1, 6)] + desc([70 + 3000 * j for j in range(1, 8)])[1:])
    mass, t0 = _mass_row(V, 303, +0.02)
    few = np.full(V, -np.inf, np.float32)
    few[[5 + 5000 * j for j in range(max(k - 2, 0))]] = [K.TOP - j for j in range(max(k - 2, 0))]
    rows = [dict(lg=one_chunk), dict(lg=per_chunk), dict(lg=mass, expect=t0), dict(lg=few)]
    prm = R.Prm(max_initial=-1)
    z4 = np.array([[K.TEXT, K.TEXT, 0, 0]] * 4)
    lg = np.stack([r["lg"] for r in rows])
    for step in (0, 2):
        ids = check_beam(V, lg, prm, z4, step, k, bitwise=True)
        assert ids[0, :k].tolist() == [4 * cs + 3 + 300 * j for j in range(k)]
        assert ids[1, :k].tolist() == [c * cs + 11 * c + 5 for c in (9, 2, 14, 0, 7, 5, 12, 3, 10)][:k]
        assert (ids[2, :k] >= beg).all() and ids[2, 0] == t0         # the rule fired: timestamps only
        assert ids[3, :k].tolist() == ([5 + 5000 * j for j in range(k - 2)] + [-1, -1])[:k]   # k - 2 survivors
    ids = check_beam(V, tie[None], prm, z4[:1], 2, k, ties=True, bitwise=True)
    assert ids[0, :k].tolist() == ([c * cs + 40 for c in (1, 6, 13)] + [70 + 3000 * j for j in range(2, 8)])[:k]
    # step 0 with blank suppression: [eot] and the blank token leave the candidates
    blank = K.crafted(304, V, [(sp["eot"], K.TOP), (K.BLANK, K.TOP - 0.5)] + desc(K.text_ladder(V))[1:])
    on, off = R.Prm(max_initial=-1), R.Prm(max_initial=-1, suppress_blank=False)
    assert check_beam(V, blank[None], on, z4[:1], 0, k, bitwise=True)[0, 0] == K.text_ladder(V)[1]
    assert check_beam(V, blank[None], off, z4[:1], 0, k, bitwise=True)[0, 0] == sp["eot"]
    assert check_beam(V, blank[None], on, z4[:1], 1, k, bitwise=True)[0, 0] == sp["eot"]


@pytest.mark.parametrize("k", (0, 9))
@pytest.mark.parametrize("chunked", (0, 1))
def test_beam_k_out_of_range(k, chunked):
    V = 1000
    sp, smask = K.vocab(V)
    with pytest.raises(TranscriptionError) as e:
        D.sample_beam(K.base(1, V), _words(V, smask), D.SampleParams(), eot=sp["eot"], beg=sp["beg"], blank=K.BLANK,
                      row=[[0, 0, 0, 0]], step=0, k=k, chunked=chunked)
    assert e.value.status == L.SPT_ERR_INVALID_ARG and "1..8 candidates" in str(e.value)


# ---- K/V gather ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ("f32", "bf16", "f16"))
@pytest.mark.parametrize("pos0", (0, 1, 7, 16))
def test_kv_gather(dtype, pos0):
    """Positions below pos0 take the source row's values, positions at or above keep dst's pre-fill,
    bit for bit."""
    Ln, B, H, ctx = 2, 5, 3, 16
    rows = [3, 3, 0, 4, 1]
    g = np.random.default_rng(pos0)
    src = g.standard_normal((Ln, 2, B, H, ctx, 64)).astype(np.float32)
    dst = g.standard_normal((Ln, 2, B, H, ctx, 64)).astype(np.float32) + 100
    got = D.kv_gather(src, dst, rows, pos0, dtype)
    want = R.kv_gather(src, dst, rows, pos0, dtype)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(got[:, :, :, :, pos0:], R.round_dtype(dst, dtype)[:, :, :, :, pos0:])
    if pos0:
        assert np.array_equal(got[:, :, 1, :, :pos0], R.round_dtype(src, dtype)[:, :, 3, :, :pos0])


# ---- hook errors --------------------------------------------------------------------------------
def test_hook_argument_errors():
    V = 1000
    sp, smask = K.vocab(V)
    emb, pos = K.tables(V)
    kw = dict(eot=sp["eot"], beg=sp["beg"], blank=K.BLANK, seek=0, seek_end=FAR, emb=emb, pos=pos)
    big = np.zeros((1, 1, 53249), np.float32)
    cases = [(dict(logits=np.zeros((1, 1, 8), np.float32), n_vocab=0), "empty vocabulary"),
             (dict(logits=big, n_vocab=53249), "above 53248"),
             (dict(logits=K.base(1, V)[None], n_vocab=V + 1), "ldl below"),
             (dict(logits=np.zeros((1, 0, V), np.float32)), "rows"),
             (dict(logits=None, n_vocab=V), "null")]
    for a, msg in cases:
        with pytest.raises(TranscriptionError) as e:
            D.sample_tokens(a.pop("logits"), _words(V, smask), D.SampleParams(), **kw, **a)
        assert e.value.status == L.SPT_ERR_INVALID_ARG and msg in str(e.value), (msg, e.value)
