"""The cases of tests/test_gpu_gemv.py and tests/test_gemv_ref.py: shapes, seeded inputs and, through
tests/gemv_ref.py, what each launch must return.  A case is a dict; build(case) gives the keyword arguments
of spittle_amd.gemv_debug.gemv (kw) and the arrays the reference needs; expect(case, built, dtype) the
reference outputs and bars.

Shapes are the smallest at which each path of dec_gemv.h exists (K for the 16-bit dtypes; f32 has 64-element
super-steps, so half the K gives the same count): 1 super-step, 3 (tiny.en), 10 and 12 (the exact 10- and
12-wave shapes), 8 / 16 (four and eight waves); R = 1, 5, 17: one row, more rows than four waves, more rows
than 8 / 10 / 12 waves (the second-round rows reload their slabs) and two row groups; N = 40 has a ragged
last tile, 192 = 3 x 64 is the smallest QKV, 4112 = 4096 + 16 takes the two-tile shapes, 1000 leaves a
logits tile of 8 columns."""
from __future__ import annotations

import numpy as np

from tests import gemv_ref as R

LN_PAIRS = [("qkv_cache", 0), ("qkv_cache", 1), ("qkv_cache", 2), ("qkv_cache", 4), ("bias", 0), ("bias", 2),
            ("bias_gelu", 0), ("logits", 0), ("logits", 1), ("logits", 2), ("logits", 4)]
K16_PEND = (128, 384, 1280, 1536)
K32 = (64, 256, 640, 768, 1024)
ROWS = (1, 5, 17)
ATTN_H = (2, 12, 20, 24)
ATTN_S = (2, 3, 4, 8)
CACHE_GEOM = ((1, 1, 0, 1), (2, 3, 5, 16), (5, 4, 0, 8), (3, 1, 15, 16), (16, 4, 2, 8))   # B, Tq, pos0, ctx
CACHE_H = (2, 6)
TIE_GROUPS = ((33, 38), (70, 130), (200, 201, 520), (49, 54), (86, 146), (216, 217, 536))
MASKS = ("none", "half", "all_but_one", "one_tile", "last_word")
# the decoder's (mode, A source) pairs (SPT_GV_PAIRS of dec_gemv.h), n_pend / S as the third entry
PAIRS = [(m, "ln", n) for m, n in LN_PAIRS] + [("partial", "direct", 0), ("bias_resid", "direct", 0)] + \
        [("bias_resid", "attn", s) for s in ATTN_S]


def pend_k(dtype):
    return K32 if dtype == "f32" else K16_PEND


def _seed(c):
    return [sum(ord(ch) for ch in c["mode"] + c["a_src"]), c["K"], c["N"], c["R"], c.get("n_pend", 0), c.get("S", 0),
            c.get("seed", 0)]


def case(mode, a_src, K, N, Rr, **kw):
    c = dict(mode=mode, a_src=a_src, K=K, N=N, R=Rr)
    c.update(kw)
    c["id"] = "-".join(f"{k}{v}" for k, v in c.items() if k not in ("mode", "a_src")) + f"-{mode}-{a_src}"
    return c


def pend_case(mode, n_pend, K, Rr, N=None, **kw):
    if mode == "qkv_cache":   # one token per sequence appended at position 2 of 4
        return case(mode, "ln", K, 192 if N is None else N, Rr, n_pend=n_pend, B=Rr, Tq=1, pos0=2, ctx=4, H=1, **kw)
    return case(mode, "ln", K, 40 if N is None else N, Rr, n_pend=n_pend, **kw)


class Built:
    pass


def make_partials(rng, Rr, H, S):
    """Random o, m spread over +-30, l > 0; (row 0, head 0): chunk 1 empty (m = -inf, l = 0, o = NaN: what an
    unwritten chunk may hold -- it must be skipped, not multiplied by zero); (last row, last head): all mass in
    the last chunk (the others 60 below it).  Never all chunks empty: the engine cannot produce that (every
    query sees at least its own key block), and O / L would be 0 / 0."""
    p = np.zeros((Rr, H, S, 66), np.float32)
    p[..., :64] = rng.standard_normal((Rr, H, S, 64))
    p[..., 64] = rng.uniform(-30, 30, (Rr, H, S))
    p[..., 65] = rng.uniform(0.5, 40.0, (Rr, H, S))
    p[0, 0, 1, :64] = np.nan
    p[0, 0, 1, 64] = -np.inf
    p[0, 0, 1, 65] = 0.0
    p[-1, -1, :, 64] = -30.0
    p[-1, -1, -1, 64] = 30.0
    # ... with o = +1 in that chunk and -1 in the others, l = 1: the merge gives +1 there, a merge without
    # the 2^(m_c - M) weights (2 - S) / S <= 0 (output column 2 reads these 64 columns alone: build())
    p[-1, -1, :, :64] = -1.0
    p[-1, -1, -1, :64] = 1.0
    p[-1, -1, :, 65] = 1.0
    return p


def make_mask(rng, N, kind):
    """The suppression words (ceil(N / 32) of them; the last is partial for N = 1000: 8 bits in use)."""
    bits = np.zeros(((N + 31) // 32) * 32, bool)
    if kind == "half":
        bits[:N] = rng.integers(0, 2, N).astype(bool)
    elif kind == "all_but_one":
        bits[:N] = True
        bits[N // 2 + 3] = False
    elif kind == "one_tile":
        bits[16 * 5:16 * 6] = True
    elif kind == "last_word":
        bits[(N // 32) * 32:N] = True
        bits[N - 3] = False
    w = np.zeros(bits.size // 32, np.uint32)
    for j in range(32):
        w |= bits[j::32].astype(np.uint32) << np.uint32(j)
    return w


def build(c) -> Built:
    b = Built()
    b.case = c
    rng = np.random.default_rng(_seed(c))
    K, N, Rr = c["K"], c["N"], c["R"]
    b.W = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    b.bias = None if c["mode"] == "logits" else rng.uniform(-0.5, 0.5, N).astype(np.float32)
    kw = dict(mode=c["mode"], a_src=c["a_src"], R=Rr, N=N, K=K, bias=b.bias)
    b.lda = c.get("lda", K)
    b.a_row0 = c.get("a_row0", 0)
    b.pend = b.A = b.apart = b.ln_w = b.ln_b = b.resid = b.p_resid = None
    if c["a_src"] in ("direct", "ln"):
        n_a = (Rr - 1) * b.lda + b.a_row0 + K + c.get("a_tail", 0)
        A = rng.standard_normal(n_a).astype(np.float32)
        if c["a_src"] == "ln":
            rows = np.arange(n_a) // max(b.lda, 1)
            A = (A * (0.5 + (rows % 5)) + 0.25 * (rows % 3 - 1)).astype(np.float32)
        if c.get("poison_other_rows"):   # everything outside the rows in use is huge: it must not show
            use = np.zeros(n_a, bool)
            use[((np.arange(Rr)[:, None] * b.lda + b.a_row0) + np.arange(K)[None, :]).ravel()] = True
            A[~use] = 3.0e4 * np.where(rng.integers(0, 2, int((~use).sum())), 1.0, -1.0)
        b.A = A
        kw.update(A=A, lda=b.lda, a_row0=b.a_row0)
    if c["a_src"] == "ln":
        b.ln_w = rng.uniform(0.5, 1.5, K).astype(np.float32)
        b.ln_b = rng.uniform(-0.25, 0.25, K).astype(np.float32)
        n_pend = c.get("n_pend", 0)
        # slabs of A's size, of the order of A: every one moves the rows far beyond any bar
        b.pend = rng.standard_normal((n_pend, b.A.size)).astype(np.float32) if n_pend else None
        if n_pend:
            # the probe of a dropped slab (a random slab moves a random output by less than 100 of the
            # 16-bit bars): 16 columns of row 0 hold +-40 in x, and the last slab cancels them to exactly 0
            # with the other slabs; output column 0 reads those columns alone.  True image there: about
            # ln_b; with the last slab dropped: several units, every product positive.
            P = b.a_row0 + 3 + (K // 16) * np.arange(16)
            sgn = np.where(np.arange(16) % 2 == 0, 1.0, -1.0).astype(np.float32)
            b.A[P] = 40.0 * sgn
            b.pend[-1][P] = -R.sum_f32(b.A, b.pend[:-1])[P]
            b.W[0] = 0.0
            b.W[0, P - b.a_row0] = 0.25 * sgn
        kw.update(ln_w=b.ln_w, ln_b=b.ln_b, pend=b.pend, n_pend=n_pend, x_out=c.get("x_out", True))
    if c["a_src"] == "attn":
        b.apart = make_partials(rng, Rr, c["H"], c["S"])
        b.W[2] = 0.0
        b.W[2, K - 64:] = 0.125
        kw.update(apart=b.apart, S=c["S"], H=c["H"], merge_first=c.get("merge_first", False))
    b.ldc = c.get("ldc", 64 * c["H"] if c["mode"] == "qkv_cache" else N)
    ncol = 64 * c["H"] if c["mode"] == "qkv_cache" else N
    item = (Rr - 1) * b.ldc + ncol
    ks = c.get("ksplit", 1)
    b.c_split = c.get("c_split", item + 8 if ks > 1 else 0)
    b.c_count = (ks - 1) * b.c_split + item + c.get("c_tail", 4)
    kw.update(ldc=b.ldc, ksplit=ks, c_split=b.c_split)
    b.c_idx = ((np.arange(Rr)[:, None] * b.ldc) + np.arange(ncol)[None, :])   # [R][ncol] into one slab of C
    if c["mode"] == "bias_resid":
        b.C_in = rng.standard_normal(b.c_count).astype(np.float32)
        b.resid = b.C_in[b.c_idx]
        kw.update(C_in=b.C_in)
    else:
        kw.update(c_count=b.c_count)
    if c["mode"] == "partial" and c.get("resid"):
        pr = rng.standard_normal((Rr, b.ldc)).astype(np.float32)
        b.p_resid = pr
        b.resid = pr[:, :N]
        kw.update(p_resid=pr)
    if c["mode"] == "qkv_cache":
        kw.update(B=c["B"], Tq=c["Tq"], cache_H=c["H"], ctx=c["ctx"], pos0=c["pos0"])
        if c.get("probe"):
            # far above 100 bars apart: k and v (bias +-8 on column 3 of head 0), and the rows (column 5 of
            # every row holds +-20 by the row's parity; k column 7 of head 0 reads that column alone)
            d = 64 * c["H"]
            b.bias[d + 3], b.bias[2 * d + 3] = 8.0, -8.0
            b.A[np.arange(Rr) * b.lda + b.a_row0 + 5] = np.where(np.arange(Rr) % 2 == 0, 20.0, -20.0)
            b.W[d + 7] = 0.0
            b.W[d + 7, 5] = 1.0
        if c.get("clamp"):   # one k and one v column beyond +-65504: f16's to_cache clamps, the others store it
            d = 64 * c["H"]
            b.bias[d + 5] = 1.0e5
            b.bias[2 * d + 9] = -1.0e5
    if c["mode"] == "logits":
        b.mask = make_mask(rng, N, c.get("mask", "none"))
        b.step = c.get("step", 0)
        b.blank0, b.blank1 = c.get("blank0", -1), c.get("blank1", -1)
        v_ln = R.rows_of(R.sum_f32(b.A, b.pend), Rr, b.lda, b.a_row0, K).astype(np.float64)
        img = R.layernorm(v_ln, b.ln_w, b.ln_b)
        if c.get("poison_other_rows") and b.a_row0:
            # the probe of an ignored a_row0: column 1 follows the signs of the (huge) row the fault would read
            b.W[1] = (np.sign(b.A[:K]) / np.sqrt(K)).astype(np.float32)
        if c.get("blank") == "winners":
            # columns 100 and 900 follow the signs of row 0's and the last row's image (16 / K in size: about
            # +13 there): each wins its row by far unless the blank rule suppresses it
            b.W[100] = (np.sign(img[0]) * (16.0 / K)).astype(np.float32)
            b.W[900] = (np.sign(img[-1]) * (16.0 / K)).astype(np.float32)
        if c.get("ties"):
            # duplicate rows of W give exactly equal logits: inside tile 2 (columns 33, 38), across tiles
            # (columns 70, 130) and a triple (200, 201, 520); scaled up so that they are the row's largest
            # (signs of row 0's LayerNorm image, 16 / K in size: about +13 in row 0, of either sign below it)
            big = (np.sign(img[0]) * (16.0 / K)).astype(np.float32)
            # and each group's negation 16 columns on, so that whatever the sign of big . a one of the two
            # is its tile's best
            for n in (33, 38, 70, 130):
                b.W[n], b.W[n + 16] = big, -big
            for n in (200, 201, 520):
                b.W[n], b.W[n + 16] = big * np.float32(0.5), -big * np.float32(0.5)
        kw.update(suppress=b.mask, blank0=b.blank0, blank1=b.blank1, step=b.step)
    b.kw = kw
    return b


def expect(b: Built, dtype: str, fault=None):
    """Reference outputs of the launch: dict with C (ref, bar in the shape of b.c_idx, or [ksplit] of them),
    x (the float32-summed flat rows) and cache (ref, bar, written)."""
    c = b.case
    a, da, x = R.image(c["a_src"], dtype, A=b.A, R=c["R"], K=c["K"], lda=b.lda, a_row0=b.a_row0, pend=b.pend,
                       ln_w=b.ln_w, ln_b=b.ln_b, apart=b.apart, fault=fault)
    out = dict(x=x, a=a)
    mode = c["mode"]
    if mode == "partial":
        out["C"] = R.partial_slabs(a, da, b.W, dtype, c.get("ksplit", 1), b.bias, b.resid)
        return out
    y, lin = R.linear(a, da, b.W, dtype, b.bias, b.resid if mode == "bias_resid" else None)
    if mode in ("logits", "bias_resid"):
        out["C"] = (y, lin)
    elif mode == "bias_gelu":
        out["C"] = R.gelu_out(y, lin, dtype)
    elif mode == "bias":
        out["C"] = R.stored(y, lin, dtype)
    else:
        d = 64 * c["H"]
        out["C"] = R.stored(y[:, :d], lin[:, :d], dtype)
        yb = R.stored(np.clip(y, -R.F16_MAX, R.F16_MAX) if dtype == "f16" else y, lin, dtype)
        out["cache"] = R.cache_ref(yb[0], yb[1], c["B"], c["Tq"], c["H"], c["ctx"], c["pos0"], dtype, fault)
    return out


# ------------------------------------------------------------------------------------------ case lists
def logits_cases():
    out = []
    for K in (384, 1280):
        for Rr in (1, 5):
            for i, mask in enumerate(MASKS):
                # Tq = 3 rows per sequence, the last one read (the final LayerNorm's row selection), the
                # other rows huge
                out.append(case("logits", "ln", K, 1000, Rr, n_pend=(0, 1, 2, 4, 0)[i], lda=3 * K, a_row0=2 * K,
                                poison_other_rows=True, mask=mask, seed=i))
            for step in (0, 1):
                out.append(case("logits", "ln", K, 1000, Rr, n_pend=0, lda=3 * K, a_row0=2 * K, poison_other_rows=True,
                                mask="none", step=step, blank="winners", blank0=100, blank1=900))
            out.append(case("logits", "ln", K, 1000, Rr, n_pend=0, lda=3 * K, a_row0=2 * K, poison_other_rows=True,
                            mask="none", ties=True))
    return out


def attn_cases(dtype):
    if dtype == "f32":   # H = 12: K = 768, the exact 12-wave shape
        return [case("bias_resid", "attn", 768, 40, Rr, H=12, S=S, merge_first=S == 8) for S in ATTN_S for Rr in ROWS]
    return [case("bias_resid", "attn", 64 * H, 40, Rr, H=H, S=S, merge_first=S == 8)
            for H in ATTN_H for S in ATTN_S for Rr in ROWS]


def cache_cases():
    out = []
    for H in CACHE_H:
        for i, (B, Tq, pos0, ctx) in enumerate(CACHE_GEOM):
            out.append(case("qkv_cache", "ln", 64 * H, 192 * H, B * Tq, n_pend=(0, 1, 2, 4, 0)[i], B=B, Tq=Tq, pos0=pos0,
                            ctx=ctx, H=H, clamp=i == 1, probe=True))
    return out


def direct_cases(dtype):
    if dtype == "f32":
        out = [case(m, "direct", K, 40, Rr, ldc=48, resid=True) for m in ("partial", "bias_resid") for K in K32
               for Rr in ROWS]
        out.append(case("partial", "direct", 2048, 40, 5, ksplit=4, resid=True))
        return out
    out = [case(m, "direct", K, 40, Rr, ldc=48, resid=True) for m in ("partial", "bias_resid")
           for K in (128, 1280, 1536, 5120) for Rr in ROWS]
    out.append(case("partial", "direct", 5120, 40, 5, ksplit=4, resid=True))
    out.append(case("bias_resid", "direct", 384, 40, 5, lda=3 * 384, a_row0=384, poison_other_rows=True))
    return out


# ------------------------------------------------------------------------------------------ the step hook
STEP_TILES = (1, 63, 1024, 1025, 3242)
STEP_B = (1, 5, 64)


def step_inputs(n_tiles, B, d, *, n_steps=3, seed=0, Tq=1, ctx=16, pos0=3, step0=0, out_cap=8, ignore_eot=False):
    """Partials [n_steps][B][n_tiles] of a vocabulary of 16 n_tiles - 8 tokens with, per (step, sequence), a
    unique winner, except the crafted rows below; eot is token 7 (tile 0) when the vocabulary allows."""
    rng = np.random.default_rng([seed, n_tiles, B, d])
    n_vocab = 16 * n_tiles - 8
    eot = min(7, n_vocab - 1)
    v1 = rng.standard_normal((n_steps, B, n_tiles)).astype(np.float32)
    v2 = (v1 - rng.uniform(0.01, 1.0, v1.shape)).astype(np.float32)
    i1 = (16 * np.arange(n_tiles)[None, None, :] + rng.integers(0, 8, v1.shape)).astype(np.int64)
    o = dict(n_tiles=n_tiles, B=B, d=d, n_steps=n_steps, Tq=Tq, ctx=ctx, n_vocab=n_vocab, eot=eot, out_cap=out_cap,
             ignore_eot=ignore_eot, state=(pos0, step0, 41, 0))
    o["emb"] = rng.standard_normal((n_vocab, d)).astype(np.float32)
    o["pos"] = rng.standard_normal((ctx, d)).astype(np.float32)
    o["forced"] = None
    o["done"] = np.zeros(B, np.int32)
    o["v"] = (v1, i1, v2)
    return o


def step_parts(o):
    return R.parts_words(*o["v"])
