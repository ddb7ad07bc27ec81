"""float64 reference of the Parakeet encoder kernels and of the TDT decode step on the inputs the
spt_debug_pk_* hooks take, with their error bars.  Shared by tests/test_pk_ref.py (CPU: the reference against torch float64,
each case's preconditions and sensitivity) and tests/test_gpu_pk_kernels.py (the kernels against it).

It states the arithmetic contract from the dtype-rounded inputs and knows no tile, wave, block or skew.
Its one intermediate rounding is the MFMA attention kernel's documented one, round_f16(f32(q) + u) and
round_f16(f32(q) + v) (mfma=True); the VALU kernel has none.  fault=... recomputes with a named fault."""
from __future__ import annotations

import numpy as np

from tests.attn_ref import half_ulp, round_dtype  # noqa: F401  (re-exported)

U32 = 2.0 ** -24          # half an ulp of f32, relative: one rounding
ULP1 = 2.0 ** -23         # one f32 ulp, relative: v_exp_f32, v_rcp_f32, expf (DESIGN 9.8 names the sources)
BN_EPS = 1e-5


def halve(n):
    return (n - 1) // 2 + 1


# ------------------------------------------------------------------------------------------ subsampling
def conv3x3s2(x, w, bias, t_valid, relu):
    """x [B][T][F][C] float64 (frames >= t_valid[b] read as zero), w [C][3][3], bias [C] ->
    y [B][halve(T)][halve(F)][C]: the depthwise 3 x 3, stride 2, padding 1 convolution (conv0: C copies of the
    one input channel), ReLU optional."""
    x = np.asarray(x, np.float64)
    B, T, F, C = x.shape
    w = np.asarray(w, np.float64).reshape(C, 3, 3)
    To, Fo = halve(T), halve(F)
    xp = np.zeros((B, T + 2, F + 2, C))
    for b in range(B):
        n = min(int(t_valid[b]), T)
        xp[b, 1:1 + n, 1:1 + F] = x[b, :n]
    y = np.zeros((B, To, Fo, C)) + np.asarray(bias, np.float64)
    for i in range(3):
        for j in range(3):
            y += w[:, i, j] * xp[:, i:i + 2 * To:2, j:j + 2 * Fo:2]
    return np.maximum(y, 0.0) if relu else y


def conv0(mel, lens, w, bias, col=0, shift=0):
    """pk_conv0: mel [B][Tp][F] -> [B][To][Fo][C].  Faults: col (the lens column read), shift (taps moved)."""
    mel = np.asarray(mel, np.float64)
    C = len(bias)
    w = np.roll(np.asarray(w, np.float64).reshape(C, 3, 3), shift, 1) if shift else w
    return conv3x3s2(np.repeat(mel[..., None], C, -1), w, bias, np.asarray(lens)[:, col], True)


def dwconv(x, lens, stage, w, bias, shift=0):
    C = len(bias)
    w = np.roll(np.asarray(w, np.float64).reshape(C, 3, 3), shift, 1) if shift else w
    return conv3x3s2(x, w, bias, np.asarray(lens)[:, stage], False)


# --------------------------------------------------------------------------------------- conv module
def sigmoid(x):
    with np.errstate(over="ignore"):  # exp(+large) = inf: the sigmoid is 0
        return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


def conv_module(a, lens, dw_w, dw_b, bn_g, bn_b, bn_m, bn_v, Tp, fault=None, parts=False):
    """a [B * Tp][2 d] -> GLU -> depthwise 9 taps over the frames [0, T3_b) (others zero) -> BatchNorm
    (eval, eps 1e-5) -> Swish -> [B * Tp][d]; rows t >= T3_b are zero.
    Faults: `shift` (taps moved by one frame), `tp_valid` (Tp for T3 in the validity test), `lens_col`
    (column 2 read).  parts=True also returns (z, sum |w g| + |b|) for the bar."""
    a = np.asarray(a, np.float64)
    B = len(lens)
    d = a.shape[1] // 2
    a = a.reshape(B, Tp, 2 * d)
    w = np.asarray(dw_w, np.float64).reshape(d, 9)
    out, zs, mags = np.zeros((B, Tp, d)), np.zeros((B, Tp, d)), np.zeros((B, Tp, d))
    s = np.asarray(bn_g, np.float64) / np.sqrt(np.asarray(bn_v, np.float64) + BN_EPS)
    sh = 1 if fault == "shift" else 0
    for b in range(B):
        T3 = int(np.asarray(lens)[b, 2 if fault == "lens_col" else 3])
        T3 = min(T3, Tp)
        nv = Tp if fault == "tp_valid" else T3
        g = np.zeros((Tp + 8 + 2, d))
        g[5:5 + nv] = a[b, :nv, :d] * sigmoid(a[b, :nv, d:])
        acc = np.zeros((Tp, d)) + np.asarray(dw_b, np.float64)
        mag = np.zeros((Tp, d)) + np.abs(np.asarray(dw_b, np.float64))
        for j in range(9):
            acc += w[:, j] * g[1 + j + sh:1 + j + sh + Tp]
            mag += np.abs(w[:, j] * g[1 + j + sh:1 + j + sh + Tp])
        z = (acc - np.asarray(bn_m, np.float64)) * s + np.asarray(bn_b, np.float64)
        out[b, :T3] = (z * sigmoid(z))[:T3]
        zs[b, :T3], mags[b, :T3] = z[:T3], mag[:T3]   # rows t >= T3 are exact zeros: no bar
    out = out.reshape(B * Tp, d)
    return (out, zs.reshape(B * Tp, d), mags.reshape(B * Tp, d)) if parts else out


def conv_module_bar(a, z, mag, bn, dtype):
    """Per element.  GLU: x * rcp(1 + exp2(-log2e g)): one rounding of the exponent (ln 2 |g log2 e| U32 on
    the power), v_exp, one add, v_rcp, one product: (|g| + 2) U32 + 2 ULP1 relative, so each tap's g carries
    that; the 9 fma and the bias add 10 U32 on sum |w g| + |b|.  BatchNorm: s = g / sqrt(v + eps) (3 roundings
    and the f32 constant 1e-5f), t = b - m s (2), z = acc s + t (2, of which s and t each carry theirs):
    |dz| <= |s| dacc + 6 U32 (|acc s| + |m s| + |b|).  Swish(z) = z sigmoid(z):
    d/dz bounded by 1.1, plus (|z| + 2) U32 + 2 ULP1 relative of its own.  x 4 for second-order terms, plus half
    an ulp of a 16-bit output and 2^-126 for a flushed subnormal."""
    g, b, m, v = (np.asarray(x, np.float64) for x in bn)
    s = np.abs(g / np.sqrt(v + BN_EPS))
    gmax = np.abs(np.asarray(a, np.float64)[:, a.shape[1] // 2:]).max()
    glu_rel = (gmax + 2) * U32 + 2 * ULP1
    dacc = (glu_rel + 10 * U32) * mag
    # |acc| <= mag
    dz = s * dacc + 6 * U32 * (mag * s + np.abs(m) * s + np.abs(b))
    sw = z * sigmoid(z)
    lin = 1.1 * dz + ((np.abs(z) + 2) * U32 + 2 * ULP1) * np.abs(sw)
    return 4 * lin + half_ulp(sw, dtype) + 2.0 ** -126


# --------------------------------------------------------------------------------------------- relpos
def relpos(Tp, d):
    """pe [2 Tp - 1][d]: row r is position Tp - 1 - r; columns (2k, 2k + 1) = sin, cos(pos * 10000^(-2k / d))."""
    pos = (Tp - 1 - np.arange(2 * Tp - 1, dtype=np.float64))[:, None]
    div = np.exp(-(2.0 * np.arange(d // 2, dtype=np.float64)) * np.log(10000.0) / d)[None, :]
    pe = np.zeros((2 * Tp - 1, d))
    pe[:, 0::2] = np.sin(pos * div)
    pe[:, 1::2] = np.cos(pos * div)
    return pe


def relpos_bar(Tp, d, pe, dtype):
    """The kernel computes in double and rounds to f32, then to dtype: half an f32 ulp of the value, half an
    ulp of dtype, and the double evaluation itself: the argument pos * div carries a few 2^-53 relative (exp,
    log, the products: 8 taken), i.e. 8 * 2^-53 * Tp absolute on sin / cos, which have unit slope."""
    return np.abs(pe) * U32 + half_ulp(pe, dtype) + 8 * 2.0 ** -53 * Tp + 2.0 ** -126


# ------------------------------------------------------------------------------------------ attention
def f16_add(q, u):
    """round_f16(f32(q) + u): the MFMA kernel's (q + u) operand."""
    return (np.asarray(q, np.float32) + np.asarray(u, np.float32)).astype(np.float16).astype(np.float64)


def rel_attn(qkv, p, pu, pv, lens, *, B, Tp, H, dk, ldp, p_off=0, p_bstride=0, mfma=False, fault=None, parts=False):
    """qkv [B * Tp][3 d] (q | k | v), p flat with row r of utterance b at p_off + b p_bstride + r ldp, pu / pv
    [H][dk], lens [B][4] -> out [B * Tp][d] float64:
        ac[i][j] = (q_i + u) . k_j,  bd[i][j] = (q_i + v) . p[Tp - 1 - i + j],
        softmax over j < T3_b of (ac + bd) / sqrt(dk), times V; rows i >= T3_b are zero.
    Faults: skew+1 / skew-1 (the relative index off by one), clamp_early (the position rows clamped one row
    inside the table), drop_last, admit_one (key T3 admitted), read_pad (every key below Tp admitted), swap_uv,
    no_scale, lens_col (column 2 for T3), p_col0 (the column offset ignored), p_shared (p_bstride ignored).
    parts=True returns a dict: out, and per (utterance, row, head) amax = sum_e |qu k| + |qv p| maximised over
    the keys (before the scale), vmax = max |v| over the visible keys, nvis = their count, arg = the best
    key, gap = its lead over the second, smax = max |score|."""
    d = H * dk
    qkv = np.asarray(qkv, np.float64).reshape(B, Tp, 3 * d)
    p = np.asarray(p, np.float64).reshape(-1)
    pu = np.asarray(pu, np.float64).reshape(H, dk)
    pv = np.asarray(pv, np.float64).reshape(H, dk)
    if fault == "swap_uv":
        pu, pv = pv, pu
    if fault == "p_col0":
        p_off = 0
    if fault == "p_shared":
        p_bstride = 0
    nr = 2 * Tp - 1
    out = np.zeros((B, Tp, d))
    amax, vmax, nvis, gap, smax = (np.zeros((B, Tp, H)) for _ in range(5))
    arg = np.full((B, Tp, H), -1, np.int64)
    scale = 1.0 if fault == "no_scale" else 1.0 / np.sqrt(dk)
    for b in range(B):
        T3 = int(np.asarray(lens)[b, 2 if fault == "lens_col" else 3])
        T3 = max(0, min(T3, Tp))
        nk = {"drop_last": max(T3 - 1, 0), "admit_one": min(T3 + 1, Tp), "read_pad": Tp}.get(fault, T3)
        if T3 == 0 or nk == 0:
            continue
        base = p_off + b * p_bstride
        rows = base + np.arange(nr)[:, None] * ldp
        for h in range(H):
            cs = slice(h * dk, (h + 1) * dk)
            q = qkv[b, :T3, cs]
            k = qkv[b, :nk, d + h * dk:d + (h + 1) * dk]
            v = qkv[b, :nk, 2 * d + h * dk:2 * d + (h + 1) * dk]
            ph = p[rows + h * dk + np.arange(dk)[None, :]]     # [nr][dk]
            if mfma:
                qu, qv = f16_add(q, pu[h]), f16_add(q, pv[h])
            else:
                qu, qv = q + pu[h], q + pv[h]
            ridx = Tp - 1 - np.arange(T3)[:, None] + np.arange(nk)[None, :]
            ridx = ridx + {"skew+1": 1, "skew-1": -1}.get(fault, 0)
            lo, hi = (1, nr - 2) if fault == "clamp_early" else (0, nr - 1)
            ridx = np.clip(ridx, lo, max(hi, lo))
            G = qv @ ph.T                                       # [T3][nr]
            s = (qu @ k.T + np.take_along_axis(G, ridx, 1)) * scale
            e = np.exp(s - s.max(1, keepdims=True))
            out[b, :T3, cs] = (e @ v) / e.sum(1, keepdims=True)
            if parts:
                Ga = np.abs(qv) @ np.abs(ph).T
                amax[b, :T3, h] = (np.abs(qu) @ np.abs(k).T + np.take_along_axis(Ga, ridx, 1)).max(1)
                vmax[b, :T3, h] = np.abs(v).max()
                nvis[b, :T3, h] = nk
                arg[b, :T3, h] = s.argmax(1)
                top = np.sort(s, 1)
                gap[b, :T3, h] = top[:, -1] - top[:, -2] if nk > 1 else np.inf
                smax[b, :T3, h] = np.abs(s).max(1)
    out = out.reshape(B * Tp, d)
    if parts:
        return dict(out=out, amax=amax, vmax=vmax, nvis=nvis, arg=arg, gap=gap, smax=smax)
    return out


def rel_attn_bar(ref, amax, vmax, nvis, *, dk, dtype, mfma, **_):
    """[B * Tp][d], following DESIGN 2c.  VALU (f32 arithmetic from exact conversions): q + u (1 rounding),
    dk fma per dot product, ac + bd, the scale, s - max: |ds| <= (dk + 4) U32 (sum |qu k| + |qv p|) / sqrt(dk);
    a probability moves by 2 |ds| relative (numerator and denominator), expf is within 1 ulp (ULP1), one
    accumulation per key in l and in P.V, one division.  MFMA (f16): the same chain on f32 accumulators (the
    adds of q + u are the reference's), v_exp_f32 within 1 ulp, one rescale of l and o per 32-key tile; P is
    rounded to f16 before P.V (numerator only: 2^-11 max|v| relative to l, plus 2^-25 per key for a P below
    f16's normal range, l >= 1) and the output to f16.  The tolerance is 4 x the linear bound x max|v| over the
    visible keys (4: second-order terms, numerator and denominator), plus those roundings, plus half an ulp of a
    16-bit output at the reference value."""
    B, Tp, H = amax.shape
    ds = (dk + 4) * U32 * amax / np.sqrt(dk)
    ntile = np.ceil(nvis / 32.0)
    lin = 2 * ds + 2 * ULP1 + (2 * nvis + (2 * ntile if mfma else 0) + 2) * U32
    tol = 4 * lin * vmax
    if mfma:
        tol = tol + (2.0 ** -11 + nvis * 2.0 ** -25) * vmax
    tol = np.repeat(tol.reshape(B * Tp, H), dk, 1)
    return tol + half_ulp(ref, dtype)


# --------------------------------------------------------------------------------------- TDT greedy step
STATE_FIELDS = ("t", "at_t", "n_out", "done", "upd", "tok", "t3p")
NAN_BITS = np.uint32(0xFFFFFFFF)   # what spt_debug_pk_tdt's output arrays hold before a kernel writes them


def merge_top2(part, fault=None):
    """part [n_tiles][4] (f32 best, i32 index as stored, f32 runner-up, unused) -> (best, index, second): the best
    of the tiles' bests (the lowest index on a tie) and the largest of everything else: every runner-up and every
    other tile's best.  Faults: tie_high (the highest index wins a tie), second_win_tile (the second best taken
    from the winning tile only)."""
    part = np.ascontiguousarray(part, np.float32)
    v1, i1, v2 = part[:, 0], part[:, 1].copy().view(np.int32), part[:, 2]
    cand = np.flatnonzero(v1 == v1.max())
    win = cand[np.argmax(i1[cand]) if fault == "tie_high" else np.argmin(i1[cand])]
    second = v2[win] if fault == "second_win_tile" else np.max(np.concatenate([v2, np.delete(v1, win)]))
    return np.float32(v1[win]), int(i1[win]), np.float32(second)


def tdt_rule(row, tk, d, T3, V, max_symbols, fault=None):
    """One row's step of joint_fin_kernel's rules on the merged token tk and the duration logits d:
    (t, at_t, n_out, done, upd, tok) -> the new row and, for a token, (its frame, its slot in the output)."""
    t, at_t, n_out, done, upd, tok = row
    d = np.asarray(d)
    skip = int(len(d) - 1 - np.argmax(d[::-1])) if fault == "dur_ge" else int(np.argmax(d))
    emit = None
    if tk != V:
        emit = (t, n_out)
        n_out, upd, tok, at_t = n_out + 1, 1, tk, at_t + 1
    else:
        upd = 0
    if skip == 0 and (tk == V or at_t >= max_symbols):
        skip = 1
    if skip > 0:
        at_t = 0
    t += skip
    if t >= T3:
        done = 1
    return (t, at_t, n_out, done, upd, tok), emit


def tdt_run(part, dur, lens, emb, fe, *, V, max_symbols, cap, T3p, fault=None):
    """joint_fin_kernel's rules, line by line, after pk_state_init: part [n_steps][B][n_tiles][4], dur
    [n_steps][B][n_dur] -> the arrays spt_debug_pk_tdt returns (state [n_steps + 1][B][7], xemb, fecur
    [n_steps + 1][B][P], out_tok, out_frame, out_t1, out_t2 [n_steps][B * cap + 1] with untouched elements as
    0xFF bytes).  Fault dur_ge: the last maximum of the duration logits wins."""
    part, dur = np.asarray(part, np.float32), np.asarray(dur, np.float32)
    emb, fe = np.asarray(emb, np.float32), np.asarray(fe, np.float32).reshape(len(lens), T3p, -1)
    ns, B = part.shape[:2]
    P = emb.shape[1]
    T3 = np.asarray(lens)[:, 3]
    st = np.zeros((ns + 1, B, 7), np.int32)
    st[0, :, 3], st[0, :, 4], st[0, :, 5], st[0, :, 6] = T3 <= 0, 1, V, T3p
    xemb, fecur = np.zeros((ns + 1, B, P), np.float32), np.zeros((ns + 1, B, P), np.float32)
    fecur[0] = fe[:, 0]
    no = B * cap + 1
    otok, ofr = np.full((ns, no), -1, np.int32), np.full((ns, no), -1, np.int32)
    o1, o2 = (np.full((ns, no), NAN_BITS, np.uint32).view(np.float32) for _ in range(2))
    for s in range(ns):
        st[s + 1], xemb[s + 1], fecur[s + 1] = st[s], xemb[s], fecur[s]
        if s:
            otok[s], ofr[s], o1[s], o2[s] = otok[s - 1], ofr[s - 1], o1[s - 1], o2[s - 1]
        for b in range(B):
            t, at_t, n_out, done, upd, tok, _ = (int(x) for x in st[s + 1, b])
            if done:
                continue
            v1, tk, v2 = merge_top2(part[s, b], fault)
            (t, at_t, n_out, done, upd, tok), emit = tdt_rule((t, at_t, n_out, done, upd, tok), tk, dur[s, b], T3[b], V,
                                                              max_symbols, fault)
            if emit is not None and emit[1] < cap:
                o = b * cap + emit[1]
                otok[s, o], ofr[s, o], o1[s, o], o2[s, o] = tk, emit[0], v1, v2
            st[s + 1, b] = (t, at_t, n_out, done, upd, tok, T3p)
            if upd:
                xemb[s + 1, b] = emb[tok]
            fecur[s + 1, b] = fe[b, min(t, T3p - 1)]
    return dict(state=st, xemb=xemb, fecur=fecur, out_tok=otok, out_frame=ofr, out_t1=o1, out_t2=o2)


# ------------------------------------------------------------------------------- the decode stages
def dot_abs(x, W, b):
    """sum_k |x_k w_nk| + |b_n|: what an f32 dot product's bar is evaluated from."""
    return np.abs(np.asarray(x, np.float64)) @ np.abs(np.asarray(W, np.float64)).T + np.abs(np.asarray(b, np.float64))


def lstm_cell(x, h, c, W_ih, W_hh, b_ih, b_hh, upd, fault=None, parts=False):
    """torch's LSTMCell (gate rows i, f, g, o of W [4P][P]) in float64; rows with upd = 0 keep h and c.
    Faults: gate_order (g and o exchanged), neighbour (a unit's four rows taken from the next unit), upd_ignored."""
    x, h, c = (np.asarray(v, np.float64) for v in (x, h, c))
    P = x.shape[1]
    W = np.concatenate([np.asarray(W_ih, np.float64), np.asarray(W_hh, np.float64)], 1)      # [4P][2P]
    b = np.asarray(b_ih, np.float64) + np.asarray(b_hh, np.float64)
    xh = np.concatenate([x, h], 1)
    g = (xh @ W.T + b).reshape(-1, 4, P)
    mag = (np.abs(xh) @ np.abs(W).T + np.abs(np.asarray(b_ih, np.float64)) + np.abs(np.asarray(b_hh, np.float64))).reshape(-1, 4, P)
    if fault == "neighbour":
        g = np.roll(g, -1, 2)
    gi, gf, gg, go = (g[:, q] for q in ((0, 1, 3, 2) if fault == "gate_order" else (0, 1, 2, 3)))
    c2 = sigmoid(gf) * c + sigmoid(gi) * np.tanh(gg)
    h2 = sigmoid(go) * np.tanh(c2)
    keep = np.zeros(len(x), bool) if fault == "upd_ignored" else np.asarray(upd) == 0
    h2[keep], c2[keep] = h[keep], c[keep]
    return (h2, c2, g, mag) if parts else (h2, c2)


def lstm_bar(c, g, mag):
    """(bar of h', bar of c').  A gate is a 2P-term f32 dot product and two biases: (2P + 3) U32 on sum |x w| + |b|.
    sig_(x) = 1 / (1 + expf(-x)): expf within 1 ulp and tanhf within 2 ulp (the HIP math API's table), one add and
    one division: 4 U32 relative, slope <= 1/4; tanh has slope <= 1.  Then c' = sf c + si tg (three roundings) and
    h' = so tanh(c') (one).  x 2 for second-order terms."""
    P = g.shape[2]
    dg = (2 * P + 3) * U32 * mag
    gi, gf, gg, go = (g[:, q] for q in range(4))
    c = np.asarray(c, np.float64)
    si, sf, so, tg = sigmoid(gi), sigmoid(gf), sigmoid(go), np.tanh(gg)
    dsi, dsf, dso = (0.25 * dg[:, q] + 4 * U32 * s for q, s in ((0, si), (1, sf), (3, so)))
    dtg = dg[:, 2] + 4 * U32 * np.abs(tg)
    c2 = sf * c + si * tg
    dc = np.abs(c) * dsf + dsi * np.abs(tg) + si * dtg + 3 * U32 * (np.abs(sf * c) + np.abs(si * tg))
    tc = np.tanh(c2)
    dh = dso * np.abs(tc) + so * (dc + 4 * U32 * np.abs(tc)) + U32 * np.abs(so * tc)
    return 2 * dh + 2.0 ** -126, 2 * dc + 2.0 ** -126


def pred_proj(h1, W, b, gp_in, upd, fault=None):
    """gp rows with upd = h1 W^T + b; the others as given (fault upd_ignored: all)."""
    y = np.asarray(h1, np.float64) @ np.asarray(W, np.float64).T + np.asarray(b, np.float64)
    on = np.ones(len(y), bool) if fault == "upd_ignored" else np.asarray(upd) != 0
    return np.where(on[:, None], y, np.asarray(gp_in, np.float64))


def joint(fe, gp, W, b, V, n_dur, fault=None):
    """x = ReLU(fe + gp) (one f32 rounding, made here in np.float32 as the kernel's only one before the products),
    logits = x W^T + b over N = V + 1 + n_dur -> (logits [B][N], x).  Tokens are n <= V (V: the blank), durations
    the rest."""
    x = np.maximum(np.asarray(fe, np.float32) + np.asarray(gp, np.float32), np.float32(0)).astype(np.float64)
    return x @ np.asarray(W, np.float64).T + np.asarray(b, np.float64), x


def tile_top2(logits, V, fault=None):
    """Per 64-output tile of one row's logits, over the tokens n <= V (fault blank_out: n < V): (v1, i1, v2) with the
    first index on ties and v2 the largest of the tile's other tokens; a tile without a token is (-inf, any, -inf)."""
    N = len(logits)
    nt = (N + 63) // 64
    lim = V - 1 if fault == "blank_out" else V
    v1, i1, v2 = np.full(nt, -np.inf), np.full(nt, 0x7FFFFFFF, np.int64), np.full(nt, -np.inf)
    for t in range(nt):
        n = np.arange(64 * t, min(64 * t + 64, lim + 1))
        if len(n) == 0:
            continue
        v = np.asarray(logits)[n]
        w = int(np.argmax(v))                      # first maximum
        v1[t], i1[t] = v[w], n[w]
        if len(n) > 1:
            v2[t] = np.delete(v, w).max()
    return v1, i1, v2


def tdt_steps(lstm, pred_w, pred_b, joint_w, joint_b, emb, fe, lens, *, V, n_dur, max_symbols, cap, T3p, n_steps):
    """The whole decode step in float64, n_steps times after the init: per row LSTM layer 0 on the pending token's
    embedding, layer 1, the prediction projection (all three only where upd), the joint on the row's current frame,
    the first maximum over the tokens n <= V and over the durations, and tdt_rule.  lstm [2] = (W_ih, W_hh, b_ih,
    b_hh).  -> dict(state [n_steps + 1][B][7], out_tok, out_frame [B * cap + 1] (-1 where unwritten), out_t1, out_t2
    (NaN where unwritten), gap: the smallest lead of a token or duration decision over its runner-up, bar: the
    largest f32 bar of a joint logit met on the way)."""
    fe = np.asarray(fe, np.float64).reshape(len(lens), T3p, -1)
    B, P = len(lens), fe.shape[2]
    T3 = np.asarray(lens)[:, 3]
    st = np.zeros((n_steps + 1, B, 7), np.int32)
    st[0, :, 3], st[0, :, 4], st[0, :, 5], st[0, :, 6] = T3 <= 0, 1, V, T3p
    h, c = np.zeros((2, B, P)), np.zeros((2, B, P))
    xemb, gp = np.zeros((B, P)), np.zeros((B, P))
    fecur = fe[:, 0].copy()
    no = B * cap + 1
    otok, ofr = np.full(no, -1, np.int32), np.full(no, -1, np.int32)
    o1, o2 = np.full(no, np.nan), np.full(no, np.nan)
    gap, bar = np.inf, 0.0
    for s in range(n_steps):
        st[s + 1] = st[s]
        upd = st[s, :, 4]
        h[0], c[0] = lstm_cell(xemb, h[0], c[0], *lstm[0], upd)
        h[1], c[1] = lstm_cell(h[0], h[1], c[1], *lstm[1], upd)
        gp = pred_proj(h[1], pred_w, pred_b, gp, upd)
        x = np.maximum(fecur + gp, 0.0)
        logits = x @ np.asarray(joint_w, np.float64).T + np.asarray(joint_b, np.float64)
        lbar = (P + 2) * U32 * dot_abs(x, joint_w, joint_b)
        for b in range(B):
            t, at_t, n_out, done, u, tok, _ = (int(v) for v in st[s + 1, b])
            if done:
                continue
            tl, d = logits[b, :V + 1], logits[b, V + 1:]
            tk = int(np.argmax(tl))
            srt, sd = np.sort(tl), np.sort(d)
            gap = min(gap, srt[-1] - srt[-2], sd[-1] - sd[-2])
            bar = max(bar, lbar[b].max())
            row, emit = tdt_rule((t, at_t, n_out, done, u, tok), tk, d, T3[b], V, max_symbols)
            if emit is not None and emit[1] < cap:
                o = b * cap + emit[1]
                otok[o], ofr[o], o1[o], o2[o] = tk, emit[0], srt[-1], srt[-2]
            st[s + 1, b, :6] = row
            if row[4]:
                xemb[b] = np.asarray(emb, np.float64)[row[5]]
            fecur[b] = fe[b, min(row[0], T3p - 1)]
    return dict(state=st, out_tok=otok, out_frame=ofr, out_t1=o1, out_t2=o2, gap=gap, bar=bar)
