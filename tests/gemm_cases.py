"""The cases of tests/test_gpu_gemm.py: shapes at the edges k_gemm.hip and k_norm.hip
handle explicitly, with inputs built so that a dropped, duplicated or misplaced element changes the
result.  tests/test_gemm_ref.py checks on the CPU that they are what they claim to be.

Exact cases.  A holds odd integers over the whole range that is exact in the dtype (|a| <= 255 bf16,
2047 f16, 4095 f32); W holds odd integers |w| <= wmax except at the first k of every 128-byte slab, which
is even: each slab's share of each output element is a sum of an odd number of odd terms and one even
one, so it is odd, never zero.  W[:, 0] is one large power of two for every column, so a row's values are
spread by its A[m][0]; bias and residual are integers; wmax and the ranges keep
sum |a w| + |bias| + |resid| below 2^24 (and the same with alpha applied, in units of the finest bit), so
every partial sum in any order is an integer f32 holds exactly.  Rows that agree with another row in some
column, or columns that agree in some row, are redrawn until none is left."""
import functools
import types

import numpy as np

from tests import gemm_ref as R

DT = ("f32", "bf16", "f16")
DT16 = ("bf16", "f16")
AMAX = {"bf16": 255, "f16": 2047, "f32": 4095}
SLAB = {"bf16": 64, "f16": 64, "f32": 32}     # elements of K per 128-byte slab
EXACT_EPI = ("bias_f32", "resid", "bias", "relu", "partial")


def _k(K16, dtype):
    """K is listed for the 16-bit types; f32 takes half, so the slab counts match."""
    return K16 // 2 if dtype == "f32" else K16


def case(variant, dtype, M, N, K16, epi, kind="exact", **kw):
    c = dict(variant=variant, dtype=dtype, M=M, N=N, K=_k(K16, dtype), epi=epi, kind=kind, batch=1, ksplit=1,
             a_pad=0, c_pad=0, ldc_pad=0, conv=0, kv_T=0, seed=0)
    c.update(kw)
    extra = "".join(f"-{k}{v}" for k, v in kw.items() if k != "seed")
    c["id"] = f"v{variant}-{dtype}-{epi}-{M}x{N}x{c['K']}{extra}" + ("" if kind == "exact" else f"-{kind}")
    return c


def _grid(variant, dtypes, Ms, Ns, K16s, epis=EXACT_EPI, **kw):
    """Every M with every K; N and the epilogue rotate so each M and each K meets every N, and every
    epilogue is met several times per variant and dtype."""
    out = []
    for t, dtype in enumerate(dtypes):
        for i, M in enumerate(Ms):
            for j, K in enumerate(K16s):
                out.append(case(variant, dtype, M, Ns[(i + j) % len(Ns)], K, epis[(i + 2 * j + t) % len(epis)], **kw))
    return out


def _extras(variant, N, Ms_big):
    """ksplit 1 / 2 with every slab returned, batch 2 with padded strides, ldc > N, and grids that are not
    a multiple of 8 (the XCD remap)."""
    out = []
    for dtype in DT:
        out += [case(variant, dtype, 129, N, 256, "partial", ksplit=2, c_pad=64),
                case(variant, dtype, 129, N, 128, "resid", batch=2, a_pad=8 * 5, c_pad=N * 3),
                case(variant, dtype, 65, N, 128, "bias", batch=2, a_pad=8 * 3, c_pad=N),
                case(variant, dtype, 129, N, 128, "bias_f32", ldc_pad=12),
                case(variant, dtype, 65, N, 64, "relu", ldc_pad=8)]
        out += [case(variant, dtype, M, N, 128, "resid", wgs="odd") for M in Ms_big]
    return out


GEMM_EXACT = (
    _grid(1, DT, (1, 127, 128, 129, 300), (128, 384), (64, 128, 192, 320)) + _extras(1, 384, (300, 1100)) +
    _grid(4, DT, (1, 63, 64, 65, 130), (128, 384), (64, 128, 192, 320)) + _extras(4, 384, (300, 1100)) +
    _grid(5, DT, (1, 63, 64, 65, 130), (64, 192), (64, 128, 192, 320)) + _extras(5, 192, (300, 1100)) +
    _grid(2, DT16, (1, 255, 256, 257, 300), (256, 512), (64, 128, 192, 448)) +
    [c for dtype in DT16 for c in (case(2, dtype, 257, 256, 256, "partial", ksplit=2, c_pad=64),
                                   case(2, dtype, 257, 256, 128, "resid", batch=2, a_pad=8 * 5, c_pad=256 * 3),
                                   case(2, dtype, 300, 512, 128, "bias", batch=2, a_pad=8, c_pad=512),
                                   case(2, dtype, 257, 256, 128, "bias_f32", ldc_pad=12))])


def _skinny():
    out = []
    epis = ("bias", "resid", "relu", "bias_f32", "partial")
    for t, dtype in enumerate(DT16):
        for i, M in enumerate((1, 15, 16, 17, 33, 48, 49, 64)):
            for j, Kw in enumerate((128, 256, 512, 640)):
                ks = (1, 2, 4)[(i + j + t) % 3]
                epi = "partial" if ks > 1 else epis[(i + 2 * j + t) % len(epis)]
                out.append(case(3, dtype, M, (16, 48)[(i + j) % 2], Kw * ks, epi, ksplit=ks, c_pad=16 if ks > 1 else 0))
    return out


GEMM_SKINNY = _skinny()

# the conv stem: C = 64 channels, K = 3 C, rows that overlap (lda = C: stride 1, 2 C: stride 2), batch 2,
# C starting one row into each item's M + 2 rows
GEMM_CONV = [case(v, dtype, M, N, 0, epi, kind="conv", conv=s, batch=2)
             for v, N in ((1, 128), (4, 128), (2, 256)) for dtype in (DT16 if v == 2 else DT)
             for s, M, epi in ((1, 130, "bias_f32"), (2, 67, "bias"))]

# EPI_KVSPLIT: kv_H = 2, two layers (N = 512), kv_B = 2
GEMM_KV = [case(v, dtype, 2 * T, 512, 128, "kvsplit", kind="kv", kv_T=T)
           for v in (1, 2, 4, 5) for dtype in (DT16 if v == 2 else DT) for T in (1, 31, 33, 50)]

# rounded cases: seeded inputs of order 1
ROUNDED_EPI = ("bias", "resid", "bias_f32", "relu", "partial")
GEMM_ROUNDED = (
    [case(v, dtype, M, N, K, ROUNDED_EPI[(i + t) % 5], kind="rounded")
     for v, shapes in ((1, ((129, 128, 320), (300, 384, 128))), (4, ((65, 128, 320), (130, 384, 128))),
                       (5, ((65, 64, 320), (130, 192, 128))))
     for t, dtype in enumerate(DT) for i, (M, N, K) in enumerate(shapes)] +
    [case(2, dtype, M, N, K, ROUNDED_EPI[(i + t) % 5], kind="rounded")
     for t, dtype in enumerate(DT16) for i, (M, N, K) in enumerate(((257, 256, 448), (300, 512, 128)))] +
    [case(3, dtype, M, N, K, ROUNDED_EPI[(i + t) % 5], kind="rounded")
     for t, dtype in enumerate(DT16) for i, (M, N, K) in enumerate(((17, 48, 640), (64, 16, 512)))] +
    [case(0, dtype, 300, 512, 128, "bias", kind="rounded") for dtype in DT])

# activation cases: one-hot rows of A select entries of W, so the pre-activation value is exact
GEMM_ACT = (
    [case(v, dtype, M, N, 64 if dtype != "f32" else 128, epi, kind="act")
     for v, M, N in ((1, 130, 128), (4, 130, 128), (5, 130, 64), (2, 257, 256))
     for dtype in (DT16 if v == 2 else DT) for epi in ("gelu_pos", "gelu", "swish")] +
    [case(3, dtype, 64, 48, 128, epi, kind="act") for dtype in DT16 for epi in ("gelu", "swish")])

# the variant-2 tail rows: the pre-loaded residual / pos rows are clamped at M = 257
GEMM_TAIL = [case(2, dtype, 257, 512, 192, "resid", seed=1) for dtype in DT16]

# every tile on one shape all of them accept: the same bits for every epilogue
CROSS_SHAPE = dict(M=300, N=512, K16=192, kv_T=150)


def cross_cases(dtype, epi):
    vs = (1, 4, 5) if dtype == "f32" else (1, 2, 4, 5)
    kw = dict(kv_T=CROSS_SHAPE["kv_T"]) if epi == "kvsplit" else {}
    return [case(v, dtype, CROSS_SHAPE["M"], CROSS_SHAPE["N"], CROSS_SHAPE["K16"], epi, kind="rounded", seed=7, **kw)
            for v in vs]


# ------------------------------------------------------------------------------------------- builders
def _odd(rng, amax, size):
    return (2 * rng.integers(0, (amax + 1) // 2, size) + 1) * rng.choice((-1, 1), size)


def _layout(c):
    """Where A and C live in their flat arrays."""
    M, N, K, batch = c["M"], c["N"], c["K"], c["batch"]
    L = types.SimpleNamespace()
    if c["conv"]:
        ch = 64
        K = 3 * ch
        L.lda = ch * c["conv"]
        in_rows = (M - 1) * c["conv"] + 3
        L.sA, L.a_off, L.a_count = in_rows * ch + 8, 0, batch * (in_rows * ch + 8)
        L.ldc, L.c_off, L.sC = N, N, (M + 2) * N
        L.c_count = batch * L.sC
        L.in_rows, L.ch = in_rows, ch
    else:
        L.lda = K
        L.a_off = 8 if c["a_pad"] else 0
        L.sA = M * K + c["a_pad"]
        L.a_count = L.a_off + batch * L.sA
        L.ldc = N + c["ldc_pad"]
        L.c_off = 8 if c["c_pad"] or c["ldc_pad"] else 0
        L.sC = M * L.ldc + c["c_pad"]
        L.c_count = L.c_off + max(batch, c["ksplit"]) * L.sC + 4
    if c["epi"] == "kvsplit":  # C is the cache: two layers from c_off, then a margin
        L.c_off, L.c_count = 64, 128 + 2 * R.kv_layer_elems(2, 2, c["kv_T"])
    L.K = K
    return L


def _c_index(c, L):
    """Flat index into C of every element the launch writes: [batch or ksplit][M][N] (kvsplit: [1][M][N])."""
    M, N = c["M"], c["N"]
    if c["epi"] == "kvsplit":
        return (R.kv_index(N, 2, 2, c["kv_T"]) + L.c_off)[None]
    z = max(c["batch"], c["ksplit"])
    return L.c_off + L.sC * np.arange(z)[:, None, None] + L.ldc * np.arange(M)[None, :, None] + np.arange(N)[None, None, :]


def _collisions(v):
    """Rows of the 2-d integer array v that equal another row in some column."""
    order = np.argsort(v, axis=0, kind="stable")
    s = np.take_along_axis(v, order, 0)
    hit = s[1:] == s[:-1]
    return np.unique(order[1:][hit])


@functools.lru_cache(maxsize=None)
def _build(key):
    c = dict(key)
    return _BUILDERS[c["kind"]](c)


def build(c):
    """The inputs, the call and the float64 reference of a case (cached: a reference is computed once)."""
    return _build(tuple(sorted(c.items())))


def _finish(c, L, A, W, bias, pos, C_in, resid, alpha):
    dtype, epi = c["dtype"], c["epi"]
    b = types.SimpleNamespace(case=c, L=L, alpha=alpha, bias=bias, pos=pos, resid=resid)
    b.A = R.round_dtype(A, dtype)
    b.W = R.round_dtype(W, dtype)
    b.A3 = R.rows(b.A, L.a_off, L.lda, c["M"], L.K, c["batch"], L.sA)
    b.idx = _c_index(c, L)
    out_dt = "f32" if epi in R.F32_OUT else dtype
    b.out_dtype = out_dt
    b.C_in = R.round_dtype(C_in, out_dt)          # what the hook uploads
    if resid is not None:
        b.C_in[b.idx] = resid
    if epi == "partial":
        Kc = L.K // c["ksplit"]
        b.ref = np.stack([R.gemm(epi, b.A3[0][:, s * Kc:(s + 1) * Kc], b.W[:, s * Kc:(s + 1) * Kc], bias)
                          for s in range(c["ksplit"])])
    else:
        b.ref = R.gemm(epi, b.A3, b.W, bias, alpha, resid, None if pos is None else pos[None])
    b.kw = dict(M=c["M"], N=c["N"], K=L.K, dtype=dtype, epi=epi, variant=c["variant"], batch=c["batch"], a_off=L.a_off,
                lda=L.lda, sA=L.sA if c["batch"] > 1 else 0, bias=bias, pos=pos, c_off=L.c_off, ldc=L.ldc,
                sC=L.sC if c["batch"] > 1 else 0, alpha=alpha, ksplit=c["ksplit"],
                c_split=L.sC if c["ksplit"] > 1 else 0, kv=(2, c["kv_T"], 2) if epi == "kvsplit" else (0, 0, 0))
    return b


def _exact(c):
    dtype, epi, M, N = c["dtype"], c["epi"], c["M"], c["N"]
    L = _layout(c)
    K, S, amax = L.K, SLAB[dtype], AMAX[dtype]
    rng = np.random.default_rng([c["seed"], M, N, K, c["variant"], DT.index(dtype), R.EPI.index(epi)])
    small = dtype == "f16" and epi not in R.F32_OUT      # the stored value must mostly stay finite in f16
    w_hi = 32 if small else 2 ** int(np.log2(2 ** 21 / amax))
    wmax = 1 if small else max(1, (int(2 ** 21 / (amax * K)) - 1) // 2 * 2 + 1)
    b_rng = 4096 if small else 2 ** 20
    A = _odd(rng, amax, L.a_count).astype(np.int64)
    if c["conv"]:  # the zero pad rows of each item's input are the caller's
        a2 = A.reshape(c["batch"], -1)
        a2[:, :L.ch] = 0
        a2[:, (L.in_rows - 1) * L.ch:] = 0
    W = _odd(rng, wmax, (N, K))
    W[:, ::S] = 2 * _odd(rng, (wmax + 1) // 2 * 2 - 1, (N, len(range(0, K, S))))
    W[:, 0] = w_hi
    has_bias = epi != "partial"
    bias = rng.choice(np.arange(-b_rng, b_rng), N, replace=False) if has_bias else None
    if not has_bias:
        # no bias to tell the columns apart: A[:, 1] = 31 in every row and W[n][1] a code of its own, one of
        # the 2048 values +-m 2^e (m 128..255, e 1..8: exact in every dtype, even), so column n is offset
        # by 31 code(n), over +-2^21; W[:, 2] is even too, which keeps the odd terms of slab 0 odd in number
        codes = np.array([s_ * m * 2 ** e for s_ in (-1, 1) for e in range(1, 9) for m in range(128, 256)])
        A[L.a_off + 1 + L.sA * np.arange(c["batch"])[:, None] + L.lda * np.arange(M)[None, :]] = 31
        W[:, 1] = rng.choice(codes, N, replace=False)
        W[:, 2] = 2 * _odd(rng, (wmax + 1) // 2 * 2 - 1, N)
    resid = rng.integers(-2 ** 20, 2 ** 20, (c["batch"], M, N)) if epi == "resid" else None

    def ref2d():
        A3 = R.rows(A, L.a_off, L.lda, M, K, c["batch"], L.sA).astype(np.float64)
        v = (A3 @ W.T.astype(np.float64)).reshape(-1, N)  # integers far below 2^53: exact
        return v + bias if has_bias else v
    for _ in range(200):  # redraw what collides (few: the values are spread over +-2^22)
        if small:  # +-65504 cannot hold that many distinct values: these cases check the store, not the place
            break
        v = ref2d()
        rows_, cols_ = _collisions(v), _collisions(v.T)
        if not len(rows_) and not len(cols_):
            break
        for r in rows_:
            z, m = divmod(int(r), M)
            k = int(rng.integers(2, K))
            i = L.a_off + z * L.sA + m * L.lda + k
            if c["conv"] and (i % L.sA < L.ch or i % L.sA >= (L.in_rows - 1) * L.ch):
                continue
            A[i] = _odd(rng, amax, 1)[0]
        for n in cols_:
            if has_bias:
                bias[n] = rng.integers(-b_rng, b_rng)
            else:
                W[n, 1] = rng.choice(np.setdiff1d(codes, W[:, 1]))
    else:
        raise AssertionError(f"{c['id']}: rows or columns still collide")
    alpha = 1.0
    if epi in ("resid", "bias_f32"):
        mag = (np.abs(R.rows(A, L.a_off, L.lda, M, K, c["batch"], L.sA)).astype(np.float64) @ np.abs(W).T.astype(np.float64) +
               np.abs(bias)).max()
        alpha = 2.0 if 2 * mag + 2 ** 20 < 2 ** 24 else 0.5
    C_in = rng.integers(-120, 121, L.c_count)
    return _finish(c, L, A.astype(np.float32), W.astype(np.float32), None if bias is None else bias.astype(np.float32),
                   None, C_in.astype(np.float32), None if resid is None else resid.astype(np.float32), alpha)


def _normal(rng, size, dtype):
    """Order-1 values that stay normal numbers in every dtype."""
    x = rng.standard_normal(size).astype(np.float32)
    x = np.where(np.abs(x) < 2.0 ** -10, np.copysign(np.float32(2.0 ** -10), x), x)
    return R.round_dtype(x, dtype)


def _rounded(c):
    dtype, epi, M, N = c["dtype"], c["epi"], c["M"], c["N"]
    L = _layout(c)
    rng = np.random.default_rng([c["seed"], M, N, L.K, DT.index(dtype)])  # the same inputs for every variant and epilogue
    A = _normal(rng, L.a_count, dtype)
    W = _normal(rng, (N, L.K), dtype)
    bias = _normal(rng, N, "f32")
    resid_all = _normal(rng, (c["batch"], M, N), "f32")
    pos_all = _normal(rng, (M, N), "f32")
    C_in = rng.integers(-120, 121, L.c_count).astype(np.float32)
    return _finish(c, L, A, W, None if epi == "partial" else bias, pos_all if epi == "gelu_pos" else None, C_in,
                   resid_all if epi == "resid" else None, 0.5 if epi in ("resid", "bias_f32") else 1.0)


def act_values(dtype, n):
    """n pre-activation values: -12..12 densely, 0, -0, +-1e4 and (bf16, f32; nothing that large is an f16)
    values whose cube overflows f32 -- rounded to dtype, so they are exact operands."""
    special = [0.0, -0.0, 1e4, -1e4, 1.0, -1.0]
    if dtype != "f16":
        special += [1e13, -1e13, 3e38, -3e38]
    x = np.concatenate([np.linspace(-12.0, 12.0, n - len(special)), special]).astype(np.float32)
    x = R.round_dtype(x, dtype)
    tiny = {"f16": 2.0 ** -14, "bf16": 2.0 ** -126, "f32": 2.0 ** -126}[dtype]
    return np.where((x != 0) & (np.abs(x) < tiny), np.float32(0.0), x)


def _act(c):
    dtype, epi, M, N = c["dtype"], c["epi"], c["M"], c["N"]
    L = _layout(c)
    K = L.K
    rng = np.random.default_rng([3, M, N, K])
    Ku = min(M, K)  # the columns of W some row selects; the others hold 1
    W = np.ones((N, K), np.float32)
    W[:, :Ku] = act_values(dtype, N * Ku)[rng.permutation(N * Ku)].reshape(N, Ku)
    A = np.zeros((M, K), np.float32)
    A[np.arange(M), np.arange(M) % K] = 1.0
    pos = None
    if epi == "gelu_pos":  # rows that pass K get a nonzero pos: its indexing, at the cost of one rounding
        pos = np.zeros((M, N), np.float32)
        pos[K:] = rng.integers(-4, 5, (M - K, N)) if M > K else 0
    C_in = rng.integers(-120, 121, L.c_count).astype(np.float32)
    b = _finish(c, L, A.ravel(), W, None, pos, C_in, None, 1.0)
    b.x = b.W.T[np.arange(M) % K][None].astype(np.float64)  # [1][M][N]: the exact pre-activation values
    return b


_BUILDERS = {"exact": _exact, "conv": _exact, "kv": _exact, "rounded": _rounded, "act": _act}


# --------------------------------------------------------------------------------------- LayerNorm
LN_D = (4, 252, 256, 260, 512, 1024, 1280, 1536)
LN_M = (1, 3, 4, 5, 9)
LN_KS = (1, 2, 3, 4, 8)
ROW_TYPES = ("seeded", "mean1000", "constant")


def row_type(m, di):
    return ROW_TYPES[(m + di) % 3]


@functools.lru_cache(maxsize=None)
def ln_inputs(d, M, ks=0, pad=0):
    """x [M][d], w, b (and for ks > 0 the slabs as a flat array with slab_stride = M d + pad, pbias, alpha
    = 0.5, w2, b2): row m is seeded, has mean 1000 and deviation 1, or is constant, by row_type."""
    di = LN_D.index(d) if d in LN_D else 0
    rng = np.random.default_rng([11, d, M, ks])
    o = types.SimpleNamespace(d=d, M=M, ks=ks, alpha=0.5, stride=M * d + pad)
    o.w = (1.0 + 0.25 * rng.standard_normal(d)).astype(np.float32)
    o.b = (0.5 * rng.standard_normal(d)).astype(np.float32)
    o.w2 = (1.0 + 0.25 * rng.standard_normal(d)).astype(np.float32)
    o.b2 = (0.5 * rng.standard_normal(d)).astype(np.float32)
    o.types = [row_type(m, di) for m in range(M)]
    x = rng.standard_normal((M, d)).astype(np.float32)
    if ks:
        sl = rng.standard_normal((ks, M, d)).astype(np.float32)
        o.pbias = rng.standard_normal(d).astype(np.float32)
    for m, t in enumerate(o.types):
        if t == "mean1000":
            x[m] += 1000.0
        elif t == "constant":   # every sum below is a small dyadic number: v = 1 + 0.5 (ks + 2) exactly
            x[m] = 3.0 if not ks else 1.0
            if ks:
                sl[:, m] = 1.0
    if ks:
        if "constant" in o.types:  # a constant v needs a constant pbias: the rows share it
            o.pbias[:] = 2.0
        flat = rng.standard_normal((ks - 1) * o.stride + M * d + pad).astype(np.float32)
        for q in range(ks):
            flat[q * o.stride:q * o.stride + M * d] = sl[q].ravel()
        o.slab_flat, o.slabs = flat, sl
    o.x = x
    return o
