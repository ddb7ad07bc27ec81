"""Float64 reference of the GEMM epilogues (k_gemm.hip) and the LayerNorm kernels (k_norm.hip), and the
error bars of tests/test_gpu_gemm.py.  Plain numpy: no tile, slab, swizzle or wave.

    C = alpha * act(A . W^T + bias) (+ residual / pos)        act: none, ReLU, GELU (tanh form), swish
    y = (v - mean(v)) / sqrt(var(v) + 1e-5) * w + b           two passes, population variance
    v = x + alpha * (slab_0 + .. + slab_{ks-1} + pbias)       layernorm_pend / layernorm_pend2

Operands are rounded to the engine dtype first (attn_ref.round_dtype), as the hooks round them."""
import numpy as np

from tests.attn_ref import half_ulp, round_dtype  # noqa: F401  (re-exported)

U32 = 2.0 ** -24          # unit roundoff of f32
TINY = 2.0 ** -126        # smallest normal f32: results below it may be flushed to zero
EPI = ("bias", "gelu", "gelu_pos", "resid", "kvsplit", "swish", "relu", "bias_f32", "partial")
F32_OUT = ("gelu_pos", "resid", "bias_f32", "partial")   # the others store the engine dtype
SKINNY_EPI = ("bias", "gelu", "resid", "swish", "relu", "bias_f32", "partial")
C_GELU = 0.7978845608028654  # sqrt(2 / pi)


# --------------------------------------------------------------------------------------------- GEMM
def rows(flat, off, ld, M, K, batch=1, stride=0) -> np.ndarray:
    """The [batch][M][K] operand a flat array holds: item z's row m at off + z * stride + m * ld (rows
    overlap where ld < K: the conv stem)."""
    flat = np.asarray(flat).ravel()
    idx = off + stride * np.arange(batch)[:, None, None] + ld * np.arange(M)[None, :, None] + np.arange(K)[None, None, :]
    return flat[idx]


def gelu(x) -> np.ndarray:
    """0.5 x (1 + tanh z), z = sqrt(2 / pi) (x + 0.044715 x^3), written as x / (1 + e^(-2 z)): the same
    function, without the cancellation of 1 + tanh z in the negative tail (float64 gives 0 below z = -19
    where the value is 1e-16 x and more)."""
    x = np.asarray(x, np.float64)
    with np.errstate(over="ignore"):
        return x / (1.0 + np.exp(-2.0 * C_GELU * (x + 0.044715 * x * x * x)))


def swish(x) -> np.ndarray:
    x = np.asarray(x, np.float64)
    with np.errstate(over="ignore"):
        return x / (1.0 + np.exp(-x))


def act(epi, x) -> np.ndarray:
    if epi in ("gelu", "gelu_pos"):
        return gelu(x)
    if epi == "swish":
        return swish(x)
    if epi == "relu":
        return np.maximum(x, 0.0)
    return np.asarray(x, np.float64)


def product(A, W) -> np.ndarray:
    """A [.., M, K] . W [N, K]^T in float64."""
    return np.asarray(A, np.float64) @ np.asarray(W, np.float64).T


def gemm(epi, A, W, bias=None, alpha=1.0, resid=None, pos=None) -> np.ndarray:
    """The value the epilogue stores, before the store's rounding: A [.., M, K], W [N, K] (already rounded
    to the dtype), bias [N], resid / pos [.., M, N].  "partial" and "kvsplit" return the plain product
    (+ bias): the caller sums the slabs / addresses the cache."""
    v = product(A, W)
    if bias is not None:
        v = v + np.asarray(bias, np.float64)
    if epi == "resid":
        return np.asarray(resid, np.float64) + alpha * v
    if epi == "bias_f32":
        return alpha * v
    if epi == "gelu_pos":
        return gelu(v) + np.asarray(pos, np.float64)
    return act(epi, v)


def store(v, epi, dtype) -> np.ndarray:
    """Round-to-nearest-even of the float64 value v into what the epilogue stores (f32, or the engine
    dtype; EPI_KVSPLIT in f16 clamps to +-65504 first: to_cache), as f32."""
    v32 = np.asarray(v, np.float64).astype(np.float32)
    if epi in F32_OUT or dtype == "f32":
        return v32
    if epi == "kvsplit" and dtype == "f16":
        v32 = np.clip(v32, -65504.0, 65504.0)
    with np.errstate(over="ignore"):  # an f16 store of a value beyond 65504 is inf, as the kernel's is
        return round_dtype(v32, dtype)


def kv_layer_elems(B, H, T) -> int:
    return (T + 31) // 32 * B * H * 4096


def kv_offset(l, kvi, b, h, t, e, B, H, T):
    """kernels.h kv_offset: [layer][ceil(T/32)][B][H][2][32][64]."""
    return l * kv_layer_elems(B, H, T) + (((t >> 5) * B + b) * H + h) * 4096 + kvi * 2048 + (t & 31) * 64 + e


def kv_index(N, B, H, T) -> np.ndarray:
    """[B*T][N] -> the cache element row b * T + t, column n is stored at."""
    n = np.arange(N)
    d = H * 64
    l, rem = n // (2 * d), n % (2 * d)
    kvi, h, e = rem // d, (rem % d) >> 6, rem & 63
    r = np.arange(B * T)
    b, t = r // T, r % T
    return kv_offset(l[None, :], kvi[None, :], b[:, None], h[None, :], t[:, None], e[None, :], B, H, T)


def abs_product(A, W, bias=None) -> np.ndarray:
    """sum_k |a_k w_k| + |bias|: what the linear bound scales with, per output element."""
    s = product(np.abs(A), np.abs(W))
    return s if bias is None else s + np.abs(np.asarray(bias, np.float64))


def gemm_bar(A, W, bias, K, ref, out_dtype, extra=0.0) -> np.ndarray:
    """4 x the linear bound (K + 2) 2^-24 (sum |a w| + |bias|) of an f32 accumulation in any order (K - 1
    adds, the bias add, the alpha product or residual add), + half an ulp of a 16-bit output at ref."""
    return 4.0 * (K + 2) * U32 * (abs_product(A, W, bias) + extra) + half_ulp(ref, out_dtype)


def act_rel(kind, x) -> np.ndarray:
    """Linear relative bound of common.h's gelu_tanh / swish at the exact f32 argument x, in units of 1:
    the result is x / (1 + e), e = 2^u.
      gelu_tanh  u = c2 * (x + 0.044715f * x * x * x): three products and one add (four roundings), the
                 product with c2, and the two constants' own roundings: 7 relative errors of 2^-24 on u
                 (x and x^3 share a sign, so nothing cancels)
      swish      u = -log2(e) * x: one product and the constant: 2
    An error d on u is a relative error ln 2 |u| d on e; v_exp_f32 and v_rcp_f32 are ASSUMED good to one
    ulp (2^-23 relative) each; 1 + e and the last product round once each.  e's error reaches the result
    through e / (1 + e)."""
    x = np.asarray(x, np.float64)
    if kind == "gelu":
        u = -2.0 * C_GELU * np.log2(np.e) * (x + 0.044715 * x ** 3)
        n = 7
    else:
        u = -np.log2(np.e) * x
        n = 2
    with np.errstate(over="ignore"):
        s = np.where(u > 0, 1.0 / (1.0 + np.exp2(-np.abs(u))), np.exp2(-np.abs(u)) / (1.0 + np.exp2(-np.abs(u))))
    return s * (np.log(2.0) * np.abs(u) * n * U32 + 2 * U32) + U32 + 2 * U32 + U32


def act_bar(kind, x, ref, out_dtype) -> np.ndarray:
    """4 x act_rel x |ref|, + (|x| + 1) 2^-126 (a reciprocal or a result below the smallest normal f32 may
    be flushed to zero; subnormal behaviour is not asserted), + half an ulp of a 16-bit output."""
    x = np.asarray(x, np.float64)
    return 4.0 * act_rel(kind, x) * np.abs(ref) + (np.abs(x) + 1.0) * TINY + half_ulp(ref, out_dtype)


# ---------------------------------------------------------------------------------------- LayerNorm
EPS = 1e-5


def layernorm(x, w, b) -> np.ndarray:
    x = np.asarray(x, np.float64)
    mean = x.mean(-1, keepdims=True)
    a = x - mean
    var = (a * a).mean(-1, keepdims=True)
    return a / np.sqrt(var + EPS) * np.asarray(w, np.float64) + np.asarray(b, np.float64)


def pend(x, slabs, pbias, alpha) -> np.ndarray:
    """x + alpha * (sum of slabs [ks][M][d] + pbias)."""
    return np.asarray(x, np.float64) + alpha * (np.asarray(slabs, np.float64).sum(0) + np.asarray(pbias, np.float64))


def slabs(flat, ks, stride, M, d) -> np.ndarray:
    """[ks][M][d] of a flat slab array: slab q's row m at q * stride + m * d."""
    return rows(flat, 0, d, M, d, ks, stride)


def layernorm_onepass_f32(x, w, b) -> np.ndarray:
    """The fault the mean-1000 rows are built for: var = E[x^2] - mean^2, accumulated in f32 in order."""
    x = np.asarray(x, np.float32)
    d = np.float32(x.shape[-1])
    mean = np.cumsum(x, -1, dtype=np.float32)[..., -1:] / d
    var = np.cumsum(x * x, -1, dtype=np.float32)[..., -1:] / d - mean * mean
    with np.errstate(invalid="ignore"):
        r = np.float32(1.0) / np.sqrt(var + np.float32(EPS))
    return ((x - mean) * r * np.asarray(w, np.float32) + np.asarray(b, np.float32)).astype(np.float64)


def ln_depth(d) -> int:
    """Adds on the longest path of the kernels' row sum: ceil(d / 256) float4 per lane, each summed as
    (x + y) + (z + w) and added to the lane's total, then six butterfly steps over the wave."""
    return -(-d // 256) + 2 + 6


def ln_bar(v, w, b, out_dtype, v_err=None) -> np.ndarray:
    """4 x the linear bound of the two-pass f32 LayerNorm of the row v (float64, [.., d]), per element,
    + half an ulp of a 16-bit output.  With D = ln_depth(d), u = 2^-24 and e_i = v_err, the error the
    kernel's own v_i carries (pend_err; 0 for the plain LayerNorm):
      mean     D adds and the division: |dmean| <= (D + 1) u mean|v| + mean(e)
      a_i      v_i - mean: |da_i| <= |dmean| + e_i + u |a_i|
      var      the squares, their sum and the division: relative (D + 4) u (dmean moves sum a^2 in second
               order only: sum a_i = 0), and 2 max(e) / sqrt(var) from e (Cauchy-Schwarz on sum a_i e_i);
               + eps, sqrt, reciprocal: 3 u more on rstd (sqrtf and the division are taken as correctly
               rounded); so rstd is off by at most ((D + 4) / 2 + 3) u + max(e) rstd, relatively
      y_i      a_i * rstd * w_i + b_i: three more roundings
    so |dy_i| <= |w_i| rstd (|dmean| + e_i + |a_i| (((D + 4) / 2 + 7) u + max(e) rstd)) + u |y_i|."""
    v = np.asarray(v, np.float64)
    d = v.shape[-1]
    D = ln_depth(d)
    e = np.zeros_like(v) if v_err is None else np.asarray(v_err, np.float64)
    mean = v.mean(-1, keepdims=True)
    a = v - mean
    rstd = 1.0 / np.sqrt((a * a).mean(-1, keepdims=True) + EPS)
    dmean = (D + 1) * U32 * np.abs(v).mean(-1, keepdims=True) + e.mean(-1, keepdims=True)
    w = np.asarray(w, np.float64)
    y = a * rstd * w + np.asarray(b, np.float64)
    lin = np.abs(w) * rstd * (dmean + e + np.abs(a) * (((D + 4) / 2.0 + 7.0) * U32 + e.max(-1, keepdims=True) * rstd)) + \
        U32 * np.abs(y)
    return 4.0 * lin + half_ulp(y, out_dtype)


def pend_err(x, slabs_, pbias, alpha) -> np.ndarray:
    """Linear bound of the f32 evaluation of pend(): ks - 1 slab adds, the bias add, the product with
    alpha and the add to x: (ks + 2) u (|x| + |alpha| (sum |slab| + |pbias|))."""
    ks = np.asarray(slabs_).shape[0]
    mag = np.abs(np.asarray(x, np.float64)) + abs(alpha) * (np.abs(np.asarray(slabs_, np.float64)).sum(0) +
                                                            np.abs(np.asarray(pbias, np.float64)))
    return (ks + 2) * U32 * mag
