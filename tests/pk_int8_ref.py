"""numpy restatement of the Parakeet int8 mode's arithmetic (TEST INFRASTRUCTURE).

The int8 export runs every encoder Linear and pointwise convolution as ONNX
DynamicQuantizeLinear -> MatMulInteger / ConvInteger; the op definitions are ONNX's, the order of
the float operations the quantize_dynamic pattern [upstream, recalled].  Every float step is one
f32 operation (numpy float32 arithmetic), the product exact integers.

`encode` is the whole-encoder reference: tests/pk_torch.encode with its linears and 1 x 1
convolutions substituted (the module is imported and its `F` namespace swapped for the call; it
is not copied or edited)."""
from __future__ import annotations

import contextlib

import numpy as np

from tests import onnx_parakeet

F32 = np.float32


def dynamic_quantize(x):
    """DynamicQuantizeLinear over all of x -> (q uint8, s_a float32, z_a int)."""
    x = np.asarray(x, F32)
    lo = F32(min(F32(0), x.min()))
    hi = F32(max(F32(0), x.max()))
    s = F32((hi - lo) / F32(255))
    if s == 0:  # an all-zero input: an all-zero product
        return np.zeros(x.shape, np.uint8), s, 0
    z = int(np.clip(np.rint((F32(0) - lo) / s), 0, 255))
    q = np.clip(np.rint(x / s) + F32(z), 0, 255).astype(np.uint8)
    return q, s, z


def matmul_integer(q, z_a, w, z_w):
    """acc[m][n] = sum_k (q[m][k] - z_a)(w[n][k] - z_w[n]); w [N][K] int8 or uint8 values."""
    a = q.astype(np.int64) - int(z_a)
    w = np.asarray(w).astype(np.int64)
    b = w - np.broadcast_to(np.asarray(z_w, np.int64).reshape(-1), (w.shape[0],))[:, None]
    # |acc| <= 255 * 255 * K < 2^53: the f64 product (BLAS) is the exact integer
    acc = np.rint(a.astype(np.float64) @ b.T.astype(np.float64)).astype(np.int64)
    assert np.abs(acc).max(initial=0) < 2 ** 31
    return acc.astype(np.int32)


def activation(y, act):
    y = np.asarray(y, F32)
    if act == "relu":
        return np.maximum(y, F32(0))
    if act == "swish":
        y64 = y.astype(np.float64)
        with np.errstate(over="ignore"):  # exp(-y) -> inf: y / inf = -0
            return (y64 / (1.0 + np.exp(-y64))).astype(F32)
    assert act is None
    return y


def qlinear(x, group_len, w, s_w, z_w, bias=None, act=None):
    """A quantised layer on rows x [M][K] split into utterances of group_len rows; w [N][K] stored
    integers, s_w / z_w one value or N.  -> dict(q, sa, za, acc, y_pre (before the activation), y)."""
    x = np.asarray(x, F32)
    N = np.asarray(w).shape[0]
    s_w = np.broadcast_to(np.asarray(s_w, F32).reshape(-1), (N,))
    z_w = np.broadcast_to(np.asarray(z_w, np.int64).reshape(-1), (N,))
    out = dict(q=[], sa=[], za=[], acc=[], y_pre=[])
    m = 0
    for n in group_len:
        q, s, z = dynamic_quantize(x[m:m + n])
        acc = matmul_integer(q, z, w, z_w)
        y = acc.astype(F32) * (s * s_w)[None, :]
        if bias is not None:
            y = y + np.asarray(bias, F32)[None, :]
        for k, v in (("q", q), ("sa", s), ("za", z), ("acc", acc), ("y_pre", y.astype(F32))):
            out[k].append(v)
        m += n
    assert m == x.shape[0]
    res = {k: np.concatenate(out[k]) for k in ("q", "acc", "y_pre")}
    res["sa"] = np.array(out["sa"], F32)
    res["za"] = np.array(out["za"], np.int32)
    res["y"] = activation(res["y_pre"], act)
    return res


def quantize_weight(w):
    """An f32 weight [N][K] of a quantised layer, quantised at load: symmetric per tensor
    (tests/onnx_parakeet.quantize "int8") -> (q int8 [N][K], scale float32, dequantised f32)."""
    q, s, _, deq = onnx_parakeet.quantize(np.asarray(w, F32), "int8", 0)
    return q, F32(s), deq


def ulp_diff(a, b):
    """distance in f32 units in the last place (finite values)"""
    def key(v):
        i = np.asarray(v, F32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


# ------------------------------------------------------------------ the whole encoder
class _Shim:
    """torch.nn.functional with linear and 1 x 1 conv2d replaced."""

    def __init__(self, real, mode, rng, eps):
        self._real, self._mode, self._rng, self._eps = real, mode, rng, eps

    def __getattr__(self, name):
        return getattr(self._real, name)

    def _rows(self, x, W, b):
        import torch
        xr = x.detach().numpy().astype(F32)
        if self._rng is not None:  # the sensitivity probe: each quantised layer's input moved by eps relative
            xr = (xr * (F32(1) + F32(self._eps) * self._rng.uniform(-1, 1, xr.shape).astype(F32))).astype(F32)
        q, s, deq = quantize_weight(W.detach().numpy())
        bias = None if b is None else b.detach().numpy()
        if self._mode == "deq":
            y = xr @ deq.T
            if bias is not None:
                y = y + bias
            return torch.from_numpy(y.astype(F32))
        return torch.from_numpy(qlinear(xr, [xr.shape[0]], q, s, 0, bias)["y"])

    def linear(self, x, W, b=None):
        return self._rows(x.reshape(-1, x.shape[-1]), W, b).reshape(*x.shape[:-1], W.shape[0])

    def conv2d(self, x, W, b=None, *a, **kw):
        if tuple(W.shape[2:]) != (1, 1) or kw.get("groups", 1) != 1:
            return self._real.conv2d(x, W, b, *a, **kw)
        B, C, T, Fq = x.shape  # one utterance: one range over the whole tensor
        assert B == 1
        y = self._rows(x[0].permute(1, 2, 0).reshape(T * Fq, C), W.reshape(W.shape[0], C), b)
        return y.reshape(T, Fq, -1).permute(2, 0, 1)[None]


@contextlib.contextmanager
def _patched(mode, rng, eps):
    from tests import pk_torch
    real = pk_torch.F
    pk_torch.F = _Shim(real, mode, rng, eps)
    try:
        yield pk_torch
    finally:
        pk_torch.F = real


def encode(model, dims, mel, mode="int8", perturb_seed=None, eps=1e-6):
    """Encoder output [T3][d] of one utterance's normalised log-mel [n_mels][T] (numpy).
    mode "int8": every quantised layer as DynamicQuantizeLinear -> MatMulInteger on the weight
    quantised at load; "deq": the same network in f32 on those weights dequantised.
    perturb_seed: every quantised layer's input moved by eps relative (the arithmetic's own
    sensitivity to differences smaller than two correct f32 LayerNorms make)."""
    import torch
    rng = None if perturb_seed is None else np.random.default_rng(perturb_seed)
    with _patched(mode, rng, eps) as pk_torch, torch.no_grad():
        return pk_torch.encode(model, dims, torch.from_numpy(np.ascontiguousarray(mel, F32))).numpy()


def rel_rms(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(((a - b) ** 2).mean() / (b ** 2).mean()))
