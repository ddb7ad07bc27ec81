"""The Parakeet int8 mode on the CPU: the numpy reference of its arithmetic (tests/pk_int8_ref.py,
DESIGN.md §9.7) on hand-made cases, and the model-directory loader's integer accessor
(spt_parakeet_onnx_qtensor): the integers, scales and zero points exactly as the file stores them."""
import numpy as np
import pytest

from oracle import parakeet as P
from tests import onnx_parakeet, pk_int8_ref as R


def test_rounding_is_half_to_even():
    # range 255 -> scale exactly 1, zero point 0
    x = np.array([0.0, 0.5, 1.5, 2.5, 255.0], np.float32)
    q, s, z = R.dynamic_quantize(x)
    assert s == np.float32(1) and z == 0
    assert list(q) == [0, 0, 2, 2, 255]


def test_zero_points_of_one_sided_ranges():
    q, s, z = R.dynamic_quantize(np.array([1.0, 2.0, 3.0], np.float32))
    assert z == 0 and s == np.float32(3) / np.float32(255) and q[-1] == 255
    q, s, z = R.dynamic_quantize(np.array([-1.0, -2.0, -3.0], np.float32))
    assert z == 255 and q[-1] == 0 and q.max() <= 255
    q, s, z = R.dynamic_quantize(np.zeros(7, np.float32))
    assert s == 0 and z == 0 and not q.any()


def test_saturation_at_both_ends():
    x = np.array([-1.0, 0.0, 2.0], np.float32)
    q, s, z = R.dynamic_quantize(x)
    assert q[0] == 0 and q[2] == 255 and q[1] == z == 85
    # values outside the range the scale was taken from clamp (the engine's padded rows)
    y = np.clip(np.rint(np.array([-5.0, 9.0], np.float32) / s) + np.float32(z), 0, 255)
    assert list(y) == [0, 255]


def test_extreme_k4096_stays_in_int32():
    K = 4096
    q = np.full((1, K), 255, np.uint8)
    for w, zw in ((np.full((2, K), 255, np.uint8), 0), (np.full((2, K), -128, np.int8), 127)):
        acc = R.matmul_integer(q, 0, w, zw)
        assert acc.dtype == np.int32 and abs(int(acc[0, 0])) == 255 * 255 * K
    assert 255 * 255 * K < 2 ** 31


def test_qlinear_groups_have_their_own_ranges():
    rng = np.random.default_rng(0)
    x = rng.standard_normal((5, 64)).astype(np.float32)
    x[3:] *= 7
    w = rng.integers(-127, 128, (16, 64)).astype(np.int8)
    r = R.qlinear(x, [3, 2], w, np.float32(0.01), 0)
    a = R.qlinear(x[:3], [3], w, np.float32(0.01), 0)
    b = R.qlinear(x[3:], [2], w, np.float32(0.01), 0)
    assert r["sa"][0] == a["sa"][0] and r["sa"][1] == b["sa"][0] and r["sa"][0] != r["sa"][1]
    assert np.array_equal(r["y"], np.concatenate([a["y"], b["y"]]))


@pytest.fixture(scope="module")
def small():
    d = P.dims_for("test-small")
    return d, P.Model(d, seed=21)


SHAPES = {5: lambda d: (d.sub_ch, d.sub_ch), 11: lambda d: (d.d, d.sub_ch * (d.n_mels // 8)),
          1002: lambda d: (d.ff, d.d), 1016: lambda d: (d.d, d.d), 1029: lambda d: (d.d, d.d)}


@pytest.mark.parametrize("quant", ["int8", "uint8pc"])
def test_loader_keeps_the_stored_integers(tmp_path, small, quant):
    from spittle_amd.parakeet import OnnxModelDir
    d, m = small
    onnx_parakeet.write_dir(str(tmp_path), m, d, quant=quant)
    h = OnnxModelDir(str(tmp_path))
    for tid, shape in SHAPES.items():
        N, K = shape(d)
        w = m.tensor(tid).reshape(N, K)
        # what the writer stores: Linear weights quantised as W^T [K][N] along N, convolutions
        # [out][in][1][1] along out -- per tensor, or per output channel: the rows of [N][K] either way
        q, s, zp, deq = onnx_parakeet.quantize(w, quant, 0)
        got = h.qtensor(tid)
        assert got is not None, tid
        gq, gs, gz = got
        assert gq.dtype == np.int16 and gq.size == N * K
        assert np.array_equal(gq.reshape(N, K), q.astype(np.int16)), tid
        assert np.array_equal(gs, np.atleast_1d(s)) and gs.dtype == np.float32, tid
        assert np.array_equal(gz, np.atleast_1d(zp).astype(np.int32)), tid
        assert gs.size == (1 if quant == "int8" else N)
        # and the dequantised tensor is still what the f32 accessor returns
        f = h.tensor(tid)
        want = ((gq.reshape(N, K).astype(np.float32) - gz.astype(np.float32)[:, None]) * gs[:, None]).ravel()
        assert np.array_equal(f, want) and np.array_equal(f, deq.ravel()), tid
    assert h.qtensor(1000) is None and h.qtensor(6) is None  # LayerNorm weight, a bias: no integer op
    h.close()


def test_qdq_and_float_directories_have_no_integer_tensors(tmp_path, small):
    from spittle_amd.parakeet import OnnxModelDir
    d, m = small
    for i, kw in enumerate((dict(quant="int8", qdq=True), dict(quant=""))):
        p = tmp_path / str(i)
        onnx_parakeet.write_dir(str(p), m, d, **kw)
        h = OnnxModelDir(str(p))
        assert h.qtensor(1002) is None and h.tensor(1002) is not None
        h.close()
