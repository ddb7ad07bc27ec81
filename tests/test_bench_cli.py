"""bench.py's command line (CPU): a plain run asks for nothing beside the headline figure, --full
switches the other legs on, and --dump-outputs writes one batched call's results as float arrays."""
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import bench


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_and_full_options(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "3", "--warmup", "1")
    assert (a.gpus, a.steps, a.warmup) == (1, 3, 1) and not a.full and a.dump_outputs is None
    a = _parse(monkeypatch, "--full", "--dump-outputs", "d")
    assert a.full and a.dump_outputs == "d"
    assert _parse(monkeypatch, "--full", "--parakeet-only").parakeet_only


def test_parakeet_only_needs_full(monkeypatch):
    with pytest.raises(SystemExit):
        _parse(monkeypatch, "--parakeet-only")


def test_dump_outputs_writes_float_arrays(tmp_path):
    res = [SimpleNamespace(tokens=[50257 + i, 7, 51864], top1=np.float32([-0.5, -1.0, -2.0 - i]),
                           top2=np.float32([-3.0, -4.0, -5.0])) for i in range(2)]
    bench.dump_outputs(str(tmp_path / "o"), res, 0)
    bench.dump_outputs(str(tmp_path / "o"), res, 1)
    tok = np.load(tmp_path / "o" / "tokens.npy")
    assert tok.dtype == np.float64 and tok.tolist() == [[50257, 7, 51864], [50258, 7, 51864]]
    for n in ("top1", "top2"):
        a = np.load(tmp_path / "o" / f"{n}.npy")
        assert a.dtype == np.float32 and a.shape == (2, 3)
        np.testing.assert_array_equal(a, np.stack([getattr(r, n) for r in res]))
    assert sorted(p.name for p in (tmp_path / "o").iterdir()) == [
        "tokens.npy", "tokens_rank1.npy", "top1.npy", "top1_rank1.npy", "top2.npy", "top2_rank1.npy"]
