"""``bench.py --dump-outputs DIR``: what a timed step returned is written as DIR/<name>.npy in float32,
and past the size budget as the elements at fixed seeded indices, the same on every call.  CPU only."""

import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import bench  # noqa: E402


def test_dump_names_and_dtype(tmp_path):
    out = (torch.arange(6, dtype=torch.bfloat16).reshape(2, 3), None, {"a": torch.ones(4, dtype=torch.bool), "b": 2.5})
    bench.dump_outputs(str(tmp_path / "d"), out)
    assert sorted(os.listdir(tmp_path / "d")) == ["out0.npy", "out2_a.npy", "out2_b.npy"]
    a = np.load(tmp_path / "d" / "out0.npy")
    assert a.dtype == np.float32 and a.shape == (2, 3) and np.array_equal(a.reshape(-1), np.arange(6))
    assert float(np.load(tmp_path / "d" / "out2_b.npy")) == 2.5


def test_dump_sample_is_bounded_and_fixed(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 4000)
    x, y = torch.randn(50, 40), torch.randn(3000)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"x": x, "y": y}, "o")
    a = {n: np.load(tmp_path / "a" / n) for n in ("o_x.npy", "o_y.npy")}
    assert sum(v.nbytes for v in a.values()) <= 4000 and all(v.ndim == 1 and v.dtype == np.float32 for v in a.values())
    assert a["o_x.npy"].size == 400 and a["o_y.npy"].size == 600  # shares of the budget by size
    assert np.isin(a["o_x.npy"], x.numpy()).all()
    for n, v in a.items():
        assert np.array_equal(v, np.load(tmp_path / "b" / n))


def test_no_dump_without_the_option(tmp_path):
    bench.dump_outputs(None, torch.zeros(3))
    assert os.listdir(tmp_path) == []
