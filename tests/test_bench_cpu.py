"""bench.py without a device: the options of a plain run and the row sample --dump-outputs writes on meshes larger than
DUMP_MAX_ROWS (the GPU side is tests/test_gpu_bench_contract.py)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


class _Op:
    """the two diagnostics calls dump_outputs makes"""

    def update_diagnostics(self):
        pass

    def get_diagnostics(self):
        from rdycore_amd.operator import CourantNumberDiagnostics
        return CourantNumberDiagnostics(0.25, 17, 4)


def test_plain_run_is_the_default():
    a = bench.parse(["--gpus", "1", "--steps", "5", "--warmup", "1"])
    assert a.full is False and a.dump_outputs is None and a.steps == 5 and a.warmup == 1
    assert bench.parse(["--full", "--dump-outputs", "d"]).full is True


def test_dump_sample_is_fixed_and_bounded(tmp_path, monkeypatch):
    # the bound at the real sample size: F rows and their indices, float64
    assert bench.DUMP_MAX_ROWS * (3 + 1) * 8 <= 64e6
    monkeypatch.setattr(bench, "DUMP_MAX_ROWS", 1000)
    f = torch.arange(3 * 25000, dtype=torch.float64).reshape(25000, 3)
    got = []
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), _Op(), f)
        got.append([np.load(tmp_path / run / (n + ".npy")) for n in ("rhs", "rhs_rows", "courant")])
    (rhs, rows, courant), (rhs2, rows2, courant2) = got
    assert rhs.dtype == rows.dtype == courant.dtype == np.float64
    assert rows.shape == (1000,) and np.all(np.diff(rows) > 0) and rows[-1] < 25000
    assert np.array_equal(rhs, f.numpy()[rows.astype(np.int64)])
    assert np.array_equal(rows, rows2) and np.array_equal(rhs, rhs2) and np.array_equal(courant, courant2)
    assert courant.tolist() == [0.25, 17.0, 4.0]
