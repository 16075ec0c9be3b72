"""bench.py --dump-outputs, host side: every array lands as float32 DIR/<name>.npy, the dump stays within 64 MB, arrays
that fit are written whole, and the sample of one that does not is the same on every run (two builds are compared
output for output). The GPU side is tests/test_bench_line_gpu.py."""
import os

import numpy as np

import bench


def _arrays():
    rng = np.random.default_rng(3)
    return {"loss": np.float32([0.75]), "loss_terms": rng.random(3, dtype=np.float32),
            "distance": rng.random((8, 1, 100, 100), dtype=np.float32),
            "parameters": rng.random(10_581_723, dtype=np.float32),  # hidden 32: 42 MB of weights, as many gradients
            "gradients": rng.random(10_581_723, dtype=np.float32), "buffers": rng.random(10_126).astype(np.float64)}


def test_dump_fits_the_budget_and_samples_the_same_elements_every_run(tmp_path):
    arrays = _arrays()
    bench.write_outputs(arrays, str(tmp_path / "a"))
    bench.write_outputs(arrays, str(tmp_path / "b"))
    names = sorted(f for f in os.listdir(tmp_path / "a"))
    assert names == sorted(k + ".npy" for k in arrays)
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in names) <= bench.DUMP_MAX_BYTES
    for f in names:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype == np.float32 and np.array_equal(a, b), f
    for k in ("loss", "loss_terms", "distance", "buffers"):
        assert np.array_equal(np.load(tmp_path / "a" / (k + ".npy")), arrays[k].astype(np.float32)), k
    p = np.load(tmp_path / "a" / "parameters.npy")
    assert 0 < p.size < arrays["parameters"].size and np.isin(p, arrays["parameters"]).all()
