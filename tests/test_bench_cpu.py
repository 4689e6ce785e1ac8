"""bench.py's output dump (--dump-outputs), on host tensors: no GPU needed."""
import numpy as np
import torch

import bench


def test_dump_outputs_writes_float32_arrays_whole_when_they_fit(tmp_path):
    a = torch.arange(24, dtype=torch.float32).reshape(4, 2, 3)
    b = torch.ones((4, 5))
    bench.dump_outputs(str(tmp_path / "out"), {"sinogram": a, "grad_image": b})
    got_a, got_b = np.load(tmp_path / "out" / "sinogram.npy"), np.load(tmp_path / "out" / "grad_image.npy")
    assert got_a.dtype == np.float32 and np.array_equal(got_a, a.numpy())
    assert got_b.dtype == np.float32 and np.array_equal(got_b, b.numpy())


def test_dump_outputs_keeps_the_same_seeded_objects_under_the_cap(tmp_path):
    """Beyond the cap every array keeps the same fixed choice of whole objects, within the cap in all, run after run."""
    a = torch.arange(100 * 6, dtype=torch.float32).reshape(100, 6)
    b = torch.arange(100 * 10, dtype=torch.float32).reshape(100, 10) * -1.0
    limit = a.numel() + b.numel()                  # a quarter of their bytes (4 per element)
    for run in ("one", "two"):
        bench.dump_outputs(str(tmp_path / run), {"a": a, "b": b}, limit=limit)
    got_a, got_b = np.load(tmp_path / "one" / "a.npy"), np.load(tmp_path / "one" / "b.npy")
    assert got_a.nbytes + got_b.nbytes <= limit and got_a.shape == (25, 6) and got_b.shape == (25, 10)
    idx = got_a[:, 0].astype(np.int64) // 6
    assert np.all(np.diff(idx) > 0) and np.array_equal(got_a, a.numpy()[idx]) and np.array_equal(got_b, b.numpy()[idx])
    assert np.array_equal(got_a, np.load(tmp_path / "two" / "a.npy")) and np.array_equal(got_b, np.load(tmp_path / "two" / "b.npy"))
