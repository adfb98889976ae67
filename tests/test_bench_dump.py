"""bench.py --dump-outputs (CPU): float64 files, a fixed sample of an array beyond its share, the same sample run after run."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_writes_float64_and_samples_large_arrays_the_same_way_every_time(tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(bench, "DUMP_BYTES", {"particles": 8 * 300, "ancestors": 8 * 50})
    rng = np.random.default_rng(1)
    arrays = {"ll": [-1.25], "particles": rng.standard_normal((3, 1000)), "ancestors": np.arange(40, dtype=np.uint32),
              "ll_steps": rng.standard_normal(20)}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays)
    got = {f: np.load(tmp_path / "a" / f) for f in sorted(os.listdir(tmp_path / "a"))}
    assert sorted(got) == ["ancestors.npy", "ll.npy", "ll_steps.npy", "particles.npy"]
    assert all(a.dtype == np.float64 for a in got.values())
    for f, a in got.items():
        assert np.array_equal(a, np.load(tmp_path / "b" / f))
    # within its share: whole; beyond it: columns of the cloud, every latent component of the same particles
    assert np.array_equal(got["ancestors.npy"], np.arange(40)) and got["ll.npy"].tolist() == [-1.25]
    p = got["particles.npy"]
    assert p.shape == (3, 100)
    idx = np.sort(np.random.default_rng(0).choice(1000, 100, replace=False))
    assert np.array_equal(p, arrays["particles"][:, idx])


def test_dump_shares_stay_within_64_mb():
    sys.path.insert(0, ROOT)
    import bench
    assert sum(bench.DUMP_BYTES.values()) + (1 << 20) <= 64 << 20
