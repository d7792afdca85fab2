"""bench.py --dump-outputs (bench.dump_outputs) on CPU tensors: dtypes, values, the size budget and its fixed row sample."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")


def _step_like(n=12, k=16, d=32, seed=0):
    g = torch.Generator().manual_seed(seed)
    cnt = torch.randint(0, k + 1, (n - 1,), generator=g, dtype=torch.int32)
    return {"idx": torch.randint(0, 784, (n, k), generator=g, dtype=torch.int32),
            "descriptors": torch.randn((n, k, d), generator=g),
            "matches": torch.randint(0, k, (n - 1, k, 2), generator=g, dtype=torch.int64),
            "quality": torch.rand((n - 1, k), generator=g),
            "match_count": cnt, "n_local_pairs": n - 1}


def _load(path):
    return {f[:-4]: np.load(os.path.join(path, f)) for f in sorted(os.listdir(path))}


def test_dump_writes_every_tensor_as_float_with_its_values(tmp_path):
    import bench
    out = _step_like()
    info = bench.dump_outputs(out, str(tmp_path))
    got = _load(tmp_path)
    assert sorted(got) == ["descriptors", "idx", "match_count", "matches", "quality"] and info["sampled_rows"] == {}
    assert got["descriptors"].dtype == np.float32 and got["quality"].dtype == np.float32
    assert got["idx"].dtype == np.float64 and got["matches"].dtype == np.float64 and got["match_count"].dtype == np.float64
    for k in got:
        assert np.array_equal(got[k], out[k].numpy()), k


def test_dump_stays_within_its_budget_with_a_fixed_row_sample(tmp_path):
    import bench
    out = _step_like(n=64, k=32, d=128)
    budget = 200_000                      # descriptors alone: 64 x 32 x 128 x 4 B = 1 MiB
    a, b = tmp_path / "a", tmp_path / "b"
    info = bench.dump_outputs(out, str(a), budget=budget)
    bench.dump_outputs(_step_like(n=64, k=32, d=128), str(b), budget=budget)
    got = _load(a)
    assert sum(v.nbytes for v in got.values()) == info["bytes"] <= budget
    assert "descriptors" in info["sampled_rows"] and "descriptors_rows" in got
    rows = got["descriptors_rows"].astype(np.int64)
    assert 1 <= rows.size < 64 and np.all(np.diff(rows) > 0)
    assert np.array_equal(got["descriptors"], out["descriptors"].numpy()[rows])
    other = _load(b)                      # same shapes and content: the same files, bit for bit
    assert sorted(other) == sorted(got) and all(np.array_equal(other[k], got[k]) for k in got)
