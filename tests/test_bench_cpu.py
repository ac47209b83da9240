"""bench.py --dump-outputs (bench.dump_outputs): every array in float64, and above the size limit the same seeded sample of
leaves from each array, with their indices."""
import os

import numpy as np

import bench


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def test_dump_outputs_writes_every_array_in_float64(tmp_path):
    L = 1000
    params = np.arange(2 * L, dtype=np.float64).reshape(L, 2) / 7
    errs = np.arange(L, dtype=np.uint64) * 3
    bench.dump_outputs(str(tmp_path), {"leaf_params": params, "leaf_max_error": errs}, [1.5, 2, 3])
    got = _load(str(tmp_path))
    assert sorted(got) == ["aggregates", "leaf_max_error", "leaf_params"]
    assert all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(got["leaf_params"], params)
    assert np.array_equal(got["leaf_max_error"], errs.astype(np.float64))
    assert np.array_equal(got["aggregates"], [1.5, 2.0, 3.0])


def test_dump_outputs_samples_the_same_leaves_under_the_limit(tmp_path):
    L, limit = 200_000, 2_000_000
    params = np.random.default_rng(1).random((L, 2))
    errs = np.arange(L, dtype=np.uint64)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"leaf_params": params, "leaf_max_error": errs}, [0.5], limit=limit)
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert sorted(a) == ["aggregates", "leaf_index", "leaf_max_error", "leaf_params"]
    assert all(np.array_equal(a[k], b[k]) for k in a)                   # a fixed sample: two runs compare file for file
    idx = a["leaf_index"].astype(np.int64)
    assert 0 < len(idx) < L and np.all(np.diff(idx) > 0)
    assert np.array_equal(a["leaf_params"], params[idx]) and np.array_equal(a["leaf_max_error"], idx.astype(np.float64))
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= limit
