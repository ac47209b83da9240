"""bench.py as it is run for every change: a plain run prints the headline line and nothing that takes runs of its own, and
--dump-outputs writes what its last timed step computed -- the arrays a Trainer gives for the same generated keys."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_plain_run_dumps_its_last_step(tmp_path):
    n, L = 2_000_000, 16384
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "6", "--warmup", "2",
           "--keys", str(n), "--leaves", str(L), "--dump-outputs", str(out)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert d["unit"] == "keys/s" and d["higher_is_better"] is True and d["dtype"] == "f64" and d["steps"] == 6
    assert d["ms_per_step"] > 0 and d["value"] > 0
    assert d["cpu_baseline"] is None and not {"configs", "parity_check", "fast_mode", "long_protocol", "env"} & set(d)

    got = {f[:-4]: np.load(os.path.join(out, f)) for f in os.listdir(out)}
    assert sorted(got) == ["aggregates", "leaf_count", "leaf_max_error", "leaf_params", "leaf_start"]
    assert all(a.dtype == np.float64 for a in got.values())

    from rmi_amd import train
    tr = train.Trainer(device=0)
    tr.generate_keys("uniform", np.uint64, n, 0, n)
    g = tr.train_leaves(tr.fit_root("linear", L), "linear", L).materialize()
    tr.close()
    assert np.array_equal(got["leaf_params"], g.leaf_params)
    assert np.array_equal(got["leaf_max_error"], g.last_layer_max_l1s.astype(np.float64))
    assert np.array_equal(got["leaf_count"], g.leaf_counts.astype(np.float64))
    assert np.array_equal(got["leaf_start"], g.leaf_starts[:-1].astype(np.float64))
    assert got["aggregates"][4] == g.model_max_error and got["aggregates"][5] == g.model_max_error_idx
    assert np.allclose(got["aggregates"][:4], [g.model_avg_error, g.model_avg_l2_error, g.model_avg_log2_error, g.model_max_log2_error],
                       rtol=1e-12, atol=0.0)
