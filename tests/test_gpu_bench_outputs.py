"""bench.py --dump-outputs: two runs with the same arguments time exactly --steps steps and write the same answers of their last
timed step (the inputs are seeded): one row per query the step answered, scores float32, ids / counts / totals float64.  A plain run
and a --full run of the same arguments write the same answers."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--quick", "--no-topk-count", "--steps", "3", "--warmup", "1",
           "--dump-outputs", str(out_dir)] + list(extra)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    dumped = {f[:-4]: np.load(os.path.join(out_dir, f)) for f in os.listdir(out_dir)}
    return line, dumped


@pytest.mark.parametrize("workload,rows,k", [("bm25", 2 * 1000, 10), ("vec", 64, 100)])  # (--quick: 2 calls of 1000 queries per step)
def test_bench_dumps_the_last_step_the_same_from_run_to_run(tmp_path, workload, rows, k):
    runs = [_bench(tmp_path / f"run{i}", "--workload", workload) for i in range(2)]
    for line, dumped in runs:
        assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
        assert sorted(dumped) == ["count", "doc", "score", "total"]
        assert dumped["score"].dtype == np.float32 and dumped["score"].shape == (rows, k)
        assert dumped["doc"].dtype == np.float64 and dumped["doc"].shape == (rows, k)
        assert np.all(dumped["count"] == k) and np.all(np.diff(dumped["score"], axis=1) <= 0)
    (_, a), (_, b) = runs
    for n in a:
        assert np.array_equal(a[n], b[n]), n


@pytest.mark.parametrize("workload", ["bm25", "vec"])
def test_bench_full_run_answers_like_the_plain_run(tmp_path, workload):
    """--full adds the secondary legs around the timed steps of a plain run: the same headline keys, the same answers of the last
    timed step; the plain line carries no secondary section"""
    plain, a = _bench(tmp_path / "plain", "--workload", workload)
    full, b = _bench(tmp_path / "full", "--workload", workload, "--full")
    for key in ("metric", "unit", "higher_is_better", "dtype", "steps", "warmup", "config"):
        assert plain[key] == full[key], key
    assert plain["ms_per_step"] > 0 and full["ms_per_step"] > 0
    assert "roofline" in full and "details" in full
    assert not {"roofline", "latency_ms", "cpu_baseline", "vector", "details"} & set(plain), sorted(plain)
    assert sorted(a) == sorted(b)
    for n in a:
        assert np.array_equal(a[n], b[n]), n
