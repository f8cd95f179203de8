"""bench.py's command line: --dump-outputs writes what the last timed step returned, --steps sets the timed steps, and a
plain run carries the headline only (the extras and the CPU baseline come with --full)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_writes_float_arrays(tmp_path):
    from bench import dump_outputs
    outs = {"pairs": np.arange(20, dtype=np.float64).reshape(10, 2), "T": np.eye(4), "counts": np.array([10.0, 3.0])}
    dump_outputs(outs, str(tmp_path / "d"))
    for name, a in outs.items():
        b = np.load(tmp_path / "d" / f"{name}.npy")
        assert b.dtype == np.float64 and np.array_equal(a, b)


def test_dump_outputs_samples_the_same_rows_over_budget(tmp_path):
    from bench import dump_outputs
    n = 100_000
    rows = np.arange(n, dtype=np.float64)
    outs = {"pairs": np.stack([rows, rows + 0.5], axis=1), "pts1": np.stack([rows] * 3, axis=1), "T": np.eye(4)}
    budget = 1 << 20
    for d in ("a", "b"):
        dump_outputs(outs, str(tmp_path / d), budget=budget)
    got = {name: np.load(tmp_path / "a" / f"{name}.npy") for name in outs}
    assert sum(a.nbytes for a in got.values()) <= budget
    assert 4096 <= got["pairs"].shape[0] < n
    assert np.array_equal(got["pairs"][:, 0], got["pts1"][:, 0])           # the same rows of both arrays
    assert np.array_equal(got["T"], np.eye(4))
    for name in outs:                                                        # fixed seed: the same sample every run
        assert np.array_equal(got[name], np.load(tmp_path / "b" / f"{name}.npy"))


def test_help_names_full_and_dump_outputs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    assert "--full" in r.stdout and "--dump-outputs" in r.stdout


@pytest.mark.gpu
def test_plain_run_dumps_the_same_outputs_twice(tmp_path):
    """Two plain runs with the same arguments: headline fields only, the given number of timed steps, identical outputs."""
    args = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--model-points", "200000", "--surface-points", "20000"]
    lines = []
    for d in ("a", "b"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args + ["--dump-outputs", str(tmp_path / d)],
                           capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        lines.append(json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1]))
    line = lines[0]
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == 3 and line["knn_kernel"]["launches_timed"] == 3 and line["ms_per_step"] > 0
    assert "extras" not in line and "cpu_baseline" not in line and "cfg5_batch" not in line
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(["pairs.npy", "pts1.npy", "pts2.npy", "T.npy", "inlier_idx.npy", "counts.npy"])
    for name in names:
        a, b = np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), name
    counts = np.load(tmp_path / "a" / "counts.npy")
    pairs = np.load(tmp_path / "a" / "pairs.npy")
    assert counts[0] == line["ransac"]["n_pairs"] == pairs.shape[0] > 1000
    assert counts[3] == line["ransac"]["max_inliers"] and counts[2] == line["ransac"]["num_success"]
