"""bench.py's command line: the plain run (headline figure only), --dump-outputs and --full.

CPU: the conversion of ScanPipeline.results() to the dumped float arrays and the size budget.
GPU: one plain run and one --full run of a small batch, each in a child process as the driver
starts it; the dumped arrays must equal a direct ScanPipeline run of warmup + steps calls."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
from lidar_slam_amd.pipeline import LANDMARK_DTYPE, MODEL_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCANS, STEPS, WARMUP, L = 48, 3, 1, 20
NAMES = {"mask", "y_proj", "models", "landmarks", "lmk_count", "ukf_x", "ukf_P"}


def fake_results(S=5, cap=4, per_scan=(3, 2)):
    rng = np.random.default_rng(7)
    C, P = S * len(per_scan), S * sum(per_scan)
    models = np.zeros(C, MODEL_DTYPE)
    for i, n in enumerate(MODEL_DTYPE.names):
        models[n] = rng.integers(1, 100, C) + i
    lm = np.zeros((S, cap), LANDMARK_DTYPE)
    for i, n in enumerate(LANDMARK_DTYPE.names):
        lm[n] = rng.integers(1, 100, (S, cap)) + i
    return {"mask": rng.integers(0, 2, P).astype(np.uint8), "y_proj": rng.normal(size=P), "models": models,
            "landmarks": lm, "lmk_count": np.array([0, 1, cap, 2, 3], np.int32)[:S],
            "ukf_x": rng.normal(size=(S, 3)), "ukf_P": rng.normal(size=(S, 3, 3))}


def test_output_arrays_fields_and_dtypes():
    r = fake_results()
    out = bench.output_arrays(r)
    assert set(out) == NAMES
    assert out["mask"].dtype == np.float32 and np.array_equal(out["mask"], r["mask"])
    assert all(a.dtype == np.float64 for k, a in out.items() if k != "mask")
    cols = [n for n in MODEL_DTYPE.names if n != "reserved"]
    assert out["models"].shape == (len(r["models"]), len(cols))
    for j, n in enumerate(cols):
        assert np.array_equal(out["models"][:, j], r["models"][n])
    # list slots at or past lmk_count are zero, the live ones are the records' fields
    for s, c in enumerate(r["lmk_count"]):
        assert not out["landmarks"][s, c:].any()
        for j, n in enumerate(LANDMARK_DTYPE.names):
            assert np.array_equal(out["landmarks"][s, :c, j], r["landmarks"][n][s, :c])
    assert np.array_equal(out["ukf_P"], r["ukf_P"])


def test_dump_outputs_budget_and_repeatability(tmp_path, monkeypatch):
    r = fake_results()
    full = bench.output_arrays(r)
    bench.dump_outputs(str(tmp_path / "a"), r)
    for k, a in full.items():
        assert np.array_equal(np.load(tmp_path / "a" / (k + ".npy")), a)
    total = sum(a.nbytes for a in full.values())
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", total // 2)
    bench.dump_outputs(str(tmp_path / "b"), r)
    bench.dump_outputs(str(tmp_path / "c"), r)
    got = {k: np.load(tmp_path / "b" / (k + ".npy")) for k in full}
    assert sum(a.nbytes for a in got.values()) <= total // 2
    for k, a in got.items():
        assert 1 <= len(a) < len(full[k]) and a.shape[1:] == full[k].shape[1:]
        assert np.array_equal(a, np.load(tmp_path / "c" / (k + ".npy")))


def run_bench(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup",
           str(WARMUP), "--scans", str(SCANS)] + list(extra)
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs(tmp_path):
    from lidar_slam_amd.device import Context
    from lidar_slam_amd.pipeline import ScanPipeline
    d = run_bench("--dump-outputs", str(tmp_path))
    assert d["steps"] == STEPS and d["warmup"] == WARMUP and d["n_gpus"] == 1
    assert d["unit"] == "scans/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["ms_per_step"] > 0
    assert abs(d["value"] - SCANS / (d["ms_per_step"] * 1e-3)) <= 1e-3 * d["value"]
    assert d["roofline"] is None and d["cpu_baseline"] is None and d["coupled"] is None and "c4" not in d
    assert d["capacity_overflows"] == 0
    assert {f[:-4] for f in os.listdir(tmp_path)} == NAMES
    # the same batch through the pipeline directly: warmup + steps calls from the initial state
    ids = list(range(SCANS))
    b, ukf = bench.make_workload(ids, 720, L)
    p = ScanPipeline(Context(0), b["xy"], b["scan_chunk_off"], b["chunk_pt_off"], seeds=np.array(ids, np.uint32),
                     max_trials=100, lmk_capacity=64, want_yproj=True, ukf=ukf)
    for _ in range(WARMUP + STEPS):
        p.run()
    want = bench.output_arrays(p.results())
    for k, a in want.items():
        got = np.load(tmp_path / (k + ".npy"))
        assert got.dtype == a.dtype and got.shape == a.shape, k
        assert np.array_equal(got, a, equal_nan=True), k


@pytest.mark.gpu
def test_full_run_adds_the_other_legs():
    d = run_bench("--full", "--cpu-sample", "4", "--cpu-per-proc", "1", "--cpu-procs", "2", "--cpu-sample-1core", "2")
    assert d["steps"] == STEPS and d["ms_per_step"] > 0 and d["unit"] == "scans/s"
    r = d["roofline"]
    assert r["bound"] == "valu" and r["kernel_ms"] > 0 and r["kernel_alone_ms"] > 0
    assert r["consensus"]["ms"] > 0 and r["pipeline"]["ms"] > 0
    assert d["cpu_baseline"]["value"] > 0 and d["cpu_baseline"]["value_1core"] > 0
    assert d["coupled"]["ms_per_step"] > 0 and d["coupled"]["all_finite"] is True
