"""bench.py's command line: the plain run's result line, --dump-outputs and --full (the benchmark itself runs on the
GPU; its options and the dump format are checked here)."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench_mod", BENCH)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_bench_options_are_declared():
    res = subprocess.run([sys.executable, BENCH, "--help"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    for opt in ("--steps", "--warmup", "--gpus", "--full", "--dump-outputs"):
        assert opt in res.stdout


def test_bench_refuses_zero_steps_before_touching_a_device():
    res = subprocess.run([sys.executable, BENCH, "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 2 and "--steps" in res.stderr


def test_dump_outputs_writes_small_outputs_whole(tmp_path):
    bench = _bench_module()
    y = torch.randn(2, 3, 50)
    bench.dump_outputs(str(tmp_path), y)
    got = np.load(tmp_path / "y.npy")
    assert got.dtype == np.float32 and np.array_equal(got, y.numpy())
    assert not (tmp_path / "y_index.npy").exists()


def test_dump_outputs_samples_large_outputs_at_fixed_positions(tmp_path, monkeypatch):
    bench = _bench_module()
    monkeypatch.setattr(bench, "DUMP_FULL_BYTES", 4 * 1000)
    monkeypatch.setattr(bench, "DUMP_SAMPLES", 500)
    y = torch.randn(4, 8, 300)
    for sub in ("a", "b"):
        bench.dump_outputs(str(tmp_path / sub), y)
    idx = np.load(tmp_path / "a" / "y_index.npy")
    sample = np.load(tmp_path / "a" / "y.npy")
    assert idx.dtype == np.float64 and sample.dtype == np.float32 and idx.shape == sample.shape == (500,)
    assert np.all(np.diff(idx) > 0) and idx[-1] < y.numel()
    assert np.array_equal(sample, y.reshape(-1).numpy()[idx.astype(np.int64)])
    assert np.array_equal(idx, np.load(tmp_path / "b" / "y_index.npy"))       # seeded: the same positions every run


def _run_bench(tmp_path, tag, *extra):
    out_dir = tmp_path / tag
    res = subprocess.run([sys.executable, BENCH, "--config", "cfg0", "--steps", "5", "--warmup", "2",
                          "--dump-outputs", str(out_dir), *extra], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-2000:])
    line = json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1])
    return line, np.load(out_dir / "y.npy")


@pytest.mark.gpu
def test_plain_bench_run_reports_its_steps_and_dumps_the_last_output(tmp_path):
    line, y = _run_bench(tmp_path, "graph")
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in line
    assert line["steps"] == 5 and line["warmup"] == 2 and line["ms_per_step"] > 0
    assert not {"roofline", "end_to_end", "cpu_baseline"} & set(line)          # a plain run is the headline only
    assert y.dtype == np.float32 and y.shape == (1, 8, 32768 - 128 + 1) and np.isfinite(y).all()
    # the eager launches of the same steps compute the same output from the same seeded inputs
    _, y_eager = _run_bench(tmp_path, "eager", "--no-graph")
    assert np.array_equal(y, y_eager)
