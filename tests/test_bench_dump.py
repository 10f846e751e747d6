"""bench.py --dump-outputs: what the timed path computed, as float32 .npy files within 64 MB, the same rows every run.  CPU only."""
import importlib.util
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_dump_is_exact_bounded_and_reproducible(tmp_path):
    b = _bench()
    rng = np.random.default_rng(7)
    status = rng.integers(0, 10, 1 << 19, dtype=np.uint8)
    gt = rng.integers(0, 256, (1 << 19, 384), dtype=np.uint8)             # 192 MiB of Gt bytes: must be sampled
    for d in ("a", "b"):
        b.dump_outputs(str(tmp_path / d), {"status": status, "gt": gt})
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["gt.npy", "gt_rows.npy", "status.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= b.DUMP_BUDGET_BYTES
    for f in files:
        a = np.load(tmp_path / "a" / f)
        assert a.dtype in (np.float32, np.float64)
        assert np.array_equal(a, np.load(tmp_path / "b" / f))
    assert np.array_equal(np.load(tmp_path / "a" / "status.npy"), status)  # small enough: whole and exact
    rows = np.load(tmp_path / "a" / "gt_rows.npy").astype(np.int64)
    assert np.all(np.diff(rows) > 0) and np.array_equal(np.load(tmp_path / "a" / "gt.npy"), gt[rows])


def test_dump_and_steps_arguments_are_checked_before_any_gpu_work():
    for extra, msg in ((["--steps", "0"], "--steps must be >= 1"), (["--workload", "hash", "--dump-outputs", "x"], "--dump-outputs")):
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + extra, capture_output=True, text=True, timeout=120)
        assert p.returncode != 0 and msg in p.stderr, p.stderr
