"""bench.py's result line and `--dump-outputs DIR`: a plain run times the headline step only and can write what its last timed
step handed the caller (logits, loss, parameter gradients) as float32 .npy within 64 MB; `--full` keeps the roofline, the
per-launch times and the secondary runs.  The budget and the argument checks need no GPU; the runs do."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE_KEYS = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _bench(*argv, timeout=600):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], env=env, capture_output=True, text=True,
                          timeout=timeout)


def _line(res):
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    return json.loads(lines[0])


def test_dump_keeps_whole_logits_within_the_budget(tmp_path):
    import bench
    logits = np.arange(2 * 3 * 50, dtype=np.float32).reshape(2, 3, 50, 1)
    bench.write_outputs(str(tmp_path), {"logits": logits, "loss": np.float32(0.5), "grad.w": np.ones((4, 4), np.float32)})
    assert sorted(os.listdir(tmp_path)) == ["grad.w.npy", "logits.npy", "loss.npy"]
    assert np.array_equal(np.load(tmp_path / "logits.npy"), logits)
    assert np.load(tmp_path / "loss.npy").dtype == np.float32 and float(np.load(tmp_path / "loss.npy")) == 0.5


def test_dump_samples_points_beyond_the_budget(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 40_000)
    logits = np.arange(4 * 5 * 2000, dtype=np.float32).reshape(4, 5, 2000, 1)      # 160 kB: does not fit
    arrays = {"logits": logits, "loss": np.float32(1.0), "grad.w": np.ones((8, 8), np.float32)}
    bench.write_outputs(str(tmp_path), arrays)
    files = sorted(os.listdir(tmp_path))
    assert files == ["grad.w.npy", "logits_points_sample.npy", "logits_points_sample_index.npy", "loss.npy"]
    assert sum(os.path.getsize(tmp_path / f) for f in files) <= 40_000
    sample, idx = np.load(tmp_path / "logits_points_sample.npy"), np.load(tmp_path / "logits_points_sample_index.npy")
    assert sample.dtype == np.float32 and idx.dtype == np.float64 and sample.shape == (4, 5, idx.size, 1) and idx.size > 0
    assert np.array_equal(sample, logits[:, :, idx.astype(np.int64)])
    other = tmp_path / "again"
    bench.write_outputs(str(other), arrays)                                         # the sample is fixed: same points every run
    assert np.array_equal(np.load(other / "logits_points_sample_index.npy"), idx)


@pytest.mark.parametrize("argv", [("--steps", "0"), ("--warmup", "-1")])
def test_step_counts_are_checked_before_anything_runs(argv):
    res = _bench(*argv, timeout=120)
    assert res.returncode == 2 and argv[0] in res.stderr, res.stderr[-2000:]


@pytest.mark.gpu
def test_plain_run_times_the_headline_and_dumps_its_last_step(tmp_path):
    out = _line(_bench("--config", "2", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path)))
    assert all(k in out for k in HEADLINE_KEYS)
    assert out["steps"] == 3 and out["warmup"] == 1 and out["ms_per_step"] > 0 and out["higher_is_better"] is True
    assert out["value"] == pytest.approx(4 * 10000 / (out["ms_per_step"] * 1e-3))
    for k in ("roofline", "launches", "cpu_baseline"):                                # --full only
        assert k not in out
    assert not {"named_modes", "dropout_off", "math_fp32", "default_path"} & set(out["config"])
    files = sorted(os.listdir(tmp_path))
    assert "logits.npy" in files and "loss.npy" in files and any(f.startswith("grad.") for f in files)
    assert sum(os.path.getsize(tmp_path / f) for f in files) <= 64 * 1000 * 1000
    logits = np.load(tmp_path / "logits.npy")
    assert logits.dtype == np.float32 and logits.shape == (4, 39, 10000, 1) and np.isfinite(logits).all()
    assert float(np.load(tmp_path / "loss.npy")) == pytest.approx(out["config"]["loss"], rel=1e-6)
    gn = np.sqrt(sum(float((np.load(tmp_path / f).astype(np.float64) ** 2).sum()) for f in files if f.startswith("grad.")))
    assert gn == pytest.approx(out["config"]["grad_norm"], rel=1e-5)


@pytest.mark.gpu
def test_full_run_keeps_the_roofline_and_the_launches():
    out = _line(_bench("--full", "--headline-only", "--no-cpu-baseline", "--config", "2", "--steps", "2", "--warmup", "1"))
    assert all(k in out for k in HEADLINE_KEYS) and out["steps"] == 2
    assert out["roofline"]["launch_ms"] > 0 and out["launches"] and out["launches_live"]
