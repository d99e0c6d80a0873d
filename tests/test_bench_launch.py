"""bench.py's launch paths, executed here on the CPU emulator build of the kernels (--emu, gloo):
`python bench.py --gpus 2` outside any launcher starts its own two ranks (the command the driver uses for N = 1 is the
same file, same function), a plain N = 1 run ends with the headline figure, and with --full the N = 1 path carries `parity`
and `cpu_baseline` from the oracle leg."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = ["--emu", "--steps", "1", "--warmup", "0", "--windows", "1", "--height", "32", "--width", "40", "--dtype", "fp32"]


def _run(extra, tiny=TINY):
    env = dict(os.environ, MAPNET_EMU_THREADS="4")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + extra + tiny, env=env, capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]  # ONE JSON line, from rank 0 only
    return json.loads(lines[0])


@pytest.mark.slow
def test_bench_self_launches_two_ranks():
    d = _run(["--gpus", "2", "--no-cpu-baseline"])
    assert d["n_gpus"] == 2 and d["config"]["n_ranks_seen"] == 2 and d["config"]["parallelism"] == "dp2"
    assert d["config"]["launcher"] == "torch.distributed.run"
    assert d["config"]["global_windows"] == 2 and d["scaling"] == "weak"
    assert d["value"] > 0 and d["unit"] == "images/s" and "cpu_baseline" not in d


@pytest.mark.slow
def test_bench_single_rank_reports_parity_and_cpu_baseline():
    d = _run(["--gpus", "1", "--full"])
    assert d["n_gpus"] == 1 and d["config"]["launcher"].startswith("none") and d["full"] is True
    p = d["parity"]
    assert p["dtype"] == "fp32" and p["loss_rel"] <= 1e-4 and p["pose_abs_max"] <= 1e-3, p
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["value"] > 0 and c["cores"] >= 1 and c["cpu"]


@pytest.mark.slow
def test_bench_plain_run_ends_with_the_headline_figure():
    """without --full: the result line of the timed steps and none of the legs that take runs of their own"""
    d = _run(["--gpus", "1"])
    assert d["full"] is False and d["n_gpus"] == 1 and d["steps"] == 1 and d["warmup"] == 0
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["unit"] == "images/s" and d["higher_is_better"] is True
    assert d["metric"] and d["dtype"] == "f32" and d["roofline"] is None
    for leg in ("cpu_baseline", "parity", "meets_tolerance", "fast_mode", "parity_mode", "parity_mode_full", "experimental_mode",
                "input_feed", "eval_metric"):
        assert leg not in d, leg


@pytest.mark.gpu
def test_bench_plain_run_on_the_device_takes_no_run_of_its_own():
    """on the device, where --emu drops no leg by itself: a plain run in the default dtype carries no leg that takes a run of its own
    and no event-timed pass (`roofline` null)"""
    d = _run(["--gpus", "1"], ["--steps", "2", "--warmup", "1", "--windows", "2", "--height", "64", "--width", "85"])
    assert d["full"] is False and d["dtype_mode"] == "fp16x2m" and d["steps"] == 2 and d["warmup"] == 1
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["roofline"] is None and "not a measurement" not in d["data"].lower()
    for leg in ("cpu_baseline", "parity", "meets_tolerance", "fast_mode", "parity_mode", "parity_mode_full", "experimental_mode",
                "input_feed", "value_pcie_inclusive", "eval_metric"):
        assert leg not in d, leg


def test_bench_all_modes_needs_full():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--all-modes"] + TINY, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 2 and "--full" in r.stderr


@pytest.mark.slow
def test_bench_dumps_what_the_last_timed_step_returned(tmp_path):
    """the last timed step starts from the seeded initial state, so it returns what the first warm-up step returned"""
    d = _run(["--gpus", "1", "--no-cpu-baseline", "--dump-outputs", str(tmp_path)], TINY + ["--warmup", "1", "--steps", "2"])
    assert d["steps"] == 2 and d["ms_per_step"] > 0
    assert abs(d["config"]["loss_last"] - d["config"]["loss_first"]) <= 1e-4 * max(1.0, abs(d["config"]["loss_first"]))
    loss, poses = np.load(tmp_path / "loss.npy"), np.load(tmp_path / "poses.npy")
    assert loss.dtype == np.float64 and loss.shape == (1,) and poses.dtype == np.float32 and poses.shape == (1, 3, 6)
    assert np.isfinite(poses).all() and abs(float(loss[0]) - d["config"]["loss_last"]) <= 5e-5 * max(1.0, abs(float(loss[0])))
    assert sorted(d["dump_outputs"]["arrays"]) == ["loss", "poses"]


def test_bench_steps_are_the_timed_steps_in_all():
    """--steps K times K steps in all, split into at most --repeats regions of nearly equal length"""
    sys.path.insert(0, ROOT)
    import bench
    for steps in (1, 2, 5, 7, 50, 101):
        for repeats in (1, 3, 5, 200):
            sizes = bench.region_sizes(steps, repeats)
            assert sum(sizes) == steps and len(sizes) == min(steps, repeats) and max(sizes) - min(sizes) <= 1


def test_bench_rejects_a_launcher_rank_count_mismatch():
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"] + TINY, env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode != 0 and "started 1 ranks" in (r.stdout + r.stderr)
