"""bench.py's two modes: a plain run measures the headline alone; --full adds the bare-fill ceiling, the CPU baseline, the
secondary workloads (N = 1) and the gather-inclusive sample (N > 1, tests/test_gpu_world2.py)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def test_plain_arguments_turn_every_extra_measurement_off():
    import bench
    plain = bench.parse(["--steps", "3", "--warmup", "1"])
    assert not plain.full and plain.no_cpu and plain.no_secondary and plain.no_fill and plain.allgather_chunks == 0
    full = bench.parse(["--steps", "3", "--warmup", "1", "--full"])
    assert full.full and not (full.no_cpu or full.no_secondary or full.no_fill) and full.allgather_chunks == 8
    assert bench.parse(["--full", "--no-fill"]).no_fill


def _bench(args, timeout=600):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True,
                       timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert all(k in line for k in HEADLINE), sorted(line)
    rows = 2 * 4096 * 1031  # steps x witnesses x rows
    assert line["steps"] == 2 and abs(line["value"] * line["ms_per_step"] * 2 / 1e3 - rows) < 1e-6 * rows
    assert line["roofline"]["launches_timed"] == 2
    return line


@pytest.mark.gpu
def test_plain_run_is_the_headline_alone():
    line = _bench(["--gpus", "1", "--steps", "2", "--warmup", "1", "--log2-batch", "12"])
    assert "secondary" not in line and "cpu_baseline" not in line and "after_180_ms_of_warm_up" not in line
    assert "bare_fill" not in line["roofline"]


@pytest.mark.gpu
def test_full_run_measures_the_rest():
    line = _bench(["--gpus", "1", "--steps", "2", "--warmup", "1", "--log2-batch", "12", "--full", "--no-cpu"])
    assert "best" in line["roofline"]["bare_fill"], line["roofline"]["bare_fill"]
    sec = line["secondary"]
    for name in ("c3", "c4", "c2_values", "next_rows"):
        assert name in sec and "error" not in sec[name], (name, sec.get(name))
    assert "cpu_baseline" not in line  # (--no-cpu)
