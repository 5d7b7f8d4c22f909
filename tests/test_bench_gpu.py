"""bench.py's two kinds of run, each in a process of its own on a 10k-tet cube: a plain run prints the headline line and
nothing that takes steps or runs of its own; `--full` adds them (here `--full --no-cpu-baseline`: the roofline steps)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
BESIDE = ("roofline", "roofline_assembly", "roofline_combine", "concurrent_solves", "edit_loop", "scan_like", "config3", "batch64", "cpu_baseline",
          "resonator_bank", "cpu_bank_baseline")


def _bench(*extra):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--workload", "cube_s10k", *extra],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


def test_plain_run_is_the_headline_alone():
    line = _bench()
    assert all(k in line for k in HEADLINE)
    assert line["unit"] == "eigenpairs/s" and line["higher_is_better"] is True and line["dtype"] == "f64" and line["steps"] == 2 and line["warmup"] == 1
    assert line["value"] > 0 and line["ms_per_step"] > 0
    assert abs(line["value"] - line["config"]["eigenpairs_per_mesh"] * 1e3 / line["ms_per_step"]) < 1e-6 * line["value"]
    assert not [k for k in BESIDE if k in line]


def test_full_run_adds_the_roofline_steps():
    line = _bench("--full", "--no-cpu-baseline")
    assert all(k in line for k in HEADLINE) and line["value"] > 0
    assert line["roofline"]["launches"] > 0 and line["roofline"]["achieved"] > 0 and "measured_in" in line["roofline"]
    assert line["roofline_assembly"]["launches"] > 0 and line["roofline_combine"]["launches"] > 0
    assert not [k for k in ("concurrent_solves", "scan_like", "cpu_baseline", "resonator_bank") if k in line]
