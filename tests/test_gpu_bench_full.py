"""GPU: a plain `bench.py` run prints the headline line and measures nothing beyond its timed steps; `--full` adds, in the same
process, the further timed blocks, the roofline of an instrumented step and the CPU baseline."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("ms_per_step_blocks", "ms_per_step_median_of_blocks", "roofline", "kernel_time_breakdown_ms", "roofline_by_kernel",
             "legs", "modes", "max_rel_err_vs_oracle", "cpu_baseline")


def _bench(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "2", "--batch", "2",
           "--blocks", "1", *extra]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_prints_the_headline_only_and_full_adds_the_rest():
    plain = _bench()
    assert plain["metric"] == "G+D train-step images/sec" and plain["unit"] == "images/s" and plain["higher_is_better"] is True
    assert plain["dtype"] == "fp32h" and plain["steps"] == 2 and plain["ms_per_step"] > 0 and plain["losses_finite"]
    assert plain["value"] == pytest.approx(2 * 1000.0 / plain["ms_per_step"], rel=1e-6)
    assert not set(FULL_ONLY) & set(plain), sorted(set(FULL_ONLY) & set(plain))

    full = _bench("--full", "--blocks-timed", "1", "--cpu-steps", "1")
    assert full["dtype"] == "fp32h" and full["steps"] == 2 and full["ms_per_step"] > 0 and full["losses_finite"]
    assert len(full["ms_per_step_blocks"]) == 1 and full["ms_per_step_median_of_blocks"] > 0
    assert full["roofline"]["frac"] > 0 and full["kernel_time_breakdown_ms"] and full["roofline_by_kernel"]
    assert full["cpu_baseline"]["value"] > 0 and full["cpu_baseline"]["kind"] == "port"
