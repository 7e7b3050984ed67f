"""GPU: `bench.py --dump-outputs DIR` writes what the last timed step computed (losses, generator output, G / EMA / D parameters)
as float32 / float64 .npy files within 64 MB, from inputs that are the same on every run with the same arguments.  The benchmark's
step runs in the deterministic mode (fixed-order reductions, tests/test_gpu_deterministic.py), so two runs with the default arithmetic
must write identical files; a run with one more timed step must not (the dump is the state after the timed steps)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir, steps):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "2", "--batch", "2",
           "--blocks", "1", "--no-cpu-baseline", "--no-roofline", "--blocks-timed", "0", "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0]), {f[:-4]: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))}


def test_dump_outputs_of_two_runs_are_identical(tmp_path):
    line, a = _bench(tmp_path / "a", 3)
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["losses_finite"] and line["config"]["deterministic"]
    assert {"loss_l_g_pix", "loss_l_g_gan", "loss_l_d_real", "loss_l_d_fake", "output", "d_sn_uv"} <= set(a), sorted(a)
    for net in ("g_params", "g_ema_params", "d_params"):
        assert net in a or net + "_sample" in a, (net, sorted(a))
    assert a["output"].shape == (2, 3, 128, 128)
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    for k, v in a.items():
        assert v.dtype in (np.float32, np.float64) and np.isfinite(v).all(), k
    _, b = _bench(tmp_path / "b", 3)
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), f"'{k}' differs between two runs with the same arguments"
    # the dump is the state after the timed steps: one more timed step moves the parameters and the generator output
    _, c = _bench(tmp_path / "c", 4)
    assert sorted(a) == sorted(c)
    for k in [n for n in a if n.startswith(("g_params", "g_ema_params", "d_params"))] + ["output"]:
        assert not np.array_equal(a[k], c[k]), f"'{k}' is the same after 3 and 4 timed steps"
