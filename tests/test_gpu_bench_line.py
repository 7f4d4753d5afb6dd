"""bench.py on one GPU without --full: the lean line (the headline figure and nothing that needs runs of its own) and the arrays
--dump-outputs writes, which must be the same on two runs with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("time_to_converge_ms", "one_shot_ms_including_upload", "class_surface", "class_surface_rig", "per_solve_us_per_iteration",
             "converged", "roofline", "roofline_fp64", "sweep_kernel_alone", "kernel_ms_per_launch", "strong_scaling", "configs",
             "cpu_baseline", "speedup_vs_cpu_1thread")


def _run(out_dir, frames, steps):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "3", "--frames", str(frames),
           "--points", "120", "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_line_and_its_outputs(tmp_path):
    frames, steps = 100, 10
    lines, outs = [], []
    for i in range(2):
        d = _run(tmp_path / f"run{i}", frames, steps)
        lines.append(d)
        outs.append({n[:-4]: np.load(tmp_path / f"run{i}" / n) for n in os.listdir(tmp_path / f"run{i}")})
    d = lines[0]
    assert d["steps"] == steps and d["n_gpus"] == 1 and d["unit"] == "residuals/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["ms_per_step"] > 0 and abs(d["value"] - 2 * d["config"]["observations_total"] / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    assert not set(FULL_ONLY) & set(d), sorted(set(FULL_ONLY) & set(d))
    o = outs[0]
    assert sorted(o) == ["frame_quaternions", "frame_translations", "intrinsics", "solve_summary"]
    assert all(a.dtype == np.float64 and np.isfinite(a).all() for a in o.values())
    assert o["intrinsics"].shape == (9,) and o["frame_quaternions"].shape == (frames, 4) and o["frame_translations"].shape == (frames, 3)
    assert np.allclose(np.linalg.norm(o["frame_quaternions"], axis=1), 1.0, atol=1e-12)
    its, cost0, cost1 = o["solve_summary"]
    assert its == min(d["iterations_per_solve"], steps) and 0 < cost1 < cost0   # the run ends on a full solve
    for k in o:   # same arguments, same inputs: the same results
        np.testing.assert_allclose(outs[1][k], o[k], rtol=1e-12, atol=0, err_msg=k)
