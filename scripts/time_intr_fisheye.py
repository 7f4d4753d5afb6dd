"""What the fisheye camera model of the intrinsics solve costs per LM iteration, on one box, the two sides of every comparison
alternating inside one process. Both sides see the same boards and poses (the fixture generator's); the fisheye side's pixels
are those points projected through a fisheye lens (fx = fy = 1000, k = -0.035 0.004 -0.0009 0.0001, 0.3 px noise), so that
each model solves data of its own kind from the same Zhang start.

Steps, each a child process of its own under `timeout` (a step that fails or runs out of time ends the script; nothing is
started behind it):
  two_kernel -- CC_INTR_PERSIST=0: the fisheye handle (k_intr_sweep_fisheye) against a radial-tangential handle in the same
                two-kernel form, FRAMESxPOINTS from --shapes (200x200, 1000x500);
  persistent -- default environment at 1000x500: the fisheye solve (two kernels per iteration, by choice) against the default
                persistent solve -- what a fisheye user gives up;
  radtan_only, with --baseline-lib PATH -- the radial-tangential side alone, --pairs times with the other build of the library
                (the parent commit's) and with this one, alternating, in both forms at the last shape: the existing paths agree
                when the two sets of runs overlap.
A time per LM iteration is the median over --reps solves with the tolerances switched off (20 iterations in one chunk, host
wall clock around a call that ends in a device synchronisation) divided by the solve's rounds (iterations + the initial
evaluation); the minimum rides along. One JSON line per step on stdout and appended to --out.

    python scripts/time_intr_fisheye.py [--out profiles/r11/intr_fisheye.jsonl] [--reps 30] [--shapes 200x200,1000x500]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEP_SECONDS = 240
FISH_INTR = np.array([1000.0, 1000.0, 800.0, 500.0, -0.035, 0.004, -0.0009, 0.0001, 0.0])


def _rotations(q):
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], 1),
                     np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], 1),
                     np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1)], 1)


def problems(F, M):
    """(radial-tangential problem, fisheye problem): same boards, same start."""
    from camera_calibrator_amd import capi
    off, uv, xyz = capi.make_intrinsics_problem(F, M)
    K0, q0, t0 = capi.zhang_init(off, uv, xyz)
    q0, t0 = q0.astype(np.float64), t0.astype(np.float64)
    intr0 = np.array([K0[0, 0], K0[1, 1], K0[0, 2], K0[1, 2], 0, 0, 0, 0, 0], dtype=np.float64)
    frame = np.repeat(np.arange(F), np.diff(off))
    Xc = np.einsum("nij,nj->ni", _rotations(q0)[frame], xyz.astype(np.float64)) + t0[frame]
    rho = np.hypot(Xc[:, 0], Xc[:, 1])
    th = np.arctan2(rho, Xc[:, 2])
    fx, fy, px, py, k1, k2, k3, k4 = FISH_INTR[:8]
    s = th * (1 + k1 * th**2 + k2 * th**4 + k3 * th**6 + k4 * th**8) / np.maximum(rho, 1e-300)
    uvf = np.stack([fx * s * Xc[:, 0] + px, fy * s * Xc[:, 1] + py], 1) + np.random.default_rng(3).normal(scale=0.3, size=(len(rho), 2))
    radtan = dict(off=off, uv=uv, xyz=xyz, intr0=intr0, q0=q0, t0=t0)
    return radtan, dict(radtan, uv=uvf.astype(np.float32))


def us(fn):
    t = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t) * 1e6, r


def fixed_options():
    from camera_calibrator_amd import capi
    return capi.default_options(function_tolerance=-1.0, gradient_tolerance=-1.0, parameter_tolerance=-1.0, max_iterations=20, check_interval=20)


def stats(times, iterations):
    rounds = iterations + 1
    return {"iterations": int(iterations), "iter_us": float(np.median(times)) / rounds, "iter_us_min": float(np.min(times)) / rounds}


def step_pair(F, M, reps, warmup, label):
    """Two handles, one per model, their solves alternating; the form each side ran in is reported with it."""
    from camera_calibrator_amd import capi
    pr, pf = problems(F, M)
    hs = {}
    for side, p, model in (("radtan", pr, capi.MODEL_RADTAN), ("fisheye", pf, capi.MODEL_FISHEYE)):
        hs[side] = capi.IntrinsicsProblem(p["off"], p["uv"], p["xyz"])
        hs[side].set_model(model)
        hs[side].set_state(p["intr0"], p["q0"], p["t0"])
    fixed, dflt = fixed_options(), capi.default_options()
    t, its, forms, full = {"radtan": [], "fisheye": []}, {}, {}, {}
    for rep in range(warmup + reps):
        for side, h in hs.items():
            h.reset()
            dt, it = us(lambda: h.solve_lean(fixed))
            its[side] = it
            if rep >= warmup:
                t[side].append(dt)
    for side, h in hs.items():   # what a default solve takes, for the record
        h.reset()
        s = h.solve(dflt)
        forms[side] = h.solver_status()[0]
        full[side] = {"iterations": s["iterations"], "termination": s["termination"], "fx": float(h.get_state()[0][0]),
                      "rms_px": float(np.sqrt(2 * s["final_cost"] / len(pr["uv"])))}
        h.close()
    a, b = stats(t["radtan"], its["radtan"]), stats(t["fisheye"], its["fisheye"])
    return {"step": label, "frames": F, "pts": M, "reps": reps, "env_CC_INTR_PERSIST": os.environ.get("CC_INTR_PERSIST"),
            "form_radtan": forms["radtan"], "form_fisheye": forms["fisheye"], "radtan": a, "fisheye": b,
            "fisheye_over_radtan": b["iter_us"] / a["iter_us"], "default_solve_radtan": full["radtan"], "default_solve_fisheye": full["fisheye"]}


def step_radtan_only(F, M, reps, warmup, label):
    """Any build of the library (it may not know the model): the radial-tangential side alone."""
    from camera_calibrator_amd import capi
    p, _ = problems(F, M)
    h = capi.IntrinsicsProblem(p["off"], p["uv"], p["xyz"])
    h.set_state(p["intr0"], p["q0"], p["t0"])
    fixed = fixed_options()
    t, it = [], 0
    for rep in range(warmup + reps):
        h.reset()
        dt, it = us(lambda: h.solve_lean(fixed))
        if rep >= warmup:
            t.append(dt)
    form = h.solver_form()
    h.close()
    return {"step": label, "frames": F, "pts": M, "reps": reps, "env_CC_INTR_PERSIST": os.environ.get("CC_INTR_PERSIST"),
            "lib": os.environ.get("CC_BASELINE_LABEL", "this build"), "form": form, "radtan": stats(t, it)}


def child(a):
    from camera_calibrator_amd import capi
    if capi.device_count() < 1:
        raise SystemExit("time_intr_fisheye.py needs a GPU: a timing taken without one says nothing")
    F, M = (int(x) for x in a.shape.split("x"))
    line = step_radtan_only(F, M, a.reps, a.warmup, a.step) if a.step.startswith("radtan_only") else step_pair(F, M, a.reps, a.warmup, a.step)
    print("RESULT " + json.dumps(line), flush=True)


def run_step(a, step, shape, env_extra):
    env = dict(os.environ, **env_extra)
    cmd = ["timeout", "-k", "10", str(STEP_SECONDS), sys.executable, os.path.abspath(__file__), "--child", "--step", step, "--shape", shape,
           "--reps", str(a.reps), "--warmup", str(a.warmup)]
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        print(r.stdout[-3000:])
        raise SystemExit("step %s %s ended with status %d: nothing further is started" % (step, shape, r.returncode))
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][len("RESULT "):]
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shapes", default="200x200,1000x500")
    ap.add_argument("--persistent-shape", default="1000x500")
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--baseline-label", default="the parent commit's build", help="what the result line calls --baseline-lib (not its path)")
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--step", default=None)
    ap.add_argument("--shape", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a)
    for shape in a.shapes.split(","):
        run_step(a, "two_kernel", shape, {"CC_INTR_PERSIST": "0"})
    run_step(a, "persistent", a.persistent_shape, {})
    if a.baseline_lib:
        base = {"CC_LIB_PATH": os.path.abspath(a.baseline_lib), "CC_BASELINE_LABEL": a.baseline_label}
        for form, env in (("two_kernel", {"CC_INTR_PERSIST": "0"}), ("persistent", {})):
            for _ in range(a.pairs):
                run_step(a, "radtan_only_" + form, a.persistent_shape, dict(env, **base))
                run_step(a, "radtan_only_" + form, a.persistent_shape, env)


if __name__ == "__main__":
    main()
