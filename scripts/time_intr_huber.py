"""What the Huber loss of the intrinsics solve costs per LM iteration, on one box, the two sides of every comparison
alternating inside one process (dirty fixture data: 10 % of the observations displaced by 5 - 30 px; a = 1 px).

Four configurations, each a child process of its own under `timeout` (a step that fails or runs out of time ends the script;
nothing is started behind it):
  two_kernel -- CC_INTR_PERSIST=0: the two-kernel form with the loss on against the same form with it off, one handle each,
                FRAMESxPOINTS from --shapes (200x200, 1000x500);
  batch      -- the batched solve of 8 x (20 x 88) with the loss on for every problem against the same batch without;
  batch_mixed -- the same batch with the loss on every other problem: both sweeps run, the plain one over the whole batch;
  persistent -- default environment at 1000x500: the loss-on solve (two kernels per iteration, by choice) against the default
                persistent solve -- what a user of the loss gives up.
A time per LM iteration is the median over --reps solves with the tolerances switched off (20 iterations in one chunk, host
wall clock around a call that ends in a device synchronisation) divided by the solve's rounds (iterations + the initial
evaluation); the minimum rides along. --baseline-lib PATH: the loss-off side of two_kernel once more with another build of the
library (the parent commit's), which must agree with this one's within the spread.
One JSON line per step on stdout and appended to --out.

    python scripts/time_intr_huber.py [--out profiles/r10/intr_huber.jsonl] [--reps 30] [--shapes 200x200,1000x500]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HUBER_A = 1.0
STEP_SECONDS = 240


def dirty_problem(F, M):
    from camera_calibrator_amd import capi
    off, uv, xyz = capi.make_intrinsics_problem(F, M)
    rng = np.random.default_rng(3)
    n = len(uv)
    idx = rng.choice(n, n // 10, replace=False)
    shift = rng.uniform(5.0, 30.0, size=(len(idx), 2)) * rng.choice([-1.0, 1.0], size=(len(idx), 2))
    uv = uv.astype(np.float64)
    uv[idx] += shift
    uv = uv.astype(np.float32)
    K0, q0, t0 = capi.zhang_init(off, uv, xyz)
    intr0 = np.array([K0[0, 0], K0[1, 1], K0[0, 2], K0[1, 2], 0, 0, 0, 0, 0], dtype=np.float64)
    return dict(off=off, uv=uv, xyz=xyz, intr0=intr0, q0=q0.astype(np.float64), t0=t0.astype(np.float64))


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


def step_single(F, M, reps, warmup, label):
    """Two handles on the same problem, one without the loss and one with it (a handle keeps its captured graph while its loss
    stays as it is), their solves alternating; the form each side ran in is reported with it."""
    from camera_calibrator_amd import capi
    p = dirty_problem(F, M)
    hs = {}
    for side, a in (("off", 0.0), ("on", HUBER_A)):
        hs[side] = capi.IntrinsicsProblem(p["off"], p["uv"], p["xyz"])
        hs[side].set_state(p["intr0"], p["q0"], p["t0"])
        hs[side].set_huber(a)
    fixed, dflt = fixed_options(), capi.default_options()
    t, its, forms, full = {"off": [], "on": []}, {}, {}, {}
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
        full[side] = {"iterations": s["iterations"], "termination": s["termination"], "fx": float(h.get_state()[0][0])}
        h.close()
    off, on = stats(t["off"], its["off"]), stats(t["on"], its["on"])
    return {"step": label, "frames": F, "pts": M, "huber_a": HUBER_A, "reps": reps, "env_CC_INTR_PERSIST": os.environ.get("CC_INTR_PERSIST"),
            "lib": os.environ.get("CC_LIB_PATH", "this build"), "form_off": forms["off"], "form_on": forms["on"], "loss_off": off, "loss_on": on,
            "on_over_off": on["iter_us"] / off["iter_us"], "default_solve_off": full["off"], "default_solve_on": full["on"]}


def step_single_off_only(F, M, reps, warmup, label):
    """Another build of the library (it may not know the loss): the loss-off side alone."""
    from camera_calibrator_amd import capi
    p = dirty_problem(F, M)
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
            "lib": "baseline-lib (%s)" % os.environ.get("CC_BASELINE_LABEL", "another build"), "form_off": form, "loss_off": stats(t, it)}


def step_batch(B, F, M, reps, warmup, mixed=False):
    """mixed: the loss on every other problem only -- the plain sweep then runs over the whole batch in front of the robust one
    (the plain problems keep its bits), so the problems with the loss are swept twice a round."""
    from camera_calibrator_amd import capi
    probs = [dirty_problem(F, M) for _ in range(B)]   # (the same dirty problem B times: the time does not depend on the noise)
    b = capi.IntrinsicsBatch([(p["off"], p["uv"], p["xyz"]) for p in probs])
    intr0 = np.array([p["intr0"] for p in probs])
    q0, t0 = np.concatenate([p["q0"] for p in probs]), np.concatenate([p["t0"] for p in probs])
    fixed = fixed_options()
    t, its = {"off": [], "on": []}, {}
    for rep in range(warmup + reps):
        for side, a in (("off", None), ("on", [HUBER_A if (p % 2 == 0 or not mixed) else 0.0 for p in range(B)])):
            b.set_state(intr0, q0, t0)
            b.set_huber(a)
            dt, it = us(lambda: b.solve_lean(fixed))
            its[side] = max(it)
            if rep >= warmup:
                t[side].append(dt)
    b.close()
    off, on = stats(t["off"], its["off"]), stats(t["on"], its["on"])
    return {"step": "batch_mixed" if mixed else "batch", "problems_with_loss": (B + 1) // 2 if mixed else B, "problems": B, "frames": F, "pts": M, "huber_a": HUBER_A, "reps": reps, "loss_off": off, "loss_on": on,
            "on_over_off": on["iter_us"] / off["iter_us"]}


def child(a):
    from camera_calibrator_amd import capi
    if capi.device_count() < 1:
        raise SystemExit("time_intr_huber.py needs a GPU: a timing taken without one says nothing")
    dims = [int(x) for x in a.shape.split("x")]
    if a.step in ("batch", "batch_mixed"):
        line = step_batch(*dims, a.reps, a.warmup, mixed=a.step == "batch_mixed")
    elif a.step == "off_only":
        line = step_single_off_only(*dims, a.reps, a.warmup, "two_kernel_baseline_lib")
    else:
        line = step_single(*dims, a.reps, a.warmup, a.step)
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
    ap.add_argument("--batch-shape", default="8x20x88")
    ap.add_argument("--persistent-shape", default="1000x500")
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--baseline-label", default="the parent commit's build", help="what the result line calls --baseline-lib (not its path)")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--step", default=None)
    ap.add_argument("--shape", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a)
    for shape in a.shapes.split(","):
        run_step(a, "two_kernel", shape, {"CC_INTR_PERSIST": "0"})
        if a.baseline_lib:
            run_step(a, "off_only", shape, {"CC_INTR_PERSIST": "0", "CC_LIB_PATH": os.path.abspath(a.baseline_lib), "CC_BASELINE_LABEL": a.baseline_label})
    run_step(a, "batch", a.batch_shape, {})
    run_step(a, "batch_mixed", a.batch_shape, {})
    run_step(a, "persistent", a.persistent_shape, {})


if __name__ == "__main__":
    main()
