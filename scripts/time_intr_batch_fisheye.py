"""The fisheye model in the batched intrinsics solve (cc_intrinsics_batch_set_model, k_intrb_sweep_fisheye), on one box, both
sides of every comparison alternating inside one process, medians over --reps runs:

  (a) the fisheye batch against the same problems one after another through the single fisheye handle (the two-kernel form,
      cc_intrinsics_set_model): `solve` -- IntrinsicsBatch.solve of the whole batch / the B handles' solves in a row, default
      options, handles and data resident; `one-shot` -- capi.intrinsics_batch_estimate(model=FISHEYE) (upload, Zhang, solve, read
      back) / B calls of capi.intrinsics_estimate(model=FISHEYE);
  (b) microseconds per LM round of the fisheye batch against the radial-tangential batch of the same shape (each on data of
      its own kind): a solve with the tolerances switched off, 20 iterations in one chunk, divided by its 21 rounds.

Data: B problems of F frames x M points from the geometry of tests/fisheye_ref.py's generator (boards of half-size 0.30 m at
about 0.45 m, tilted by up to 0.35 rad, the fixture's lens fisheye_ref.TRUE_INTR, 0.3 px noise, one seed per problem), projected
with its numpy model in float64 (its 50-digit projection takes minutes at these sizes and changes nothing a timing sees); the
radial-tangential side of (b) takes the harness generator's problems, as scripts/time_intr_batch.py does. Every problem starts
from Zhang's initialisation. Each shape runs in a child process of its own under `timeout`; a shape that fails or runs out of
time ends the script, nothing is started behind it. Host wall clock around calls that end in a device synchronisation. One JSON
line per shape on stdout and appended to --out.

    python scripts/time_intr_batch_fisheye.py [--out profiles/r13/intr_batch_fisheye.jsonl] [--reps 30] [--shapes 8x20x88,64x20x88,8x200x200]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEP_SECONDS = 300
DEFAULT_SHAPES = "8x20x88,64x20x88,8x200x200"


def fisheye_problem(F, M, seed):
    """One problem of F frames x M points: fisheye_ref.make_case's geometry and noise, the numpy model for the projection."""
    from camera_calibrator_amd import capi
    from tests import fisheye_ref as fr
    from tests.rig_inner_ref import quat_plus
    _, half, dist, tilt, sigma = fr.SHAPES["8x40"]
    rng = np.random.default_rng(seed)
    off = (np.arange(F + 1) * M).astype(np.int64)
    X = fr._board(M, half)
    uv = np.zeros((F * M, 2), np.float32)
    zero = np.zeros((M, 2), np.float32)
    for f in range(F):
        ang = rng.uniform(-tilt, tilt, size=3) * np.array([1.0, 1.0, 0.3])
        qf = quat_plus(np.array([1.0, 0.0, 0.0, 0.0]), ang / 2)
        tf = np.array([rng.uniform(-0.05, 0.05), rng.uniform(-0.05, 0.05), dist * rng.uniform(0.9, 1.2)])
        p, _ = fr.fisheye_model(fr.TRUE_INTR, qf, tf, X, zero)   # (the residual against (0, 0) is the projection)
        uv[f * M:(f + 1) * M] = (p + rng.normal(scale=sigma, size=p.shape)).astype(np.float32)
    xyz = np.tile(X, (F, 1))
    K0, q0, t0 = capi.zhang_init(off, uv, xyz)
    intr0 = np.array([K0[0, 0], K0[1, 1], K0[0, 2], K0[1, 2], 0, 0, 0, 0, 0], dtype=np.float64)
    return dict(off=off, uv=uv, xyz=xyz, intr0=intr0, q0=q0.astype(np.float64), t0=t0.astype(np.float64))


def us(fn):
    t = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t) * 1e6, r


def measure(B, F, M, reps, warmup):
    from camera_calibrator_amd import capi
    from scripts.time_intr_batch import make_batch
    FISH = capi.MODEL_FISHEYE
    probs = [fisheye_problem(F, M, 100 + b) for b in range(B)]
    radtan = make_batch(B, F, M)
    layout = lambda ps: [(p["off"], p["uv"], p["xyz"]) for p in ps]
    state = lambda ps: (np.array([p["intr0"] for p in ps]), np.concatenate([p["q0"] for p in ps]), np.concatenate([p["t0"] for p in ps]))
    batch = capi.IntrinsicsBatch(layout(probs))
    batch.set_model(FISH)
    batch_r = capi.IntrinsicsBatch(layout(radtan))
    singles = [capi.IntrinsicsProblem(p["off"], p["uv"], p["xyz"]) for p in probs]
    for h, p in zip(singles, probs):
        h.set_model(FISH)
        h.set_state(p["intr0"], p["q0"], p["t0"])
    st_f, st_r = state(probs), state(radtan)
    dflt = capi.default_options()
    fixed = capi.default_options(function_tolerance=-1.0, gradient_tolerance=-1.0, parameter_tolerance=-1.0, max_iterations=20, check_interval=20)

    def batch_solve(b, st, opt):
        b.set_state(*st)
        return us(lambda: b.solve_lean(opt))

    def seq_solve(opt):
        for h in singles:
            h.reset()
        return us(lambda: [h.solve_lean(opt) for h in singles])

    keys = ("b_solve", "s_solve", "b_fixed", "r_fixed", "s_fixed", "b_shot", "s_shot")
    t = {k: [] for k in keys}
    for rep in range(warmup + reps):
        a, its_b = batch_solve(batch, st_f, dflt)
        b, its_s = seq_solve(dflt)
        c, fixed_b = batch_solve(batch, st_f, fixed)
        d, fixed_r = batch_solve(batch_r, st_r, fixed)
        e, fixed_s = seq_solve(fixed)
        f, shot_b = us(lambda: capi.intrinsics_batch_estimate(layout(probs), model=FISH, log_capacity=1))
        g, shot_s = us(lambda: [capi.intrinsics_estimate(p["off"], p["uv"], p["xyz"], model=FISH, log_capacity=1) for p in probs])
        if rep >= warmup:
            for k, v in zip(keys, (a, b, c, d, e, f, g)):
                t[k].append(v)
    # faster and different is not faster: the two paths end at the same minimisers
    ib, is_ = shot_b[1], np.array([s[1] for s in shot_s])
    rel = float(np.max(np.abs(ib - is_) / np.maximum(np.abs(is_), 1.0)))
    forms = sorted({h.solver_form() for h in singles})
    for h in [batch, batch_r] + singles:
        h.close()
    med = {k: float(np.median(v)) for k, v in t.items()}
    lo = {k: float(np.min(v)) for k, v in t.items()}
    rounds_b, rounds_r, rounds_s = max(fixed_b) + 1, max(fixed_r) + 1, sum(i + 1 for i in fixed_s)
    return {
        "problems": B, "frames": F, "pts": M, "frames_total": B * F, "reps": reps,
        "iterations_batch": its_b, "iterations_sequential": its_s, "sequential_forms": forms,
        "solve_us_batch": med["b_solve"], "solve_us_sequential": med["s_solve"],
        "solve_us_batch_min": lo["b_solve"], "solve_us_sequential_min": lo["s_solve"],
        "oneshot_us_batch": med["b_shot"], "oneshot_us_sequential": med["s_shot"],
        "oneshot_us_batch_min": lo["b_shot"], "oneshot_us_sequential_min": lo["s_shot"],
        "speedup_solve": med["s_solve"] / med["b_solve"], "speedup_oneshot": med["s_shot"] / med["b_shot"],
        "round_us_fisheye_batch_all_problems": med["b_fixed"] / rounds_b, "round_us_radtan_batch_all_problems": med["r_fixed"] / rounds_r,
        "round_us_fisheye_batch_min": lo["b_fixed"] / rounds_b, "round_us_radtan_batch_min": lo["r_fixed"] / rounds_r,
        "round_fisheye_over_radtan": (med["b_fixed"] / rounds_b) / (med["r_fixed"] / rounds_r),
        "round_us_sequential_one_problem": med["s_fixed"] / rounds_s,
        "fixed_iterations_fisheye_batch": max(fixed_b), "fixed_iterations_radtan_batch": max(fixed_r),
        "max_rel_diff_intrinsics": rel,
    }


def child(a):
    from camera_calibrator_amd import capi
    if capi.device_count() < 1:
        raise SystemExit("time_intr_batch_fisheye.py needs a GPU: a timing taken without one says nothing")
    B, F, M = (int(x) for x in a.shape.split("x"))
    print("RESULT " + json.dumps(measure(B, F, M, a.reps, a.warmup)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shapes", default=DEFAULT_SHAPES)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--shape", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a)
    for shape in a.shapes.split(","):
        cmd = ["timeout", "-k", "10", str(STEP_SECONDS), sys.executable, os.path.abspath(__file__), "--child", "--shape", shape,
               "--reps", str(a.reps), "--warmup", str(a.warmup)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            print(r.stdout[-3000:])
            raise SystemExit("shape %s ended with status %d: nothing further is started" % (shape, r.returncode))
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][len("RESULT "):]
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as fh:
                fh.write(line + "\n")


if __name__ == "__main__":
    main()
