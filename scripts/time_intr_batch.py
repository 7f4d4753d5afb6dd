"""The batched intrinsics solve against the same problems solved one after another, on one box, alternating the two.

Per shape (B problems of F frames x M points, every problem with its own noise) it times, as medians over REPS runs:
  solve      -- IntrinsicsBatch.solve of the whole batch (default options) / the B problems through IntrinsicsProblem.solve on
                one handle each, one after the other (the existing path, in the form it picks: the persistent kernel where it fits);
  round      -- the batch's time per LM round (sweep + step for ALL problems): a solve with the tolerances switched off,
                20 iterations in one chunk, divided by its 21 rounds; the sequential loop's time per round of ONE problem
                the same way;
  one-shot   -- cc_intrinsics_batch_optimize (create, upload, solve, read back, destroy) / B calls of cc_intrinsics_optimize.
Host wall clock around calls that end in a device synchronisation. One JSON line per shape on stdout and appended to --out.

    python scripts/time_intr_batch.py [--out profiles/r09/intr_batch.jsonl] [--reps 30] [--shapes 1x20x88,8x20x88,...]

--kernels-only: nothing but REPS fixed-iteration solves of the batch (every launch does work), for a kernel trace that splits a
round into its two kernels:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/time_intr_batch.py --kernels-only --shapes 8x200x200"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from camera_calibrator_amd import capi  # noqa: E402

DEFAULT_SHAPES = "1x20x88,8x20x88,64x20x88,8x200x200,4x1000x500"


def make_batch(B, F, M):
    """B problems of F x M cut from one run of the generator (the noise differs from problem to problem), each with its
    Zhang initialisation."""
    off, uv, xyz = capi.make_intrinsics_problem(B * F, M)
    probs = []
    for b in range(B):
        o = off[b * F:(b + 1) * F + 1]
        p_off = (o - o[0]).astype(np.int64)
        p_uv, p_xyz = np.ascontiguousarray(uv[o[0]:o[-1]]), np.ascontiguousarray(xyz[o[0]:o[-1]])
        K0, q0, t0 = capi.zhang_init(p_off, p_uv, p_xyz)
        intr0 = np.array([K0[0, 0], K0[1, 1], K0[0, 2], K0[1, 2], 0, 0, 0, 0, 0], dtype=np.float64)
        probs.append(dict(off=p_off, uv=p_uv, xyz=p_xyz, intr0=intr0, q0=q0.astype(np.float64), t0=t0.astype(np.float64)))
    return probs


def us(fn):
    t = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t) * 1e6, r


def one_shot_batch(lib, opt, poff, foff, uv, xyz, intr0, q0, t0, ss):
    intr, q, t = intr0.copy(), q0.copy(), t0.copy()
    capi._check(lib.cc_intrinsics_batch_optimize(C.byref(opt), C.c_int32(0), C.c_int64(len(poff) - 1), capi._p(poff, C.c_int64),
                                                 capi._p(foff, C.c_int64), capi._p(uv, C.c_float), capi._p(xyz, C.c_float),
                                                 capi._p(intr, C.c_double), None, capi._p(q, C.c_double), capi._p(t, C.c_double), ss))
    return intr


def one_shot_each(lib, opt, probs, s):
    out = []
    for p in probs:
        intr, q, t = p["intr0"].copy(), p["q0"].copy(), p["t0"].copy()
        capi._check(lib.cc_intrinsics_optimize(C.byref(opt), C.c_int32(0), C.c_int64(len(p["off"]) - 1), capi._p(p["off"], C.c_int64),
                                               capi._p(p["uv"], C.c_float), capi._p(p["xyz"], C.c_float), capi._p(intr, C.c_double),
                                               C.c_uint32(0), capi._p(q, C.c_double), capi._p(t, C.c_double), C.byref(s)))
        out.append(intr)
    return np.array(out)


def measure(B, F, M, reps, warmup):
    lib = capi.lib()
    probs = make_batch(B, F, M)
    batch = capi.IntrinsicsBatch([(p["off"], p["uv"], p["xyz"]) for p in probs])
    singles = [capi.IntrinsicsProblem(p["off"], p["uv"], p["xyz"]) for p in probs]
    for h, p in zip(singles, probs):
        h.set_state(p["intr0"], p["q0"], p["t0"])
    intr0 = np.array([p["intr0"] for p in probs])
    q0, t0 = np.concatenate([p["q0"] for p in probs]), np.concatenate([p["t0"] for p in probs])
    poff, foff, uv, xyz = capi._batch_layout([(p["off"], p["uv"], p["xyz"]) for p in probs])
    dflt = capi.default_options()
    fixed = capi.default_options(function_tolerance=-1.0, gradient_tolerance=-1.0, parameter_tolerance=-1.0, max_iterations=20, check_interval=20)
    lean = capi.Summary()
    lean_b = (capi.Summary * B)()

    def batch_solve(opt):
        batch.set_state(intr0, q0, t0)
        return us(lambda: batch.solve_lean(opt))

    def seq_solve(opt):
        for h in singles:
            h.reset()
        return us(lambda: [h.solve_lean(opt) for h in singles])

    t = {k: [] for k in ("b_solve", "s_solve", "b_fixed", "s_fixed", "b_shot", "s_shot")}
    its_b = its_s = fixed_b = fixed_s = None
    for rep in range(warmup + reps):
        a, its_b = batch_solve(dflt)
        b, its_s = seq_solve(dflt)
        c, fixed_b = batch_solve(fixed)
        d, fixed_s = seq_solve(fixed)
        e, ib = us(lambda: one_shot_batch(lib, dflt, poff, foff, uv, xyz, intr0, q0, t0, lean_b))
        f, is_ = us(lambda: one_shot_each(lib, dflt, probs, lean))
        if rep >= warmup:
            for k, v in zip(("b_solve", "s_solve", "b_fixed", "s_fixed", "b_shot", "s_shot"), (a, b, c, d, e, f)):
                t[k].append(v)
    # faster and different is not faster: the two paths end at the same minimisers
    rel = float(np.max(np.abs(ib - is_) / np.maximum(np.abs(is_), 1.0)))
    forms = sorted({h.solver_form() for h in singles})
    batch.close()
    for h in singles:
        h.close()
    med = {k: float(np.median(v)) for k, v in t.items()}
    lo = {k: float(np.min(v)) for k, v in t.items()}
    rounds_b = max(fixed_b) + 1
    rounds_s = sum(i + 1 for i in fixed_s)
    return {
        "problems": B, "frames": F, "pts": M, "frames_total": B * F, "reps": reps,
        "iterations_batch": its_b, "iterations_sequential": its_s, "sequential_forms": forms,
        "solve_us_batch": med["b_solve"], "solve_us_sequential": med["s_solve"],
        "solve_us_batch_min": lo["b_solve"], "solve_us_sequential_min": lo["s_solve"],
        "round_us_batch_all_problems": med["b_fixed"] / rounds_b, "round_us_sequential_one_problem": med["s_fixed"] / rounds_s,
        "fixed_iterations_batch": max(fixed_b), "oneshot_us_batch": med["b_shot"], "oneshot_us_sequential": med["s_shot"],
        "oneshot_us_batch_min": lo["b_shot"], "oneshot_us_sequential_min": lo["s_shot"],
        "speedup_solve": med["s_solve"] / med["b_solve"], "speedup_oneshot": med["s_shot"] / med["b_shot"],
        "max_rel_diff_intrinsics": rel,
    }


def kernels_only(B, F, M, reps):
    probs = make_batch(B, F, M)
    batch = capi.IntrinsicsBatch([(p["off"], p["uv"], p["xyz"]) for p in probs])
    intr0 = np.array([p["intr0"] for p in probs])
    q0, t0 = np.concatenate([p["q0"] for p in probs]), np.concatenate([p["t0"] for p in probs])
    fixed = capi.default_options(function_tolerance=-1.0, gradient_tolerance=-1.0, parameter_tolerance=-1.0, max_iterations=20, check_interval=20)
    for _ in range(reps):
        batch.set_state(intr0, q0, t0)
        its = batch.solve_lean(fixed)
    batch.close()
    print(json.dumps({"problems": B, "frames": F, "pts": M, "solves": reps, "iterations": its}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shapes", default=DEFAULT_SHAPES)
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args()
    if capi.device_count() < 1:
        raise SystemExit("time_intr_batch.py needs a GPU: a timing taken without one says nothing")
    for shape in a.shapes.split(","):
        B, F, M = (int(x) for x in shape.split("x"))
        if a.kernels_only:
            kernels_only(B, F, M, a.reps)
            continue
        line = json.dumps(measure(B, F, M, a.reps, a.warmup))
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as fh:
                fh.write(line + "\n")


if __name__ == "__main__":
    main()
