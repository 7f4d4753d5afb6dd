"""What the fisheye camera model of the rig solve with intrinsics (cc_rigk_set_model) costs per LM iteration, on one box, the
sides of every comparison alternating inside one process. All sides see the same rig, frames, world points and start
(camera_calibrator_amd.harness.rigk_case); the fisheye side's pixels are those points projected through a fisheye lens
(fx = fy = 1000, k = -0.035 0.004 -0.0009 0.0001, 0.3 px noise) from the true poses, so that each model solves data of its own kind.

Steps, each a child process of its own under `timeout` (a step that fails or runs out of time ends the script; nothing is
started behind it):
  pair CxFxP [per_camera] -- three handles alternating: radial-tangential in the tile form (CC_RIG_K_COMPACT=0, k_rig_sweep_adjk),
                fisheye (k_rig_sweep_lens: always tiles) and the DEFAULT radial-tangential handle (k_rig_sweep_k2 from
                ~450 observations per group on). fisheye / tile is the model's own cost, fisheye / default what a fisheye user
                gives up by having no compact-record form;
  radtan_only, with --baseline-lib PATH -- the default radial-tangential handle alone at the first shape, --pairs times with the
                other build of the library (the parent commit's) and with this one, alternating: the existing path did not move
                when the two sets of runs overlap.
A time per LM iteration is the median over --reps solves with the tolerances switched off (20 iterations in one chunk, host
wall clock around a call that ends in a device synchronisation) divided by the solve's rounds (iterations + the initial
evaluation); the minimum rides along. One JSON line per step on stdout and appended to --out.

    python scripts/time_rigk_fisheye.py [--out profiles/r14/rigk_fisheye.jsonl] [--reps 30] [--shapes 4x400x300,8x2000x500,8x2000x500pc]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEP_SECONDS = 420
FISH_INTR = np.array([1000.0, 1000.0, 800.0, 500.0, -0.035, 0.004, -0.0009, 0.0001, 0.0])


def _rotations(q):
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], 1),
                     np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], 1),
                     np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1)], 1)


def fisheye_pixels(k, K):
    """Pixels of every observation of scenario k through the fisheye sets K [cams][9] from the true poses, + N(0, 0.3) px."""
    off = k["frame_offsets"]
    Rf, Rc = _rotations(k["frame_q_true"]), _rotations(k["cam_q_true"])
    uv = np.empty((int(off[-1]), 2), dtype=np.float32)
    rng = np.random.default_rng(3)
    step = 64
    for f0 in range(0, len(off) - 1, step):
        f1 = min(f0 + step, len(off) - 1)
        s = slice(int(off[f0]), int(off[f1]))
        frame = np.repeat(np.arange(f0, f1), np.diff(off[f0:f1 + 1]))
        cam = k["obs_cam"][s].astype(np.int64)
        X = k["world_xyz"][k["obs_world"][s].astype(np.int64)].astype(np.float64)
        Xr = np.einsum("nij,nj->ni", Rf[frame], X) + k["frame_t_true"][frame]
        Xc = np.einsum("nij,nj->ni", Rc[cam], Xr) + k["cam_t_true"][cam]
        rho = np.hypot(Xc[:, 0], Xc[:, 1])
        th = np.arctan2(rho, Xc[:, 2])
        kk = K[cam]
        sc = th * (1 + kk[:, 4] * th**2 + kk[:, 5] * th**4 + kk[:, 6] * th**6 + kk[:, 7] * th**8) / np.maximum(rho, 1e-300)
        p = np.stack([kk[:, 0] * sc * Xc[:, 0] + kk[:, 2], kk[:, 1] * sc * Xc[:, 1] + kk[:, 3]], 1)
        uv[s] = (p + rng.normal(scale=0.3, size=p.shape)).astype(np.float32)
    return uv


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


def handle(k, uv, per_camera, model, compact):
    """A handle at the scenario's start; compact: None (the handle's own choice) or 0 / 1 for CC_RIG_K_COMPACT at creation."""
    from camera_calibrator_amd import capi
    if compact is None:
        os.environ.pop("CC_RIG_K_COMPACT", None)
    else:
        os.environ["CC_RIG_K_COMPACT"] = str(compact)
    h = capi.RigProblem(k["cams"], k["frame_offsets"], k["obs_cam"], k["obs_world"], uv, k["world_xyz"], k["cam_frozen"], huber_a=0.0,
                        with_intrinsics="per_camera" if per_camera else True)
    if model is not None:
        h.set_model(model)
    intr0 = np.atleast_2d(k["intr0"])
    if per_camera:
        for c in range(k["cams"]):
            h.set_camera_intrinsics(c, intr0[c], 0)
    else:
        h.set_intrinsics(intr0[0], 0)
    h.set_state(k["cam_q0"], k["cam_t0"], k["frame_q0"], k["frame_t0"])
    os.environ.pop("CC_RIG_K_COMPACT", None)
    return h


def parse_shape(shape):
    pc = shape.endswith("pc")
    return tuple(int(x) for x in shape[:-2 if pc else None].split("x")) + (pc,)


def step_pair(shape, reps, warmup, label):
    from camera_calibrator_amd import capi
    from camera_calibrator_amd.harness import rigk_case
    C, F, M, pc = parse_shape(shape)
    k = rigk_case(C, F, M, per_camera=pc)
    K = np.tile(FISH_INTR, (C, 1))
    if pc:
        K[:, :2] *= np.atleast_2d(k["intr_true"])[:, :2] / 1000.0
    uvf = fisheye_pixels(k, K)
    hs = {"radtan_tile": handle(k, k["obs_uv_pix"], pc, capi.MODEL_RADTAN, 0), "fisheye": handle(k, uvf, pc, capi.MODEL_FISHEYE, None),
          "radtan_default": handle(k, k["obs_uv_pix"], pc, None, None)}
    fixed = fixed_options()
    t, its = {s: [] for s in hs}, {}
    for rep in range(warmup + reps):
        for side, h in hs.items():
            h.reset()
            dt, s = us(lambda: h.solve(fixed))
            its[side] = s["iterations"]
            if rep >= warmup:
                t[side].append(dt)
    full = {}
    for side, h in hs.items():   # what a default solve takes, for the record
        h.reset()
        s = h.solve(capi.default_options(max_iterations=200))
        full[side] = {"iterations": s["iterations"], "termination": s["termination"], "rms_px": float(np.sqrt(2 * s["final_cost"] / len(uvf)))}
        h.close()
    st = {s: stats(t[s], its[s]) for s in hs}
    return {"step": label, "cams": C, "frames": F, "pts": M, "per_camera": pc, "reps": reps, **st,
            "fisheye_over_radtan_tile": st["fisheye"]["iter_us"] / st["radtan_tile"]["iter_us"],
            "fisheye_over_radtan_default": st["fisheye"]["iter_us"] / st["radtan_default"]["iter_us"], "default_solves": full}


def step_radtan_only(shape, reps, warmup, label):
    """Any build of the library (it may not know the model): the default radial-tangential handle alone."""
    from camera_calibrator_amd.harness import rigk_case
    C, F, M, pc = parse_shape(shape)
    k = rigk_case(C, F, M, per_camera=pc)
    h = handle(k, k["obs_uv_pix"], pc, None, None)
    fixed = fixed_options()
    t, it = [], 0
    for rep in range(warmup + reps):
        h.reset()
        dt, s = us(lambda: h.solve(fixed))
        it = s["iterations"]
        if rep >= warmup:
            t.append(dt)
    h.close()
    return {"step": label, "cams": C, "frames": F, "pts": M, "per_camera": pc, "reps": reps,
            "lib": os.environ.get("CC_BASELINE_LABEL", "this build"), "radtan": stats(t, it)}


def child(a):
    from camera_calibrator_amd import capi
    if capi.device_count() < 1:
        raise SystemExit("time_rigk_fisheye.py needs a GPU: a timing taken without one says nothing")
    line = step_radtan_only(a.shape, a.reps, a.warmup, a.step) if a.step.startswith("radtan_only") else step_pair(a.shape, a.reps, a.warmup, a.step)
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
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="4x400x300,8x2000x500,8x2000x500pc")
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--baseline-label", default="the parent commit's build", help="what the result line calls --baseline-lib (not its path)")
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--step", default=None)
    ap.add_argument("--shape", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a)
    shapes = [s for s in a.shapes.split(",") if s]
    for shape in shapes:
        run_step(a, "pair", shape, {})
    if a.baseline_lib:
        base = {"CC_LIB_PATH": os.path.abspath(a.baseline_lib), "CC_BASELINE_LABEL": a.baseline_label}
        for _ in range(a.pairs):
            run_step(a, "radtan_only", shapes[0] if shapes else "4x400x300", base)
            run_step(a, "radtan_only", shapes[0] if shapes else "4x400x300", {})


if __name__ == "__main__":
    main()
