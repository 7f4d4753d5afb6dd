"""What a pixel model per camera (cc_rigk_set_camera_model) costs the rig solve with intrinsics per LM iteration, on one box, the
sides of every comparison alternating inside one process, by the method of scripts/time_rigk_fisheye.py (whose scenario,
fisheye pixels, handles and statistics this script imports). Sets per camera; in the mixed handle the even cameras are
radial-tangential and the odd ones fisheye, each camera solving pixels of its own kind.

Steps, each a child process of its own under `timeout` (a step that fails or runs out of time ends the script; nothing is
started behind it):
  quad CxFxP    -- four handles alternating: the mixed handle (k_rig_sweep_lens over a list, one launch per model), the homogeneous
                radial-tangential handle in the tile form (CC_RIG_K_COMPACT=0, k_rig_sweep_adjk), the homogeneous fisheye handle
                (k_rig_sweep_lens without a list) and the DEFAULT radial-tangential handle (k_rig_sweep_k2 from ~450 observations per
                group on). The mixed handle does half the groups of each tile form and pays one launch more per round;
  radtan_only, with --baseline-lib PATH -- the default radial-tangential handle alone at the first shape, --pairs times with the
                other build of the library (the parent commit's) and with this one, alternating: the existing path did not move
                when the two sets of runs overlap.
A time per LM iteration is the median over --reps solves with the tolerances switched off (20 iterations in one chunk) divided
by the solve's rounds; the minimum rides along. One JSON line per step on stdout and appended to --out.

    python scripts/time_rigk_mixed.py [--out profiles/r18/rigk_mixed.jsonl] [--reps 30] [--shapes 4x400x300,8x2000x500]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import time_rigk_fisheye as tf   # noqa: E402

STEP_SECONDS = 420


def mixed_handle(k, uv, models):
    from camera_calibrator_amd import capi
    os.environ.pop("CC_RIG_K_COMPACT", None)
    h = capi.RigProblem(k["cams"], k["frame_offsets"], k["obs_cam"], k["obs_world"], uv, k["world_xyz"], k["cam_frozen"], huber_a=0.0,
                        with_intrinsics="per_camera")
    for c, m in enumerate(models):
        h.set_camera_model(c, m)
    for c in range(k["cams"]):
        h.set_camera_intrinsics(c, k["intr0"][c], 0)
    h.set_state(k["cam_q0"], k["cam_t0"], k["frame_q0"], k["frame_t0"])
    return h


def step_quad(shape, reps, warmup, label):
    from camera_calibrator_amd import capi
    from camera_calibrator_amd.harness import rigk_case
    C, F, M = (int(x) for x in shape.split("x"))
    k = rigk_case(C, F, M, per_camera=True)
    K = np.tile(tf.FISH_INTR, (C, 1))
    K[:, :2] *= k["intr_true"][:, :2] / 1000.0
    uvf = tf.fisheye_pixels(k, K)
    models = [capi.MODEL_FISHEYE if c % 2 else capi.MODEL_RADTAN for c in range(C)]
    fish = np.asarray(models)[k["obs_cam"].astype(np.int64)] == capi.MODEL_FISHEYE
    uvm = np.where(fish[:, None], uvf, k["obs_uv_pix"]).astype(np.float32)
    hs = {"mixed": mixed_handle(k, uvm, models), "radtan_tile": tf.handle(k, k["obs_uv_pix"], True, capi.MODEL_RADTAN, 0),
          "fisheye": tf.handle(k, uvf, True, capi.MODEL_FISHEYE, None), "radtan_default": tf.handle(k, k["obs_uv_pix"], True, None, None)}
    assert hs["mixed"].get_model() == capi.MODEL_MIXED
    fixed = tf.fixed_options()
    t, its = {s: [] for s in hs}, {}
    for rep in range(warmup + reps):
        for side, h in hs.items():
            h.reset()
            dt, s = tf.us(lambda: h.solve(fixed))
            its[side] = s["iterations"]
            if rep >= warmup:
                t[side].append(dt)
    full = {}
    for side, h in hs.items():   # what a default solve takes, for the record
        h.reset()
        s = h.solve(capi.default_options(max_iterations=200))
        full[side] = {"iterations": s["iterations"], "termination": s["termination"], "rms_px": float(np.sqrt(2 * s["final_cost"] / len(uvf)))}
        h.close()
    st = {s: tf.stats(t[s], its[s]) for s in hs}
    return {"step": label, "cams": C, "frames": F, "pts": M, "per_camera": True, "models": models, "reps": reps, **st,
            "mixed_over_radtan_tile": st["mixed"]["iter_us"] / st["radtan_tile"]["iter_us"],
            "mixed_over_fisheye": st["mixed"]["iter_us"] / st["fisheye"]["iter_us"],
            "mixed_over_radtan_default": st["mixed"]["iter_us"] / st["radtan_default"]["iter_us"], "default_solves": full}


def child(a):
    from camera_calibrator_amd import capi
    if capi.device_count() < 1:
        raise SystemExit("time_rigk_mixed.py needs a GPU: a timing taken without one says nothing")
    if a.step.startswith("radtan_only"):
        line = tf.step_radtan_only(a.shape + "pc", a.reps, a.warmup, a.step)
    else:
        line = step_quad(a.shape, a.reps, a.warmup, a.step)
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
    ap.add_argument("--shapes", default="4x400x300,8x2000x500")
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
        run_step(a, "quad", shape, {})
    if a.baseline_lib:
        base = {"CC_LIB_PATH": os.path.abspath(a.baseline_lib), "CC_BASELINE_LABEL": a.baseline_label}
        for _ in range(a.pairs):
            run_step(a, "radtan_only", shapes[0] if shapes else "4x400x300", base)
            run_step(a, "radtan_only", shapes[0] if shapes else "4x400x300", {})


if __name__ == "__main__":
    main()
