"""Convergence record of the rig solve with and without Ceres' inner iterations (cc_rig_set_inner_iterations), on the HIP path.

Per shape: the reference's rig scenario (oracle generator), solved from its perturbed starting cameras with inner iterations off
and on, and from the true cameras (inner iterations off) for the level a converged solve reaches. One JSON line per run:
final cost / truth-start cost, the largest camera error against cam_T_true (translation distance and rotation angle),
iterations, passes, useful passes, microseconds per outer iteration. Recorded, not asserted.

    python scripts/rig_inner_convergence.py [--out profiles/r07/rig_inner_convergence.jsonl] [--shapes 8x200x60,4x400x300]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from camera_calibrator_amd import capi  # noqa: E402
from oracle import pyoracle as po  # noqa: E402


def cam_errors(cq, ct, cam_T_true):
    tq, tt = po.affine_to_qt(cam_T_true)
    dt = np.linalg.norm(ct - tt, axis=1).max()
    dots = np.abs(np.sum(cq / np.linalg.norm(cq, axis=1, keepdims=True) * tq, axis=1))
    ang = 2.0 * np.arccos(np.clip(dots, -1.0, 1.0)).max()
    return float(dt), float(ang)


def run(sc, cam_q, cam_t, inner):
    C_ = len(sc["cam_T"])
    fq, ft = po.affine_to_qt(sc["frame_T"])
    p = capi.RigProblem(C_, sc["frame_offsets"], sc["obs_cam"], sc["obs_world"], sc["obs_uv"], sc["world_xyz"], sc["cam_frozen"])
    p.set_state(cam_q, cam_t, fq, ft)
    if inner:
        p.set_inner_iterations(True)
    s = p.solve()
    cq, ct, _, _, _ = p.get_state(want_cost=False)
    st = p.inner_status()
    p.close()
    return s, cq, ct, st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07", "rig_inner_convergence.jsonl"))
    ap.add_argument("--shapes", default="8x200x60,4x400x300,8x2000x500")
    a = ap.parse_args()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        for shape in a.shapes.split(","):
            C_, F, M = (int(v) for v in shape.split("x"))
            sc = po.rig_scenario(C_, F, M)
            q0, t0 = po.affine_to_qt(sc["cam_T"])
            qt, tt = po.affine_to_qt(sc["cam_T_true"])
            s_true, _, _, _ = run(sc, qt, tt, False)
            for inner in (False, True):
                s, cq, ct, st = run(sc, q0, t0, inner)
                dt, ang = cam_errors(cq, ct, sc["cam_T_true"])
                row = dict(shape=shape, inner_iterations=inner, measured_on="MI355X (HIP path)",
                           final_cost=s["final_cost"], truth_start_cost=s_true["final_cost"],
                           cost_over_truth_start=s["final_cost"] / s_true["final_cost"],
                           max_cam_translation_error=dt, max_cam_rotation_error_rad=ang,
                           iterations=s["iterations"], termination=s["termination"], passes=st["passes"],
                           useful_passes=st["useful_passes"], inner_enabled_at_end=st["enabled_at_end"],
                           us_per_outer_iteration=1e6 * s["seconds"] / max(1, s["iterations"]))
                fh.write(json.dumps(row) + "\n")
                fh.flush()
                print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
