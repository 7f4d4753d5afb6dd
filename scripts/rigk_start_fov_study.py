"""How far off the axis the pixel start of a fisheye rig (cc_rigk_estimate_start) still gives the solve a start it converges
from. CPU only: the references of the tests stand in for the library (tests/rigk_start_ref.py for the start,
tests/rigk_fisheye_ref.py for scenes and the solve), so the figures are the method's, not a kernel's.

    python scripts/rigk_start_fov_study.py > profiles/rNN/rigk_start_fov_study.txt

The scene is fisheye_rig_case(2, 12, 20) with its board half-size `half` swept: the points' x and y spread widens while their
depth range stays, so the largest angle off the axis climbs towards 90 degrees. Per half-size and per choice of start
intrinsics -- intr0 (focal lengths 2 % off, no distortion: what a caller without a lens calibration has) and the true ones --
the start runs from identity poses; the solve (default options) then runs from it and, for comparison, from the scenario's own
start (poses 20 mm / 1 degree off). A start counts as one the solve converges from when every view is valid and the solve ends
within 1e-6 (relative) of the cost reached from the scenario's start. The start works on pinhole points x / z = tan(theta):
towards 90 degrees they grow without bound, their float32 spacing with them, and a pixel whose theta_d lies beyond the start
intrinsics' theta_d(pi/2) has no point at all."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import fisheye_ref as fr  # noqa: E402
from tests import rigk_fisheye_ref as rfr  # noqa: E402
from tests import rigk_start_ref as ref  # noqa: E402

HALVES = (0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, 8.0, 12.0)


def main():
    print("half   max angle  start intrinsics  points w/o root  views valid  largest |x/z|  start cost    final cost (its)        scenario start: final cost (its)  converges")
    for half in HALVES:
        k = rfr.fisheye_rig_case(2, 12, 20, half=half)
        P = rfr.problem(k, model=fr.fisheye_model)
        a = rfr.solve_case(k, P)
        for label, intr in (("intr0", k["intr0"]), ("true", k["intr_true"])):
            cq, ct, fq, ft, rep, _, pts = ref.start_from_pixels(ref.FISHEYE, intr, k["cams"], k["frame_offsets"], k["obs_cam"], k["obs_world"],
                                                                k["obs_uv_pix"], k["world_xyz"], k["cam_frozen"])
            bad = int(np.isnan(pts).any(axis=1).sum())
            big = float(np.nanmax(np.abs(pts))) if bad < len(pts) else float("nan")
            try:
                b = rfr.rigk_solve(P, k["intr0"], cq, ct, fq, ft)
                ok = rep["views_invalid"] == 0 and abs(b[6]["final_cost"] - a[6]["final_cost"]) <= 1e-6 * a[6]["final_cost"]
                end = "%.6e (%d)" % (b[6]["final_cost"], b[6]["iterations"])
                c0 = "%.4e" % b[6]["initial_cost"]
            except Exception as e:   # (a start the reference solve cannot even evaluate)
                ok, end, c0 = False, type(e).__name__, "-"
            print("%-6g %-10.2f %-17s %-16d %2d of %-6d %-14.4g %-13s %-23s %-33s %s" % (
                half, k["max_angle_deg"], label, bad, rep["views_valid"], rep["views_valid"] + rep["views_invalid"], big, c0, end,
                "%.6e (%d)" % (a[6]["final_cost"], a[6]["iterations"]), "yes" if ok else "NO"))


if __name__ == "__main__":
    main()
