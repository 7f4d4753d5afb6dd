"""What a pixel model per camera buys the rig solve with intrinsics (CPU only: tests/rigk_mixed_ref.py's reference LM in float64).

    python scripts/rigk_mixed_fit_study.py > profiles/r18/rigk_mixed_fit_study.txt

Scenario: rigk_mixed_ref.mixed_rig_case(2, 12, 20, "RF", half): camera 0 a radial-tangential lens, camera 1 a fisheye lens, each
with pixels of its own model + N(0, 0.3) px, the points' x and y stretched to +-half. Three fits from the same start, default
options, <= 200 iterations: each camera with its own model (what cc_rigk_set_camera_model gives), the radial-tangential model for
both cameras and the fisheye model for both (what one model per handle allows). RMS = sqrt(2 cost / observations), over the whole
rig and over the camera the fit's model does not belong to."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import pyoracle as po            # noqa: E402
from tests import rigk_mixed_ref as mr       # noqa: E402
from tests import rigk_fisheye_ref as rr     # noqa: E402


def fit(k, kinds):
    """(iterations, termination, rms whole rig, rms per camera) of the fit with kinds[c] as camera c's model; a camera fitted with
    the other model than its own starts from that model's start intrinsics."""
    own = k["kinds"]
    intr0 = np.array([k["intr0"][c] if kinds[c] == own[c] else (rr.INTR0 if kinds[c] == "F" else np.array([1020.0, 980.0, 805.0, 495.0, 0, 0, 0, 0, 0]))
                      for c in range(k["cams"])])
    P = mr.problem(k, kinds=kinds)
    out = rr.rigk_solve(P, intr0, k["cam_q0"], k["cam_t0"], k["frame_q0"], k["frame_t0"], options=po.default_options(max_iterations=200))
    oc, s = out[5], out[6]
    per_cam = [float(np.sqrt(2 * oc[P.by_cam[c]].sum() / len(P.by_cam[c]))) for c in range(k["cams"])]
    return s["iterations"], s["termination"], float(np.sqrt(2 * s["final_cost"] / len(oc))), per_cam


def main():
    print(__doc__.split("\n\n")[0])
    print()
    print("2 cameras x 12 frames x 20 points = 480 observations; camera 0 radial-tangential, camera 1 fisheye; 0.3 px noise per coordinate")
    print("(0.42 px per observation before the fit absorbs its share). iterations / termination / RMS whole rig [/ RMS of the camera")
    print("whose lens the fit's model is not].")
    print()
    print("%-9s %-10s %-34s %-44s %-44s" % ("half [m]", "max angle", "each camera its own model", "radial-tangential for both (fisheye camera)", "fisheye for both (radial-tangential camera)"))
    for half in (0.5, 0.8, 1.0, 1.3):
        k = mr.mixed_rig_case(2, 12, 20, "RF", half=half)
        cells = []
        for kinds, other in (("RF", None), ("RR", 1), ("FF", 0)):
            it, term, rms, per_cam = fit(k, kinds)
            cell = "%3d it %-14s %.3g px" % (it, term, rms)
            if other is not None:
                cell += " (%.3g px)" % per_cam[other]
            cells.append(cell)
        print("%-9.1f %-10s %-34s %-44s %-44s" % (half, "%.1f deg" % k["max_angle_deg"], *cells))


if __name__ == "__main__":
    main()
