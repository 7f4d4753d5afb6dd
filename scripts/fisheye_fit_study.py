"""What the fisheye model buys on a wide lens, on the CPU reference (tests/fisheye_ref.py: data from the 50-digit model, the
numpy LM): boards seen through a 140 degree fisheye (fx 620, fy 615, k = -0.035 0.004 -0.0009 0.0001, 0.3 px noise), fitted with
the radial-tangential model and with the fisheye model from the SAME Zhang (pinhole) start -- final RMS reprojection error and
fx for three shapes; how many LM iterations the pinhole start costs the fisheye solve (against a start at the generator's own
poses and K with k = 0); and a sweep over the field of view for where the Zhang start stops converging. No GPU needed.

    python scripts/fisheye_fit_study.py > profiles/r11/fisheye_fit_study.txt"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import pyoracle as po  # noqa: E402
from tests import fisheye_ref as fr  # noqa: E402

SHAPES = {"6x48": [48] * 6, "8x40": [40] * 8, "12x100": [100] * 12}


def fit(c, model, mask, intr0=None, q0=None, t0=None):
    P = fr.Problem(model, c["off"], c["uv"], c["xyz"], 0.0, mask)
    intr, _, _, s = fr.lm_solve(P, c["intr0"] if intr0 is None else intr0, c["q0"] if q0 is None else q0, c["t0"] if t0 is None else t0,
                                po.default_options())
    return intr, s, float(np.sqrt(2 * s["final_cost"] / len(c["uv"])))


def main():
    print("shape    fov_deg  zhang_fx  | radtan: iters term rms_px fx | fisheye: iters term rms_px fx | fisheye from the true poses: iters")
    for name, counts in SHAPES.items():
        c = fr.make_case(counts, 0.29, 0.22, 0.30, 0.3)
        ir, sr, rr = fit(c, fr.pinhole_model, 0)
        iff, sf, rf = fit(c, fr.fisheye_model, fr.K8_HELD)
        true0 = c["intr_true"].copy()
        true0[4:] = 0
        _, st, _ = fit(c, fr.fisheye_model, fr.K8_HELD, true0, c["q_true"], c["t_true"])
        print("%-8s %6.1f  %8.2f  | %3d %-14s %8.3f %8.2f | %3d %-10s %6.3f %8.2f | %3d" % (
            name, 2 * np.degrees(c["theta_max"]), c["intr0"][0], sr["iterations"], sr["termination"], rr, ir[0],
            sf["iterations"], sf["termination"], rf, iff[0], st["iterations"]))
    print()
    print("field of view sweep, 6x48 (board half-size varied): fisheye fit from the Zhang start")
    print("half_m  fov_deg  zhang_fx  iters term            rms_px   fx")
    for half in (0.15, 0.22, 0.29, 0.36, 0.45, 0.55, 0.70):
        c = fr.make_case([48] * 6, half, 0.22, 0.30, 0.3)
        if not np.all(np.isfinite(c["intr0"])):
            print("%5.2f   %6.1f  Zhang start not finite" % (half, 2 * np.degrees(c["theta_max"])))
            continue
        iff, sf, rf = fit(c, fr.fisheye_model, fr.K8_HELD)
        print("%5.2f   %6.1f  %8.2f  %3d  %-14s %8.3f %8.2f" % (half, 2 * np.degrees(c["theta_max"]), c["intr0"][0], sf["iterations"], sf["termination"], rf, iff[0]))


if __name__ == "__main__":
    main()
