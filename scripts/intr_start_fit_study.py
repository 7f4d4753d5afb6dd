#!/usr/bin/env python3
"""Where Zhang's pinhole start of the fisheye solve goes wrong and what the focal-length search does there (CPU reference only,
no GPU): boards placed round a fisheye lens (tests/intr_start_ref.scene), solved with tests/fisheye_ref.lm_solve at the default
options from three starts -- the generator's poses with the true fx fy px py and k = 0, Zhang's (oracle.pyoracle.zhang_init), and
the focal-length search of tests/intr_start_ref.start at its defaults.

    python scripts/intr_start_fit_study.py > profiles/r21/intr_start_fit_study.txt
    python scripts/intr_start_fit_study.py --seeds 1 40 F side half dist max_dir     # one line per seed of that geometry
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import pyoracle as po   # noqa: E402
from tests import fisheye_ref as fr   # noqa: E402
from tests import intr_start_ref as ref   # noqa: E402

SCENES = [(8, 7, 0.3, 0.45, 40.0, 1), (10, 7, 0.3, 0.40, 75.0, 2), (12, 6, 0.25, 0.35, 95.0, 3), (12, 6, 0.25, 0.35, 95.0, 5),
          (6, 5, 0.3, 0.40, 85.0, 6), (10, 7, 0.3, 0.40, 75.0, 7), (10, 7, 0.3, 0.40, 85.0, 8), (10, 7, 0.3, 0.40, 85.0, 9)]


def solve(c, intr0, q0, t0):
    P = fr.Problem(fr.fisheye_model, c["off"], c["uv"], c["xyz"], 0.0, fr.K8_HELD)
    return fr.lm_solve(P, intr0, q0, t0, po.default_options())


def row(key):
    c = ref.scene(*key)
    a = solve(c, c["intr0_true"], c["q_true"], c["t_true"])
    K, qz, tz = po.zhang_init(c["off"], c["uv"], c["xyz"])
    z = solve(c, np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2], 0, 0, 0, 0, 0], dtype=np.float64), qz.astype(np.float64), tz.astype(np.float64))
    s = ref.start(c["off"], c["uv"], c["xyz"])
    order = np.sort(s["score"][s["qualified"] == 1])
    margin = (order[1] - order[0]) / order[0] if len(order) > 1 else float("nan")
    b = solve(c, s["intr"], s["q"], s["t"])
    same = lambda x: "same" if abs(x[3]["final_cost"] - a[3]["final_cost"]) <= 1e-6 * a[3]["final_cost"] else f"ends at {x[3]['final_cost']:.6g}, fx {x[0][0]:.0f}"
    return (f"{key[0]:2d} {key[1]:2d} {key[2]:.2f} {key[3]:.2f} {key[4]:4.0f} {key[5]:3d} | {c['max_angle_deg']:6.1f} deg {100 * c['beyond_90']:5.1f} % | "
            f"{a[3]['iterations']:3d} it {a[3]['final_cost']:.6g} | Zhang fx {K[0, 0]:6.0f} centre off {np.hypot(K[0, 2] - c['intr_true'][2], K[1, 2] - c['intr_true'][3]):5.0f} px, "
            f"{z[3]['iterations']:3d} it {same(z)} | search f {s['report']['focal']:.0f} (candidate {s['best']}, {int(s['qualified'].sum())} qualified, margin {100 * margin:.1f} %), "
            f"{b[3]['iterations']:3d} it {same(b)}")


def main():
    head = " F side half dist max_dir seed | largest angle, beyond 90 | generator's poses | Zhang start | focal-length search"
    if len(sys.argv) > 1 and sys.argv[1] == "--seeds":
        lo, hi = int(sys.argv[2]), int(sys.argv[3])
        F, side, half, dist, max_dir = int(sys.argv[4]), int(sys.argv[5]), float(sys.argv[6]), float(sys.argv[7]), float(sys.argv[8])
        print(head)
        for seed in range(lo, hi):
            print(row((F, side, half, dist, max_dir, seed)), flush=True)
        return
    print("# boards round a fisheye lens (fx 620, fy 615, centre 805 495), 0.3 px noise; fisheye_ref.lm_solve, default options")
    print(head)
    for key in SCENES:
        print(row(key), flush=True)
    print("\n# the same geometry (10 boards of 7 x 7, half 0.3, distance 0.40, seed 2) with the boards' directions up to max_dir off the axis")
    print(head)
    for max_dir in (0.0, 15.0, 30.0, 45.0, 60.0, 75.0, 85.0, 95.0):
        print(row((10, 7, 0.3, 0.40, max_dir, 2)), flush=True)


if __name__ == "__main__":
    main()
