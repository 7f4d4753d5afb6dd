"""Results of the persistent intrinsics solve on a small ragged problem, recorded on the GPU from PARENT_COMMIT: the state before
the kernel's bit-preserving restructurings began (the broadcast stored by the solving wave, the Jacobi scales
folded into the row build; 4.8: both Gram row sets staged in front of one matrix burst, measured and dropped). Such changes
move LDS traffic, barriers and stores; every product and every sum keeps its operands and its place, so the solver must
reproduce these numbers BIT FOR BIT (tests/test_gpu_intr_loop_order.py). Run once, on a GPU, on a build of PARENT_COMMIT:
    python tests/golden/make_intr_loop_order.py      -> tests/golden/intr_loop_order_parent.npz
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PARENT_COMMIT = "ef9e59a"   # "Share one host-side solve driver between the intrinsics and rig handles"
# the waves of a team (64 points per wave and pass, 256 per team and pass) see zero, one and two passes, and last passes that
# are valid in part: 4 -> one wave, four lanes; 63 / 64 / 65 -> one wave short of / exactly / one lane into the second;
# 129 -> third wave; 255 / 256 / 257 -> one pass short of / exactly / one lane into the second pass; 500 -> the benchmark's frame
POINTS = [4, 63, 64, 65, 129, 255, 256, 257, 500]
TEAMS = (1, 2, 4)
MASKS = {"free": 0, "distortion_held": (1 << 8) | (1 << 6) | (1 << 7)}   # k3, p1, p2 constant


def solve_all(inputs):
    """{f"t{teams}_{mask name}_{field}": array} of the persistent solve in each form x mask (CC_INTR_PERSIST_TEAMS is read when a
    handle is created)."""
    from camera_calibrator_amd import capi
    out = {}
    for teams in TEAMS:
        os.environ["CC_INTR_PERSIST_TEAMS"] = str(teams)
        try:
            for name, mask in MASKS.items():
                prob = capi.IntrinsicsProblem(inputs["off"], inputs["uv"], inputs["xyz"])
                assert prob.solver_form() == teams, (prob.solver_form(), teams)
                prob.set_state(inputs["intr0"], inputs["q0"], inputs["t0"], const_mask=mask)
                s = prob.solve()
                intr, q, t = prob.get_state()
                form, reruns, note = prob.solver_status()
                prob.close()
                assert form == teams and reruns == 0, (form, reruns, note)   # (a rerun would be the two-kernel form's answer)
                k = "t%d_%s_" % (teams, name)
                out[k + "intr"], out[k + "q"], out[k + "t"] = intr, q, t
                out[k + "iterations"] = np.int64(s["iterations"])
                out[k + "costs"] = np.array([l["cost"] for l in s["log"]], dtype=np.float64)
                out[k + "accepted"] = np.array([l["accepted"] for l in s["log"]], dtype=np.int64)
        finally:
            del os.environ["CC_INTR_PERSIST_TEAMS"]
    return out


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    from tests.helpers import intrinsics_case
    c = intrinsics_case(len(POINTS), POINTS)
    inputs = {k: c[k] for k in ("off", "uv", "xyz", "intr0", "q0", "t0")}
    res = solve_all(inputs)
    for k, v in res.items():
        assert np.all(np.isfinite(v)), k
        if k.endswith("iterations"):
            print(k, int(v), "costs", repr(float(res[k[:-10] + "costs"][0])), "->", repr(float(res[k[:-10] + "costs"][-1])))
    dst = os.environ.get("INTR_LOOP_ORDER_OUT", os.path.join(os.path.dirname(os.path.abspath(__file__)), "intr_loop_order_parent.npz"))
    np.savez_compressed(dst, parent_commit=PARENT_COMMIT, points=np.array(POINTS), **{"in_" + k: v for k, v in inputs.items()}, **res)
    print("wrote", dst, os.path.getsize(dst), "bytes")
