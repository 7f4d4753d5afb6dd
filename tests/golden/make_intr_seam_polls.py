"""Results of the persistent intrinsics solve on a ragged problem of 37 frames, recorded on the GPU from PARENT_COMMIT: the state
before the hand-offs of a round were rescheduled (the control's gradient maximum across the lanes of its wave, the
statistics row stored from an idle wave; 4.8: the waits at the seams with a ring of polling loads in flight, measured and dropped).
Such changes move loads, waits and LDS traffic; every product, every sum and every maximum keeps its operands and its place, so the
solver must reproduce these numbers BIT FOR BIT (tests/test_gpu_intr_seam_polls.py). The problem of tests/golden/intr_loop_order_parent.npz
never has more than nine workers; here one frame per workgroup gives 37 workers (leaders with 16 / 16 / 5 rows), two give 19
(16 / 3 rows), four give 10 (one leader). Run once, on a GPU, on a build of PARENT_COMMIT:
    python tests/golden/make_intr_seam_polls.py      -> tests/golden/intr_seam_polls_parent.npz
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PARENT_COMMIT = "132cb25"   # "Test the shared device primitives against extended-precision references"
FRAMES = 37
CYCLE = [4, 63, 64, 65, 129, 255, 256, 257, 500]   # (what each size does to a team's waves: tests/golden/make_intr_loop_order.py)
POINTS = [CYCLE[i % len(CYCLE)] for i in range(FRAMES)]
TEAMS = (1, 2, 4)
MASKS = {"free": 0, "distortion_held": (1 << 8) | (1 << 6) | (1 << 7)}   # k3, p1, p2 constant
# the miss path (a decision that is not "accepted, radius at its clamp": second elimination, the rbox / e3 seam): the first reject
# set of tests/test_gpu_intr_batch_branches.py from a bad start of tests/test_gpu_lm_branches.py (seed, scale)
MISS_OPTIONS = dict(min_relative_decrease=0.99, initial_radius=1e8, max_iterations=16)
MISS_START = (0, 0.3)
# solve, continued solve (no reset: the handle's epochs run on), reset, solve -- short solves, so that the continued one has work left
SEQ_OPTIONS = dict(max_iterations=2)
FIELDS = ("iterations", "accepted", "costs", "radii", "intr", "q", "t")


def bad_start(inputs):
    """_bad_start of tests/test_gpu_lm_branches.py (a GPU test module: not imported for three lines) at MISS_START."""
    seed, scale = MISS_START
    rng = np.random.default_rng(seed)
    intr = inputs["intr0"].copy()
    intr[:2] *= 1.0 + 0.35 * scale
    intr[4:] = np.array([0.3, -0.2, 0.02, -0.02, 0.1]) * scale
    q = inputs["q0"] + 0.15 * scale * rng.normal(size=inputs["q0"].shape)
    t = inputs["t0"] * (1.0 + 0.25 * scale * rng.normal(size=inputs["t0"].shape))
    return intr, q, t


def make_inputs():
    sys.path.insert(0, ROOT)
    from tests.helpers import intrinsics_case
    c = intrinsics_case(FRAMES, POINTS)
    inputs = {k: c[k] for k in ("off", "uv", "xyz", "intr0", "q0", "t0")}
    inputs["intr_b"], inputs["q_b"], inputs["t_b"] = bad_start(inputs)
    return inputs


def _record(out, key, prob, s):
    intr, q, t = prob.get_state()
    out[key + "intr"], out[key + "q"], out[key + "t"] = intr, q, t
    out[key + "iterations"] = np.int64(s["iterations"])
    out[key + "costs"] = np.array([l["cost"] for l in s["log"]], dtype=np.float64)
    out[key + "radii"] = np.array([l["radius"] for l in s["log"]], dtype=np.float64)
    out[key + "accepted"] = np.array([l["accepted"] for l in s["log"]], dtype=np.int64)


def solve_all(inputs):
    """{f"t{teams}_{case}_{field}": array} of the persistent solve in each form (CC_INTR_PERSIST_TEAMS is read when a handle is
    created); cases: the MASKS (default options), "miss" (MISS_OPTIONS from the bad start), "seq0" / "seq1" / "seq2" (SEQ_OPTIONS on
    one handle: solve, continued solve, reset + solve)."""
    from camera_calibrator_amd import capi
    out = {}
    for teams in TEAMS:
        os.environ["CC_INTR_PERSIST_TEAMS"] = str(teams)
        try:
            def handle(intr, q, t, mask=0):
                prob = capi.IntrinsicsProblem(inputs["off"], inputs["uv"], inputs["xyz"])
                assert prob.solver_form() == teams, (prob.solver_form(), teams)
                prob.set_state(intr, q, t, const_mask=mask)
                return prob

            def finish(prob):
                form, reruns, note = prob.solver_status()
                prob.close()
                assert form == teams and reruns == 0, (form, reruns, note)   # (a rerun would be the two-kernel form's answer)

            for name, mask in MASKS.items():
                prob = handle(inputs["intr0"], inputs["q0"], inputs["t0"], mask)
                _record(out, "t%d_%s_" % (teams, name), prob, prob.solve())
                finish(prob)
            prob = handle(inputs["intr_b"], inputs["q_b"], inputs["t_b"])
            _record(out, "t%d_miss_" % teams, prob, prob.solve(capi.default_options(**MISS_OPTIONS)))
            finish(prob)
            prob = handle(inputs["intr0"], inputs["q0"], inputs["t0"])
            for i in range(3):
                if i == 2:
                    prob.reset()
                _record(out, "t%d_seq%d_" % (teams, i), prob, prob.solve(capi.default_options(**SEQ_OPTIONS)))
            finish(prob)
        finally:
            del os.environ["CC_INTR_PERSIST_TEAMS"]
    return out


if __name__ == "__main__":
    inputs = make_inputs()
    res = solve_all(inputs)
    for k, v in res.items():
        assert np.all(np.isfinite(v)), k
        if k.endswith("iterations"):
            print(k, int(v), "accepted", res[k[:-10] + "accepted"].tolist(), "costs", repr(float(res[k[:-10] + "costs"][0])), "->",
                  repr(float(res[k[:-10] + "costs"][-1])))
    dst = os.environ.get("INTR_SEAM_POLLS_OUT", os.path.join(os.path.dirname(os.path.abspath(__file__)), "intr_seam_polls_parent.npz"))
    np.savez_compressed(dst, parent_commit=PARENT_COMMIT, points=np.array(POINTS), **{"in_" + k: v for k, v in inputs.items()}, **res)
    print("wrote", dst, os.path.getsize(dst), "bytes")
