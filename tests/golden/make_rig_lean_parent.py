"""Results of the rig solve on five small problems, recorded on the GPU from PARENT_COMMIT: the state before the leftovers of
the retired glued kernel were cleared out of the rig path. That clean-up moves no arithmetic, but it may
change the code of the four lean persistent kernels (k_rig_persist_w<1|2|4>, k_rig_persist_ctl: pointer tests that are always
true removed, one broadcast wait shared with k_intr_persist), so the solver must reproduce these numbers BIT FOR BIT
(tests/test_gpu_rig_lean_bits.py). Run once, on a GPU, on a build of PARENT_COMMIT:
    python tests/golden/make_rig_lean_parent.py      -> tests/golden/rig_lean_parent.npz
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PARENT_COMMIT = "41d661c"   # "k_intr_persist: drop the control's scaling pass and two barriers"
TIGHT = dict(function_tolerance=1e-15, gradient_tolerance=1e-13, parameter_tolerance=1e-14, max_iterations=200)
# Huber-robustified steps of this scenario gain 1.6 - 1.9 times what the model predicts (tests/test_gpu_lm_branches.py), so a
# threshold of 1.55 without non-monotonic steps accepts the first steps and REJECTS the later ones (CPU oracle: ten accepted,
# then nine rejected on the ragged case; two, then nine at 2 x 260 x 4): rounds whose assumed decision holds, then miss rounds,
# where the workers eliminate a second time, with a shrinking radius.
PICKY = dict(min_relative_decrease=1.55, use_nonmonotonic_steps=0, max_iterations=60)
# name: (cameras, frames, points per frame, CC_RIG_PERSIST or None, form the handle must report (2: lean, 0: three kernels),
#        ragged + outliers, options). The lean form takes the fewest frames per workgroup that leave G <= 255 workgroups:
#        50 and 40 frames -> one, 260 -> two (130 workgroups), 520 -> four (130 workgroups).
CASES = {
    "one_2x50x4": (2, 50, 4, None, 2, False, TIGHT),          # solved down to the noise floor, every step accepted
    "one_4x40x30_ragged": (4, 40, 30, None, 2, True, PICKY),
    "two_2x260x4": (2, 260, 4, None, 2, False, PICKY),
    "four_2x520x4": (2, 520, 4, "1", 2, False, dict(max_iterations=1000)),
    "three_kernels_3x20x30": (3, 20, 30, "0", 0, False, dict(max_iterations=1000)),
}
LEAN = [n for n, c in CASES.items() if c[4] == 2]
IN_FIELDS = ("frame_offsets", "obs_cam", "obs_world", "obs_uv", "world_xyz", "cam_frozen", "cam_q0", "cam_t0", "frame_q0", "frame_t0")
OUT_FIELDS = ("cam_q", "cam_t", "frame_q", "frame_t", "obs_cost", "iterations", "termination", "accepted", "costs")


def make_inputs(name):
    """The rig tests' scenario (po.rig_scenario); ragged: random drop-outs, frame 7 empty, and a tenth of the image points
    displaced by several times the Huber constant, so that blocks sit in the loss's linear tail at the minimiser."""
    from oracle import pyoracle as po
    cams, frames, pts, _, _, ragged, _ = CASES[name]
    sc = po.rig_scenario(cams, frames, pts)
    if ragged:
        rng = np.random.default_rng(0)
        n = len(sc["obs_cam"])
        off0 = sc["frame_offsets"]
        keep = rng.uniform(size=n) > 0.3
        keep[off0[7]:off0[8]] = False
        outlier = rng.random(n) < 0.10
        shift = rng.uniform(0.02, 0.06, size=(n, 2)) * rng.choice([-1.0, 1.0], size=(n, 2))
        uv = sc["obs_uv"].astype(np.float64)
        uv[outlier] += shift[outlier]
        counts = [np.count_nonzero(keep[off0[f]:off0[f + 1]]) for f in range(frames)]
        sc = dict(sc, obs_cam=sc["obs_cam"][keep], obs_world=sc["obs_world"][keep], obs_uv=uv.astype(np.float32)[keep],
                  frame_offsets=np.concatenate([[0], np.cumsum(counts)]).astype(np.int64))
    cq, ct = po.affine_to_qt(sc["cam_T"])
    fq, ft = po.affine_to_qt(sc["frame_T"])
    sc = dict(sc, cam_q0=cq, cam_t0=ct, frame_q0=fq, frame_t0=ft)
    return {k: np.ascontiguousarray(sc[k]) for k in IN_FIELDS}


def solve_case(name, inp):
    """{field: array} of the GPU solve of one case in the form it names (CC_RIG_PERSIST is read when a handle is created)."""
    from camera_calibrator_amd import capi
    cams, _, _, env, want_form, _, opts = CASES[name]
    old = os.environ.pop("CC_RIG_PERSIST", None)
    if env is not None:
        os.environ["CC_RIG_PERSIST"] = env
    try:
        prob = capi.RigProblem(cams, inp["frame_offsets"], inp["obs_cam"], inp["obs_world"], inp["obs_uv"], inp["world_xyz"], inp["cam_frozen"])
        assert prob.solver_form() == want_form, (name, prob.solver_form(), want_form)
        prob.set_state(inp["cam_q0"], inp["cam_t0"], inp["frame_q0"], inp["frame_t0"])
        s = prob.solve(capi.default_options(**opts))
        cq, ct, fq, ft, cost = prob.get_state()
        form, reruns, note = prob.solver_status()
        prob.close()
    finally:
        os.environ.pop("CC_RIG_PERSIST", None)
        if old is not None:
            os.environ["CC_RIG_PERSIST"] = old
    assert form == want_form and reruns == 0, (name, form, reruns, note)   # (a rerun would be the three-kernel form's answer)
    return dict(cam_q=cq, cam_t=ct, frame_q=fq, frame_t=ft, obs_cost=cost, iterations=np.int64(s["iterations"]),
                termination=np.array(s["termination"]), accepted=np.array([l["accepted"] for l in s["log"]], dtype=np.int64),
                costs=np.array([l["cost"] for l in s["log"]], dtype=np.float64))


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    out = {}
    rejected = []
    for name in CASES:
        inp = make_inputs(name)
        res = solve_case(name, inp)
        assert set(res) == set(OUT_FIELDS)
        for k in ("cam_q", "cam_t", "frame_q", "frame_t", "obs_cost", "costs"):
            assert np.all(np.isfinite(res[k])), (name, k)
        assert int(res["iterations"]) >= 3, (name, int(res["iterations"]))
        if name in LEAN and np.any(res["accepted"][:-1] == 0):   # (a rejection the solve went on from)
            rejected.append(name)
        print(name, "observations", len(inp["obs_cam"]), "iterations", int(res["iterations"]), str(res["termination"]),
              "accepted", "".join(str(int(a)) for a in res["accepted"]), "cost", repr(float(res["costs"][0])), "->", repr(float(res["costs"][-1])))
        out.update({name + "_in_" + k: v for k, v in inp.items()})
        out.update({name + "_" + k: v for k, v in res.items()})
    assert rejected, "no lean case rejects a step: the workers' second elimination (a miss round) would go untested"
    dst = os.environ.get("RIG_LEAN_PARENT_OUT", os.path.join(os.path.dirname(os.path.abspath(__file__)), "rig_lean_parent.npz"))
    np.savez_compressed(dst, parent_commit=PARENT_COMMIT, lean_cases_with_a_rejected_step=np.array(rejected), **out)
    print("wrote", dst, os.path.getsize(dst), "bytes")
