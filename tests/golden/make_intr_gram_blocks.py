"""Results of the persistent intrinsics solve on a ragged problem of 26 frames, recorded on the GPU from PARENT_COMMIT: the state
before the main loop's Gram block was formed on its ten upper 4 x 4 blocks (csrc/cc_gram_blocks.hpp). The new
products form every entry from the same factors in the same order and the reduction adds the same terms in the same order, so the
solver must reproduce these numbers BIT FOR BIT (tests/test_gpu_intr_gram_blocks.py). The point counts put on a team's waves less
than one row set of four rows (1, 3), an odd number of sets (5, 7, 9 -> 2, 2, 3; 60, 63 -> 15, 16), whole and ragged waves, second
and third passes with ragged tails (257, 260, 300, 511, 513, 520) and one frame too long for the residual-only tiles (2100 > 2048);
at four teams 26 frames leave the last workgroup with two frames, and at two and four teams the frames of a workgroup differ in
length throughout. Run once, on a GPU, on a build of PARENT_COMMIT:
    python tests/golden/make_intr_gram_blocks.py      -> tests/golden/intr_gram_blocks_parent.npz
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PARENT_COMMIT = "5c25109"   # "k_intr_persist: residual-only last sweep, cost from packed products"
POINTS = [1, 3, 4, 5, 7, 8, 9, 60, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 260, 300, 511, 513, 520, 2100]
TEAMS = (1, 2, 4)
HELD_MASK = (1 << 8) | (1 << 6) | (1 << 7) | (1 << 2)   # k3, p1, p2 and cx constant: held rows / columns in three of the four component groups
# the miss fixture of tests/golden/make_intr_seam_polls.py: a bad start under a demanding acceptance threshold
MISS_OPTIONS = dict(min_relative_decrease=0.99, initial_radius=1e8, max_iterations=16)
MISS_START = (0, 0.3)
LOG_FIELDS = ("cost", "cost_change", "model_cost_change", "radius", "gradient_max_norm", "accepted")
# case -> (start, const_mask, options, final-sweep mode); mode 1 is the default
CASES = {
    "default": ("0", 0, {}, 1),
    "limit_1": ("0", 0, dict(max_iterations=1), 1),
    "limit_2": ("0", 0, dict(max_iterations=2), 1),
    "held": ("0", HELD_MASK, {}, 1),
    "miss": ("_b", 0, MISS_OPTIONS, 1),
    "mode_0": ("0", 0, {}, 0),
    "mode_2": ("0", 0, {}, 2),
    "miss_mode_2": ("_b", 0, MISS_OPTIONS, 2),
}


def make_inputs():
    sys.path.insert(0, ROOT)
    from oracle import pyoracle as po
    frames = len(POINTS)
    # (the start comes from Zhang's method, which wants a homography per frame: generated with at least eight points a frame, the
    # frames then cut down to POINTS)
    off, uv, xyz = po.make_intrinsics_problem(frames, [max(n, 8) for n in POINTS])
    K, q, t = po.zhang_init(off, uv, xyz)
    keep = np.concatenate([np.arange(off[f], off[f] + POINTS[f]) for f in range(frames)])
    inputs = dict(off=np.concatenate([[0], np.cumsum(POINTS)]).astype(np.int64), uv=np.ascontiguousarray(uv[keep]), xyz=np.ascontiguousarray(xyz[keep]),
                  intr0=np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2], 0, 0, 0, 0, 0], dtype=np.float64), q0=q.astype(np.float64), t0=t.astype(np.float64))
    seed, scale = MISS_START
    rng = np.random.default_rng(seed)
    intr = inputs["intr0"].copy()
    intr[:2] *= 1.0 + 0.35 * scale
    intr[4:] = np.array([0.3, -0.2, 0.02, -0.02, 0.1]) * scale
    inputs["intr_b"] = intr
    inputs["q_b"] = inputs["q0"] + 0.15 * scale * rng.normal(size=inputs["q0"].shape)
    inputs["t_b"] = inputs["t0"] * (1.0 + 0.25 * scale * rng.normal(size=inputs["t0"].shape))
    return inputs


def solve_all(inputs):
    """{f"t{teams}_{case}_{field}": array} of the persistent solve in each form x case (CC_INTR_PERSIST_TEAMS is read when a handle
    is created)."""
    from camera_calibrator_amd import capi
    out = {}
    for teams in TEAMS:
        os.environ["CC_INTR_PERSIST_TEAMS"] = str(teams)
        try:
            for case, (start, mask, opts, mode) in CASES.items():
                prob = capi.IntrinsicsProblem(inputs["off"], inputs["uv"], inputs["xyz"])
                assert prob.solver_form() == teams, (prob.solver_form(), teams)
                prob.set_state(inputs["intr" + start], inputs["q" + start], inputs["t" + start], const_mask=mask)
                prob.set_final_sweep(mode)
                s = prob.solve(capi.default_options(**opts))
                intr, q, t = prob.get_state()
                counts = prob.final_sweep_counts()
                form, reruns, note = prob.solver_status()
                prob.close()
                assert form == teams and reruns == 0, (form, reruns, note)   # (a rerun would be the two-kernel form's answer)
                k = "t%d_%s_" % (teams, case)
                out[k + "intr"], out[k + "q"], out[k + "t"] = intr, q, t
                out[k + "iterations"] = np.int64(s["iterations"])
                out[k + "sweeps"] = np.int64(s["sweeps"])
                out[k + "termination"] = np.array(s["termination"])
                out[k + "costs2"] = np.array([s["initial_cost"], s["final_cost"]], dtype=np.float64)
                out[k + "counts"] = np.array(counts, dtype=np.int64)
                for f in LOG_FIELDS:
                    out[k + "log_" + f] = np.array([l[f] for l in s["log"]], dtype=np.int64 if f == "accepted" else np.float64)
        finally:
            del os.environ["CC_INTR_PERSIST_TEAMS"]
    return out


def check_ends_as_intended(res):
    """Every case converges or ends as it is meant to -- checked on the parent before recording, and by the test on the recording."""
    for teams in TEAMS:
        def get(case, field):
            return res["t%d_%s_%s" % (teams, case, field)]
        for case in ("default", "held", "mode_0", "mode_2"):
            assert str(get(case, "termination")) == "FUNCTION" and int(get(case, "iterations")) >= 3, (teams, case, get(case, "termination"), get(case, "iterations"))
        for n in (1, 2):
            assert str(get("limit_%d" % n, "termination")) == "NO_CONVERGENCE" and int(get("limit_%d" % n, "iterations")) == n, (teams, n)
        for case in ("miss", "miss_mode_2"):
            acc = get(case, "log_accepted").tolist()
            assert acc.count(0) >= 2 and acc.count(1) >= 2, (teams, case, acc)
        assert tuple(get("mode_0", "counts")) == (0, 0) and get("default", "counts")[0] >= 1 and get("miss_mode_2", "counts")[1] >= 1, \
            (teams, get("mode_0", "counts"), get("default", "counts"), get("miss_mode_2", "counts"))


if __name__ == "__main__":
    inputs = make_inputs()
    res = solve_all(inputs)
    for k, v in res.items():
        if k.endswith("iterations"):
            b = k[:-10]
            print(k, int(v), str(res[b + "termination"]), "accepted", res[b + "log_accepted"].tolist(), "counts", res[b + "counts"].tolist(),
                  "costs", repr(float(res[b + "costs2"][0])), "->", repr(float(res[b + "costs2"][1])))
        elif v.dtype.kind == "f":
            assert np.all(np.isfinite(v)), k
    check_ends_as_intended(res)
    dst = os.environ.get("INTR_GRAM_BLOCKS_OUT", os.path.join(os.path.dirname(os.path.abspath(__file__)), "intr_gram_blocks_parent.npz"))
    np.savez_compressed(dst, parent_commit=PARENT_COMMIT, points=np.array(POINTS), **{"in_" + k: v for k, v in inputs.items()}, **res)
    print("wrote", dst, os.path.getsize(dst), "bytes")
