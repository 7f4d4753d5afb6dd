"""k_intr_persist sweeps the round whose decision is predicted to end the solve RESIDUAL-ONLY: no Gram block, no elimination row,
the cost formed by packed matrix products (csrc/cc_persist_pack.hpp). cc_intrinsics_set_final_sweep switches it: 0 every sweep
full (the kernel before the change), 1 the control's prediction (the default), 2 a prediction at every accepting decision, so that
the wrong prediction's path -- the full sweep made up for, the second elimination -- runs on every round. Whatever the mode, the
solve has to give the same BITS: iteration count, termination, every log record, intrinsics, poses, costs, the sweep count.
Bit equality against mode 0 of the same build (and, in the default mode, the parent commit's recordings of
tests/test_gpu_intr_seam_polls.py and its neighbours) is the whole yardstick; there is no tolerance.

Forty ragged frames whose point counts put 0, 1 and 2 passes on the waves of a team in every combination (1 and 63 points: frames
below one wave; 64 / 65, 128 / 129, 192 / 193: a wave more with ONE observation; 256 / 257, 300: a second pass on one wave, on
one wave of 44 lanes), in the forms of one, two and four frames per workgroup."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FRAMES = 40
CYCLE = [1, 63, 64, 65, 128, 129, 192, 193, 256, 257, 300]
POINTS = [CYCLE[i % len(CYCLE)] for i in range(FRAMES)]
TEAMS = (1, 2, 4)
MODES = (0, 1, 2)
MASKS = {"free": 0, "distortion_held": (1 << 8) | (1 << 6) | (1 << 7)}   # k3, p1, p2 constant
# the miss fixture of tests/golden/make_intr_seam_polls.py: a bad start under a demanding acceptance threshold
MISS_OPTIONS = dict(min_relative_decrease=0.99, initial_radius=1e8, max_iterations=16)
MISS_START = (0, 0.3)
OTHER_ENDINGS = {"no_ftol": dict(function_tolerance=0.0, max_iterations=12), "gradient": dict(function_tolerance=0.0, gradient_tolerance=1e-2)}
SEQ_OPTIONS = dict(max_iterations=2)
SEQ_MODES = {0: (0, 0, 0), 1: (1, 2, 1), 2: (2, 1, 2)}   # the mode of solve, continued solve, solve after reset -- switched in between
LOG_FIELDS = ("cost", "cost_change", "model_cost_change", "radius", "gradient_max_norm", "accepted")


def predicts_end(cc_k, cc_prev, function_tolerance, x_cost):
    """persist_predicts_end (csrc/cc_intrinsics_persist.hpp)."""
    if not (cc_k > 0.0) or not (cc_prev > 0.0):
        return False
    return cc_k * min(1.0, cc_k / cc_prev) <= function_tolerance * x_cost


def expected_counts(log, termination, mode, max_iterations, function_tolerance):
    """(residual_only, redone) the control must count on a solve with this log: its prediction rule, replayed."""
    ro = redone = 0
    stop = False
    cc_prev = 0.0
    pred = mode == 2 or (mode == 1 and 1 >= max_iterations)      # the decision on the starting point
    for i, rec in enumerate(log):                                 # the decision of iteration i + 1
        ends = i == len(log) - 1 and termination in ("NO_CONVERGENCE", "FUNCTION", "PARAMETER", "FAILURE_INVALID_STEPS")
        acc = bool(rec["accepted"])
        if pred:
            ro += 1
            if not ends:
                stop = stop or mode == 1
                redone += acc
        pred = False
        if not ends and mode and not stop and acc:
            pred = mode == 2 or i + 2 >= max_iterations or predicts_end(rec["cost_change"], cc_prev, function_tolerance, rec["cost"])
        if acc:
            cc_prev = rec["cost_change"]
    return ro, redone


def _inputs():
    from oracle import pyoracle as po
    # (the start comes from Zhang's method, which wants a homography per frame: generated with at least eight points a frame, the
    # frames then cut down to POINTS)
    gen = [max(n, 8) for n in POINTS]
    off, uv, xyz = po.make_intrinsics_problem(FRAMES, gen)
    K, q, t = po.zhang_init(off, uv, xyz)
    keep = np.concatenate([np.arange(off[f], off[f] + POINTS[f]) for f in range(FRAMES)])
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


def _record(prob, s):
    intr, q, t = prob.get_state()
    out = {"intr": intr, "q": q, "t": t, "iterations": np.int64(s["iterations"]), "sweeps": np.int64(s["sweeps"]),
           "termination": s["termination"], "costs2": np.array([s["initial_cost"], s["final_cost"]]), "counts": prob.final_sweep_counts(),
           "log": s["log"]}
    for k in LOG_FIELDS:
        out["log_" + k] = np.array([l[k] for l in s["log"]], dtype=np.int64 if k == "accepted" else np.float64)
    return out


@pytest.fixture(scope="module")
def inputs():
    return _inputs()


@pytest.fixture(scope="module")
def solved(inputs):
    """{(teams, case, mode): record} -- every solve of this module, once."""
    from camera_calibrator_amd import capi
    out = {}
    for teams in TEAMS:
        os.environ["CC_INTR_PERSIST_TEAMS"] = str(teams)
        try:
            def handle(start, mask=0):
                prob = capi.IntrinsicsProblem(inputs["off"], inputs["uv"], inputs["xyz"])
                assert prob.solver_form() == teams, (prob.solver_form(), teams)
                prob.set_state(inputs["intr" + start], inputs["q" + start], inputs["t" + start], const_mask=mask)
                return prob

            def finish(prob):
                form, reruns, note = prob.solver_status()
                prob.close()
                assert form == teams and reruns == 0, (form, reruns, note)   # (a rerun would be the two-kernel form's answer)

            for mode in MODES:
                cases = [("default_" + name, "0", mask, {}) for name, mask in MASKS.items()]
                cases += [("limit_%d" % n, "0", 0, dict(max_iterations=n)) for n in (1, 2, 3)]
                cases += [("miss", "_b", 0, MISS_OPTIONS)]
                cases += [("other_" + name, "0", 0, o) for name, o in OTHER_ENDINGS.items()]
                for case, start, mask, opts in cases:
                    prob = handle(start, mask)
                    prob.set_final_sweep(mode)
                    out[teams, case, mode] = _record(prob, prob.solve(capi.default_options(**opts)))
                    finish(prob)
                prob = handle("0")
                for i in range(3):
                    if i == 2:
                        prob.reset()
                    prob.set_final_sweep(SEQ_MODES[mode][i])
                    out[teams, "seq%d" % i, mode] = _record(prob, prob.solve(capi.default_options(**SEQ_OPTIONS)))
                finish(prob)
        finally:
            del os.environ["CC_INTR_PERSIST_TEAMS"]
    return out


def _assert_bit_equal(got, want, what):
    assert int(got["iterations"]) == int(want["iterations"]) and got["termination"] == want["termination"], (what, got["iterations"], want["iterations"], got["termination"], want["termination"])
    assert int(got["sweeps"]) == int(want["sweeps"]), (what, got["sweeps"], want["sweeps"])
    for field in ["log_" + k for k in LOG_FIELDS] + ["intr", "q", "t", "costs2"]:
        g, w = np.ascontiguousarray(got[field]), np.ascontiguousarray(want[field])
        assert g.shape == w.shape and g.dtype == w.dtype, (what, field, g.shape, w.shape)
        diff = np.flatnonzero(g.view(np.uint8).reshape(-1) != w.view(np.uint8).reshape(-1))
        assert diff.size == 0, (what, field, "first differing element", int(diff[0]) // g.itemsize, g.reshape(-1)[diff[0] // g.itemsize], w.reshape(-1)[diff[0] // g.itemsize])


def _check_case(solved, teams, case, max_iterations, function_tolerance, seq=None):
    base = solved[teams, case, 0]
    assert base["counts"] == (0, 0), base["counts"]                     # mode 0: every sweep full
    for mode in (1, 2):
        got = solved[teams, case, mode]
        print(teams, case, mode, "iterations", int(got["iterations"]), got["termination"], "accepted", got["log_accepted"].tolist(), "counts", got["counts"])
        _assert_bit_equal(got, base, (teams, case, mode))
        ran = mode if seq is None else SEQ_MODES[mode][seq]
        assert got["counts"] == expected_counts(got["log"], got["termination"], ran, max_iterations, function_tolerance), (teams, case, mode, got["counts"])


def _defaults():
    from camera_calibrator_amd import capi
    o = capi.default_options()
    return o.max_iterations, o.function_tolerance


@pytest.mark.parametrize("mask", list(MASKS))
@pytest.mark.parametrize("teams", TEAMS)
def test_default_solve_ends_on_a_predicted_residual_only_sweep(inputs, solved, teams, mask):
    from oracle import pyoracle as po
    max_it, ftol = _defaults()
    _check_case(solved, teams, "default_" + mask, max_it, ftol)
    got = solved[teams, "default_" + mask, 1]
    assert got["termination"] == "FUNCTION" and got["counts"][0] >= 1 and got["counts"][1] == 0, (got["termination"], got["counts"])
    # the fixture's own oracle log (CPU): the function-tolerance predictor fires exactly once, in front of the decision that ends the solve
    _, _, _, s = po.intrinsics_solve(inputs["off"], inputs["uv"], inputs["xyz"], inputs["intr0"], inputs["q0"], inputs["t0"], const_mask=MASKS[mask])
    assert s["termination"] == "FUNCTION", s["termination"]
    fired, cc_prev = [], 0.0
    for i, rec in enumerate(s["log"][:-1]):
        if rec["accepted"]:
            if predicts_end(rec["cost_change"], cc_prev, ftol, rec["cost"]):
                fired.append(i)
            cc_prev = rec["cost_change"]
    assert fired == [len(s["log"]) - 2], (fired, [(r["cost_change"], r["accepted"]) for r in s["log"]])


@pytest.mark.parametrize("limit", [1, 2, 3])
@pytest.mark.parametrize("teams", TEAMS)
def test_the_iteration_limit_is_a_certain_prediction(solved, teams, limit):
    _check_case(solved, teams, "limit_%d" % limit, limit, _defaults()[1])
    got = solved[teams, "limit_%d" % limit, 1]
    assert got["termination"] == "NO_CONVERGENCE" and int(got["iterations"]) == limit and got["counts"] == (1, 0), (got["termination"], got["iterations"], got["counts"])


@pytest.mark.parametrize("teams", TEAMS)
def test_wrong_predictions_on_the_miss_path_are_made_up_for(solved, teams):
    _check_case(solved, teams, "miss", MISS_OPTIONS["max_iterations"], _defaults()[1])
    got = solved[teams, "miss", 2]
    ro, redone = got["counts"]
    ended = 1 if got["termination"] in ("NO_CONVERGENCE", "FUNCTION", "PARAMETER") else 0
    # every accepted step behind a prediction was swept again, no rejected one was: at least two of each kind
    assert redone >= 2 and ro - redone - ended >= 2, (got["counts"], got["log_accepted"].tolist(), got["termination"])
    assert got["log_accepted"].tolist().count(0) >= 2 and got["log_accepted"].tolist().count(1) >= 2


@pytest.mark.parametrize("name", list(OTHER_ENDINGS))
@pytest.mark.parametrize("teams", TEAMS)
def test_other_endings_behind_wrong_predictions(solved, teams, name):
    o = OTHER_ENDINGS[name]
    _check_case(solved, teams, "other_" + name, o.get("max_iterations", _defaults()[0]), o["function_tolerance"])
    got = solved[teams, "other_" + name, 2]
    assert got["termination"] != "FUNCTION" and got["counts"][1] >= 1, (got["termination"], got["counts"])


@pytest.mark.parametrize("teams", TEAMS)
def test_solves_on_one_handle_with_the_mode_switched_in_between(solved, teams):
    for i in range(3):
        _check_case(solved, teams, "seq%d" % i, SEQ_OPTIONS["max_iterations"], _defaults()[1], seq=i)
    assert int(solved[teams, "seq0", 0]["iterations"]) >= 2 and int(solved[teams, "seq1", 0]["iterations"]) >= 1   # (the continued solve had work left)
    _assert_bit_equal(solved[teams, "seq2", 1], solved[teams, "seq0", 0], (teams, "after the reset: the first solve again"))
