"""The end of a persistent intrinsics solve (DESIGN.md 4.1 "The end of a solve"): the control workgroup hands its control block to the
host as 36 tagged words {tag32 : half} in pinned memory (csrc/cc_persist_publish.hpp; tag = the solve's sequence number), stored by
one wave in one instruction with nothing ordered in front of them or behind them, and writes the device's own copy, the intrinsics
and the last log record AFTER that. What the host takes from the pinned block must therefore be, field by field and bit for bit,
what the device holds once the stream has been synchronised -- for every way a solve ends, on the smallest shapes at which the
tail can go wrong: one frame (one worker, one team), three frames of 70 points (two waves, one partial) with one, two and four
frames per workgroup (three, two and one workers, the last with an idle team), nine frames of ragged lengths.
  (a) pinned block == device control block, for a function-tolerance ending, max_iterations = 1 and 2, a start at a converged
      point, a gradient-tolerance ending and a continued solve; get_state returns the accepted point of that block;
  (b) 300 solves on one handle, reset + solve with max_iterations changing every few solves: every summary equals that of the same
      solve on a fresh handle -- a word left by an earlier solve never satisfies a later wait;
  (c) persistent solve, profiled solve (two-kernel form, plain sequence word), persistent solve, continued persistent solve on ONE
      handle: the count the two protocols share stays consistent, no solve is rerun;
  (d) the persistent solves of (a) against the same solves with CC_INTR_PERSIST=0, under the comparison of
      tests/test_gpu_persist.py (iterations, termination and accept sequence equal; costs to 1e-9, gradient norms to 1e-6, state to 1e-9).
No wait is made to time out here (tests/test_gpu_intrinsics.py keeps the give-up case)."""
import ctypes as C

import numpy as np
import pytest

from camera_calibrator_amd import capi
from tests.helpers import TIGHT, intrinsics_case

pytestmark = pytest.mark.gpu

RAGGED = [70, 4, 33, 64, 65, 20, 70, 63, 12]
HOLD_ALL_BUT_FOCAL = 0x1fc   # one planar view: principal point and distortion held, fx fy free
# name -> (frames, CC_INTR_PERSIST_TEAMS or None, workers, solver form)
SHAPES = {"one_frame": (1, None, 1, 1), "three_frames_teams1": (3, "1", 3, 1), "three_frames_teams2": (3, "2", 2, 2),
          "three_frames_teams4": (3, "4", 1, 4), "nine_ragged_frames": (9, None, 9, 1)}
ENDINGS = ["function_tolerance", "max_iterations_1", "max_iterations_2", "converged_start", "gradient_tolerance", "continued"]
SUMMARY_FIELDS = ("iterations", "successful_steps", "termination", "initial_cost", "final_cost", "sweeps")


def _bits(x):
    return np.float64(x).tobytes()


@pytest.fixture(scope="module")
def cases():
    three, nine = intrinsics_case(3, 70), intrinsics_case(9, RAGGED)
    one = dict(off=three["off"][:2].copy(), uv=three["uv"][:70].copy(), xyz=three["xyz"][:70].copy(), intr0=three["intr0"].copy(),
               q0=three["q0"][:1].copy(), t0=three["t0"][:1].copy())
    return {1: (one, HOLD_ALL_BUT_FOCAL), 3: (three, 0), 9: (nine, 0)}


def _open(cases, shape, monkeypatch, persist=True, start=None):
    frames, teams, _, form = SHAPES[shape]
    c, mask = cases[frames]
    monkeypatch.delenv("CC_INTR_PERSIST_TEAMS", raising=False)
    monkeypatch.delenv("CC_INTR_PERSIST", raising=False)
    if teams:
        monkeypatch.setenv("CC_INTR_PERSIST_TEAMS", teams)
    if not persist:
        monkeypatch.setenv("CC_INTR_PERSIST", "0")
    prob = capi.IntrinsicsProblem(c["off"], c["uv"], c["xyz"])
    intr, q, t = start if start is not None else (c["intr0"], c["q0"], c["t0"])
    prob.set_state(intr, q, t, const_mask=mask)
    assert prob.solver_form() == (form if persist else 0), (shape, prob.solver_form())
    return prob


def _device_ctl(prob):
    """The device's control block after a stream synchronisation: twelve int32 fields, twelve doubles (LmCtl, csrc/cc_common.hpp)."""
    raw = np.zeros(18)
    capi._check(capi.lib().cc_intrinsics_debug_fetch(prob._h, b"ctl", raw.ctypes.data_as(C.POINTER(C.c_double)), C.c_int64(18)))
    i32 = raw.view(np.int32)
    return dict(done=int(i32[0]), termination=capi.TERMINATION.get(int(i32[1]), str(int(i32[1]))), iterations=int(i32[2]), successful_steps=int(i32[3]),
                log_len=int(i32[10]), sweeps=int(i32[11]), final_cost=raw[6 + 2], initial_cost=raw[6 + 5])


def _solve_checked(prob, opts):
    """One solve; the summary the host took from the pinned block against the device's control block."""
    s = prob.solve(opts, log_capacity=128)
    d = _device_ctl(prob)
    assert d["done"] == 1
    for k in ("iterations", "successful_steps", "termination", "sweeps"):
        assert s[k] == d[k], (k, s[k], d[k])
    assert len(s["log"]) == d["log_len"], (len(s["log"]), d["log_len"])
    for k in ("initial_cost", "final_cost"):
        assert _bits(s[k]) == _bits(d[k]), (k, s[k], d[k])
    return s


def _run_ending(cases, shape, ending, monkeypatch, converged, persist=True):
    """The solves of one ending on a fresh handle -> ([summary, ...], (intr, q, t))."""
    start = converged[SHAPES[shape][0]] if ending == "converged_start" else None
    prob = _open(cases, shape, monkeypatch, persist=persist, start=start)
    try:
        solve = (lambda o: _solve_checked(prob, o)) if persist else (lambda o: prob.solve(o, log_capacity=128))
        if ending in ("function_tolerance", "converged_start"):
            out = [solve(capi.default_options())]
        elif ending == "max_iterations_1":
            out = [solve(capi.default_options(max_iterations=1))]
        elif ending == "max_iterations_2":
            out = [solve(capi.default_options(max_iterations=2))]
        elif ending == "gradient_tolerance":
            out = [solve(capi.default_options(function_tolerance=0.0, parameter_tolerance=0.0, gradient_tolerance=1e-2, max_iterations=50))]
        else:
            out = [solve(capi.default_options(max_iterations=2)), solve(capi.default_options())]
        state = prob.get_state()
        cost_there, _ = prob.eval(want_blocks=False)
        return out, state, cost_there
    finally:
        prob.close()


@pytest.fixture(scope="module")
def converged(cases):
    """A converged point per frame count (tight tolerances, two-kernel form: not the code under test), and the gradient norm at the start."""
    mp = pytest.MonkeyPatch()
    out = {}
    try:
        for shape in ("one_frame", "three_frames_teams1", "nine_ragged_frames"):
            prob = _open(cases, shape, mp, persist=False)
            s = prob.solve(capi.default_options(**TIGHT), log_capacity=128)
            out[SHAPES[shape][0]] = prob.get_state()
            out["gradient_at_start", SHAPES[shape][0]] = s["log"][0]["gradient_max_norm"]
            prob.close()
    finally:
        mp.undo()
    return out


def _assert_same_solution(a, b, gradient_floor=0.0):
    """The comparison of tests/test_gpu_persist.py between two forms of one solve. gradient_floor: see the caller."""
    (sa, (ia, qa, ta), _), (sb, (ib, qb, tb), _) = a, b
    assert len(sa) == len(sb)
    for x, y in zip(sa, sb):
        assert x["iterations"] == y["iterations"] and x["termination"] == y["termination"], (x["iterations"], y["iterations"], x["termination"], y["termination"])
        assert [l["accepted"] for l in x["log"]] == [l["accepted"] for l in y["log"]]
        assert np.allclose([l["cost"] for l in x["log"]], [l["cost"] for l in y["log"]], rtol=1e-9)
        assert np.allclose([l["gradient_max_norm"] for l in x["log"]], [l["gradient_max_norm"] for l in y["log"]], rtol=1e-6, atol=gradient_floor)
    assert np.allclose(ia[:4], ib[:4], rtol=1e-9) and np.allclose(ia[4:], ib[4:], atol=1e-9)
    assert np.abs(qa - qb).max() < 1e-9 and np.abs(ta - tb).max() < 1e-9


@pytest.mark.parametrize("ending", ENDINGS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_pinned_block_is_the_devices_control_block_for_every_ending(cases, converged, monkeypatch, shape, ending):
    got = _run_ending(cases, shape, ending, monkeypatch, converged)               # (a): asserted solve by solve in _solve_checked
    summaries, _, cost_there = got
    last = summaries[-1]
    print(shape, ending, [(s["termination"], s["iterations"], s["sweeps"], len(s["log"])) for s in summaries])
    if ending == "function_tolerance":
        assert last["termination"] == "FUNCTION" and last["iterations"] >= 2
    elif ending in ("max_iterations_1", "max_iterations_2"):
        assert last["termination"] == "NO_CONVERGENCE" and last["iterations"] == int(ending[-1])
    elif ending == "converged_start":
        assert last["iterations"] <= 1
    elif ending == "gradient_tolerance":
        assert last["termination"] == "GRADIENT"
    else:
        assert summaries[0]["termination"] == "NO_CONVERGENCE" and summaries[0]["iterations"] == 2 and last["iterations"] >= 1
    # get_state returns the accepted point of that block: the cost there is the block's final cost (the same residuals summed in
    # another order: at most 560 terms, 560 x 2^-53 = 6e-14 relative) ...
    assert abs(cost_there - last["final_cost"]) <= 1e-11 * abs(last["final_cost"]), (cost_there, last["final_cost"])
    # (d) ... and the point the two-kernel form reaches in the same solves. tests/test_gpu_persist.py compares gradient norms to 1e-6
    # relative on solves that stop at the function tolerance, far above the floor. The two endings that run INTO the floor -- a gradient
    # that is what cancellation leaves of terms of the starting gradient's size, at states the comparison itself only holds to 1e-9 --
    # get that floor as an absolute term: 1e-9 x the gradient norm at the start. Everything else is compared as there.
    floor = 1e-9 * converged["gradient_at_start", SHAPES[shape][0]] if ending in ("gradient_tolerance", "converged_start") else 0.0
    _assert_same_solution(got, _run_ending(cases, shape, ending, monkeypatch, converged, persist=False), gradient_floor=floor)


def _strip(s):
    raw = lambda v: _bits(v) if isinstance(v, float) else v   # (bits, not values: a NaN equals itself)
    return tuple(raw(s[k]) for k in SUMMARY_FIELDS) + (tuple(tuple((k, raw(v)) for k, v in sorted(l.items())) for l in s["log"]),)


@pytest.mark.parametrize("shape", ["three_frames_teams2", "nine_ragged_frames"])
def test_three_hundred_solves_on_one_handle_each_equal_to_a_fresh_handles(cases, monkeypatch, shape):
    limits = [1, 50, 2, 3, 50, 1, 4]
    fresh = {}
    for m in sorted(set(limits)):
        p = _open(cases, shape, monkeypatch)
        fresh[m] = _strip(p.solve(capi.default_options(max_iterations=m), log_capacity=128))
        p.close()
    assert len({v[:2] for v in fresh.values()}) >= 3          # (the limits really end the solves differently)
    prob = _open(cases, shape, monkeypatch)
    try:
        for i in range(300):
            m = limits[(i // 3) % len(limits)]
            prob.reset()
            got = _strip(prob.solve(capi.default_options(max_iterations=m), log_capacity=128))
            assert got == fresh[m], (i, m, got[:6], fresh[m][:6])
        assert prob.solver_status()[1] == 0
    finally:
        prob.close()


@pytest.mark.parametrize("shape", ["one_frame", "three_frames_teams4", "nine_ragged_frames"])
def test_persistent_and_two_kernel_solves_share_one_handle_and_one_count(cases, monkeypatch, shape):
    ref = _open(cases, shape, monkeypatch)
    want_full = _strip(ref.solve(capi.default_options(), log_capacity=128))
    ref.reset()
    want_two = _strip(ref.solve(capi.default_options(max_iterations=2), log_capacity=128))
    want_cont = _strip(ref.solve(capi.default_options(), log_capacity=128))
    ref.close()
    prob = _open(cases, shape, monkeypatch)
    try:
        assert _strip(_solve_checked(prob, capi.default_options())) == want_full
        prob.reset()
        prof = prob.solve(capi.default_options(profile_kernels=1), log_capacity=128)          # two-kernel form: chunks published through the plain word
        assert prob.solver_status()[1] == 0
        assert prof["kernel_launches"]["sweep"] >= 1
        assert (prof["iterations"], prof["termination"]) == (want_full[0], want_full[2])
        assert [l["accepted"] for l in prof["log"]] == [dict(l)["accepted"] for l in want_full[6]]
        assert np.allclose([l["cost"] for l in prof["log"]], [np.frombuffer(dict(l)["cost"])[0] for l in want_full[6]], rtol=1e-9)
        prob.reset()
        assert _strip(_solve_checked(prob, capi.default_options(max_iterations=2))) == want_two
        assert _strip(_solve_checked(prob, capi.default_options())) == want_cont
        form, reruns, note = prob.solver_status()
        assert reruns == 0 and note == "", (form, reruns, note)
    finally:
        prob.close()
