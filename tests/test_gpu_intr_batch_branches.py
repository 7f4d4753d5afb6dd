"""The batched intrinsics solve (cc_intrinsics_batch.hip) off its easy trajectory, against the fp64 CPU oracle run per problem
with the same options and against itself: rejected and invalid steps, every termination reason and several of them in one
launch sequence, more than 64 frames, frames of more than 512 observations, empty frames and empty problems, held sets other
than k3, a non-finite observation, check_interval, a handle solved again from mixed buffers, more problems than compute units.

Tolerances are those of the single-problem test of the same scenario, none is new:
  standing (default options; tests/test_gpu_intr_batch.py::_assert_parity): costs 1e-9 relative, _assert_intrinsics_close,
            poses 1e-9;
  long     (the reject-heavy 40-iteration runs of test_gpu_lm_branches.py::test_rejected_steps_and_radius_shrinking): costs
            1e-8 relative, intrinsics rtol 1e-8 / atol 1e-10, poses 1e-9 as above;
  branch   (the other forced branches of test_gpu_lm_branches.py, _same_trajectory): costs 1e-9, intrinsics 1e-8 / 1e-10,
            poses 1e-9;
  single frame (test_gpu_edge_inputs.py::test_single_frame_problem): costs 1e-7, the state is not compared (one planar view
            does not pin it).
On top of _assert_parity every comparison includes the `valid` sequence and the logged radius at 1e-6 relative, as
_same_trajectory does. Independence ("same bits") is _assert_same_bits against the problem solved as a batch of one.

Every scenario states what the ORACLE does with it as a precondition (`_scenario_*`, no GPU involved:
tests/test_intr_batch_branches_cpu.py runs them on a machine without one), so that a change of the generator cannot quietly
empty a test."""
import numpy as np
import pytest

from camera_calibrator_amd import capi
from oracle import pyoracle as po
from tests.helpers import intrinsics_case
from tests.test_gpu_edge_inputs import _with_empty_frames
from tests.test_gpu_intr_batch import _assert_same_bits, _batch as _original_batch, _oracle, _results as _original_results, _run
from tests.test_gpu_intrinsics import _assert_intrinsics_close
from tests.test_gpu_lm_branches import _bad_start

pytestmark = pytest.mark.gpu

_cache = {}


def _memo(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _started(case, seed, scale=0.3):
    intr, q, t = _bad_start(case, seed, scale)
    return dict(case, intr0=intr, q0=q, t0=t)


def _oracles(probs, **kw):
    return [_oracle(c, m, **kw) for c, m in probs]


def _terms(oracle):
    return [o[3]["termination"] for o in oracle]


def _iters(oracle):
    return [o[3]["iterations"] for o in oracle]


def _accepted(o):
    return [l["accepted"] for l in o[3]["log"]]


def _state_norm(intr, q, t):
    """|x| as the trust-region loop has it: all nine intrinsics and every pose, held or not."""
    return float(np.sqrt((intr ** 2).sum() + (q ** 2).sum() + (t ** 2).sum()))


# ---- comparison --------------------------------------------------------------------------------------------------------------
def _assert_branch_parity(got, want, label, cost_rtol=1e-9, intr="standing", state=True):
    """_assert_parity of tests/test_gpu_intr_batch.py plus the `valid` sequence and the logged radius (1e-6 relative, as
    _same_trajectory). intr: "standing" (_assert_intrinsics_close) or "branch" (rtol 1e-8, atol 1e-10, _same_trajectory);
    state=False: trajectory only (the single-frame problem)."""
    (ig, qg, tg, sg), (io, qo, to, so) = got, want
    col = lambda s, k: np.array([l[k] for l in s["log"]], dtype=np.float64)
    cg, co, rg, ro = col(sg, "cost"), col(so, "cost"), col(sg, "radius"), col(so, "radius")
    same_len = len(cg) == len(co)
    rel = lambda a, b: float(np.max(np.abs(a - b) / np.where(b != 0, np.abs(b), 1.0))) if same_len and len(b) else None
    print(label, "iterations", sg["iterations"], so["iterations"], "termination", sg["termination"], so["termination"],
          "steps", sg["successful_steps"], so["successful_steps"], "max rel cost diff", rel(cg, co), "max rel radius diff", rel(rg, ro),
          "intr diff", np.abs(ig - io), "pose diff", float(np.abs(qg - qo).max()), float(np.abs(tg - to).max()))
    assert sg["termination"] == so["termination"] and sg["iterations"] == so["iterations"]
    assert sg["successful_steps"] == so["successful_steps"]
    assert [l["accepted"] for l in sg["log"]] == [l["accepted"] for l in so["log"]]
    assert [l["valid"] for l in sg["log"]] == [l["valid"] for l in so["log"]]
    assert np.allclose(cg, co, rtol=cost_rtol, atol=0)
    assert np.allclose(rg, ro, rtol=1e-6, atol=0)
    if not state:
        return
    if intr == "standing":
        _assert_intrinsics_close(ig, io)
    else:
        assert np.allclose(ig, io, rtol=1e-8, atol=1e-10)
    assert np.abs(qg - qo).max() < 1e-9 and np.abs(tg - to).max() < 1e-9


def _assert_alone(probs, got, **kw):
    for p in range(len(probs)):
        _assert_same_bits(got[p], _run([probs[p]], **kw)[0])


# ---- A: reject branches in a mixed batch -----------------------------------------------------------------------------------------
REJECT_SETS = [
    dict(min_relative_decrease=0.99, initial_radius=1e8),
    dict(min_relative_decrease=0.999, max_consecutive_invalid_steps=3),
    dict(min_relative_decrease=0.99, use_nonmonotonic_steps=0),
]


def _problems_a():
    def make():
        a = intrinsics_case(12, 60)
        return [(_started(a, 0), 0), (_started(a, 1), 0), (intrinsics_case(8, 50), 0),
                (intrinsics_case(7, [8, 64, 65, 300, 5, 257, 128]), 0), (intrinsics_case(5, 100), 0)]
    return _memo("problems a", make)


def _scenario_a(i):
    """(problems, oracle results) under REJECT_SETS[i] with 40 iterations; the two bad starts mix at least 10 rejected with at
    least 5 accepted steps and the problems leave the batch in different rounds."""
    def make():
        probs = _problems_a()
        oracle = _oracles(probs, max_iterations=40, **REJECT_SETS[i])
        for o in oracle[:2]:
            assert _accepted(o).count(0) >= 10 and _accepted(o).count(1) >= 5, _accepted(o)
        assert len(set(_iters(oracle))) > 1, _iters(oracle)
        if i == 0:
            assert _terms(oracle) == ["NO_CONVERGENCE", "NO_CONVERGENCE", "FUNCTION", "FUNCTION", "FUNCTION"]
            assert _iters(oracle) == [40, 40, 10, 3, 3]
            assert [_accepted(o).count(1) for o in oracle[:3]] == [16, 16, 4]
        return probs, oracle
    return _memo(("a", i), make)


def _got_a(i):
    return _memo(("got a", i), lambda: _run(_problems_a(), max_iterations=40, **REJECT_SETS[i]))


@pytest.mark.parametrize("i", range(len(REJECT_SETS)))
def test_rejected_steps_in_a_mixed_batch(i):
    probs, oracle = _scenario_a(i)
    got = _got_a(i)
    for p in range(len(probs)):
        _assert_branch_parity(got[p], oracle[p], "reject set %d, problem %d" % (i, p), cost_rtol=1e-8, intr="branch")


@pytest.mark.parametrize("i", range(len(REJECT_SETS)))
def test_rejected_steps_do_not_depend_on_the_batch(i):
    probs, _ = _scenario_a(i)
    got = _got_a(i)
    _assert_alone(probs, got, max_iterations=40, **REJECT_SETS[i])
    rev = _run(probs[::-1], max_iterations=40, **REJECT_SETS[i])[::-1]
    for p in range(len(probs)):
        _assert_same_bits(got[p], rev[p])


# ---- B: every termination reason -----------------------------------------------------------------------------------------------
TERMINATION_SETS = [
    (dict(gradient_tolerance=1e12), "GRADIENT", 0),
    (dict(parameter_tolerance=1e-1), "PARAMETER", 1),
    (dict(function_tolerance=0.999), "FUNCTION", 1),
    (dict(max_iterations=1), "NO_CONVERGENCE", 1),
    (dict(initial_radius=1e-40, min_radius=1e-32), "MIN_RADIUS", 0),
]


def _scenario_b(i):
    def make():
        kw, term, iters = TERMINATION_SETS[i]
        oracle = _oracles(_problems_a(), **kw)
        assert _terms(oracle) == [term] * 5 and _iters(oracle) == [iters] * 5, (_terms(oracle), _iters(oracle))
        return _problems_a(), oracle
    return _memo(("b", i), make)


@pytest.mark.parametrize("i", range(len(TERMINATION_SETS)))
def test_every_termination_reason_in_a_batch(i):
    probs, oracle = _scenario_b(i)
    got = _run(probs, **TERMINATION_SETS[i][0])
    for p in range(len(probs)):
        _assert_branch_parity(got[p], oracle[p], "%s, problem %d" % (TERMINATION_SETS[i][1], p), intr="branch")
    _assert_alone(probs, got, **TERMINATION_SETS[i][0])


GRADIENT_LATER = dict(gradient_tolerance=5.0, function_tolerance=-1.0, parameter_tolerance=-1.0, max_iterations=50)
NO_JACOBI = dict(jacobi_scaling=0, max_iterations=30)


def _scenario_b_gradient():
    def make():
        oracle = _oracles(_problems_a(), **GRADIENT_LATER)
        assert _terms(oracle) == ["GRADIENT"] * 5 and _iters(oracle) == [5, 5, 3, 3, 3], (_terms(oracle), _iters(oracle))
        return _problems_a(), oracle
    return _memo("b gradient", make)


def _scenario_b_no_jacobi():
    def make():
        oracle = _oracles(_problems_a(), **NO_JACOBI)
        assert min(_iters(oracle)) >= 2, _iters(oracle)
        return _problems_a(), oracle
    return _memo("b no jacobi", make)


def test_gradient_tolerance_met_in_different_rounds():
    probs, oracle = _scenario_b_gradient()
    got = _run(probs, **GRADIENT_LATER)
    for p in range(len(probs)):
        _assert_branch_parity(got[p], oracle[p], "gradient later, problem %d" % p, intr="branch")
    _assert_alone(probs, got, **GRADIENT_LATER)


def test_batch_without_jacobi_scaling():
    probs, oracle = _scenario_b_no_jacobi()
    got = _run(probs, **NO_JACOBI)
    for p in range(len(probs)):
        _assert_branch_parity(got[p], oracle[p], "no jacobi scaling, problem %d" % p, intr="branch")
    _assert_alone(probs, got, **NO_JACOBI)


MIXED_REASONS = dict(gradient_tolerance=0.5, function_tolerance=1e-5, parameter_tolerance=3e-6, max_iterations=5)
MIXED_MARGIN = 0.01


def _problems_b_mixed():
    return _problems_a() + [(_started(intrinsics_case(8, 50), 0), 0)]


def _decision_margins(case, mask, o, kw):
    """For the oracle's run `o` of one problem under `kw`: every convergence test it made, with the relative distance of the
    deciding quantity from its threshold. [(test, iteration, value, threshold, margin)]; the log has one record per
    iteration, from iteration 1 on."""
    start = lambda n, **more: _oracle(case, mask, **dict(kw, max_iterations=n, **more))
    out = []
    add = lambda name, it, value, thr: out.append((name, it, value, thr, abs(value - thr) / thr))
    # the gradient of the initial point: a first iteration that stops on the function tolerance logs it unchanged
    add("gradient", 0, start(1, function_tolerance=1e300)[3]["log"][0]["gradient_max_norm"], kw["gradient_tolerance"])
    for it in range(1, o[3]["iterations"] + 1):
        rec = o[3]["log"][it - 1]
        if not rec["valid"]:
            continue
        before = start(it - 1)                                          # the accepted point this iteration started from
        x_norm, x_cost = _state_norm(*before[:3]), before[3]["final_cost"]
        thr = kw["parameter_tolerance"] * (x_norm + kw["parameter_tolerance"])
        add("parameter", it, rec["step_norm"], thr)
        if rec["step_norm"] <= thr:
            continue                                                     # fired: the function test was not made
        add("function", it, abs(rec["cost_change"]), kw["function_tolerance"] * x_cost)
        if rec["accepted"] and it < kw["max_iterations"]:
            add("gradient", it, rec["gradient_max_norm"], kw["gradient_tolerance"])
    return out


def _scenario_b_mixed():
    def make():
        probs = _problems_b_mixed()
        oracle = _oracles(probs, **MIXED_REASONS)
        assert len(set(_terms(oracle))) >= 3, _terms(oracle)
        margins = [_decision_margins(c, m, o, MIXED_REASONS) for (c, m), o in zip(probs, oracle)]
        for p, ms in enumerate(margins):
            for name, it, value, thr, margin in ms:
                assert margin >= MIXED_MARGIN, (p, name, it, value, thr, margin)
        return probs, oracle, margins
    return _memo("b mixed", make)


def test_different_termination_reasons_side_by_side():
    """gradient_tolerance 0.5, function_tolerance 1e-5, parameter_tolerance 3e-6, max_iterations 5 over the problems of A plus
    8 x 50 from a bad start: the oracle ends them PARAMETER (iteration 5), NO_CONVERGENCE (5), GRADIENT (3), PARAMETER (4),
    PARAMETER (4) and GRADIENT (4) -- four reasons in one launch sequence, in three different rounds.

    Margins |value - threshold| / threshold of EVERY convergence test the oracle makes on the way (all iterations, not only
    the deciding one and its predecessor; _decision_margins, asserted >= 1 % in _scenario_b_mixed), smallest per problem:
      0  parameter test fires at 5: step_norm 2.31e-3 against 5.10e-3 (0.55); at 4: 0.204 against 5.10e-3 (39)
      1  nothing fires: at 5 step_norm 1.02e-2 against 5.10e-3 (1.0), |cost_change| 8.12e-4 against 5.81e-4 (0.40)
      2  gradient test fires at 3: 0.299 against 0.5 (0.40); at 2: 885 against 0.5
      3  parameter test fires at 4: 1.66e-3 against 5.10e-3 (0.67); gradient at 3: 0.871 against 0.5 (0.74)
      4  parameter test fires at 4: 3.71e-3 against 5.10e-3 (0.27); gradient at 3: 1.16 against 0.5 (1.3)
      5  gradient test fires at 4: 0.103 against 0.5 (0.79); function at 4: 1.65e-3 against 3.01e-4 (4.5)
    The smallest of all is 0.27, against costs that agree to 1e-9: no decision is a close call."""
    probs, oracle, _ = _scenario_b_mixed()
    got = _run(probs, **MIXED_REASONS)
    for p in range(len(probs)):
        _assert_branch_parity(got[p], oracle[p], "mixed reasons, problem %d" % p, intr="branch")
    _assert_alone(probs, got, **MIXED_REASONS)


# ---- C: shapes the batch has never seen --------------------------------------------------------------------------------------
EMPTY_AT = (0, 3, 7)
EMPTY_AT_END = (0, 3, 8)
SINGLE_FRAME_MASK = 0b111110000
COPY_MASKS = [0b11, 0b1100, 0b111111111, 0b011000000]


def _single_frame_case():
    full = intrinsics_case(5, 120)          # K and the pose come from a five-view estimate
    n = int(full["off"][1])
    return dict(off=full["off"][:2].copy(), uv=full["uv"][:n], xyz=full["xyz"][:n], intr0=full["intr0"], q0=full["q0"][:1], t0=full["t0"][:1])


def _scenario_c(layout):
    """70 frames (more than one frame per statistics chunk, five elimination passes with a ragged last one), frames of 1000 /
    513 / 512 / 769 observations (up to four passes of the sweep's prefetch loop, waves with different pass counts), a single
    frame with the distortion held, four copies of 5 x 100 holding fx fy / px py / everything / k2 k3, and two problems with
    empty frames: at 0, 3 and 7 of nine (the last frame has observations) and at 0, 3 and 8 (the last frame is empty: last in
    the batch it starts at the arena's end). The two go last or first."""
    def make():
        empties = [(_with_empty_frames(intrinsics_case(6, 40), list(e)), 0) for e in (EMPTY_AT, EMPTY_AT_END)]
        a = intrinsics_case(5, 100)
        probs = [(intrinsics_case(70, 12), 0), (intrinsics_case(4, [1000, 513, 512, 769]), 0), (_single_frame_case(), SINGLE_FRAME_MASK)]
        probs += [(a, m) for m in COPY_MASKS]
        names = ["70", "long", "single"] + ["mask%d" % k for k in range(4)]
        if layout == "empty_last":
            probs, names = probs + empties, names + ["empty", "empty_end"]
        else:
            probs, names = empties + probs, ["empty", "empty_end"] + names
        by = {name: p for p, name in enumerate(names)}
        for name, at in (("empty", EMPTY_AT), ("empty_end", EMPTY_AT_END)):
            off = probs[by[name]][0]["off"]
            assert len(off) == 10 and [f for f in range(9) if off[f] == off[f + 1]] == list(at), off
        assert probs[by["empty_end"]][0]["off"][-2] == len(probs[by["empty_end"]][0]["uv"])
        oracle = _oracles(probs)
        t, n = _terms(oracle), _iters(oracle)
        for name in ("70", "long", "empty", "empty_end"):
            assert (t[by[name]], n[by[name]]) == ("FUNCTION", 4), (name, t, n)
        assert (t[by["single"]], n[by["single"]]) == ("FUNCTION", 3), (t, n)
        masked = [(t[by["mask%d" % k]], n[by["mask%d" % k]]) for k in range(4)]
        assert masked == [("FUNCTION", 4), ("FUNCTION", 4), ("PARAMETER", 3), ("FUNCTION", 4)], masked
        return probs, oracle, by
    return _memo(("c", layout), make)


@pytest.mark.parametrize("layout", ["empty_last", "empty_first"])
def test_shapes_the_batch_has_not_seen(layout):
    probs, oracle, by = _scenario_c(layout)
    got = _run(probs)
    for p in range(len(probs)):
        if p == by["single"]:
            _assert_branch_parity(got[p], oracle[p], "%s, single frame" % layout, cost_rtol=1e-7, state=False)
        else:
            _assert_branch_parity(got[p], oracle[p], "%s, problem %d" % (layout, p))
    for p, (case, mask) in enumerate(probs):                             # held coordinates: the bits that went in
        held = [j for j in range(9) if (mask >> j) & 1]
        assert np.array_equal(got[p][0][held], case["intr0"][held]), (p, mask)
    for name, at in (("empty", EMPTY_AT), ("empty_end", EMPTY_AT_END)):   # empty frames: the poses that went in
        e = by[name]
        for f in at:
            assert np.array_equal(got[e][1][f], probs[e][0]["q0"][f]) and np.array_equal(got[e][2][f], probs[e][0]["t0"][f])
    _assert_alone(probs, got)


# ---- D: a problem without observations ---------------------------------------------------------------------------------------
def _empty_problem():
    return dict(off=np.zeros(4, dtype=np.int64), uv=np.zeros((0, 2), np.float32), xyz=np.zeros((0, 3), np.float32),
                intr0=np.array([1000.0, 1000, 500, 500, 0, 0, 0, 0, 0]), q0=np.tile([1.0, 0, 0, 0], (3, 1)), t0=np.tile([0.0, 0, 1], (3, 1)))


def _scenario_d():
    def make():
        probs = [(intrinsics_case(5, 100), 0), (_empty_problem(), 0), (intrinsics_case(8, 50), 0), (_empty_problem(), 0)]
        oracle = _oracles(probs)
        for p in (1, 3):
            assert oracle[p][3]["iterations"] == 0 and oracle[p][3]["final_cost"] == 0.0
        assert min(_iters([oracle[0], oracle[2]])) >= 3
        return probs, oracle
    return _memo("d", make)


def _assert_untouched_empty(got, want, case):
    assert got[3]["termination"] == want[3]["termination"] and got[3]["iterations"] == want[3]["iterations"] == 0
    assert got[3]["final_cost"] == 0.0 and got[3]["initial_cost"] == 0.0 and got[3]["successful_steps"] == 0
    assert np.array_equal(got[0], case["intr0"]) and np.array_equal(got[1], case["q0"]) and np.array_equal(got[2], case["t0"])


def test_problem_without_observations_next_to_normal_ones():
    probs, oracle = _scenario_d()
    got = _run(probs)
    for p in (1, 3):                                                      # (the second one's frames all start at the arena's end)
        _assert_untouched_empty(got[p], oracle[p], probs[p][0])
    for p in (0, 2):
        _assert_branch_parity(got[p], oracle[p], "next to an empty problem, problem %d" % p)
        _assert_same_bits(got[p], _run([probs[p]])[0])


def test_batch_without_any_observation():
    probs, oracle = _scenario_d()
    got = _run([probs[1], probs[3]])
    for k, p in enumerate((1, 3)):
        _assert_untouched_empty(got[k], oracle[p], probs[p][0])


# ---- E: invalid steps ----------------------------------------------------------------------------------------------------------
def _scenario_e():
    def make():
        case = intrinsics_case(6, 40)
        uv = case["uv"].copy()
        uv[17, 0] = np.nan
        probs = [(intrinsics_case(5, 100), 0), (dict(case, uv=uv), 0), (intrinsics_case(8, 50), 0)]
        oracle = _oracles(probs, max_iterations=20)
        s = oracle[1][3]
        assert (s["termination"], s["iterations"]) == ("FAILURE_INVALID_STEPS", 5) and [l["valid"] for l in s["log"]] == [0] * 5
        return probs, oracle
    return _memo("e", make)


def test_non_finite_observation_fails_one_problem_only():
    probs, oracle = _scenario_e()
    got = _run(probs, max_iterations=20)
    (ig, _, _, sg), (io, _, _, so) = got[1], oracle[1]
    print("termination", sg["termination"], "iterations", sg["iterations"], "intrinsics", ig, io)
    assert sg["termination"] == so["termination"] and sg["iterations"] == so["iterations"]
    assert sg["successful_steps"] == so["successful_steps"] == 0
    for k in ("valid", "accepted"):
        assert [l[k] for l in sg["log"]] == [l[k] for l in so["log"]], k
    assert np.array_equal(np.isnan(ig), np.isnan(io))
    for p in (0, 2):
        _assert_branch_parity(got[p], oracle[p], "next to a NaN, problem %d" % p)
        _assert_same_bits(got[p], _run([probs[p]], max_iterations=20)[0])


# A diagonal clamp of 1e300 makes every step far smaller than the point's rounding: the candidates are evaluated (valid
# steps, cost change exactly 0, rejected), the radius shrinks by 2, 4, 8, ... until 1e300 / radius overflows; from there the
# damped blocks are not finite, the linear solve fails and five invalid steps end the solve. The invalid steps come BEHIND
# evaluated candidates, so the statistics rows a sweep left are stale when the step kernel takes its invalid branch.
OVERFLOWING_DAMPING = dict(min_lm_diagonal=1e300, max_lm_diagonal=1e300, initial_radius=1.0, function_tolerance=-1.0,
                           parameter_tolerance=-1.0, max_iterations=30)


def _scenario_e_late():
    def make():
        probs = [(intrinsics_case(5, 100), 0), (intrinsics_case(6, 40), 0), (_started(intrinsics_case(8, 50), 0), 0)]
        oracle = _oracles(probs, **OVERFLOWING_DAMPING)
        for o in oracle:
            valid = [l["valid"] for l in o[3]["log"]]
            assert o[3]["termination"] == "FAILURE_INVALID_STEPS" and valid[-5:] == [0] * 5 and valid[:-5] == [1] * (len(valid) - 5), valid
            assert len(valid) >= 8 and o[3]["successful_steps"] == 0
            assert all(l["model_cost_change"] > 0 for l in o[3]["log"][:-5]) and all(l["model_cost_change"] == 0 for l in o[3]["log"][-5:])
            # the overflow is not a close call: the last finite damping and the first infinite one are a factor >= 16 apart
            r = [l["radius"] for l in o[3]["log"]]
            assert 1e300 / r[-7] < 1e308 / 4 and 1e300 / r[-6] == np.inf, r
        return probs, oracle
    return _memo("e late", make)


def test_invalid_steps_behind_evaluated_candidates():
    probs, oracle = _scenario_e_late()
    got = _run(probs, **OVERFLOWING_DAMPING)
    for p in range(len(probs)):
        _assert_branch_parity(got[p], oracle[p], "overflowing damping, problem %d" % p, intr="branch")
        # an invalid step's record carries no model decrease, whatever the last sweep left in the statistics rows
        for lg, lo in zip(got[p][3]["log"], oracle[p][3]["log"]):
            if not lo["valid"]:
                assert lg["model_cost_change"] == lo["model_cost_change"] == 0.0 and lg["cost_change"] == 0.0 and lg["step_norm"] == 0.0
        assert np.array_equal(got[p][0], probs[p][0]["intr0"])            # nothing was ever accepted
    _assert_alone(probs, got, **OVERFLOWING_DAMPING)


# ---- F: check_interval -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("check_interval", [1, 3, 7])
def test_check_interval_does_not_change_a_bit(check_interval):
    probs, _ = _scenario_a(0)
    want = _got_a(0)
    got = _run(probs, max_iterations=40, check_interval=check_interval, **REJECT_SETS[0])   # (raises if the loop does not end)
    for p in range(len(probs)):
        _assert_same_bits(got[p], want[p])


# ---- G: a handle solved again from mixed buffers -------------------------------------------------------------------------------
def _solve_on(b, n, **kw):
    ss = b.solve(capi.default_options(**kw))
    intr, qs, ts = b.get_state()
    return [(intr[p], qs[p], ts[p], ss[p]) for p in range(n)]


def _set(b, probs, states=None):
    states = states if states is not None else [(c["intr0"], c["q0"], c["t0"]) for c, _ in probs]
    b.set_state([s[0] for s in states], [s[1] for s in states], [s[2] for s in states], const_mask=[m for _, m in probs])


def test_second_solve_on_a_handle_whose_problems_ended_in_different_buffers():
    probs, _ = _original_batch()
    n = len(probs)
    layout = [(c["off"], c["uv"], c["xyz"]) for c, _ in probs]
    used = capi.IntrinsicsBatch(layout)
    _set(used, probs)
    one = _solve_on(used, n, max_iterations=1)
    steps = [r[3]["successful_steps"] for r in one]
    assert set(steps) == {0, 1}, steps                                    # accepted points in buffer 1 and in buffer 0
    assert steps[4] == 0 and one[4][3]["termination"] != "NO_CONVERGENCE"
    oracle = [po.intrinsics_solve(c["off"], c["uv"], c["xyz"], one[p][0], one[p][1], one[p][2], const_mask=m) for p, (c, m) in enumerate(probs)]
    assert max(_iters(oracle)) >= 2
    again = _solve_on(used, n)                                            # the begin kernel moves the buffer 1 problems only
    fresh = capi.IntrinsicsBatch(layout)
    _set(fresh, probs, [r[:3] for r in one])
    want = _solve_on(fresh, n)
    fresh.close()
    for p in range(n):
        _assert_same_bits(again[p], want[p])
        _assert_branch_parity(again[p], oracle[p], "second solve, problem %d" % p)
    _set(used, probs)                                                     # set_state on a used handle: a first solve again
    first = _solve_on(used, n)
    used.close()
    for p in range(n):
        _assert_same_bits(first[p], _original_results()[p])


# ---- H: more problems than compute units -----------------------------------------------------------------------------------------
MANY = 260


def _scenario_h():
    def make():
        distinct = [(intrinsics_case(3, 12), 0), (intrinsics_case(4, 9), 0), (intrinsics_case(3, [4, 20, 7]), 0), (intrinsics_case(5, 6), 0)]
        oracle = _oracles(distinct)
        assert min(_iters(oracle)) >= 2 and all(np.isfinite(o[3]["final_cost"]) for o in oracle), _iters(oracle)
        return distinct, oracle
    return _memo("h", make)


def test_more_problems_than_compute_units():
    distinct, oracle = _scenario_h()
    got = _run([distinct[p % 4] for p in range(MANY)])
    alone = [_run([d])[0] for d in distinct]
    for p in range(MANY):
        _assert_same_bits(got[p], alone[p % 4])
    for k in range(4):
        _assert_branch_parity(alone[k], oracle[k], "tiny problem %d" % k)
