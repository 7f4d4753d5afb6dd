"""CPU: pins the numpy restatement of one inner pass (tests/rig_inner_ref.py) before the HIP pass is measured against it."""
import numpy as np
import pytest

from oracle import pyoracle as po
from tests import rig_inner_ref as ri
from tests.helpers import rig_outlier_case

HUBER_A = float(np.float32(3.0) / np.float32(500.0))


def _data(sc, huber_a=HUBER_A):
    return ri.RigData(len(sc["cam_T"]), sc["frame_offsets"], sc["obs_cam"], sc["obs_world"], sc["obs_uv"], sc["world_xyz"],
                      sc["cam_frozen"], huber_a)


def test_jacobian_columns_match_finite_differences_of_the_oracle_residual():
    sc = rig_outlier_case(3, 4, 6)
    d = _data(sc, huber_a=1e6)
    state = [sc["cam_q0"], sc["cam_t0"], sc["frame_q0"], sc["frame_t0"]]
    for kind, i in (("t_cr", 1), ("q_cr", 2), ("t_rw", 3), ("q_rw", 0)):
        x = {"q_cr": state[0], "t_cr": state[1], "q_rw": state[2], "t_rw": state[3]}[kind][i]
        c0, g, _ = ri.block_eval(d, state, kind, i, x)
        h = 1e-7
        for k in range(3):
            e = np.zeros(3)
            e[k] = h
            xp = ri.quat_plus(x, e) if kind.startswith("q") else x + e
            xm = ri.quat_plus(x, -e) if kind.startswith("q") else x - e
            fd = (ri.block_eval(d, state, kind, i, xp)[0] - ri.block_eval(d, state, kind, i, xm)[0]) / (2 * h)
            assert abs(fd - g[k]) <= 1e-5 * max(1.0, abs(g[k])), (kind, k, fd, g[k])


@pytest.mark.parametrize("cams,frames,pts", [(3, 5, 8), (4, 4, 6)])
def test_a_pass_never_raises_the_cost_and_every_block_stops_on_a_test(cams, frames, pts):
    sc = rig_outlier_case(cams, frames, pts)
    d = _data(sc)
    state = [sc["cam_q0"], sc["cam_t0"], sc["frame_q0"], sc["frame_t0"]]
    c0 = ri.total_cost(d, state)
    cq, ct, fq, ft, its, recs = ri.inner_pass(d, *state)
    c1 = ri.total_cost(d, [cq, ct, fq, ft])
    assert c1 <= c0
    assert c1 < c0   # (the starting cameras are perturbed: the pass finds something)
    assert len(its) == 4 and all(0 <= n <= 50 for n in its)
    # every block, re-evaluated independently on the state its group started from: Ceres' gradient test met, or the mini-solve
    # stopped on its parameter / function test with the gradient brought down to under a twentieth of where it started
    where = {"q_cr": 0, "t_cr": 1, "q_rw": 2, "t_rw": 3}
    state = [np.array(a, dtype=np.float64).copy() for a in state]
    ends = {"q_cr": cq, "t_cr": ct, "q_rw": fq, "t_rw": ft}
    for kind in ri.GROUPS:
        rs = recs[kind]
        assert len(rs) == (d.cam_block.sum() if kind.endswith("cr") else d.frame_block.sum())
        for i, n, term, _ in rs:
            x0, x1 = state[where[kind]][i], ends[kind][i]
            c_start, g0, _ = ri.block_eval(d, state, kind, i, x0)
            c_end, g1, _ = ri.block_eval(d, state, kind, i, x1)
            gm0, gm1 = ri._gmax(kind, x0, g0), ri._gmax(kind, x1, g1)
            assert c_end <= c_start
            assert term in (ri.GRADIENT, ri.PARAMETER, ri.FUNCTION), (kind, i, term, n)
            if term == ri.GRADIENT:
                assert gm1 <= ri.OPTS["gradient_tolerance"]
            else:
                assert gm1 <= 0.05 * gm0, (kind, i, term, gm0, gm1)
        state[where[kind]] = ends[kind].copy()
    # frozen camera 0 is not a block and does not move
    assert np.array_equal(cq[0], sc["cam_q0"][0]) and np.array_equal(ct[0], sc["cam_t0"][0])


def test_a_block_at_its_minimum_stops_at_once():
    sc = rig_outlier_case(3, 3, 6)
    d = _data(sc)
    state = [sc["cam_q0"], sc["cam_t0"], sc["frame_q0"], sc["frame_t0"]]
    x, n, term, _ = ri.mini_solve(d, state, "t_rw", 1)
    state[3] = state[3].copy()
    state[3][1] = x
    x2, n2, term2, _ = ri.mini_solve(d, state, "t_rw", 1)
    assert n2 <= 1 and np.abs(x2 - x).max() <= 1e-9


@pytest.mark.parametrize("cams,frames,pts", [(3, 12, 20), (4, 16, 24)])
def test_numpy_outer_lm_without_inner_iterations_reproduces_the_oracle_solve(cams, frames, pts):
    sc = rig_outlier_case(cams, frames, pts)
    d = _data(sc)
    q, t, fq, ft, s = ri.rig_solve(d, sc["cam_q0"], sc["cam_t0"], sc["frame_q0"], sc["frame_t0"])
    oq, ot, ofq, oft, _, so = po.rig_solve(cams, sc["frame_offsets"], sc["obs_cam"], sc["obs_world"], sc["obs_uv"],
                                           sc["world_xyz"], sc["cam_q0"], sc["cam_t0"], sc["cam_frozen"], sc["frame_q0"],
                                           sc["frame_t0"], huber_a=HUBER_A)
    assert s["iterations"] == so["iterations"] and s["termination"] == so["termination"]
    assert len(s["log"]) == len(so["log"]) > 3
    for a, b in zip(s["log"], so["log"]):
        assert a["accepted"] == b["accepted"] and a["valid"] == b["valid"]
        assert abs(a["cost"] - b["cost"]) <= 1e-9 * b["cost"]
    for a, b in ((q, oq), (t, ot), (fq, ofq), (ft, oft)):
        assert np.abs(a - b).max() <= 1e-9


def test_numpy_outer_lm_with_inner_iterations_takes_passes_and_never_ends_above_its_start():
    sc = rig_outlier_case(3, 12, 20)
    d = _data(sc)
    *_, s = ri.rig_solve(d, sc["cam_q0"], sc["cam_t0"], sc["frame_q0"], sc["frame_t0"], inner=True)
    assert s["passes"] >= 1 and s["useful_passes"] >= 1 and s["cost_removed"] > 0.0
    assert s["final_cost"] < s["initial_cost"]
    # every accepted iteration lowered the cost (the pass only ever lowers the candidate's cost)
    costs = [e["cost"] for e in s["log"] if e["accepted"]]
    assert all(b <= a for a, b in zip(costs, costs[1:]))
