"""GPU: Ceres' inner iterations on the rig problem (cc_rig_set_inner_iterations / cc_rig_inner_pass / cc_rig_inner_status,
camera_calibrator_amd/csrc/cc_rig_inner.hip) against the numpy restatement of one pass (tests/rig_inner_ref.py)."""
import ctypes as C

import numpy as np
import pytest

from camera_calibrator_amd import capi
from tests import rig_inner_ref as ri
from tests.helpers import rig_outlier_case

pytestmark = pytest.mark.gpu
HUBER_A = capi.HUBER_A
CC_ERR_STATE = -5


def _subset(sc, keep):
    """The scenario with only the observations `keep` (frame-grouped order kept)."""
    frames = np.repeat(np.arange(len(sc["frame_offsets"]) - 1), np.diff(sc["frame_offsets"]))[keep]
    off = np.zeros(len(sc["frame_offsets"]), dtype=np.int64)
    np.add.at(off, frames + 1, 1)
    return dict(sc, obs_cam=sc["obs_cam"][keep], obs_world=sc["obs_world"][keep], obs_uv=sc["obs_uv"][keep],
                frame_offsets=np.cumsum(off))


def _case(name):
    if name == "large_blocks":   # > 1024 observations per camera, > 256 per frame: the kernels' strided loops run several trips
        return rig_outlier_case(2, 8, 150), HUBER_A
    sc = rig_outlier_case(3, 6, 10)
    huber_a = HUBER_A
    if name == "huber_off":
        huber_a = 1e6
    elif name == "ragged":   # frames of different sizes, camera 2 missing from frames 0 and 3, camera 1 frozen too
        rng = np.random.default_rng(5)
        frames = np.repeat(np.arange(6), np.diff(sc["frame_offsets"]))
        keep = rng.random(len(sc["obs_cam"])) < 0.7
        keep &= ~((sc["obs_cam"] == 2) & np.isin(frames, [0, 3]))
        sc = _subset(sc, keep)
        sc["cam_frozen"] = np.array([1, 1, 0], dtype=np.uint8)
    return sc, huber_a


def _problem(sc, huber_a):
    p = capi.RigProblem(len(sc["cam_T"]), sc["frame_offsets"], sc["obs_cam"], sc["obs_world"], sc["obs_uv"], sc["world_xyz"],
                        sc["cam_frozen"], huber_a=huber_a)
    p.set_state(sc["cam_q0"], sc["cam_t0"], sc["frame_q0"], sc["frame_t0"])
    return p


@pytest.mark.parametrize("name", ["huber_on_frozen_cam0", "huber_off", "ragged", "large_blocks"])
def test_inner_pass_matches_the_numpy_pass(name):
    sc, huber_a = _case(name)
    d = ri.RigData(len(sc["cam_T"]), sc["frame_offsets"], sc["obs_cam"], sc["obs_world"], sc["obs_uv"], sc["world_xyz"],
                   sc["cam_frozen"], huber_a)
    state0 = [sc["cam_q0"], sc["cam_t0"], sc["frame_q0"], sc["frame_t0"]]
    cq, ct, fq, ft, its, _ = ri.inner_pass(d, *state0)
    c0_ref, c1_ref = ri.total_cost(d, state0), ri.total_cost(d, [cq, ct, fq, ft])
    p = _problem(sc, huber_a)
    c0, c1, its_g = p.inner_pass()
    gq, gt, gfq, gft, _ = p.get_state(want_cost=False)
    p.close()
    assert its_g == its
    assert abs(c0 - c0_ref) <= 1e-12 * c0_ref and abs(c1 - c1_ref) <= 1e-12 * c1_ref, (c0, c0_ref, c1, c1_ref)
    for a, b in ((gq, cq), (gt, ct), (gfq, fq), (gft, ft)):
        assert np.abs(a - b).max() <= 1e-10
    assert c1 < c0


def _solve(p, inner=None, options=None):
    if inner is not None:
        p.set_inner_iterations(inner)
    s = p.solve(options=options)
    return s, p.get_state(want_cost=False)


def test_inner_iterations_explicitly_off_are_bit_identical_and_on_means_form_0():
    sc = rig_outlier_case(3, 8, 12)
    a = _problem(sc, HUBER_A)
    b = _problem(sc, HUBER_A)
    c = _problem(sc, HUBER_A)
    form = a.solver_form()
    # (all three in the three-kernel form -- profiled solves never take the lean one: the lean and the three-kernel form agree
    # to rounding only, and which one a solve gets also depends on the device's back-off state)
    o = capi.default_options(max_iterations=1000, profile_kernels=1)
    sa, xa = _solve(a, options=o)
    sb, xb = _solve(b, inner=False, options=o)
    assert sa["iterations"] == sb["iterations"] and sa["final_cost"] == sb["final_cost"]
    assert all(np.array_equal(u, v) for u, v in zip(xa[:4], xb[:4]))
    # on, then off again before the solve: the handle's form and the result are those of a handle never switched
    c.set_inner_iterations(True)
    assert c.solver_form() == 0
    c.set_inner_iterations(False)
    assert c.solver_form() == form
    sc_, xc = _solve(c, options=o)
    assert sc_["iterations"] == sa["iterations"] and sc_["final_cost"] == sa["final_cost"]
    assert all(np.array_equal(u, v) for u, v in zip(xa[:4], xc[:4]))
    assert c.inner_status()["passes"] == 0
    for p in (a, b, c):
        p.close()


@pytest.mark.parametrize("cams,frames,pts", [(3, 12, 20), (4, 16, 24)])
def test_solve_with_inner_iterations_matches_the_numpy_outer_lm(cams, frames, pts):
    """Iteration log, termination, inner-pass statistics and final state against tests/rig_inner_ref.py::rig_solve."""
    sc = rig_outlier_case(cams, frames, pts)
    d = ri.RigData(cams, sc["frame_offsets"], sc["obs_cam"], sc["obs_world"], sc["obs_uv"], sc["world_xyz"], sc["cam_frozen"], HUBER_A)
    *ref, sr = ri.rig_solve(d, sc["cam_q0"], sc["cam_t0"], sc["frame_q0"], sc["frame_t0"], inner=True)
    p = _problem(sc, HUBER_A)
    s, x = _solve(p, inner=True)
    st = p.inner_status()
    p.close()
    assert s["iterations"] == sr["iterations"] and s["termination"] == sr["termination"], (s["termination"], sr["termination"])
    assert len(s["log"]) == len(sr["log"])
    for a, b in zip(s["log"], sr["log"]):
        assert a["accepted"] == b["accepted"] and a["valid"] == b["valid"]
        assert abs(a["cost"] - b["cost"]) <= 1e-8 * b["cost"]
        assert abs(a["model_cost_change"] - b["model_cost_change"]) <= 1e-8 * max(abs(b["model_cost_change"]), 1e-12)
    assert st["passes"] == sr["passes"] >= 1 and st["useful_passes"] == sr["useful_passes"]
    assert st["enabled_at_end"] == sr["enabled_at_end"]
    assert abs(st["cost_removed"] - sr["cost_removed"]) <= 1e-8 * abs(sr["cost_removed"])
    for a, b in zip(x[:4], ref):
        assert np.abs(a - b).max() <= 1e-8


def test_solve_with_inner_iterations_is_repeatable_and_reports_its_passes():
    sc = rig_outlier_case(4, 10, 12)
    runs = []
    for _ in range(2):
        p = _problem(sc, HUBER_A)
        s, x = _solve(p, inner=True)
        runs.append((s, x, p.inner_status()))
        p.close()
    (s1, x1, st1), (s2, x2, st2) = runs
    assert s1["iterations"] == s2["iterations"] and s1["final_cost"] == s2["final_cost"]
    assert all(np.array_equal(u, v) for u, v in zip(x1[:4], x2[:4]))
    assert st1 == st2
    assert st1["passes"] >= 1 and st1["useful_passes"] >= 1 and st1["cost_removed"] > 0.0
    assert np.isfinite(s1["final_cost"]) and s1["final_cost"] < s1["initial_cost"]


def test_blocked_path_with_inner_iterations():
    """23 cameras, camera 0 frozen: 132 shared coordinates (> 127: k_rig_elim_big / k_rig_solve_big)."""
    sc = rig_outlier_case(23, 12, 6)
    p = _problem(sc, HUBER_A)
    s_off, _ = _solve(p)
    p.reset()
    s_on, _ = _solve(p, inner=True)
    st = p.inner_status()
    p.close()
    assert st["useful_passes"] >= 1
    assert s_on["final_cost"] <= s_off["final_cost"] * (1 + 1e-9), (s_on["final_cost"], s_off["final_cost"])


def test_rigk_handles_refuse_inner_iterations():
    sc = rig_outlier_case(2, 4, 8)
    p = capi.RigProblem(2, sc["frame_offsets"], sc["obs_cam"], sc["obs_world"], sc["obs_uv"], sc["world_xyz"], sc["cam_frozen"],
                        with_intrinsics=True)
    rc = capi.lib().cc_rig_set_inner_iterations(p._h, C.c_int32(1), C.c_double(1e-3))
    rc2 = capi.lib().cc_rig_inner_pass(p._h, None, None, None)
    p.close()
    assert rc == CC_ERR_STATE and rc2 == CC_ERR_STATE


def test_exchange_attached_handles_refuse_inner_iterations_and_the_reverse():
    sc = rig_outlier_case(3, 4, 8)
    p = _problem(sc, HUBER_A)
    p.exchange_attach(0, [p.exchange_export()])   # (a single rank: a valid, degenerate exchange)
    rc = capi.lib().cc_rig_set_inner_iterations(p._h, C.c_int32(1), C.c_double(1e-3))
    rc2 = capi.lib().cc_rig_inner_pass(p._h, None, None, None)
    p.close()
    q = _problem(sc, HUBER_A)
    q.set_inner_iterations(True)
    h = q.exchange_export()
    buf = (C.c_uint8 * 64).from_buffer_copy(h)
    rc3 = capi.lib().cc_rig_exchange_attach(q._h, C.c_int32(0), C.c_int32(1), buf)
    q.close()
    assert rc == CC_ERR_STATE and rc2 == CC_ERR_STATE and rc3 == CC_ERR_STATE


def test_extrinsics_calibrator_with_inner_iterations_matches_the_handle_api():
    """The reference's rig test scenario (src/test_extrinsics_calibrator.cpp:48-134, 2 cameras, camera 0 frozen) through
    pycalibrator.ExtrinsicsCalibrator with SetInnerIterations(True), against the handle API on the same float inputs."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "camera_calibrator_amd"))
    import pycalibrator as pc
    from oracle import pyoracle as po
    F, M = 40, 6
    sc = po.rig_scenario(2, F, M)
    e = pc.ExtrinsicsCalibrator()
    e.SetVerbose(False)
    e.SetInnerIterations(True)
    for c in range(2):
        e.AddCameraTRig(sc["cam_T"][c].reshape(4, 4).T, freeze=(c == 0))
    for f in range(F):
        e.AddObservationFrame(sc["frame_T"][f].reshape(4, 4).T)
    wid = 0
    for f in range(F):
        for _ in range(M):
            w = e.AddWorldPoint(f, sc["world_xyz"][wid])
            for c in range(2):
                k = (f * M + (wid - f * M)) * 2 + c
                e.AddObservation(c, w, sc["obs_uv"][k])
            wid += 1
    e.Optimize()
    assert e.LastStatus() == 0 and e.LastInnerPasses() >= 1
    # the handle API on what the class hands over: its float transforms -> quaternion / translation by the same conversion
    # (cc_affine_to_qt is AffineToQuaternionTranslation, extrinsics_calibrator.cpp)
    cq, ct = capi.affine_to_qt(sc["cam_T"])
    fq, ft = capi.affine_to_qt(sc["frame_T"])
    p = capi.RigProblem(2, sc["frame_offsets"], sc["obs_cam"], sc["obs_world"], sc["obs_uv"], sc["world_xyz"],
                        np.array([1, 0], dtype=np.uint8))
    p.set_state(cq, ct, fq, ft)
    p.set_inner_iterations(True)
    s = p.solve()
    gq, gt, gfq, gft, cost = p.get_state()
    passes = p.inner_status()["passes"]
    p.close()
    assert e.LastIterations() == s["iterations"] and e.LastFinalCost() == s["final_cost"] and e.LastInnerPasses() == passes
    # the solve itself bit for bit: per-observation costs at the end
    for f in (0, 3, F - 1):
        for k in range(2 * M):
            assert e.GetObservation(f, k)[4] == cost[sc["frame_offsets"][f] + k]
    # the poses as the class writes them back (through float, with the oracle's restatement of that conversion)
    want_cam, want_frame = po.qt_to_affine(gq, gt), po.qt_to_affine(gfq, gft)
    for c in range(2):
        assert np.abs(e.GetCameraTRig(c).T.reshape(-1) - want_cam[c]).max() <= 1e-6
    for f in range(F):
        assert np.abs(e.GetObservationFrame(f).T.reshape(-1) - want_frame[f]).max() <= 1e-6
    # several devices: CC_ERR_STATE, no exception
    e.SetDevices([0, 0])
    e.Optimize()
    assert e.LastStatus() == CC_ERR_STATE
