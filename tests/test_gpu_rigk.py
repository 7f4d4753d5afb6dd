"""EXTENSION: rig poses + 9 shared intrinsics on pixel observations (cc_rigk_*).
Nothing in the reference does this; the checker is the oracle's own restatement of the composed model
(oracle.cpp RigKProblem), itself validated on the CPU in tests/test_oracle_rigk.py."""
import numpy as np
import pytest

from camera_calibrator_amd import capi
from oracle import pyoracle as po
from tests.helpers import RIGK_INTR_TRUE, rigk_case

pytestmark = pytest.mark.gpu


def _both(k, const_mask=0, huber_a=0.0, **kw):
    prob = capi.RigProblem(k["cams"], k["frame_offsets"], k["obs_cam"], k["obs_world"], k["obs_uv_pix"], k["world_xyz"],
                           k["cam_frozen"], huber_a=huber_a, with_intrinsics=True)
    prob.set_intrinsics(k["intr0"], const_mask)
    prob.set_state(k["cam_q0"], k["cam_t0"], k["frame_q0"], k["frame_t0"])
    s = prob.solve(capi.default_options(max_iterations=200, **kw))
    g = (prob.get_intrinsics(),) + tuple(prob.get_state()) + (s,)
    prob.close()
    o = po.rigk_solve(k["cams"], k["frame_offsets"], k["obs_cam"], k["obs_world"], k["obs_uv_pix"], k["world_xyz"], k["intr0"],
                      k["cam_q0"], k["cam_t0"], k["cam_frozen"], k["frame_q0"], k["frame_t0"], const_mask=const_mask,
                      huber_a=huber_a, options=po.default_options(max_iterations=200, **kw))
    return g, o


def _assert_same(g, o):
    sg, so = g[6], o[6]
    assert sg["termination"] == so["termination"] and sg["iterations"] == so["iterations"]
    assert [l["accepted"] for l in sg["log"]] == [l["accepted"] for l in so["log"]]
    assert np.allclose([l["cost"] for l in sg["log"]], [l["cost"] for l in so["log"]], rtol=1e-9)
    assert np.allclose(g[0][:4], o[0][:4], rtol=1e-11) and np.allclose(g[0][4:], o[0][4:], atol=1e-11)   # (measured <= 5e-14: profiles/r03/rigk_deviation.jsonl)
    for a in range(1, 5):
        assert np.abs(g[a] - o[a]).max() < 1e-11
    # per-observation costs: 1/2 |r|^2 of ~0.3 px residuals formed as differences of ~1e3 px numbers -- relative floor measured
    # <= 4.7e-10 (profiles/r03/rigk_deviation.jsonl), asserted at 1e-8 (was 1e-6)
    assert np.allclose(g[5], o[5], rtol=1e-8, atol=1e-12), np.abs(g[5] / np.maximum(o[5], 1e-300) - 1).max()


@pytest.mark.parametrize("cams,frames,pts", [(2, 50, 8), (4, 60, 30), (3, 20, 300), (8, 25, 70), (1, 40, 20)])
def test_rigk_matches_oracle(cams, frames, pts):
    g, o = _both(rigk_case(cams, frames, pts))
    _assert_same(g, o)


def test_rigk_frozen_intrinsics_and_huber():
    k = rigk_case(3, 40, 25)
    mask = (1 << 8) | (1 << 5)                       # k3 and k2 held constant (cf. cam_calibration.py:308)
    g, o = _both(k, const_mask=mask, huber_a=1.0)
    _assert_same(g, o)
    assert g[0][8] == k["intr0"][8] and g[0][5] == k["intr0"][5]


def test_rigk_recovers_the_planted_camera_and_rig():
    k = rigk_case(4, 120, 40)
    g, _ = _both(k)
    assert np.abs(g[0][:2] / RIGK_INTR_TRUE[:2] - 1).max() < 5e-3 and np.abs(g[0][2:4] - RIGK_INTR_TRUE[2:4]).max() < 5.0
    assert np.abs(g[2] - k["cam_t_true"]).max() < 0.2 * np.abs(k["cam_t0"] - k["cam_t_true"]).max()
    assert np.array_equal(g[1][0], k["cam_q0"][0]) and np.array_equal(g[2][0], k["cam_t0"][0])   # frozen camera


def test_rigk_needs_its_intrinsics_and_a_plain_handle_refuses_them():
    k = rigk_case(2, 10, 6)
    prob = capi.RigProblem(2, k["frame_offsets"], k["obs_cam"], k["obs_world"], k["obs_uv_pix"], k["world_xyz"],
                           k["cam_frozen"], with_intrinsics=True)
    prob.set_state(k["cam_q0"], k["cam_t0"], k["frame_q0"], k["frame_t0"])
    with pytest.raises(capi.CcError, match="set_intrinsics"):
        prob.solve()
    prob.close()
    plain = capi.RigProblem(2, k["frame_offsets"], k["obs_cam"], k["obs_world"], k["obs_uv_pix"], k["world_xyz"], k["cam_frozen"])
    with pytest.raises(capi.CcError, match="without intrinsics"):
        plain.set_intrinsics(k["intr0"])
    plain.close()


def test_rigk_c4_full_size_matches_oracle():
    """BASELINE.json configs[3] WITH shared intrinsics: 4 cameras x 400 frames x 300 points, 480k PIXEL observations.
    Live against the oracle (~1 s): same trajectory, same minimiser."""
    g, o = _both(rigk_case(4, 400, 300))
    _assert_same(g, o)
    assert g[6]["iterations"] >= 3


def test_rigk_c5_full_size_against_the_committed_oracle_result_and_properties():
    """BASELINE.json configs[4] WITH shared intrinsics: 8 cameras x 2000 frames x 500 points, 8M pixel observations.
    The oracle's answer is a committed fixture (tests/golden/make_rigk_c5.py): same trajectory, same intrinsics,
    camera poses, a subset of the frame poses and per-observation costs. Plus size-independent properties: the
    frozen camera is untouched, the per-observation costs add up to the reported cost, a second solve from the
    solution is (nearly) a fixed point."""
    import os
    gld = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rigk_c5_oracle.npz"))
    k = rigk_case(int(gld["cams"]), int(gld["frames"]), int(gld["pts"]))
    prob = capi.RigProblem(k["cams"], k["frame_offsets"], k["obs_cam"], k["obs_world"], k["obs_uv_pix"], k["world_xyz"],
                           k["cam_frozen"], huber_a=0.0, with_intrinsics=True)
    prob.set_intrinsics(k["intr0"], 0)
    prob.set_state(k["cam_q0"], k["cam_t0"], k["frame_q0"], k["frame_t0"])
    s1 = prob.solve(capi.default_options(max_iterations=200))
    intr = prob.get_intrinsics()
    r1 = prob.get_state()
    assert s1["termination"] == str(gld["termination"]) and s1["iterations"] == int(gld["iterations"])
    assert [l["accepted"] for l in s1["log"]] == list(gld["accepted"])
    assert np.allclose([l["cost"] for l in s1["log"]], gld["costs"], rtol=1e-9)
    assert np.isclose(s1["initial_cost"], float(gld["initial_cost"]), rtol=1e-10)
    assert np.isclose(s1["final_cost"], float(gld["final_cost"]), rtol=1e-10)
    assert np.allclose(intr[:4], gld["intr"][:4], rtol=1e-11) and np.allclose(intr[4:], gld["intr"][4:], atol=1e-11)
    assert np.abs(r1[0] - gld["cam_q"]).max() < 1e-11 and np.abs(r1[1] - gld["cam_t"]).max() < 1e-11
    pick = gld["frame_pick"]
    assert np.abs(r1[2][pick] - gld["frame_q"]).max() < 1e-11 and np.abs(r1[3][pick] - gld["frame_t"]).max() < 1e-11
    assert np.allclose(r1[4][:64], gld["obs_cost_head"], rtol=1e-8, atol=1e-12)
    assert np.isclose(r1[4].sum(), float(gld["obs_cost_sum"]), rtol=1e-11)
    # properties
    assert np.array_equal(r1[0][0], k["cam_q0"][0]) and np.array_equal(r1[1][0], k["cam_t0"][0])
    assert np.isclose(r1[4].sum(), s1["final_cost"], rtol=1e-9) and r1[4].shape == (8_000_000,)
    prob.set_intrinsics(intr, 0)
    prob.set_state(r1[0], r1[1], r1[2], r1[3])
    s2 = prob.solve(capi.default_options(max_iterations=200))
    prob.close()
    assert s2["iterations"] <= 2 and s2["final_cost"] <= s1["final_cost"] * (1 + 1e-9)


# ---- one set of intrinsics per camera (cc_rigk_create_per_camera) ----

# Tolerances of the per-camera variant against the oracle (measured deviations: scripts/rigk_deviation.py,
# profiles/r03/rigk_deviation.jsonl).
# Largest deviations seen over five shapes up to 8 x 2000 x 500 (S = 114): focal lengths / principal point 2.4e-14
# relative, distortion 8.2e-14, poses 1.5e-14, per-observation costs 4.7e-10 relative, per-iteration costs 8.2e-13 --
# the rounding floor of a different summation order, nothing more: the 1e-7 / 1e-8 the round-2 tests allowed were
# simply loose. (The problem is well conditioned at that level: a 2-ulp perturbation of the initial intrinsics moves
# the oracle's own answer by 1e-14, tests/test_oracle_rigk.py.)
PC_TOL = dict(intr_rel=1e-11, dist_abs=1e-11, pose=1e-11, obs_cost_rel=1e-8)

def _both_pc(k, const_masks=None, huber_a=0.0, **kw):
    prob = capi.RigProblem(k["cams"], k["frame_offsets"], k["obs_cam"], k["obs_world"], k["obs_uv_pix"], k["world_xyz"],
                           k["cam_frozen"], huber_a=huber_a, with_intrinsics="per_camera")
    for c in range(k["cams"]):
        prob.set_camera_intrinsics(c, k["intr0"][c], 0 if const_masks is None else int(const_masks[c]))
    prob.set_state(k["cam_q0"], k["cam_t0"], k["frame_q0"], k["frame_t0"])
    s = prob.solve(capi.default_options(max_iterations=300, **kw))
    g = (prob.get_camera_intrinsics(),) + tuple(prob.get_state()) + (s,)
    prob.close()
    o = po.rigk_solve_per_camera(k["cams"], k["frame_offsets"], k["obs_cam"], k["obs_world"], k["obs_uv_pix"], k["world_xyz"],
                                 k["intr0"], k["cam_q0"], k["cam_t0"], k["cam_frozen"], k["frame_q0"], k["frame_t0"],
                                 const_masks=const_masks, huber_a=huber_a, options=po.default_options(max_iterations=300, **kw))
    return g, o


PC_TOL_HUBER = dict(intr_rel=1e-9, dist_abs=1e-9, pose=1e-9, obs_cost_rel=1e-6)   # (robust loss active: not measured separately)


def _assert_same_pc(g, o, tol=None):
    tol = tol or PC_TOL
    sg, so = g[6], o[6]
    assert sg["termination"] == so["termination"] and sg["iterations"] == so["iterations"]
    assert [l["accepted"] for l in sg["log"]] == [l["accepted"] for l in so["log"]]
    assert np.allclose([l["cost"] for l in sg["log"]], [l["cost"] for l in so["log"]], rtol=1e-9)
    assert np.allclose(g[0][:, :4], o[0][:, :4], rtol=tol["intr_rel"]) and np.allclose(g[0][:, 4:], o[0][:, 4:], atol=tol["dist_abs"])
    for a in range(1, 5):
        assert np.abs(g[a] - o[a]).max() < tol["pose"]
    assert np.allclose(g[5], o[5], rtol=tol["obs_cost_rel"], atol=1e-11)


@pytest.mark.parametrize("cams,frames,pts", [(2, 60, 20), (3, 150, 40), (8, 60, 60), (1, 40, 20)])
def test_rigk_per_camera_matches_oracle(cams, frames, pts):
    g, o = _both_pc(rigk_case(cams, frames, pts, per_camera=True))
    _assert_same_pc(g, o)


def test_rigk_per_camera_masks_huber_and_an_unobserved_camera():
    k = rigk_case(3, 60, 25, per_camera=True)
    masks = np.array([(1 << 8) | (1 << 5), 0, 1 << 8], dtype=np.uint32)
    g, o = _both_pc(k, const_masks=masks, huber_a=1.5)
    _assert_same_pc(g, o, PC_TOL_HUBER)
    assert g[0][0, 8] == k["intr0"][0, 8] and g[0][0, 5] == k["intr0"][0, 5] and g[0][2, 8] == k["intr0"][2, 8]
    keep = k["obs_cam"] != 2
    offs = np.concatenate([[0], np.cumsum([keep[k["frame_offsets"][f]:k["frame_offsets"][f + 1]].sum() for f in range(60)])])
    k2 = dict(k, frame_offsets=offs.astype(np.int64), obs_cam=k["obs_cam"][keep], obs_world=k["obs_world"][keep], obs_uv_pix=k["obs_uv_pix"][keep])
    g, o = _both_pc(k2)
    _assert_same_pc(g, o)
    assert np.array_equal(g[0][2], k["intr0"][2]) and np.array_equal(g[1][2], k["cam_q0"][2])


def test_rigk_per_camera_c5_full_size_against_the_committed_oracle_result_and_properties():
    """BASELINE.json configs[4] as worded ("full intrinsics+extrinsics co-optimisation"): 8 cameras x 2000 frames x
    500 points with a camera model of its own per camera: 114 shared coordinates. The oracle's answer is a committed
    fixture (tests/golden/make_rigk_pc_c5.py): same trajectory (accept/reject sequence, per-iteration costs), same
    intrinsics per camera, camera poses, a subset of the frame poses, per-observation costs. Plus the size-independent
    properties: planted cameras recovered, frozen pose untouched, per-observation costs add up, second solve is a
    fixed point."""
    import os
    gld = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rigk_pc_c5_oracle.npz"))
    k = rigk_case(int(gld["cams"]), int(gld["frames"]), int(gld["pts"]), per_camera=True)
    prob = capi.RigProblem(8, k["frame_offsets"], k["obs_cam"], k["obs_world"], k["obs_uv_pix"], k["world_xyz"], k["cam_frozen"],
                           huber_a=0.0, with_intrinsics="per_camera")
    for c in range(8):
        prob.set_camera_intrinsics(c, k["intr0"][c], 0)
    prob.set_state(k["cam_q0"], k["cam_t0"], k["frame_q0"], k["frame_t0"])
    s1 = prob.solve(capi.default_options(max_iterations=200))
    intr = prob.get_camera_intrinsics()
    r1 = prob.get_state()
    # against the oracle's committed result
    assert s1["termination"] == str(gld["termination"]) and s1["iterations"] == int(gld["iterations"])
    assert [l["accepted"] for l in s1["log"]] == list(gld["accepted"])
    assert np.allclose([l["cost"] for l in s1["log"]], gld["costs"], rtol=1e-9)
    assert np.isclose(s1["initial_cost"], float(gld["initial_cost"]), rtol=1e-10)
    assert np.isclose(s1["final_cost"], float(gld["final_cost"]), rtol=1e-10)
    assert np.allclose(intr[:, :4], gld["intr"][:, :4], rtol=PC_TOL["intr_rel"]) and np.allclose(intr[:, 4:], gld["intr"][:, 4:], atol=PC_TOL["dist_abs"])
    assert np.abs(r1[0] - gld["cam_q"]).max() < PC_TOL["pose"] and np.abs(r1[1] - gld["cam_t"]).max() < PC_TOL["pose"]
    pick = gld["frame_pick"]
    assert np.abs(r1[2][pick] - gld["frame_q"]).max() < PC_TOL["pose"] and np.abs(r1[3][pick] - gld["frame_t"]).max() < PC_TOL["pose"]
    assert np.allclose(r1[4][:64], gld["obs_cost_head"], rtol=PC_TOL["obs_cost_rel"], atol=1e-12)
    assert np.isclose(r1[4].sum(), float(gld["obs_cost_sum"]), rtol=1e-11)
    # properties
    assert s1["final_cost"] < 1e-2 * s1["initial_cost"]
    assert np.abs(intr[:, :2] / k["intr_true"][:, :2] - 1).max() < 2e-3 and np.abs(intr[:, 2:4] - k["intr_true"][:, 2:4]).max() < 2.0
    assert np.array_equal(r1[0][0], k["cam_q0"][0]) and np.array_equal(r1[1][0], k["cam_t0"][0])
    assert np.isclose(r1[4].sum(), s1["final_cost"], rtol=1e-9) and r1[4].shape == (8_000_000,)
    for c in range(8):
        prob.set_camera_intrinsics(c, intr[c], 0)
    prob.set_state(r1[0], r1[1], r1[2], r1[3])
    s2 = prob.solve(capi.default_options(max_iterations=200))
    prob.close()
    assert s2["iterations"] <= 2 and s2["final_cost"] <= s1["final_cost"] * (1 + 1e-9)


def test_rigk_per_camera_with_more_than_127_shared_coordinates_matches_the_oracle():
    """Ten cameras with a camera model of their own: 9 * 6 + 10 * 9 = 144 shared coordinates -- beyond the tuned kernels'
    127, solved by the plain ones (cc_rig.hip, k_rig_elim_big / k_rig_solve_big)."""
    g, o = _both_pc(rigk_case(10, 40, 30, per_camera=True))
    _assert_same_pc(g, o)


def test_rigk_shared_intrinsics_with_more_than_11_observed_cameras_matches_the_oracle():
    """Fourteen cameras, one shared camera model: 13 * 6 + 9 = 87 shared coordinates, but 14 * 135 direct sums -- more than
    the tuned elimination kernel keeps (1536); the plain kernels take over."""
    g, o = _both(rigk_case(14, 30, 20))
    _assert_same(g, o)


@pytest.mark.parametrize("cams,frames,pts", [(10, 12, 10)])
def test_rigk_shared_intrinsics_at_63_coordinates_the_last_size_of_the_four_column_factorisation(cams, frames, pts):
    """10 cameras with one shared intrinsics set: 6 * 9 + 9 = 63 shared coordinates, the last size chol_block4
    (cc_rig_dev.hpp) takes before the dispatch goes to the one-wave panels -- 63 + the right-hand side's row fill four
    16-row tile rows exactly (n16 = 4, ten tiles, kMaxT = 4 per wave), the last block has three columns."""
    g, o = _both(rigk_case(cams, frames, pts))
    _assert_same(g, o)


def test_rigk_per_camera_at_the_largest_supported_size_matches_the_oracle():
    """Seventeen cameras with a camera model of their own: 16 * 6 + 17 * 9 = 249 of at most 255 shared coordinates (reduced
    system in global memory: its packed triangle no longer fits LDS)."""
    g, o = _both_pc(rigk_case(17, 30, 24, per_camera=True))
    _assert_same_pc(g, o)
