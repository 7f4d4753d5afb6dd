"""The numpy reference of the rig start (tests/rig_start_ref.py) against planted scenes, hand-made co-visibility tables and the
CPU oracle's rig solve. No GPU: the GPU tests (tests/test_gpu_rig_start.py) compare the kernels with this reference."""
import numpy as np
import pytest

from tests import rig_start_ref as ref
from oracle import pyoracle as po

# the hand-made tables of stage T, shared with tests/cpp/rig_start_tree.cpp (same numbers there):
#   (co-visibility table, frozen flags) -> (root, root at identity, parents)
TREE_CASES = {
    # a chain 0 - 1 - 2 - 3: camera 3 shares frames with 2 only, 2 with 1, 1 with 0; camera 0 frozen
    "chain": ([[9, 5, 0, 0], [5, 9, 4, 0], [0, 4, 9, 3], [0, 0, 3, 9]], [1, 0, 0, 0], (0, False, [-1, 0, 1, 2])),
    # a tie: no frozen camera, cameras 1 and 2 have the most valid views (root = the lower index, at the identity); cameras 0
    # and 3 share equally many frames with the root (0 goes first), and camera 3 then ties between parents 0 and 1 (0 wins)
    "tie": ([[6, 4, 0, 4], [4, 8, 2, 4], [0, 2, 8, 0], [4, 4, 0, 6]], [0, 0, 0, 0], (1, True, [1, -1, 1, 0])),
    # a disconnected camera (3) and an unobserved one (4)
    "disconnected": ([[7, 3, 2, 0, 0], [3, 7, 0, 0, 0], [2, 0, 7, 0, 0], [0, 0, 0, 5, 0], [0, 0, 0, 0, 0]], [1, 0, 0, 0, 0],
                     (0, False, [-1, 0, 0, -1, -1])),
    # two frozen cameras: 2 has more valid views and is the root, 0 is placed too and is the parent camera 1 shares more with
    "two_frozen": ([[5, 4, 1, 0], [4, 6, 2, 1], [1, 2, 8, 3], [0, 1, 3, 4]], [1, 0, 1, 0], (2, False, [-1, 0, -1, 2])),
}


@pytest.mark.parametrize("name", sorted(TREE_CASES))
def test_tree_on_hand_made_tables(name):
    covis, frozen, (root, at_identity, parents) = TREE_CASES[name]
    r, ident, parent, placed, order = ref.tree(covis, frozen)
    assert (r, ident, parent) == (root, at_identity, parents)
    assert all(placed[c] == (bool(frozen[c]) or c == root or parents[c] >= 0) for c in range(len(covis)))
    assert all(placed[parent[c]] for c in order) and [c for c in order] == [c for c in order if parents[c] >= 0]


def _view_bounds(scene, f, c, X, uv):
    """First-order bound on the pose error of a converged view from the float32 rounding of ITS image points: the minimiser
    moves by J^+ (delta uv), so |delta pose| <= |delta uv|_2 / sigma_min(J), J at the planted pose; x 2 for the second-order
    terms. (The world points are float32 numbers to begin with: the planter rounds them before it projects.)"""
    Rv = scene["cam_R"][c] @ scene["frame_R"][f]
    tv = scene["cam_R"][c] @ scene["frame_t"][f] + scene["cam_t"][c]
    p = X @ Rv.T + tv
    exact = p[:, :2] / p[:, 2:3]
    duv = np.linalg.norm((uv - exact).ravel())
    smin = np.linalg.svd(ref._jacobian(Rv, tv, X), compute_uv=False)[-1]
    return Rv, tv, 2.0 * duv / smin


@pytest.mark.parametrize("planar,unit,n", [(False, 1.0, 8), (False, 1e3, 6), (True, 1.0, 5), (True, 1e3, 12), (True, 1.0, 4)])
def test_reference_returns_the_planted_poses(planar, unit, n):
    scene = ref.plant_scene(3, 4, n, seed=11 + n, planar=planar, unit=unit)
    frozen = [1, 0, 0]
    cam_q = np.stack([ref.R_to_quat(R) for R in scene["cam_R"]])
    cq, ct, fq, ft, report, vl = ref.start(3, scene["frame_offsets"], scene["obs_cam"], scene["obs_world"], scene["obs_uv"],
                                           scene["world_xyz"], frozen, cam_q=cam_q, cam_t=scene["cam_t"], refine="converged")
    assert report["views_valid"] == 12 and report[("views_planar" if planar else "views_general")] == 12
    assert report["root_camera"] == 0 and report["cameras_unplaced"] == 0 and report["frames_unplaced"] == 0
    views = ref.views_of(scene["frame_offsets"], scene["obs_cam"], scene["obs_world"], scene["obs_uv"], scene["world_xyz"])
    worst = 0.0
    for (f, c, X, uv), (_, _, kind, R, t, m) in zip(views, vl):
        Rv, tv, b = _view_bounds(scene, f, c, X, uv)
        # the six coordinates of the update R <- exp(w) R, t <- t + d that the bound is stated in
        err = np.hypot(ref.rot_angle(Rv, R), np.linalg.norm(t - tv - 0.0))
        lever = 1.0 + np.linalg.norm(tv)   # (|d| and |w| mix through the lever arm |t| when the error is read off R and t)
        print(f"view f{f} c{c}: error {err:.3e}, bound {b * lever:.3e}")
        assert err <= b * lever
        worst = max(worst, b * lever)
    # cameras and frames are means of compositions of two views each: twice the worst view bound per composition, times the
    # lever arm that the composition applies to a rotation error (1 + the largest |t| involved), with the frozen root exact
    arm = 1.0 + max(np.linalg.norm(v[4]) for v in vl)
    for c in range(3):
        assert ref.rot_angle(ref.quat_to_R(cq[c]), scene["cam_R"][c]) <= 2 * worst
        assert np.linalg.norm(ct[c] - scene["cam_t"][c]) <= 2 * worst * arm
    for f in range(4):
        assert ref.rot_angle(ref.quat_to_R(fq[f]), scene["frame_R"][f]) <= 3 * worst
        assert np.linalg.norm(ft[f] - scene["frame_t"][f]) <= 3 * worst * arm


def test_svd_and_gram_routes_agree_on_planted_views():
    """The yardstick of the GPU test of stage V: how far the closed form moves between the SVD of the rows and the
    eigen-decomposition of their Gram matrix."""
    for planar, unit in ((False, 1.0), (True, 1e3)):
        scene = ref.plant_scene(2, 3, 9, seed=5, planar=planar, unit=unit)
        for f, c, X, uv in ref.views_of(scene["frame_offsets"], scene["obs_cam"], scene["obs_world"], scene["obs_uv"], scene["world_xyz"]):
            ka, Ra, ta = ref.view_closed_form(X, uv, "svd")
            kb, Rb, tb = ref.view_closed_form(X, uv, "gram")
            assert ka == kb == (ref.PLANAR if planar else ref.GENERAL)
            assert ref.rot_angle(Ra, Rb) < 1e-6 and np.linalg.norm(ta - tb) < 1e-6 * unit * 10


def test_invalid_views_of_the_reference():
    rng = np.random.default_rng(0)
    X6 = rng.uniform(-1, 1, (6, 3)) + [0, 0, 5]
    uv = X6[:, :2] / X6[:, 2:3]
    assert ref.view_closed_form(X6[:3], uv[:3])[0] == ref.INVALID              # three points
    assert ref.view_closed_form(X6[:5], uv[:5])[0] == ref.INVALID              # five points that span space
    line = np.outer(np.linspace(-1, 1, 7), [1, 2, 0.5]) + [0, 0, 5]
    assert ref.view_closed_form(line, line[:, :2] / line[:, 2:3])[0] == ref.INVALID   # collinear
    bad = uv.copy(); bad[2, 0] = np.nan
    assert ref.view_closed_form(X6, bad)[0] == ref.INVALID
    assert ref.view_closed_form(X6, uv)[0] == ref.GENERAL


# ---- the start leads the solve where the scenario's start leads it ------------------------------------------------------------
SHAPES = [(3, 20, 12, 1), (4, 30, 8, 2), (2, 10, 6, 3), (3, 8, 6, 4), (2, 12, 7, 5), (2, 6, 6, 7), (8, 12, 10, 8)]
# Bound: both runs stop by the same rule at the tight tolerances of the rig parity tests (tight_options below: function 1e-15, gradient 1e-13, parameter 1e-14), so each
# is within the rule's slack of the common minimum. Measured on this oracle over the seven shapes (the figures the test prints;
# DESIGN 4.15 has the table): relative cost difference <= 1.92e-14, camera translations <= 3.30e-10, camera rotations
# <= 2.25e-10 rad, all three at (8, 12, 10, 8). x 10 for the stopping rule's slack:
COST_REL, CAM_T_ABS, CAM_R_ABS = 1.92e-13, 3.30e-9, 2.25e-9


def tight_options():
    return po.default_options(max_iterations=1000, function_tolerance=1e-15, gradient_tolerance=1e-13, parameter_tolerance=1e-14)


def solve_from(sc, cq, ct, fq, ft):
    return po.rig_solve(sc["cam_T"].shape[0], sc["frame_offsets"], sc["obs_cam"], sc["obs_world"], sc["obs_uv"], sc["world_xyz"],
                        cq, ct, sc["cam_frozen"], fq, ft, options=tight_options())


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d_seed%d" % s)
def test_solve_from_the_reference_start_ends_where_the_scenario_start_ends(shape):
    C, F, M, seed = shape
    sc = po.rig_scenario(C, F, M, seed=seed)
    cq0, ct0 = po.affine_to_qt(sc["cam_T"])
    fq0, ft0 = po.affine_to_qt(sc["frame_T"])
    a = solve_from(sc, cq0, ct0, fq0, ft0)
    cq, ct, fq, ft, report, _ = ref.start(C, sc["frame_offsets"], sc["obs_cam"], sc["obs_world"], sc["obs_uv"], sc["world_xyz"],
                                          sc["cam_frozen"], cam_q=cq0, cam_t=ct0)
    assert report["cameras_unplaced"] == 0 and report["frames_unplaced"] == 0
    b = solve_from(sc, cq, ct, fq, ft)
    ca, cb = a[5]["final_cost"], b[5]["final_cost"]
    dt = np.abs(a[1] - b[1]).max()
    dr = max(ref.rot_angle(ref.quat_to_R(a[0][c]), ref.quat_to_R(b[0][c])) for c in range(C))
    print(f"{shape}: cost {ca:.9e} ({a[5]['iterations']} it) vs {cb:.9e} ({b[5]['iterations']} it): rel {abs(ca - cb) / ca:.2e}, cam_t {dt:.2e}, cam_R {dr:.2e}")
    assert abs(ca - cb) <= COST_REL * ca and dt <= CAM_T_ABS and dr <= CAM_R_ABS
