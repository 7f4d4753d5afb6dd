"""The 50-digit reference of the pixel start (tests/rigk_start_ref.py) against planted points, planted scenes and the CPU
reference of the rig solve with intrinsics (tests/rigk_fisheye_ref.py). No GPU: the GPU tests (tests/test_gpu_rigk_start.py)
compare the kernel and the entry points with this reference and take their end-to-end bounds from here."""
import functools

import mpmath as mp
import numpy as np
import pytest

from camera_calibrator_amd.harness import RIGK_INTR_TRUE, rigk_case
from oracle import pyoracle as po
from tests import fisheye_ref as fr
from tests import rig_start_ref as rs
from tests import rigk_fisheye_ref as rfr
from tests import rigk_start_ref as ref
from tests.test_rig_start_ref_cpu import _view_bounds

TURNING = np.array([600.0, 600.0, 800.0, 500.0, -0.4, 0, 0, 0, 0])   # theta_d turns back at theta = 0.9129, theta_d = 0.6086


# ---- 1. round trip ----------------------------------------------------------------------------------------------------------
def _planted_points(max_deg):
    """The axis, 1e-9 from it, and rings out to max_deg off the axis in eight directions that avoid the coordinate axes."""
    pts = [(0.0, 0.0), (1e-9, 0.0), (0.0, -1e-9), (6e-10, 8e-10)]
    for deg in (1e-3, 1.0, 10.0, 25.0, 40.0, 60.0, 75.0):
        if deg <= max_deg:
            r = np.tan(np.deg2rad(deg))
            pts += [(r * np.cos(a), r * np.sin(a)) for a in np.arange(8) * np.pi / 4 + 0.3]
    return np.array(pts)


@pytest.mark.parametrize("model,intr,max_deg", [(ref.FISHEYE, fr.TRUE_INTR, 75.0), (ref.RADTAN, RIGK_INTR_TRUE, 40.0)],
                         ids=["fisheye_75deg", "radtan_40deg"])
def test_unproject_returns_the_planted_point(model, intr, max_deg):
    want = _planted_points(max_deg)
    assert model == ref.FISHEYE or (intr[6] != 0 and intr[7] != 0)   # tangential terms
    with mp.workdps(ref.DPS):
        k = [mp.mpf(float(v)) for v in intr]
        pix = [(ref.fisheye_pixel if model == ref.FISHEYE else ref.radtan_pixel)(k, mp.mpf(float(x)), mp.mpf(float(y))) for x, y in want]
    got = ref.unproject(model, intr, np.array(pix, dtype=object))
    err = np.linalg.norm(got - want, axis=1)
    rel = err / np.maximum(np.linalg.norm(want, axis=1), np.finfo(np.float64).tiny)
    print(f"largest relative error {rel.max():.2e} over {len(want)} points out to {max_deg} degrees")
    assert got[0].tolist() == [0.0, 0.0]
    assert np.all(rel[1:] <= 1e-14)


def test_unproject_has_no_point_beyond_a_polynomial_that_turns_back():
    k = TURNING
    td_max = np.sqrt(1 / 1.2) * (1 - 0.4 / 1.2)
    uv = np.array([[k[2] + k[0] * td, k[3]] for td in (0.3, 0.6, td_max - 1e-6, td_max + 1e-6, 0.62, 1.0, 3.0)])
    got = ref.unproject(ref.FISHEYE, k, uv)
    assert np.isfinite(got[:3]).all() and np.isnan(got[3:]).all()
    th = np.arctan(got[:3, 0])
    assert np.allclose(th * (1 - 0.4 * th * th), [0.3, 0.6, td_max - 1e-6], rtol=1e-14, atol=0) and np.all(th < np.sqrt(1 / 1.2))
    # the same pixels under a polynomial that keeps rising have points; non-finite pixels and a zero focal length have none
    assert np.isfinite(ref.unproject(ref.FISHEYE, fr.TRUE_INTR, uv[:5])).all()
    bad = np.array([[np.nan, 500.0], [800.0, np.inf]])
    assert np.isnan(ref.unproject(ref.FISHEYE, fr.TRUE_INTR, bad)).all() and np.isnan(ref.unproject(ref.RADTAN, RIGK_INTR_TRUE, bad)).all()
    zero_fx = fr.TRUE_INTR.copy()
    zero_fx[0] = 0.0
    assert np.isnan(ref.unproject(ref.FISHEYE, zero_fx, uv[:2])).all()
    # radial-tangential: a barrel map that turns back (k1 = -0.3: x (1 - 0.3 x^2) peaks at 0.7027 for x = 1.054)
    barrel = np.array([600.0, 600.0, 800.0, 500.0, -0.3, 0, 0, 0, 0])
    got = ref.unproject(ref.RADTAN, barrel, np.array([[800.0 + 600.0 * 0.5, 500.0], [800.0 + 600.0 * 0.9, 500.0]]))
    assert np.isfinite(got[0]).all() and np.isnan(got[1]).all()


# ---- 2. planted poses -------------------------------------------------------------------------------------------------------
def _pixels_of(scene, model, intr):
    """float32 pixels of a planted scene (tests/rig_start_ref.plant_scene, no noise) through `model`, and the exact normalised points."""
    frames = np.repeat(np.arange(len(scene["frame_offsets"]) - 1), np.diff(scene["frame_offsets"]))
    X = scene["world_xyz"].reshape(-1, 3)[scene["obs_world"].astype(np.int64)].astype(np.float64)
    uv, exact = np.zeros((len(X), 2)), np.zeros((len(X), 2))
    for i, (f, c) in enumerate(zip(frames, scene["obs_cam"])):
        p = scene["cam_R"][c] @ (scene["frame_R"][f] @ X[i] + scene["frame_t"][f]) + scene["cam_t"][c]
        x, y = p[0] / p[2], p[1] / p[2]
        exact[i] = x, y
        if model == ref.FISHEYE:
            rho = np.hypot(x, y)
            s = float(ref.fisheye_theta_d(intr, np.arctan(rho))) / rho
            uv[i] = intr[0] * x * s + intr[2], intr[1] * y * s + intr[3]
        else:
            uv[i] = ref.radtan_pixel(intr, x, y)
    return uv.astype(np.float32), exact


@pytest.mark.parametrize("model,intr,planar,n", [(ref.FISHEYE, fr.TRUE_INTR, False, 8), (ref.FISHEYE, fr.TRUE_INTR, True, 5),
                                                 (ref.RADTAN, RIGK_INTR_TRUE, False, 6), (ref.RADTAN, RIGK_INTR_TRUE, True, 12)],
                         ids=["fisheye_general", "fisheye_planar", "radtan_general", "radtan_planar"])
def test_start_from_pixels_returns_the_planted_poses(model, intr, planar, n):
    """Bound, as tests/test_rig_start_ref_cpu.py derives it for its planted test: a converged view moves by J^+ (delta uv), so
    |delta pose| <= 2 |delta uv|_2 / sigma_min(J) x (1 + |t|), delta uv = the view's float32 points minus the exact normalised
    points. Here delta uv holds two roundings instead of one -- the pixels' (2^-24 of ~1000 px over a focal length of ~600 .. 1000:
    ~1e-7, carried through the inverse map) and the points' (2^-24 of the point: ~3e-8) -- and is taken from the data as there.
    Cameras: 2 x the worst view bound (x the lever arm for translations); frames: 3 x."""
    scene = rs.plant_scene(3, 4, n, seed=31 + n, planar=planar)
    pix, exact = _pixels_of(scene, model, intr)
    cam_q = np.stack([rs.R_to_quat(R) for R in scene["cam_R"]])
    cq, ct, fq, ft, report, vl, pts = ref.start_from_pixels(model, intr, 3, scene["frame_offsets"], scene["obs_cam"], scene["obs_world"], pix,
                                                            scene["world_xyz"], [1, 0, 0], cam_q=cam_q, cam_t=scene["cam_t"], refine="converged")
    assert pts.dtype == np.float32 and np.abs(pts - exact).max() < 1e-6
    assert report["views_valid"] == 12 and report[("views_planar" if planar else "views_general")] == 12
    assert report["root_camera"] == 0 and report["cameras_unplaced"] == 0 and report["frames_unplaced"] == 0
    views = rs.views_of(scene["frame_offsets"], scene["obs_cam"], scene["obs_world"], pts, scene["world_xyz"])
    worst = 0.0
    for (f, c, X, uv), (_, _, kind, R, t, m) in zip(views, vl):
        Rv, tv, b = _view_bounds(scene, f, c, X, uv)
        err = np.hypot(rs.rot_angle(Rv, R), np.linalg.norm(t - tv))
        lever = 1.0 + np.linalg.norm(tv)
        assert err <= b * lever, (f, c, err, b * lever)
        worst = max(worst, b * lever)
    arm = 1.0 + max(np.linalg.norm(v[4]) for v in vl)
    for c in range(3):
        assert rs.rot_angle(rs.quat_to_R(cq[c]), scene["cam_R"][c]) <= 2 * worst
        assert np.linalg.norm(ct[c] - scene["cam_t"][c]) <= 2 * worst * arm
    for f in range(4):
        assert rs.rot_angle(rs.quat_to_R(fq[f]), scene["frame_R"][f]) <= 3 * worst
        assert np.linalg.norm(ft[f] - scene["frame_t"][f]) <= 3 * worst * arm


# ---- 3. the start leads the solve where the scenario's start leads it ----------------------------------------------------------
YARDSTICK_CASES = ("fisheye_2x12x20", "fisheye_3x8x12_per_camera", "radtan_2x10x6")
# Both runs stop by the same rule at the tight tolerances of the rigk parity tests (function 1e-15, gradient 1e-13, parameter
# 1e-14) from intr0, so each is within the rule's slack of the common minimum. Measured with this reference (the figures the
# test prints; DESIGN 4.16 has the table), scenario start vs reference pixel start from the identity:
#   case                        views  iterations  initial cost     cost (relative)  cam_R (rad)  cam_t     intrinsics
#   fisheye_2x12x20             24     10 / 10     45250 / 5739     8.26e-15         5.49e-17     6.75e-17  1.04e-14
#   fisheye_3x8x12_per_camera   24     12 / 12     66704 / 3894     5.00e-15         4.36e-15     5.94e-16  3.86e-13
#   radtan_2x10x6               20     32 / 61     31746 / 349.1    4.03e-15         5.78e-11     2.03e-10  4.35e-07
# (intrinsics: |difference| / max(|slot|, 1), largest slot). The two fisheye ends agree to rounding; the radial-tangential
# shape, 120 observations for 9 intrinsics, ends along its weakly determined direction (tests/golden/make_rigk.py describes
# it). One set of bounds for all shapes, the largest figure of each column x 10 for the stopping rule's slack, as DESIGN 4.15
# does:
COST_REL, CAM_R_ABS, CAM_T_ABS, INTR_REL = 8.26e-14, 5.78e-10, 2.03e-9, 4.35e-6


def tight_options():
    return po.default_options(max_iterations=1000, function_tolerance=1e-15, gradient_tolerance=1e-13, parameter_tolerance=1e-14)


@functools.lru_cache(maxsize=None)
def yardstick_case(name):
    """(scenario, model id, pixel model of the reference solve, per_camera)"""
    if name == "fisheye_2x12x20":
        return rfr.fisheye_rig_case(2, 12, 20), ref.FISHEYE, fr.fisheye_model, False
    if name == "fisheye_3x8x12_per_camera":
        return rfr.fisheye_rig_case(3, 8, 12, per_camera=True), ref.FISHEYE, fr.fisheye_model, True
    if name == "radtan_2x10x6":      # RIGK_INTR_TRUE: k1 = -0.04 and both tangential terms
        return rigk_case(2, 10, 6), ref.RADTAN, fr.pinhole_model, False
    raise KeyError(name)


def distances(a, b):
    """(relative cost difference, largest camera rotation, largest camera translation difference, largest intrinsics difference
    relative to max(|slot|, 1)) between two results of rigk_solve (or anything laid out like them)."""
    ca, cb = a[6]["final_cost"], b[6]["final_cost"]
    dr = max(rs.rot_angle(rs.quat_to_R(p), rs.quat_to_R(q)) for p, q in zip(a[1], b[1]))
    dt = float(np.abs(np.asarray(a[2]) - np.asarray(b[2])).max())
    ka, kb = np.asarray(a[0], dtype=np.float64), np.asarray(b[0], dtype=np.float64)
    return abs(ca - cb) / ca, dr, dt, float((np.abs(ka - kb) / np.maximum(np.abs(ka), 1.0)).max())


@functools.lru_cache(maxsize=None)
def yardstick(name):
    """(scenario solve, pixel-start solve, report of the reference start) at the tight tolerances, both from intr0."""
    k, model, pixel_model, per_camera = yardstick_case(name)
    P = rfr.problem(k, model=pixel_model, per_camera=per_camera)
    a = rfr.solve_case(k, P, options=tight_options())
    cq, ct, fq, ft, report, _, _ = ref.start_from_pixels(model, k["intr0"], k["cams"], k["frame_offsets"], k["obs_cam"], k["obs_world"],
                                                         k["obs_uv_pix"], k["world_xyz"], k["cam_frozen"])
    b = rfr.rigk_solve(P, k["intr0"], cq, ct, fq, ft, options=tight_options())
    return a, b, report


@pytest.mark.parametrize("name", YARDSTICK_CASES)
def test_solve_from_the_pixel_start_ends_where_the_scenario_start_ends(name):
    k = yardstick_case(name)[0]
    a, b, report = yardstick(name)
    n_views = sum(len(set(k["obs_cam"][k["frame_offsets"][f]:k["frame_offsets"][f + 1]].tolist())) for f in range(len(k["frame_offsets"]) - 1))
    assert report["views_valid"] == n_views and report["views_invalid"] == 0
    assert report["cameras_unplaced"] == 0 and report["frames_unplaced"] == 0
    d = distances(a, b)
    print(f"{name}: {n_views} views; initial cost {a[6]['initial_cost']:.6g} (scenario) / {b[6]['initial_cost']:.6g} (pixel start); final "
          f"{a[6]['final_cost']:.9e} ({a[6]['iterations']} it) / {b[6]['final_cost']:.9e} ({b[6]['iterations']} it): cost rel {d[0]:.2e}, "
          f"cam_R {d[1]:.2e}, cam_t {d[2]:.2e}, intrinsics {d[3]:.2e}")
    assert d[0] <= COST_REL and d[1] <= CAM_R_ABS and d[2] <= CAM_T_ABS and d[3] <= INTR_REL
