"""GPU: start poses of a rig problem WITH INTRINSICS from its pixels as UNIT BEARINGS, for points at and beyond 90 degrees off the
axis (cc_rigk_estimate_start_bearing / cc_rigk_start_bearings; k_rigk_start_bearing in camera_calibrator_amd/csrc/cc_rigk_start.hip,
k_rig_start_view_bearing in cc_rig_start_bearing.hip) against the reference (tests/rigk_bearing_ref.py), stage by stage and end to
end against the CPU reference of the solve. Every test calls one of the new entry points and fails on a library without them."""
import functools

import numpy as np
import pytest

from camera_calibrator_amd import capi
from camera_calibrator_amd.harness import RIGK_INTR_TRUE, rigk_case
from tests import fisheye_ref as fr
from tests import rig_start_ref as rs
from tests import rigk_bearing_ref as ref
from tests import rigk_fisheye_ref as rfr
from tests.test_rigk_bearing_ref_cpu import CAM_R_ABS, CAM_T_ABS, COST_REL, INTR_REL, WIDE_CASES, wide_case, wide_yardstick
from tests.test_rigk_start_ref_cpu import distances

pytestmark = pytest.mark.gpu
CC_ERR_STATE = -5
TIGHT = dict(max_iterations=1000, function_tolerance=1e-15, gradient_tolerance=1e-13, parameter_tolerance=1e-14)
RAGGED_VIEWS = (1, 63, 64, 65, 257, 0)   # observations of (frame 0, cameras 0 1 2), (frame 1, cameras 0 1 2): a lane alone, one
#                                          short of a wave, a wave, one more, four passes and a rest, a camera that sees nothing


def _handle(k, model, intr, per_camera=False, frozen=None, uv=None):
    """A cc_rigk_* handle of scenario k with `model` (one, or a sequence of one per camera: a mixed handle) and the start
    intrinsics intr ([9], or [cams, 9] set camera by camera; empty: none)."""
    mixed = not np.isscalar(model)
    p = capi.RigProblem(k["cams"], k["frame_offsets"], k["obs_cam"], k["obs_world"], k["obs_uv_pix"] if uv is None else uv, k["world_xyz"],
                        np.asarray(k["cam_frozen"] if frozen is None else frozen, dtype=np.uint8), huber_a=0.0,
                        with_intrinsics="per_camera" if per_camera or mixed else True)
    if mixed:
        for c, m in enumerate(model):
            p.set_camera_model(c, int(m))
    else:
        p.set_model(model)
    intr = np.asarray(intr, dtype=np.float64)
    if intr.ndim == 2:
        for c in range(k["cams"]):
            p.set_camera_intrinsics(c, intr[c], 0)
    elif intr.size:
        p.set_intrinsics(intr, 0)
    return p


def _same(a, b):
    return all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


def _report_key(rep):
    return {k: (v.tolist() if k == "parent" else v) for k, v in rep.items()}


def _device_views(k, bearings):
    """The scenario's views with the DEVICE's bearings: what the reference's stages V and R are run on next to the kernel's."""
    return ref.views_of(k["frame_offsets"], k["obs_cam"], k["obs_world"], bearings, k["world_xyz"])


def _route_yardstick(views):
    """16 x the largest difference between the reference's SVD and Gram routes on these views (rotation in radians, translation in
    metres), floor 1e-12: the rule of tests/test_gpu_rig_start.py for the kernel's closed form, which takes the Gram route."""
    dr = dt = 0.0
    for _, _, X, b in views:
        ka, Ra, ta = ref.view_closed_form(X, b, "svd")
        kb, Rb, tb = ref.view_closed_form(X, b, "gram")
        if ka != ref.INVALID and kb != ref.INVALID:
            dr, dt = max(dr, rs.rot_angle(Ra, Rb)), max(dt, np.linalg.norm(ta - tb))
    return max(16 * dr, 1e-12), max(16 * dt, 1e-12), dr, dt


# ---- 1. the bearings ----------------------------------------------------------------------------------------------------------
def _f32_principal_point(K):
    K = np.array(K, dtype=np.float64)
    K[..., 2:4] = K[..., 2:4].astype(np.float32)   # a principal point that a float32 pixel can sit on: the axis itself is reachable
    return K


@functools.lru_cache(maxsize=None)
def _ragged(name):
    """(scenario, model(s), per_camera, start intrinsics, reference bearings): three cameras, two frames cut to RAGGED_VIEWS, the TRUE
    intrinsics of the scene; two pixels put on the axis of their camera and one on the next float32 pixel beside it.
    fisheye: a wide scene (x, y +-3 m, z +-1 m about 0.6 - 1.2 m), so that both hemispheres occur; radtan: rigk_case;
    mixed: rigk_case's pixels with camera 1 read as a fisheye camera under the fisheye scenes' intrinsics."""
    per_camera = name.endswith("per_camera") or name == "mixed"
    if name.startswith("fisheye"):
        k = rfr._cut(ref.wide_rig_case(3, 2, 257, per_camera=per_camera, half=3.0, zhalf=1.0), RAGGED_VIEWS)
        model, intr = ref.FISHEYE, _f32_principal_point(k["intr_true"])
    else:
        k = rfr._cut(dict(rigk_case(3, 2, 257, per_camera=per_camera)), RAGGED_VIEWS)
        model, intr = ref.RADTAN, _f32_principal_point(k["intr_true"])
        if name == "mixed":
            model = (ref.RADTAN, ref.FISHEYE, ref.RADTAN)
            intr[1] = _f32_principal_point(fr.TRUE_INTR)
    uv = k["obs_uv_pix"].copy()
    cams = k["obs_cam"].astype(np.int64)
    pp = (intr[cams] if per_camera else np.tile(intr, (len(uv), 1)))[:, 2:4].astype(np.float32)
    for i in (5, 100):
        uv[i] = pp[i]
    uv[200] = pp[200][0], np.nextafter(pp[200][1], np.float32(np.inf))
    k = dict(k, obs_uv_pix=uv)
    return k, model, per_camera, intr, ref.bearing_vectors(model, intr, k["obs_cam"], uv)


def _component_ok(got, want):
    """Per component: within one float32 unit in the last place of the reference's component, or within 2^-40 absolute -- a unit
    bearing's direction resolves 6e-8 in float32 and the fp64 root is good to ~1e-15; 2^-40 sits between the two and only excuses
    components that are numerically zero (whose own last place is far finer than the direction resolves)."""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    ulp = (got == want) | (got == np.nextafter(want, np.float32(np.inf))) | (got == np.nextafter(want, np.float32(-np.inf)))
    return ulp | (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= 2.0 ** -40)


@pytest.mark.parametrize("name", ["fisheye_shared", "fisheye_per_camera", "radtan_shared", "radtan_per_camera", "mixed"])
def test_bearings_match_the_50_digit_inverse(name, monkeypatch):
    k, model, per_camera, intr, want = _ragged(name)
    assert np.isfinite(want).all() and [int(np.sum(k["obs_cam"][a:b] == c)) for a, b in zip(k["frame_offsets"][:-1], k["frame_offsets"][1:])
                                        for c in range(3)] == list(RAGGED_VIEWS)
    if name.startswith("fisheye"):
        assert (want[:, 2] < -0.05).sum() > 10 and (want[:, 2] > 0.05).sum() > 10   # both hemispheres
    results = []
    for waves in (None, 1, 4):
        if waves is None:
            monkeypatch.delenv("CC_RIG_SWEEP_WG_WAVES", raising=False)
        else:
            monkeypatch.setenv("CC_RIG_SWEEP_WG_WAVES", str(waves))
        p = _handle(k, model, intr, per_camera)
        rep = p.estimate_start_bearings()
        got, bad = p.start_bearings()
        if waves is None:
            rep2 = p.estimate_start_bearings()
            got2, bad2 = p.start_bearings()
            assert got2.tobytes() == got.tobytes() and bad2 == bad and _report_key(rep2) == _report_key(rep)
        results.append((got, bad, rep, p.start_views()))
        p.close()
    got, bad, rep, views = results[0]
    for g2, b2, r2, v2 in results[1:]:
        assert g2.tobytes() == got.tobytes() and b2 == bad and _report_key(r2) == _report_key(rep) and _same(views.values(), v2.values())
    ok = _component_ok(got, want)
    far = np.abs(got.astype(np.float64) - want.astype(np.float64)).max()
    print(f"{name}: {len(got)} bearings, {int((got != want).sum())} components differ from the reference's rounding (largest difference "
          f"{far:.2e}), {int((~ok).sum())} by more than the criterion allows")
    assert bad == 0 and got.shape == want.shape and ok.all()
    assert np.abs(np.linalg.norm(got.astype(np.float64), axis=1) - 1.0).max() < 1.2e-7
    # the axis gives exactly (0, 0, 1); the next pixel beside it stays beside it (the tangential terms move a radial-tangential
    # point off the line by ~p2 y^2, so x is exactly 0 for a fisheye camera only)
    assert got[5].tolist() == [0.0, 0.0, 1.0] and got[100].tolist() == [0.0, 0.0, 1.0] and 0.0 < got[200][1] < 1e-6 and got[200][2] == 1.0
    fish200 = (model if np.isscalar(model) else model[int(k["obs_cam"][200])]) == ref.FISHEYE
    assert not fish200 or got[200][0] == 0.0
    # the one-point view is invalid for the start, and its bearing is there
    assert list(views["kind"]) == [0, 2, 2, 2, 2] and (rep["views_invalid"], rep["views_valid"]) == (1, 4)
    one = np.nonzero((k["obs_cam"] == 0) & (np.arange(len(got)) < k["frame_offsets"][1]))[0]
    assert len(one) == 1 and np.isfinite(got[one[0]]).all()


# ---- 2. the closed form -------------------------------------------------------------------------------------------------------
# one camera, one view per frame (tests/rigk_bearing_ref.plant_views): 4 and 5 coplanar points, 6 and 7 general ones, 64 / 65 / 130
# points (one pass of the wave, one more observation, two passes and a rest) of both kinds; a view of each kind with half its
# points beyond 90 degrees; a board whose centre lies behind the camera's plane (the sign rule)
CLOSED_FORM_SPECS = (("board", 4), ("board", 5), ("board", 64), ("board", 65), ("board", 130), ("general", 6), ("general", 7), ("general", 64),
                     ("general", 65), ("general", 130), ("general_wide", 40), ("board_wide", 30), ("board_cut", 30))
CLOSED_FORM_KINDS = [1] * 5 + [2] * 5 + [2, 1, 1]


def _start_views(sc, refine_iterations, uv=None):
    p = _handle(sc, ref.FISHEYE, sc["intr"], uv=uv)
    rep = p.estimate_start_bearings(refine_iterations=refine_iterations)
    out = rep, p.start_bearings(), p.start_views()
    p.close()
    return out


def test_closed_form_matches_the_reference():
    """refine_iterations = 0: the closed form as it is, against the reference's SVD route on the device's own bearings (test 1 holds
    those against the 50-digit inverse). Bound: 16 x the reference's SVD-to-Gram distance on the same views."""
    sc = ref.plant_views(CLOSED_FORM_SPECS, seed=11)
    rep, (bearings, bad), got = _start_views(sc, 0)
    assert bad == 0 and list(got["kind"]) == CLOSED_FORM_KINDS and list(got["frame"]) == list(range(len(CLOSED_FORM_SPECS)))
    assert (rep["views_planar"], rep["views_general"], rep["views_invalid"]) == (7, 6, 0)
    views = _device_views(sc, bearings)
    behind = [int((v[3][:, 2] < 0).sum()) for v in views]
    assert behind[10] == 20 and behind[11] == 15 and behind[12] > 15 and not any(behind[:10])
    bound_r, bound_t, dr, dt = _route_yardstick(views)
    worst_r = worst_t = 0.0
    for i, (_, _, X, b) in enumerate(views):
        kind, R, t = ref.view_closed_form(X, b, "svd")
        Rg = rs.quat_to_R(got["q"][i])
        assert kind == CLOSED_FORM_KINDS[i]
        worst_r, worst_t = max(worst_r, rs.rot_angle(R, Rg)), max(worst_t, np.linalg.norm(t - got["t"][i]))
        # the kernel's rms^2 is the reference's chord at the kernel's own pose
        assert got["rms2"][i] == pytest.approx(ref.rms2(Rg, got["t"][i], X, b), rel=1e-9)
    # (that the reference's closed form returns a planted pose on either side of the camera's plane is pinned on the CPU,
    # tests/test_rigk_bearing_ref_cpu.py; with 0.3 px of noise a minimal view of four points is not near it by any fixed margin)
    print(f"SVD vs Gram route {dr:.2e} rad / {dt:.2e} m; kernel vs SVD {worst_r:.2e} rad ({worst_r / bound_r:.3f} of bound) / {worst_t:.2e} m "
          f"({worst_t / bound_t:.3f} of bound)")
    assert worst_r <= bound_r and worst_t <= bound_t


def test_invalid_views_are_counted_and_leave_the_other_views_alone():
    """Three points, five points that span space, collinear points, one NaN pixel: each view invalid and counted, every other
    view's record bit-identical to a run without them."""
    valid = (("general", 8), ("board", 9), ("general_wide", 40))
    dirty = ref.plant_views(valid[:1] + (("three", 3), ("five", 5)) + valid[1:2] + (("line", 7), ("general", 12)) + valid[2:], seed=12)
    clean = ref.plant_views(valid, seed=12)
    uv = dirty["obs_uv_pix"].copy()
    uv[int(dirty["frame_offsets"][5]) + 2, 1] = np.nan
    rd, (bd, nd), vd = _start_views(dirty, 10, uv=uv)
    rc, (bc, nc), vc = _start_views(clean, 10)
    assert list(vd["kind"]) == [2, 0, 0, 1, 0, 0, 2] and list(vc["kind"]) == [2, 1, 2]
    assert (rd["views_invalid"], rd["views_valid"], rd["views_planar"], rd["views_general"]) == (4, 3, 1, 2) and rc["views_invalid"] == 0
    assert (nd, nc) == (1, 0) and np.array_equal(np.isnan(bd).all(axis=1), np.isnan(bd).any(axis=1)) and np.isnan(bd[int(dirty["frame_offsets"][5]) + 2]).all()
    keep = np.array([0, 3, 6])
    for n in ("kind", "q", "t", "rms2"):
        assert vd[n][keep].tobytes() == vc[n].tobytes(), n
        assert not np.asarray(vd[n])[[1, 2, 4, 5]].any(), n


# ---- 3. the refinement --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["wide_3x8x12_per_camera", "boards_2x8x30_per_camera"])
def test_refined_views_match_the_converged_reference(name):
    """Ten specified steps on the device against scipy's least_squares on the same chord from the reference's closed form, on the
    device's bearings. Bound: 16 x (the reference's ten steps against least_squares), over the views whose ten steps have
    converged (thirty end within 1e-8 of them) -- the rule of tests/test_gpu_rig_start.py."""
    k = wide_case(name)
    p = _handle(k, ref.FISHEYE, k["intr_true"], per_camera=True)
    p.estimate_start_bearings(refine_iterations=10)
    bearings, bad = p.start_bearings()
    got = p.start_views()
    p.close()
    views = _device_views(k, bearings)
    assert bad == 0 and (bearings[:, 2] < 0).mean() >= 0.05
    rows = []
    for i, (_, _, X, b) in enumerate(views):
        kind, R0, t0 = ref.view_closed_form(X, b)
        Ra, ta = ref.refine_lm(R0, t0, X, b, 10)
        Rb, tb = ref.refine_lm(R0, t0, X, b, 30)
        if rs.rot_angle(Ra, Rb) > 1e-8 or np.linalg.norm(ta - tb) > 1e-8:
            continue
        Rc, tc = ref.refine_converged(R0, t0, X, b)
        rows.append((i, Rc, tc, rs.rot_angle(Ra, Rc), np.linalg.norm(ta - tc)))
    assert len(rows) >= 0.9 * len(views), (len(rows), len(views))
    bound_r, bound_t = 16 * max(r[3] for r in rows), 16 * max(r[4] for r in rows)
    worst_r = max(rs.rot_angle(Rc, rs.quat_to_R(got["q"][i])) for i, Rc, tc, _, _ in rows)
    worst_t = max(np.linalg.norm(tc - got["t"][i]) for i, Rc, tc, _, _ in rows)
    print(f"{name}: {len(rows)} of {len(views)} views; reference LM vs least_squares {bound_r / 16:.2e} rad / {bound_t / 16:.2e} m; "
          f"kernel vs least_squares {worst_r:.2e} rad ({worst_r / bound_r:.3f} of bound) / {worst_t:.2e} m ({worst_t / bound_t:.3f} of bound)")
    assert all(got["kind"][i] == (1 if name.startswith("boards") else 2) for i in range(len(views)))
    assert worst_r <= bound_r and worst_t <= bound_t
    for i, _, _, _, _ in rows:
        assert got["rms2"][i] == pytest.approx(ref.rms2(rs.quat_to_R(got["q"][i]), got["t"][i], views[i][2], views[i][3]), rel=1e-9)


# ---- 4. stages C and F, and the state -------------------------------------------------------------------------------------------
def test_poses_are_the_reference_means_and_become_the_state(monkeypatch):
    monkeypatch.setenv("CC_RIG_PERSIST", "0")   # bits are compared in the three-kernel form (tests/test_gpu_rig_start.py says why)
    name = "wide_3x8x12_per_camera"
    k = wide_case(name)
    C, F = k["cams"], len(k["frame_offsets"]) - 1
    rng = np.random.default_rng(43)
    # the caller's poses: the scenario's for the frozen camera, arbitrary (and unnormalised) ones elsewhere
    cq, ct = k["cam_q0"] * rng.uniform(0.5, 2.0, (C, 1)), k["cam_t0"] + np.where(np.asarray(k["cam_frozen"], dtype=bool)[:, None], 0.0, rng.normal(size=(C, 3)))
    fq, ft = rng.normal(size=(F, 4)), rng.normal(size=(F, 3))
    p = _handle(k, ref.FISHEYE, k["intr0"], per_camera=True)
    p.set_state(k["cam_q0"], k["cam_t0"], k["frame_q0"], k["frame_t0"])   # a state, so that the intrinsics can be read
    intr_before, model_before = p.get_camera_intrinsics(), p.get_model()
    rep = p.estimate_start_bearings(cq, ct, fq, ft)
    bearings = p.start_bearings()[0]
    got, start = p.start_views(), p.get_state(want_cost=True)
    assert rep["views_invalid"] == 0 and rep["cameras_unplaced"] == 0 and rep["frames_unplaced"] == 0 and rep["root_camera"] == 0
    assert p.get_camera_intrinsics().tobytes() == intr_before.tobytes() and p.get_model() == model_before == ref.FISHEYE
    # stages T, C and F of the reference on the DEVICE's view results, within the closed form's bound on these views
    vl = [(int(f), int(c), int(kd), rs.quat_to_R(q) if kd else None, t, m)
          for f, c, kd, q, t, m in zip(got["frame"], got["camera"], got["kind"], got["q"], got["t"], got["rms2"])]
    rq, rt, rfq, rft, rrep = rs.poses_from_views(C, F, vl, k["cam_frozen"], cq, ct, fq, ft)
    assert rep["root_camera"] == rrep["root_camera"] and list(rep["parent"]) == rrep["parent"] and bool(rep["root_at_identity"]) == rrep["root_at_identity"]
    bound_r, bound_t, _, _ = _route_yardstick(_device_views(k, bearings))
    worst = 0.0
    for a, b, ta, tb in list(zip(start[0], rq, start[1], rt)) + list(zip(start[2], rfq, start[3], rft)):
        worst = max(worst, rs.rot_angle(rs.quat_to_R(a), rs.quat_to_R(b)) / bound_r, np.linalg.norm(ta - tb) / bound_t)
    print(f"{name}: device means vs reference means, worst fraction of the bound ({bound_r:.2e} rad, {bound_t:.2e} m) {worst:.1e}")
    assert worst <= 1.0
    # the frozen root keeps the caller's pose, bit for bit
    assert start[0][0].tobytes() == cq[0].tobytes() and start[1][0].tobytes() == ct[0].tobytes()
    # the state is what set_state with the read-back poses gives, through a solve
    p2 = _handle(k, ref.FISHEYE, k["intr0"], per_camera=True)
    p2.set_state(*start[:4])
    assert _same(start, p2.get_state(want_cost=True))
    s1, s2 = p.solve(capi.default_options(**TIGHT)), p2.solve(capi.default_options(**TIGHT))
    assert s1["iterations"] == s2["iterations"] and s1["final_cost"] == s2["final_cost"]
    assert _same(p.get_state(want_cost=False)[:4], p2.get_state(want_cost=False)[:4])
    assert p.get_camera_intrinsics().tobytes() == p2.get_camera_intrinsics().tobytes() != intr_before.tobytes()
    p2.close()
    # a start after a solve reads the START intrinsics again: the same bearings, the same state
    p.estimate_start_bearings(cq, ct, fq, ft)
    assert p.start_bearings()[0].tobytes() == bearings.tobytes() and _same(start, p.get_state(want_cost=True))
    assert p.get_camera_intrinsics().tobytes() == intr_before.tobytes()
    # reset returns to the started state
    p.solve(capi.default_options(**TIGHT))
    p.reset()
    assert _same(start, p.get_state(want_cost=True)) and p.get_camera_intrinsics().tobytes() == intr_before.tobytes() and p.get_model() == model_before
    p.close()


# ---- 5. end to end ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(WIDE_CASES))
def test_bearing_start_then_solve_ends_at_the_references_minimum(name, monkeypatch):
    """From identity poses and intr0: estimate_start_bearings, then the solve at the tight tolerances (three-kernel form), against the
    reference's solve from the SCENARIO's start. Bounds: tests/test_rigk_bearing_ref_cpu.py (the reference's own distance between
    its two starts x 10)."""
    monkeypatch.setenv("CC_RIG_PERSIST", "0")
    k, per_camera = wide_case(name), WIDE_CASES[name]["per_camera"]
    want = wide_yardstick(name)[0]
    p = _handle(k, ref.FISHEYE, k["intr0"], per_camera)
    rep = p.estimate_start_bearings()
    assert rep["views_invalid"] == 0 and rep["cameras_unplaced"] == 0 and rep["frames_unplaced"] == 0 and p.start_bearings()[1] == 0
    assert rep["views_planar" if name.startswith("boards") else "views_general"] == rep["views_valid"]
    cost0 = p.eval()
    summary = p.solve(capi.default_options(**TIGHT))
    end = p.get_state(want_cost=True)
    intr = p.get_camera_intrinsics() if per_camera else p.get_intrinsics()
    p.close()
    d = distances(want, (intr,) + end + (summary,))
    print(f"{name}: start cost {cost0:.6g}; reference {want[6]['final_cost']:.9e} ({want[6]['iterations']} it) vs start + solve "
          f"{summary['final_cost']:.9e} ({summary['iterations']} it): cost rel {d[0]:.2e} ({d[0] / COST_REL:.3f} of bound), cam_R {d[1]:.2e} "
          f"({d[1] / CAM_R_ABS:.3f}), cam_t {d[2]:.2e} ({d[2] / CAM_T_ABS:.3f}), intrinsics {d[3]:.2e} ({d[3] / INTR_REL:.3f})")
    assert d[0] <= COST_REL and d[1] <= CAM_R_ABS and d[2] <= CAM_T_ABS and d[3] <= INTR_REL
    # the one-shot call is the same sequence
    one = capi.rigk_estimate(k["cams"], k["frame_offsets"], k["obs_cam"], k["obs_world"], k["obs_uv_pix"], k["world_xyz"], k["cam_frozen"],
                             k["intr0"], model=ref.FISHEYE, per_camera=per_camera, options=capi.default_options(**TIGHT), start="bearing")
    assert np.asarray(one[0]).tobytes() == np.asarray(intr).tobytes() and _same(one[1:6], end)
    assert one[6]["iterations"] == summary["iterations"] and _report_key(one[7]) == _report_key(rep)


# ---- 6. refusals and bookkeeping ------------------------------------------------------------------------------------------------
def _refused(call, *needles):
    with pytest.raises(capi.CcError) as e:
        call()
    assert "cc error %d" % CC_ERR_STATE in str(e.value) and all(n in str(e.value) for n in needles), str(e.value)


def test_refusals_leave_the_handle_as_it_was():
    k = dict(rigk_case(2, 10, 6))
    poses = (k["cam_q0"], k["cam_t0"], k["frame_q0"], k["frame_t0"])
    K = RIGK_INTR_TRUE
    # a poses-only handle: the message names the call that is meant for it
    uvn = ((k["obs_uv_pix"] - K[2:4]) / K[:2]).astype(np.float32)
    p = capi.RigProblem(2, k["frame_offsets"], k["obs_cam"], k["obs_world"], uvn, k["world_xyz"], k["cam_frozen"])
    p.set_state(*poses)
    before = p.get_state(want_cost=False)
    _refused(p.estimate_start_bearings, "cc_rig_estimate_start")
    _refused(p.start_bearings)
    assert _same(before[:4], p.get_state(want_cost=False)[:4])
    p.close()
    # no intrinsics yet
    p = _handle(k, ref.RADTAN, np.zeros(0))
    p.set_state(*poses)
    before = p.get_state(want_cost=False)
    _refused(p.estimate_start_bearings, "cc_rigk_set_intrinsics")
    _refused(p.start_bearings)
    assert _same(before[:4], p.get_state(want_cost=False)[:4])
    p.close()
    # a camera whose model changed since its intrinsics were set
    p = _handle(k, ref.RADTAN, np.tile(k["intr0"], (2, 1)), per_camera=True)
    p.set_state(*poses)
    p.set_camera_model(1, ref.FISHEYE)
    before = p.get_state(want_cost=False)
    _refused(p.estimate_start_bearings, "cc_rigk_set_intrinsics")
    _refused(p.start_bearings)
    assert _same(before[:4], p.get_state(want_cost=False)[:4]) and p.get_model() == capi.MODEL_MIXED
    p.close()
    with pytest.raises(ValueError, match="start"):
        capi.rigk_estimate(2, k["frame_offsets"], k["obs_cam"], k["obs_world"], k["obs_uv_pix"], k["world_xyz"], k["cam_frozen"], k["intr0"], start="chord")


def test_each_start_reads_back_its_own_buffer_only():
    """start_bearings before a bearing start and after a pixel start, start_points after a bearing start: CC_ERR_STATE; and
    cc_rigk_estimate_start after a bearing start on the same handle returns the bits a fresh handle gives."""
    k = rfr.fisheye_rig_case(2, 12, 20)
    fresh = _handle(k, ref.FISHEYE, k["intr0"])
    frep = fresh.estimate_start_pixels()
    want = fresh.start_points(), fresh.start_views(), fresh.get_state(want_cost=True)
    _refused(fresh.start_bearings, "cc_rigk_estimate_start_bearing")
    fresh.close()
    p = _handle(k, ref.FISHEYE, k["intr0"])
    _refused(p.start_bearings, "cc_rigk_estimate_start_bearing")
    _refused(p.start_points)
    brep = p.estimate_start_bearings()
    b, bad = p.start_bearings()
    bviews = p.start_views()
    assert bad == 0 and brep["views_valid"] == 24 and np.isfinite(b).all()
    _refused(p.start_points, "cc_rigk_start_bearings")
    rep = p.estimate_start_pixels()
    got = p.start_points(), p.start_views(), p.get_state(want_cost=True)
    _refused(p.start_bearings, "cc_rigk_estimate_start_bearing")
    p.close()
    assert _report_key(rep) == _report_key(frep) and got[0][0].tobytes() == want[0][0].tobytes() and got[0][1] == want[0][1]
    assert _same(got[1].values(), want[1].values()) and _same(got[2], want[2])
    # inside 90 degrees the two forms see the same views: the same kinds, poses within the noise of each other
    assert list(bviews["kind"]) == list(got[1]["kind"]) and np.abs(bviews["t"] - got[1]["t"]).max() < 0.05
