"""GPU: start poses of a rig problem WITH INTRINSICS from its pixel observations (cc_rigk_estimate_start / cc_rigk_start_points,
k_rigk_start_unproject in camera_calibrator_amd/csrc/cc_rigk_start.hip) against the 50-digit reference (tests/rigk_start_ref.py),
against the poses-only start on the same points, and end to end against the CPU reference of the solve. Every test calls one of
the new entry points and fails on a library without them."""
import functools

import numpy as np
import pytest

from camera_calibrator_amd import capi
from camera_calibrator_amd.harness import RIGK_INTR_TRUE, rigk_case
from tests import fisheye_ref as fr
from tests import rigk_fisheye_ref as rfr
from tests import rigk_start_ref as ref
from tests.test_rigk_start_ref_cpu import (CAM_R_ABS, CAM_T_ABS, COST_REL, INTR_REL, TURNING, YARDSTICK_CASES, distances, yardstick,
                                           yardstick_case)

pytestmark = pytest.mark.gpu
CC_ERR_STATE = -5
TIGHT = dict(max_iterations=1000, function_tolerance=1e-15, gradient_tolerance=1e-13, parameter_tolerance=1e-14)
RAGGED_VIEWS = (1, 63, 64, 65, 257, 0)   # observations of (frame 0, cameras 0 1 2), (frame 1, cameras 0 1 2): a lane alone, one
#                                          short of a wave, a wave, one more, four passes and a rest, a camera that sees nothing


def _handle(k, model, intr, per_camera=False, frozen=None, masks=0, uv=None):
    """A cc_rigk_* handle of scenario k with `model` and the start intrinsics intr ([9], or [cams, 9] set camera by camera)."""
    p = capi.RigProblem(k["cams"], k["frame_offsets"], k["obs_cam"], k["obs_world"], k["obs_uv_pix"] if uv is None else uv, k["world_xyz"],
                        np.asarray(k["cam_frozen"] if frozen is None else frozen, dtype=np.uint8), huber_a=0.0,
                        with_intrinsics="per_camera" if per_camera else True)
    p.set_model(model)
    intr = np.asarray(intr, dtype=np.float64)
    if intr.ndim == 2:
        for c in range(k["cams"]):
            p.set_camera_intrinsics(c, intr[c], int(np.broadcast_to(masks, (k["cams"],))[c]))
    elif intr.size:
        p.set_intrinsics(intr, int(masks))
    return p


def _same(a, b):
    return all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


def _report_key(rep):
    return {k: (v.tolist() if k == "parent" else v) for k, v in rep.items()}


def _within_one_ulp(got, want):
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    return (got == want) | (got == np.nextafter(want, np.float32(np.inf))) | (got == np.nextafter(want, np.float32(-np.inf)))


# ---- 1. the points ----------------------------------------------------------------------------------------------------------
def _f32_principal_point(K):
    K = np.array(K, dtype=np.float64)
    K[..., 2:4] = K[..., 2:4].astype(np.float32)   # a principal point that a float32 pixel can sit on: the axis itself is reachable
    return K


@functools.lru_cache(maxsize=None)
def _ragged(model, per_camera):
    """(scenario, start intrinsics, reference points): three cameras, two frames cut to RAGGED_VIEWS; the TRUE intrinsics of the
    scene (distortion and, radial-tangential, tangential terms: the root search has work to do); two pixels put on the axis of
    their camera and one on the next float32 pixel beside it."""
    if model == ref.FISHEYE:
        k = rfr._cut(rfr.fisheye_rig_case(3, 2, 257, per_camera=per_camera), RAGGED_VIEWS)
    else:
        k = rfr._cut(dict(rigk_case(3, 2, 257, per_camera=per_camera)), RAGGED_VIEWS)
    intr = _f32_principal_point(k["intr_true"])
    uv = k["obs_uv_pix"].copy()
    cams = k["obs_cam"].astype(np.int64)
    pp = (intr[cams] if per_camera else np.tile(intr, (len(uv), 1)))[:, 2:4].astype(np.float32)
    for i in (5, 100):
        uv[i] = pp[i]
    uv[200] = pp[200][0], np.nextafter(pp[200][1], np.float32(np.inf))
    k = dict(k, obs_uv_pix=uv)
    return k, intr, ref.normalised_points(model, intr, k["obs_cam"], uv)


@pytest.mark.parametrize("per_camera", [False, True], ids=["shared", "per_camera"])
@pytest.mark.parametrize("model", [ref.FISHEYE, ref.RADTAN], ids=["fisheye", "radtan"])
def test_points_match_the_50_digit_inverse(model, per_camera, monkeypatch):
    """Every finite point within one float32 unit in the last place of the reference's float64 root rounded to float32 (the
    double root is far inside a float32 spacing: only the final rounding can differ), the NaN pattern and the count identical,
    the same bits whatever CC_RIG_SWEEP_WG_WAVES says and on a second call."""
    k, intr, want = _ragged(model, per_camera)
    assert np.isfinite(want).all() and [int(np.sum(k["obs_cam"][a:b] == c)) for a, b in zip(k["frame_offsets"][:-1], k["frame_offsets"][1:])
                                        for c in range(3)] == list(RAGGED_VIEWS)
    results = []
    for waves in (None, 1, 4):
        if waves is None:
            monkeypatch.delenv("CC_RIG_SWEEP_WG_WAVES", raising=False)
        else:
            monkeypatch.setenv("CC_RIG_SWEEP_WG_WAVES", str(waves))
        p = _handle(k, model, intr, per_camera)
        rep = p.estimate_start_pixels()
        got, bad = p.start_points()
        if waves is None:
            rep2 = p.estimate_start_pixels()
            got2, bad2 = p.start_points()
            assert got2.tobytes() == got.tobytes() and bad2 == bad and _report_key(rep2) == _report_key(rep)
        results.append((got, bad, rep, p.start_views()))
        p.close()
    got, bad, rep, views = results[0]
    for g2, b2, r2, v2 in results[1:]:
        assert g2.tobytes() == got.tobytes() and b2 == bad and _report_key(r2) == _report_key(rep) and _same(views.values(), v2.values())
    ok = _within_one_ulp(got, want)
    print(f"{len(got)} points: {int((got != want).sum())} coordinates differ from the reference's rounding, {int((~ok).sum())} by more than one unit")
    assert bad == 0 and ok.all()
    # the axis maps to itself; the next pixel beside it stays beside it (the tangential terms move a radial-tangential point off
    # the line by ~p2 y^2, so x is exactly 0 for the fisheye model only)
    assert got[5].tolist() == [0.0, 0.0] and got[100].tolist() == [0.0, 0.0] and 0.0 < got[200][1] < 1e-6
    assert model != ref.FISHEYE or got[200][0] == 0.0
    # the one-point view is invalid for the start, and its point is there
    assert list(views["kind"]) == [0, 2, 2, 2, 2] and (rep["views_invalid"], rep["views_valid"]) == (1, 4)
    one = np.nonzero((k["obs_cam"] == 0) & (np.arange(len(got)) < k["frame_offsets"][1]))[0]
    assert len(one) == 1 and np.isfinite(got[one[0]]).all()


# ---- 2. the twin: the poses-only start on the same points ---------------------------------------------------------------------
@pytest.mark.parametrize("frozen", [[1, 0], [0, 0]], ids=["camera0_frozen", "no_frozen"])
@pytest.mark.parametrize("name", ["fisheye_2x12x20", "radtan_2x10x6"])
def test_pixel_start_is_the_poses_only_start_on_its_points(name, frozen):
    k, model, _, _ = yardstick_case(name)
    intr = fr.TRUE_INTR if model == ref.FISHEYE else RIGK_INTR_TRUE
    rng = np.random.default_rng(7)
    C, F = k["cams"], len(k["frame_offsets"]) - 1
    cq, ct = k["cam_q0"] * rng.uniform(0.5, 2.0, (C, 1)), k["cam_t0"] + rng.normal(size=(C, 3)) * 0.01
    fq, ft = rng.normal(size=(F, 4)), rng.normal(size=(F, 3))
    p = _handle(k, model, intr, frozen=frozen)
    rep = p.estimate_start_pixels(cq, ct, fq, ft)
    pts, bad = p.start_points()
    views, state = p.start_views(), p.get_state(want_cost=False)
    p.close()
    assert bad == 0
    twin = capi.RigProblem(C, k["frame_offsets"], k["obs_cam"], k["obs_world"], pts, k["world_xyz"], np.asarray(frozen, dtype=np.uint8))
    trep = twin.estimate_start(cq, ct, fq, ft)
    tviews, tstate = twin.start_views(), twin.get_state(want_cost=False)
    twin.close()
    assert _report_key(rep) == _report_key(trep) and rep["views_valid"] == 2 * F
    assert rep["root_at_identity"] == (0 if frozen[0] else 1)
    assert sorted(views) == sorted(tviews) and all(views[n].tobytes() == tviews[n].tobytes() for n in views)
    assert _same(state[:4], tstate[:4])


# ---- 3. the state -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fisheye_3x8x12_per_camera", "radtan_2x10x6"])
def test_start_becomes_the_state_and_leaves_the_intrinsics_alone(name):
    k, model, _, per_camera = yardstick_case(name)
    C = k["cams"]
    read = (lambda q: q.get_camera_intrinsics()) if per_camera else (lambda q: q.get_intrinsics())
    p = _handle(k, model, k["intr0"], per_camera)
    # a state before the start, so that the intrinsics can be read: the scenario's
    p.set_state(k["cam_q0"], k["cam_t0"], k["frame_q0"], k["frame_t0"])
    intr_before, model_before = read(p), p.get_model()
    rep = p.estimate_start_pixels(k["cam_q0"], k["cam_t0"])
    assert rep["views_invalid"] == 0 and rep["cameras_unplaced"] == 0 and rep["frames_unplaced"] == 0 and rep["root_camera"] == 0
    pts = p.start_points()[0]
    start = p.get_state(want_cost=True)
    assert read(p).tobytes() == intr_before.tobytes() and p.get_model() == model_before == model
    # the frozen root keeps the caller's pose, bit for bit; every estimated pose is a unit quaternion away from the caller's
    assert start[0][0].tobytes() == k["cam_q0"][0].tobytes() and start[1][0].tobytes() == k["cam_t0"][0].tobytes()
    assert np.allclose(np.linalg.norm(start[0], axis=1), 1.0, atol=1e-12) and np.allclose(np.linalg.norm(start[2], axis=1), 1.0, atol=1e-12)
    assert not np.array_equal(start[2], np.tile([1.0, 0, 0, 0], (len(start[2]), 1)))
    # ... and is what set_state with the read-back poses gives
    p2 = _handle(k, model, k["intr0"], per_camera)
    p2.set_state(*start[:4])
    assert _same(start, p2.get_state(want_cost=True))
    s1, s2 = p.solve(capi.default_options(**TIGHT)), p2.solve(capi.default_options(**TIGHT))
    assert s1["iterations"] == s2["iterations"] and s1["final_cost"] == s2["final_cost"]
    assert _same(p.get_state(want_cost=False)[:4], p2.get_state(want_cost=False)[:4]) and read(p).tobytes() == read(p2).tobytes()
    assert read(p).tobytes() != intr_before.tobytes()
    p2.close()
    # a second start reads the START intrinsics, not what the solve made of them: the same points, the same state
    p.estimate_start_pixels(k["cam_q0"], k["cam_t0"])
    assert p.start_points()[0].tobytes() == pts.tobytes() and _same(start, p.get_state(want_cost=True))
    assert read(p).tobytes() == intr_before.tobytes()
    # reset returns to the started state
    p.solve(capi.default_options(**TIGHT))
    p.reset()
    assert _same(start, p.get_state(want_cost=True)) and read(p).tobytes() == intr_before.tobytes()
    p.close()
    assert C == len(start[0])


# ---- 4. end to end ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", YARDSTICK_CASES)
def test_pixel_start_then_solve_ends_at_the_references_minimum(name):
    """From identity poses and intr0: estimate_start_pixels, then the solve at the tight tolerances, against the reference's
    solve from the SCENARIO's start. Bounds: tests/test_rigk_start_ref_cpu.py (the reference's own distance between its two
    starts x 10)."""
    k, model, _, per_camera = yardstick_case(name)
    want = yardstick(name)[0]
    p = _handle(k, model, k["intr0"], per_camera)
    rep = p.estimate_start_pixels()
    assert rep["views_invalid"] == 0 and rep["cameras_unplaced"] == 0 and rep["frames_unplaced"] == 0
    cost0 = p.eval()
    summary = p.solve(capi.default_options(**TIGHT))
    end = p.get_state(want_cost=True)
    intr = p.get_camera_intrinsics() if per_camera else p.get_intrinsics()
    p.close()
    got = (intr,) + end + (summary,)
    d = distances(want, got)
    print(f"{name}: start cost {cost0:.6g}; reference {want[6]['final_cost']:.9e} ({want[6]['iterations']} it) vs start + solve "
          f"{summary['final_cost']:.9e} ({summary['iterations']} it): cost rel {d[0]:.2e} ({d[0] / COST_REL:.3f} of bound), cam_R {d[1]:.2e} "
          f"({d[1] / CAM_R_ABS:.3f}), cam_t {d[2]:.2e} ({d[2] / CAM_T_ABS:.3f}), intrinsics {d[3]:.2e} ({d[3] / INTR_REL:.3f})")
    assert d[0] <= COST_REL and d[1] <= CAM_R_ABS and d[2] <= CAM_T_ABS and d[3] <= INTR_REL
    # the one-shot call is the same sequence
    one = capi.rigk_estimate(k["cams"], k["frame_offsets"], k["obs_cam"], k["obs_world"], k["obs_uv_pix"], k["world_xyz"], k["cam_frozen"],
                             k["intr0"], model=model, per_camera=per_camera, options=capi.default_options(**TIGHT))
    assert np.asarray(one[0]).tobytes() == np.asarray(intr).tobytes() and _same(one[1:6], end)
    assert one[6]["iterations"] == summary["iterations"] and _report_key(one[7]) == _report_key(rep)


# ---- 5. one pixel without a root ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["beyond_the_turning_point", "nan"])
def test_one_pixel_without_a_root_costs_its_view_only(what):
    k = rfr.fisheye_rig_case(2, 12, 20, half=0.2)   # narrow enough for every pixel to have a root under TURNING (theta_d < 0.6086)
    i = int(k["frame_offsets"][3]) + 7
    f_bad, c_bad = 3, int(k["obs_cam"][i])
    uv = k["obs_uv_pix"].copy()
    if what == "beyond_the_turning_point":
        uv[i] = TURNING[2] + TURNING[0] * 0.7, TURNING[3]
    else:
        uv[i] = np.nan, k["obs_uv_pix"][i][1]
    out = []
    for pix in (k["obs_uv_pix"], uv):
        p = _handle(k, ref.FISHEYE, TURNING, uv=pix)
        rep = p.estimate_start_pixels()
        out.append((rep, p.start_points(), p.start_views()))
        p.close()
    (rep0, (pts0, bad0), v0), (rep1, (pts1, bad1), v1) = out
    assert bad0 == 0 and rep0["views_invalid"] == 0
    assert bad1 == 1 and np.isnan(pts1[i]).all() and np.array_equal(np.isnan(pts1).any(axis=1), np.arange(len(uv)) == i)
    assert np.delete(pts0, i, axis=0).tobytes() == np.delete(pts1, i, axis=0).tobytes()
    assert (rep1["views_invalid"], rep1["views_valid"]) == (1, rep0["views_valid"] - 1)
    hit = (v1["frame"] == f_bad) & (v1["camera"] == c_bad)
    assert hit.sum() == 1 and v1["kind"][hit][0] == 0 and v0["kind"][hit][0] != 0
    for n in v0:
        assert v0[n][~hit].tobytes() == v1[n][~hit].tobytes(), n


# ---- 6. the start intrinsics of the moment ------------------------------------------------------------------------------------
def test_points_follow_the_current_start_intrinsics_of_their_camera_only():
    k, model, _, _ = yardstick_case("fisheye_3x8x12_per_camera")
    p = _handle(k, model, k["intr_true"], per_camera=True)
    p.estimate_start_pixels()
    a = p.start_points()[0]
    changed = k["intr_true"][1].copy()
    changed[0] *= 1.01
    changed[4] *= 0.5
    p.set_camera_intrinsics(1, changed)
    p.estimate_start_pixels()
    b = p.start_points()[0]
    p.close()
    cam1 = k["obs_cam"] == 1
    assert a[~cam1].tobytes() == b[~cam1].tobytes() and np.all(a[cam1] != b[cam1])
    want = ref.normalised_points(model, np.stack([k["intr_true"][0], changed, k["intr_true"][2]]), k["obs_cam"], k["obs_uv_pix"])
    assert _within_one_ulp(b, want).all()


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------
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
    _refused(p.estimate_start_pixels, "cc_rig_estimate_start")
    _refused(p.start_points)
    assert _same(before[:4], p.get_state(want_cost=False)[:4])
    p.close()
    # no intrinsics yet
    p = _handle(k, ref.RADTAN, np.zeros(0))
    p.set_state(*poses)
    before = p.get_state(want_cost=False)
    _refused(p.estimate_start_pixels, "cc_rigk_set_intrinsics")
    _refused(p.start_points)
    assert _same(before[:4], p.get_state(want_cost=False)[:4])
    # ... and none any more after a change of the model; the old entry point still refuses the handle
    p.set_intrinsics(K)
    _refused(p.estimate_start, "cc_rigk_estimate_start")
    _refused(p.start_points)
    p.set_model(ref.FISHEYE)
    before = p.get_state(want_cost=False)
    _refused(p.estimate_start_pixels, "cc_rigk_set_intrinsics")
    _refused(p.start_points)
    assert _same(before[:4], p.get_state(want_cost=False)[:4]) and p.get_model() == ref.FISHEYE
    p.close()
    # an exchange attached (a single rank is a valid, degenerate exchange)
    p = _handle(k, ref.RADTAN, k["intr0"])
    p.set_state(*poses)
    p.exchange_attach(0, [p.exchange_export()])
    before = p.get_state(want_cost=False)
    _refused(p.estimate_start_pixels, "exchange")
    _refused(p.start_points)
    assert _same(before[:4], p.get_state(want_cost=False)[:4]) and p.get_intrinsics().tobytes() == k["intr0"].tobytes()
    p.close()


def test_intrinsics_without_any_point_are_not_an_error():
    k = dict(rigk_case(2, 10, 6))
    rng = np.random.default_rng(3)
    cq, ct = rng.normal(size=(2, 4)), rng.normal(size=(2, 3))
    fq, ft = rng.normal(size=(10, 4)), rng.normal(size=(10, 3))
    bad = k["intr0"].copy()
    bad[0] = 0.0
    p = _handle(k, ref.RADTAN, bad, frozen=[0, 0])
    rep = p.estimate_start_pixels(cq, ct, fq, ft)
    pts, n = p.start_points()
    state = p.get_state(want_cost=False)
    kinds = p.start_views()["kind"]
    p.close()
    assert n == len(pts) and np.isnan(pts).all() and not kinds.any()
    assert (rep["views_valid"], rep["views_invalid"], rep["cameras_placed"], rep["frames_placed"], rep["root_camera"]) == (0, 20, 0, 0, -1)
    assert _same(state[:4], (cq, ct, fq, ft))
