"""GPU: the fisheye focal-length start (cc_intrinsics_estimate_start_fisheye, cc_intrinsics_start_scores,
cc_intrinsics_estimate_views_start; k_intr_start_extent / _view / _pick in camera_calibrator_amd/csrc/cc_intr_start.hip) against its
numpy reference (tests/intr_start_ref.py), stage by stage, and end to end against the CPU reference of the solve
(tests/fisheye_ref.lm_solve). Every test calls one of the new entry points and fails on a library without them; the scenes, the
yardstick and its bounds are tests/test_intr_start_ref_cpu.py's."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from camera_calibrator_amd import capi
from tests import fisheye_ref as fr
from tests import intr_start_ref as ref
from tests import rig_start_ref as rs
from tests.test_intr_start_ref_cpu import COST_REL, INTR_REL, ROT_ABS, SCENES, T_ABS, distances, scene_of, start_of, truth_solve

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "camera_calibrator_amd"))
pytestmark = pytest.mark.gpu
FISH = capi.MODEL_FISHEYE
CC_ERR_BAD_ARGUMENT, CC_ERR_STATE = -1, -5
TIGHT = dict(max_iterations=1000, function_tolerance=1e-15, gradient_tolerance=1e-13, parameter_tolerance=1e-14)
STRIDE, COST_SLOT, KIND_SLOT = 24, 17, 18


def _problem(c, uv=None, model=FISH):
    p = capi.IntrinsicsProblem(c["off"], c["uv"] if uv is None else uv, c["xyz"])
    if model:
        p.set_model(model)
    return p


def _fetch(p, name, n):
    buf = np.zeros(n)
    capi._check(capi.lib().cc_intrinsics_debug_fetch(p._h, name, buf.ctypes.data_as(C.POINTER(C.c_double)), C.c_int64(n)))
    return buf.reshape(-1, STRIDE)


def _rc(fn):
    """The status a call ends with (0: it went through)."""
    try:
        fn()
    except capi.CcError as e:
        return int(str(e).split()[2].rstrip(":"))
    return 0


def _bits(*arrays):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)


# ---- 1. extent ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_nan", [False, True])
def test_extent_is_numpys_on_the_float32_pixels(with_nan):
    """Bounding-box centre and r_max, bit for bit -- min and max have no rounding, the distance is one fp64 expression without a
    fused product -- with one NaN pixel left out of both; and r_max about a centre the caller gives. 1296 pixels: six workgroups."""
    c = scene_of("95deg_seed3")   # 12 views of 36 points
    rng = np.random.default_rng(5)
    uv = np.concatenate([c["uv"]] * 3) + rng.uniform(-3, 3, (1296, 2)).astype(np.float32)
    uv[432:864] *= np.float32(-1)   # (negative coordinates too)
    off = np.array([0, 432, 864, 1296], dtype=np.int64)
    xyz = np.concatenate([c["xyz"]] * 3)
    if with_nan:
        uv[int(np.argmax(uv[:, 0])), 1] = np.nan   # the pixel that would set the box's right edge
    p = _problem(dict(off=off, uv=uv, xyz=xyz))
    _, _, _, rep = p.estimate_start_fisheye(candidates=1, search_views=1, refine_iterations=0)
    centre, r_max = ref.extent(uv)
    assert _bits(rep["centre"][0], rep["centre"][1], rep["r_max"]) == _bits(centre[0], centre[1], r_max), (rep, centre, r_max)
    given = (801.25, 498.5)
    _, _, _, rep = p.estimate_start_fisheye(candidates=1, search_views=1, refine_iterations=0, centre=given)
    p.close()
    assert rep["centre"] == given and _bits(rep["r_max"]) == _bits(ref.extent(uv, given)[1])


# ---- 2. the pairs ---------------------------------------------------------------------------------------------------------------
def _pairs_run(C_, refine):
    c = ref.pairs_scene()
    p = _problem(c)
    intr, q, t, rep = p.estimate_start_fisheye(candidates=C_, search_views=0, refine_iterations=refine, centre=tuple(c["centre"]))
    f, score, qualified = p.start_scores()
    rec = _fetch(p, b"start_records", C_ * 8 * STRIDE).reshape(C_, 8, STRIDE)
    views = _fetch(p, b"start_views", 8 * STRIDE)
    p.close()
    return c, dict(intr=intr, q=q, t=t, report=rep, f=f, score=score, qualified=qualified, rec=rec, views=views)


@pytest.mark.parametrize("C_", [1, 2, 24])
def test_closed_form_pairs_match_the_reference(C_):
    """refine_iterations = 0 on boards of the ragged counts (4, 9, 25, 64, 65, 144 points; rectangular, so that the closed form is
    defined: intr_start_ref.pairs_scene says why) and two general views (6, 65): every (view,
    candidate) record against the reference's SVD route. Bound: 16 x the reference's own SVD-to-Gram distance on the same pairs
    (the kernel takes the Gram route), floor 1e-12 -- the rule of DESIGN 4.18; the scores to the same relative bound. The
    64-point view holds a pixel on the centre: its bearing (0, 0, 1) is exact, or the view would have no pose."""
    c, g = _pairs_run(C_, 0)
    a = ref.start(c["off"], c["uv"], c["xyz"], centre=c["centre"], candidates=C_, search_views=0, refine_iterations=0, route="svd")
    b = ref.start(c["off"], c["uv"], c["xyz"], centre=c["centre"], candidates=C_, search_views=0, refine_iterations=0, route="gram")
    assert _bits(g["f"]) == _bits(a["f"])
    dr = dt = worst_r = worst_t = 0.0
    for (j, k), (kind, R, t, cost) in a["pairs"].items():
        _, Rb, tb, _ = b["pairs"][j, k]
        dr, dt = max(dr, rs.rot_angle(R, Rb)), max(dt, float(np.linalg.norm(t - tb)))
        r = g["rec"][j, k]
        assert int(r[KIND_SLOT]) == kind == (ref.GENERAL if k >= 6 else ref.PLANAR), (j, k, r[KIND_SLOT], kind)
        Rg = rs.quat_to_R(r[:4])
        worst_r, worst_t = max(worst_r, rs.rot_angle(R, Rg)), max(worst_t, float(np.linalg.norm(t - r[4:7])))
        # the kernel's cost is the reference's chord at the kernel's own pose
        sl = slice(int(c["off"][k]), int(c["off"][k + 1]))
        assert r[COST_SLOT] == pytest.approx(ref.chord_cost(Rg, r[4:7], c["xyz"][sl].astype(np.float64), ref.bearings(c["uv"][sl], c["centre"], a["f"][j])), rel=1e-9, abs=1e-24)
    bound_r, bound_t = max(16 * dr, 1e-12), max(16 * dt, 1e-12)
    ds = float(np.max(np.abs(a["score"] - b["score"]) / np.abs(a["score"])))
    worst_s = float(np.max(np.abs(g["score"] - a["score"]) / np.abs(a["score"])))
    bound_s = max(16 * ds, 1e-12)
    print(f"C = {C_}: SVD vs Gram {dr:.2e} rad / {dt:.2e} m / scores {ds:.2e}; kernel vs SVD {worst_r:.2e} rad ({worst_r / bound_r:.3f} of bound) / "
          f"{worst_t:.2e} m ({worst_t / bound_t:.3f}) / scores {worst_s:.2e} ({worst_s / bound_s:.3f})")
    assert worst_r <= bound_r and worst_t <= bound_t and worst_s <= bound_s
    assert list(g["qualified"]) == [1] * C_ and g["report"]["best_candidate"] == a["best"] and g["report"]["views_invalid"] == 0
    # the pose pass repeats the search's records of the winner, bit for bit
    assert _bits(g["views"]) == _bits(g["rec"][a["best"]])


def test_refined_pairs_scores_and_pick_match_the_reference():
    """Three specified steps, C = 24, every view searched: EVERY (view, candidate) record -- rotation, translation, cost -- against
    the reference's own three steps from its SVD closed form (intr_start_ref.pair). The kernel and the reference make the same
    specified steps (the same Jacobian, damping schedule and acceptance rule) from closed forms that agree to the bound of the test
    above, so the rule is that test's: 16 x the reference's own distance between its two routes, SVD and Gram, AFTER the three steps,
    floor 1e-12 (measured on the CPU: 4.5e-14 rad, 4.0e-15 m, 6.9e-14 relative in the cost, 9.5e-16 in the scores). A wrong entry of
    J^T J or J^T r, a wrong lambda or a wrong acceptance moves a record by many orders more. The scores are held to the costs' bound.
    The picked index is the reference's; f, centre and the report are identical."""
    c, g = _pairs_run(24, 3)
    a = ref.start(c["off"], c["uv"], c["xyz"], centre=c["centre"], candidates=24, search_views=0, refine_iterations=3, route="svd")
    b = ref.start(c["off"], c["uv"], c["xyz"], centre=c["centre"], candidates=24, search_views=0, refine_iterations=3, route="gram")
    dr = dt = dc = worst_r = worst_t = worst_c = 0.0
    moved = 0
    for (j, k), (kind, Ra, ta, cost) in a["pairs"].items():
        _, Rb, tb, cb = b["pairs"][j, k]
        r = g["rec"][j, k]
        assert int(r[KIND_SLOT]) == kind
        dr, dt = max(dr, rs.rot_angle(Ra, Rb)), max(dt, float(np.linalg.norm(ta - tb)))
        worst_r, worst_t = max(worst_r, rs.rot_angle(Ra, rs.quat_to_R(r[:4]))), max(worst_t, float(np.linalg.norm(ta - r[4:7])))
        if k:   # (the four-point view is fitted exactly: its cost is rounding, 1e-30, and has no relative error to speak of)
            dc, worst_c = max(dc, abs(cost - cb) / cost), max(worst_c, abs(r[COST_SLOT] - cost) / cost)
            sl = slice(int(c["off"][k]), int(c["off"][k + 1]))
            moved += ref.pair(c["xyz"][sl], c["uv"][sl], c["centre"], a["f"][j], 0)[3] > 1.001 * cost
    assert moved >= 0.9 * 7 * 24, moved   # the steps do something: they lower the closed form's cost on nearly every pair (all 168 here)
    bound_r, bound_t, bound_c = max(16 * dr, 1e-12), max(16 * dt, 1e-12), max(16 * dc, 1e-12)
    worst_s = float(np.max(np.abs(g["score"] - a["score"]) / np.abs(a["score"])))
    print(f"{len(a['pairs'])} pairs, {moved} lowered by the steps; reference SVD vs Gram after three steps {dr:.2e} rad / {dt:.2e} m / cost {dc:.2e}; kernel vs reference "
          f"{worst_r:.2e} rad ({worst_r / bound_r:.3f} of bound) / {worst_t:.2e} m ({worst_t / bound_t:.3f}) / cost {worst_c:.2e} ({worst_c / bound_c:.3f}) / "
          f"scores {worst_s:.2e} ({worst_s / bound_c:.3f})")
    assert worst_r <= bound_r and worst_t <= bound_t and worst_c <= bound_c and worst_s <= bound_c
    assert g["report"] == a["report"], (g["report"], a["report"])
    assert _bits(g["intr"]) == _bits(a["intr"]) and _bits(g["f"]) == _bits(a["f"]) and list(g["qualified"]) == list(a["qualified"])


@pytest.mark.parametrize("C_", [1, 2, 24])
def test_closed_form_rotations_on_the_square_ragged_set(C_):
    """refine_iterations = 0 on the ragged set on SQUARE grids (4, 9, 25, 64, 65, 144 points): a square grid's scatter has two equal
    in-plane eigenvalues, the path of the classification on which the board's basis is the eigen-solver's choice. The translation
    depends on that choice when the focal length is off (intr_start_ref.pairs_scene), the rotation does not (4e-14 between bases
    30 - 75 degrees apart, on every candidate): kind and rotation of every record against the reference's SVD route, bound 16 x the
    reference's SVD-to-Gram rotation, floor 1e-12."""
    c = ref.ragged_scene()
    p = _problem(c)
    _, _, _, rep = p.estimate_start_fisheye(candidates=C_, search_views=0, refine_iterations=0)
    rec = _fetch(p, b"start_records", C_ * 6 * STRIDE).reshape(C_, 6, STRIDE)
    p.close()
    a = ref.start(c["off"], c["uv"], c["xyz"], candidates=C_, search_views=0, refine_iterations=0, route="svd")
    b = ref.start(c["off"], c["uv"], c["xyz"], candidates=C_, search_views=0, refine_iterations=0, route="gram")
    dr = worst = 0.0
    for (j, k), (kind, R, t, cost) in a["pairs"].items():
        assert int(rec[j, k][KIND_SLOT]) == kind == ref.PLANAR, (j, k)
        dr, worst = max(dr, rs.rot_angle(R, b["pairs"][j, k][1])), max(worst, rs.rot_angle(R, rs.quat_to_R(rec[j, k][:4])))
    bound = max(16 * dr, 1e-12)
    print(f"square ragged set, C = {C_}: SVD vs Gram {dr:.2e} rad; kernel vs SVD {worst:.2e} rad ({worst / bound:.3f} of bound)")
    assert worst <= bound and rep["views_invalid"] == 0 and rep["candidates_qualified"] == C_


# ---- 3. search_views ------------------------------------------------------------------------------------------------------------
def test_search_views_picks_floor_k_F_over_S_and_returns_every_pose():
    c = scene_of("95deg_seed3")   # F = 12
    p = _problem(c)
    intr, q, t, rep = p.estimate_start_fisheye(search_views=5)
    rec = _fetch(p, b"start_records", 24 * 5 * STRIDE).reshape(24, 5, STRIDE)
    views = _fetch(p, b"start_views", 12 * STRIDE)
    a = ref.start(c["off"], c["uv"], c["xyz"], search_views=5)
    assert a["searched"] == [0, 2, 4, 7, 9] and rep == a["report"] and rep["views_searched"] == 5 and rep["views"] == 12
    # the searched set: the pose pass's record of view floor(k F / S) is the search's record k of the winner, bit for bit
    for k, v in enumerate(a["searched"]):
        assert _bits(views[v]) == _bits(rec[rep["best_candidate"], k]), (k, v)
    assert not any(_bits(views[v]) == _bits(rec[rep["best_candidate"], k]) for k in range(5) for v in range(12) if v != a["searched"][k])
    assert np.all(views[:, KIND_SLOT] == ref.PLANAR) and np.all(np.abs(np.linalg.norm(q, axis=1) - 1) < 1e-12) and np.all(np.linalg.norm(t, axis=1) > 0.1)
    # S = 0 and S >= F search every view
    full = start_of("95deg_seed3")["report"]
    for S in (0, 12, 40):
        assert p.estimate_start_fisheye(search_views=S)[3] == full, S
    p.close()


# ---- 4. reproducibility and the handle's state --------------------------------------------------------------------------------
def test_same_bits_again_and_the_handle_is_left_alone():
    c = scene_of("85deg_seed6")
    opt = capi.default_options(**TIGHT)
    p = _problem(c)
    p.set_state(c["intr0_true"], c["q_true"], c["t_true"])
    before = p.get_state()
    one = p.estimate_start_fisheye()
    sc1 = p.start_scores()
    two = p.estimate_start_fisheye()
    assert _bits(*one[:3]) == _bits(*two[:3]) and one[3] == two[3] and _bits(*sc1) == _bits(*p.start_scores())
    assert p.get_model() == FISH and _bits(*p.get_state()) == _bits(*before)
    s1 = p.solve(opt)
    st1 = p.get_state()
    p.close()
    fresh = _problem(c)
    three = fresh.estimate_start_fisheye()
    assert _bits(*one[:3]) == _bits(*three[:3]) and one[3] == three[3] and _bits(*sc1) == _bits(*fresh.start_scores())
    fresh.set_state(c["intr0_true"], c["q_true"], c["t_true"])   # a handle that never ran the start before its solve
    s2 = fresh.solve(opt)
    assert _bits(*fresh.get_state()) == _bits(*st1) and s1["iterations"] == s2["iterations"] and s1["final_cost"] == s2["final_cost"]
    fresh.close()


# ---- 5. end to end --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SCENES))
def test_start_then_solve_ends_at_the_references_minimum(name):
    """Start + set_state + solve at the tight tolerances against the reference solve from the generator's poses. Bounds: 10 x the
    largest figure of each column of the yardstick (tests/test_intr_start_ref_cpu.py), the reference's own two solves."""
    c = scene_of(name)
    want = truth_solve(name)
    p = _problem(c)
    intr, q, t, rep = p.estimate_start_fisheye()
    assert rep == start_of(name)["report"]
    p.set_state(intr, q, t)
    s = p.solve(capi.default_options(**TIGHT))
    got = p.get_state() + (s,)
    p.close()
    d = distances(want, got)
    print(f"{name}: f {rep['focal']:.1f}; {want[3]['iterations']} it (reference) / {s['iterations']} it, {s['termination']}; cost rel {d[0]:.2e} ({d[0] / COST_REL:.3f} of bound), "
          f"rotation {d[1]:.2e} ({d[1] / ROT_ABS:.3f}), translation {d[2]:.2e} ({d[2] / T_ABS:.3f}), intrinsics {d[3]:.2e} ({d[3] / INTR_REL:.3f})")
    assert d[0] <= COST_REL and d[1] <= ROT_ABS and d[2] <= T_ABS and d[3] <= INTR_REL


def test_one_shot_with_the_start_ends_at_the_references_minimum_and_the_class_follows():
    """The same through capi.intrinsics_estimate(start="fisheye") at the tight tolerances, held to the same bounds; and through
    pycalibrator (SetStart), which solves at the class's default options and keeps float32: it is held to the one-shot call at
    those options, one float32 unit in the last place."""
    import pycalibrator as pc
    name = "75deg_seed2"
    c = scene_of(name)
    want = truth_solve(name)
    K, intr, q, t, s = capi.intrinsics_estimate(c["off"], c["uv"], c["xyz"], model=FISH, start="fisheye", options=capi.default_options(**TIGHT))
    rep = start_of(name)["report"]
    assert K.tolist() == [[np.float32(rep["focal"]), 0, np.float32(rep["centre"][0])], [0, np.float32(rep["focal"]), np.float32(rep["centre"][1])], [0, 0, 1]]
    d = distances(want, (intr, q, t, s))
    print(f"one-shot {name}: {s['iterations']} it; cost rel {d[0]:.2e}, rotation {d[1]:.2e}, translation {d[2]:.2e}, intrinsics {d[3]:.2e}")
    assert d[0] <= COST_REL and d[1] <= ROT_ABS and d[2] <= T_ABS and d[3] <= INTR_REL
    _, intr_d, _, _, s_d = capi.intrinsics_estimate(c["off"], c["uv"], c["xyz"], model=FISH, start="fisheye")
    cal = pc.Calibrator(1600, 1000)
    cal.SetCameraModel(pc.CameraModel.Fisheye)
    cal.SetStart(pc.Start.FisheyeFocalSearch)
    img = [c["uv"][c["off"][f]:c["off"][f + 1]] for f in range(len(c["off"]) - 1)]
    world = [c["xyz"][c["off"][f]:c["off"][f + 1]] for f in range(len(c["off"]) - 1)]
    cal.Estimate(img, world)
    assert cal.LastStatus() == 0 and cal.LastIterations() == s_d["iterations"] and cal.GetStart() == pc.Start.FisheyeFocalSearch
    assert cal.LastStartFocal() == float(np.float32(rep["focal"]))   # (float32, as K holds it: calibrator.hh)
    Kc = cal.GetK()
    got = np.concatenate([[Kc[0, 0], Kc[1, 1], Kc[0, 2], Kc[1, 2]], cal.GetDistortion()]).astype(np.float32)
    wantf = intr_d[:8].astype(np.float32)
    assert np.abs(got.view(np.int32).astype(np.int64) - wantf.view(np.int32).astype(np.int64)).max() <= 1
    # the start belongs to the fisheye model and to Estimate
    r = pc.Calibrator(1600, 1000)
    r.SetStart(pc.Start.FisheyeFocalSearch)
    with pytest.raises(ValueError):
        r.Estimate(img, world)
    with pytest.raises(ValueError):
        pc.EstimateMany([cal], [img], [world])


# ---- 6. refusals and edges ------------------------------------------------------------------------------------------------------
def test_refusals():
    c = scene_of("85deg_seed6")
    p = _problem(c, model=0)
    assert _rc(lambda: p.start_scores()) == CC_ERR_STATE
    assert _rc(lambda: p.estimate_start_fisheye()) == CC_ERR_STATE            # a radial-tangential handle
    p.comm_init(capi.comm_get_unique_id(), 0, 1)
    # a handle after comm_init: refused -- by its model, as it happens: comm_init and set_model(fisheye) refuse each other, so no
    # fisheye handle has a communicator or an exchange and the start's own guard against one cannot be reached from outside
    assert _rc(lambda: p.estimate_start_fisheye()) == CC_ERR_STATE
    assert _rc(lambda: p.set_model(FISH)) == CC_ERR_STATE
    p.close()
    p = _problem(c)
    assert _rc(lambda: p.start_scores()) == CC_ERR_STATE                      # before any start
    for bad in (dict(candidates=0), dict(candidates=65), dict(theta_lo=0.0), dict(theta_lo=-0.1), dict(theta_hi=np.pi), dict(theta_lo=1.0, theta_hi=0.9),
                dict(search_views=-1), dict(refine_iterations=-1), dict(theta_lo=float("nan"))):
        assert _rc(lambda: p.estimate_start_fisheye(**bad)) == CC_ERR_BAD_ARGUMENT, bad
    assert _rc(lambda: p.start_scores()) == CC_ERR_STATE
    assert p.estimate_start_fisheye(candidates=1, theta_lo=1.7, theta_hi=1.7)[3]["best_candidate"] == 0   # lo == hi is allowed
    assert [len(v) for v in p.start_scores()] == [1, 1, 1]
    p.estimate_start_fisheye(candidates=5)
    before = p.start_scores()
    for bad in (dict(candidates=0), dict(candidates=65)):   # a refused call leaves the last search and its read-back as they were
        assert _rc(lambda: p.estimate_start_fisheye(**bad)) == CC_ERR_BAD_ARGUMENT
        assert [len(v) for v in p.start_scores()] == [5, 5, 5] and _bits(*p.start_scores()) == _bits(*before)
    p.close()
    for kw in (dict(model=0, start="fisheye"), dict(model=FISH, start="fisheye", start_options=dict(candidates=0))):
        assert _rc(lambda: capi.intrinsics_estimate(c["off"], c["uv"], c["xyz"], **kw)) == CC_ERR_BAD_ARGUMENT, kw


def test_invalid_views_are_counted_given_the_identity_and_leave_the_others_alone():
    """A collinear view, a 3-point view and a view with a NaN pixel between the views of a clean scene: each is counted and gets
    q = (1, 0, 0, 0), t = 0, and each makes the one-shot call fail with its own index; every other view's record is the clean run's,
    bit for bit (the centre is given: the added pixels must not move it)."""
    c = scene_of("85deg_seed6")   # six views of 25 points
    off, uv, xyz = c["off"], c["uv"], c["xyz"]
    view = lambda f: (uv[off[f]:off[f + 1]], xyz[off[f]:off[f + 1]])
    line = np.stack([np.linspace(-0.3, 0.3, 7), np.linspace(-0.1, 0.2, 7), np.zeros(7)], axis=1).astype(np.float32)
    nan_uv = view(2)[0].copy()
    nan_uv[3, 0] = np.nan
    parts = [view(0), (view(1)[0][:7], line), view(1), (view(3)[0][:3], view(3)[1][:3]), view(2), (nan_uv, view(2)[1]), view(3), view(4), view(5)]
    d_uv, d_xyz = np.concatenate([a for a, _ in parts]), np.concatenate([b for _, b in parts])
    d_off = np.concatenate([[0], np.cumsum([len(a) for a, _ in parts])]).astype(np.int64)
    centre = (900.0, 600.0)
    clean, dirty = _problem(c), _problem(dict(off=d_off, uv=d_uv, xyz=d_xyz))
    ic, qc, tc, rc = clean.estimate_start_fisheye(centre=centre, search_views=0)
    idt, qd, td, rd = dirty.estimate_start_fisheye(centre=centre, search_views=0)
    vc, vd = _fetch(clean, b"start_views", 6 * STRIDE), _fetch(dirty, b"start_views", 9 * STRIDE)
    clean.close(); dirty.close()
    keep, bad = [0, 2, 4, 6, 7, 8], [1, 3, 5]
    assert (rd["views_invalid"], rd["views"], rc["views_invalid"]) == (3, 9, 0)
    assert rd["best_candidate"] == rc["best_candidate"] and rd["candidates_qualified"] == rc["candidates_qualified"] == 24 and rd["r_max"] == rc["r_max"]
    assert _bits(vd[keep]) == _bits(vc) and not vd[bad].any() and _bits(qd[keep], td[keep], idt) == _bits(qc, tc, ic)
    assert qd[bad].tolist() == [[1.0, 0.0, 0.0, 0.0]] * 3 and not td[bad].any()
    with pytest.raises(capi.CcError, match="view 1 has no pose") as e:   # all three: the first is named
        capi.intrinsics_estimate(d_off, d_uv, d_xyz, model=FISH, start="fisheye", start_options=dict(centre=centre))
    assert str(e.value).startswith(f"cc error {CC_ERR_BAD_ARGUMENT}:")
    for at in bad:   # each alone, where it stands among the clean views
        some = [parts[i] for i in range(9) if i == at or i in keep]
        index = sorted(keep + [at]).index(at)
        s_off = np.concatenate([[0], np.cumsum([len(a) for a, _ in some])]).astype(np.int64)
        with pytest.raises(capi.CcError, match=f"view {index} has no pose") as e:
            capi.intrinsics_estimate(s_off, np.concatenate([a for a, _ in some]), np.concatenate([b for _, b in some]), model=FISH, start="fisheye",
                                     start_options=dict(centre=centre))
        assert str(e.value).startswith(f"cc error {CC_ERR_BAD_ARGUMENT}:")


# ---- 7. the defaults are what they were -----------------------------------------------------------------------------------------
def test_calls_without_a_start_return_what_they_returned():
    """capi.intrinsics_estimate(model=fisheye) without start= and a Calibrator that never calls SetStart go through
    cc_intrinsics_estimate_views_model as before; cc_intrinsics_estimate_views_start with a NULL start is that call: the same bits
    from the two entry points in one process."""
    import pycalibrator as pc
    c = fr.case("8x40")
    a = capi.intrinsics_estimate(c["off"], c["uv"], c["xyz"], model=FISH)
    off = np.ascontiguousarray(c["off"], dtype=np.int64)
    F = len(off) - 1
    uv_views, xyz_views, counts, _keep = capi._views(off, capi._f32(c["uv"]), capi._f32(c["xyz"]))
    opt, s = capi.default_options(), capi.Summary()
    s.log, s.log_capacity = None, 0
    K = np.zeros(9, dtype=np.float32)
    intr, q, t = np.zeros(9), np.zeros((F, 4)), np.zeros((F, 3))
    capi._check(capi.lib().cc_intrinsics_estimate_views_start(C.byref(opt), C.c_int32(0), C.c_int64(F), uv_views, xyz_views, capi._p(counts, C.c_int64), None,
                                                               C.c_uint32(0), capi._p(K, C.c_float), capi._p(intr, C.c_double), capi._p(q, C.c_double),
                                                               capi._p(t, C.c_double), C.byref(s), C.c_double(0.0), C.c_int32(FISH), None))
    assert _bits(K, intr, q, t) == _bits(a[0], a[1], a[2], a[3]) and s.iterations == a[4]["iterations"] and s.final_cost == a[4]["final_cost"]
    cal = pc.Calibrator(1600, 1000)
    cal.SetCameraModel(pc.CameraModel.Fisheye)
    img = [c["uv"][c["off"][f]:c["off"][f + 1]] for f in range(F)]
    world = [c["xyz"][c["off"][f]:c["off"][f + 1]] for f in range(F)]
    cal.Estimate(img, world)
    Kc = cal.GetK()
    got = np.concatenate([[Kc[0, 0], Kc[1, 1], Kc[0, 2], Kc[1, 2]], cal.GetDistortion()]).astype(np.float32)
    assert cal.GetStart() == pc.Start.Zhang and cal.LastStartFocal() == 0.0 and cal.LastIterations() == a[4]["iterations"]
    assert _bits(got) == _bits(a[1][:8].astype(np.float32))
