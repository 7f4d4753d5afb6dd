"""GPU: start poses of a rig problem from its own observations (cc_rig_estimate_start / cc_rig_start_views / cc_rig_estimate,
camera_calibrator_amd/csrc/cc_rig_start.hip) against the numpy reference (tests/rig_start_ref.py), stage by stage and end to end.
Every test fails on a library without the entry points."""
import numpy as np
import pytest

from camera_calibrator_amd import capi
from oracle import pyoracle as po
from tests import rig_start_ref as ref
from tests.test_rig_start_ref_cpu import CAM_R_ABS, CAM_T_ABS, COST_REL, SHAPES

pytestmark = pytest.mark.gpu
CC_ERR_STATE = -5


def _problem(sc, frozen, **kw):
    return capi.RigProblem(sc["n_cams"], sc["frame_offsets"], sc["obs_cam"], sc["obs_world"], sc["obs_uv"], sc["world_xyz"],
                           np.asarray(frozen, dtype=np.uint8), **kw)


def _views(sc):
    return ref.views_of(sc["frame_offsets"], sc["obs_cam"], sc["obs_world"], sc["obs_uv"], sc["world_xyz"])


def _route_yardstick(views, unit=1.0):
    """16 x the largest difference between the reference's SVD and Gram routes on these views (rotation in radians,
    translation in the scene's unit), floor 1e-12: the bound on the kernel's closed form, which takes the Gram route."""
    dr = dt = 0.0
    for _, _, X, uv in views:
        ka, Ra, ta = ref.view_closed_form(X, uv, "svd")
        kb, Rb, tb = ref.view_closed_form(X, uv, "gram")
        if ka != ref.INVALID and kb != ref.INVALID:
            dr, dt = max(dr, ref.rot_angle(Ra, Rb)), max(dt, np.linalg.norm(ta - tb) / unit)
    return max(16 * dr, 1e-12), max(16 * dt, 1e-12) * unit, dr, dt


# ---- 1. stage V -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("unit", [1.0, 1e3], ids=["metres", "millimetres"])
def test_closed_form_matches_the_reference(unit):
    """One camera, one view per frame: 4 and 5 coplanar points, 6 and 7 general ones, 64 / 65 / 130 points (one pass of the wave,
    one more observation, two passes and a rest) general and planar, a board on z = 0 and boards rotated and shifted off every
    axis. refine_iterations = 0: the closed form as it is."""
    kw = dict(unit=unit, noise=1e-3)
    scenes = [ref.plant_scene(1, 1, 4, seed=1, planar=True, **kw), ref.plant_scene(1, 1, 5, seed=2, planar=True, **kw),
              ref.plant_scene(1, 1, 6, seed=3, **kw), ref.plant_scene(1, 1, 7, seed=4, **kw),
              ref.plant_scene(1, 1, 64, seed=5, **kw), ref.plant_scene(1, 1, 65, seed=6, planar=True, **kw),
              ref.plant_scene(1, 1, 130, seed=7, **kw), ref.plant_scene(1, 1, 130, seed=8, planar=True, **kw),
              ref.plant_scene(1, 1, 0, seed=9, planar=True, board=(6, 5), on_z0=True, **kw),
              ref.plant_scene(1, 1, 0, seed=10, planar=True, board=(6, 5), **kw)]
    sc = ref.merge_scenes(scenes)
    views = _views(sc)
    p = _problem(sc, [0])
    rep = p.estimate_start(refine_iterations=0)
    got = p.start_views()
    p.close()
    want_kinds = [1, 1, 2, 2, 2, 1, 2, 1, 1, 1]
    assert list(got["kind"]) == want_kinds and list(got["frame"]) == list(range(10)) and not got["camera"].any()
    assert (rep["views_planar"], rep["views_general"], rep["views_invalid"], rep["views_valid"]) == (6, 4, 0, 10)
    bound_r, bound_t, dr, dt = _route_yardstick(views, unit)
    worst_r = worst_t = 0.0
    for k, (_, _, X, uv) in enumerate(views):
        kind, R, t = ref.view_closed_form(X, uv, "svd")
        Rg = ref.quat_to_R(got["q"][k])
        assert kind == want_kinds[k]
        worst_r, worst_t = max(worst_r, ref.rot_angle(R, Rg)), max(worst_t, np.linalg.norm(t - got["t"][k]))
        # the kernel's rms^2 is the reference's residual function at the kernel's own pose
        assert got["rms2"][k] == pytest.approx(ref.rms2(Rg, got["t"][k], X, uv), rel=1e-9)
    print(f"unit {unit}: SVD vs Gram route {dr:.2e} rad / {dt:.2e}; kernel vs SVD {worst_r:.2e} rad ({worst_r / bound_r:.3f} of bound) "
          f"/ {worst_t / unit:.2e} ({worst_t / bound_t:.3f} of bound)")
    assert worst_r <= bound_r and worst_t <= bound_t


# ---- 2. stage R -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["general_3x20x12", "planar_3x10_board6x5"])
def test_refined_views_match_the_converged_reference(name):
    if name.startswith("general"):
        sc = ref.plant_scene(3, 20, 12, seed=21, noise=1e-3)
    else:
        sc = ref.plant_scene(3, 10, 0, seed=22, planar=True, board=(6, 5), noise=1e-3)
    views = _views(sc)
    p = _problem(sc, [1, 0, 0])
    p.estimate_start(refine_iterations=10)
    got = p.start_views()
    p.close()
    # the reference against itself: ten specified steps against least_squares; a view counts when the ten steps have converged:
    # thirty steps end within 1e-8 of them -- well under what least_squares itself resolves with its finite-difference
    # Jacobian (~1e-6, the yardstick printed below), so a counted view's bound is least_squares' own error, not leftover descent
    rows = []
    for k, (_, _, X, uv) in enumerate(views):
        kind, R0, t0 = ref.view_closed_form(X, uv)
        Ra, ta = ref.refine_lm(R0, t0, X, uv, 10)
        Rb, tb = ref.refine_lm(R0, t0, X, uv, 30)
        if ref.rot_angle(Ra, Rb) > 1e-8 or np.linalg.norm(ta - tb) > 1e-8:
            continue
        Rc, tc = ref.refine_converged(R0, t0, X, uv)
        rows.append((k, Rc, tc, ref.rot_angle(Ra, Rc), np.linalg.norm(ta - tc)))
    assert len(rows) >= 0.9 * len(views), (len(rows), len(views))
    bound_r, bound_t = 16 * max(r[3] for r in rows), 16 * max(r[4] for r in rows)
    worst_r = max(ref.rot_angle(Rc, ref.quat_to_R(got["q"][k])) for k, Rc, tc, _, _ in rows)
    worst_t = max(np.linalg.norm(tc - got["t"][k]) for k, Rc, tc, _, _ in rows)
    print(f"{name}: {len(rows)} of {len(views)} views; reference LM vs least_squares {bound_r / 16:.2e} rad / {bound_t / 16:.2e}; "
          f"kernel vs least_squares {worst_r:.2e} rad ({worst_r / bound_r:.3f} of bound) / {worst_t:.2e} ({worst_t / bound_t:.3f} of bound)")
    assert all(got["kind"][k] == (2 if name.startswith("general") else 1) for k in range(len(views)))
    assert worst_r <= bound_r and worst_t <= bound_t
    for k, Rc, tc, _, _ in rows:
        assert got["rms2"][k] == pytest.approx(ref.rms2(ref.quat_to_R(got["q"][k]), got["t"][k], views[k][2], views[k][3]), rel=1e-9)


# ---- 3. invalid views -------------------------------------------------------------------------------------------------------
def _drop(sc, keep, extra=None):
    """The scene with the observations `keep` (a mask), then `extra` = [(frame, camera, X, uv)] appended to their frames."""
    frames = np.repeat(np.arange(len(sc["frame_offsets"]) - 1), np.diff(sc["frame_offsets"]))
    cam, world, uv, fr = sc["obs_cam"][keep], sc["obs_world"][keep], sc["obs_uv"][keep], frames[keep]
    xyz = sc["world_xyz"].reshape(-1, 3)
    for f, c, X, m in extra or []:
        cam = np.concatenate([cam, np.full(len(X), c, dtype=np.uint32)])
        world = np.concatenate([world, np.arange(len(xyz), len(xyz) + len(X)).astype(np.uint64)])
        uv = np.concatenate([uv, np.asarray(m, dtype=np.float32)])
        fr = np.concatenate([fr, np.full(len(X), f)])
        xyz = np.concatenate([xyz, np.asarray(X, dtype=np.float32)])
    order = np.argsort(fr, kind="stable")
    off = np.concatenate([[0], np.cumsum(np.bincount(fr, minlength=len(sc["frame_offsets"]) - 1))]).astype(np.int64)
    return dict(sc, frame_offsets=off, obs_cam=cam[order], obs_world=world[order], obs_uv=uv[order], world_xyz=xyz)


def test_invalid_views_are_skipped_and_counted():
    sc = ref.plant_scene(2, 7, 8, seed=31, noise=1e-3)
    frames = np.repeat(np.arange(7), np.diff(sc["frame_offsets"]))
    idx = np.arange(len(frames))
    cam1 = sc["obs_cam"] == 1

    def first(f, n):   # mask of all but the first n observations of camera 1 in frame f
        k = idx[cam1 & (frames == f)]
        m = np.zeros(len(frames), dtype=bool)
        m[k[n:]] = True
        return m
    # frame 0: three points; frame 1: five points that span space; frame 2: collinear points; frame 3: a NaN image coordinate;
    # frame 4: camera 1 sees nothing; frames 5, 6 untouched
    line = np.outer(np.linspace(-1, 1, 7), [1.0, 0.5, 0.25]) + [0.3, -0.2, 5.0]
    dirty = _drop(sc, ~(first(0, 3) | first(1, 5) | (cam1 & np.isin(frames, [2, 4]))), [(2, 1, line, line[:, :2] / line[:, 2:3])])
    k = np.nonzero((dirty["obs_cam"] == 1) & (np.repeat(np.arange(7), np.diff(dirty["frame_offsets"])) == 3))[0][2]
    dirty["obs_uv"] = dirty["obs_uv"].copy()
    dirty["obs_uv"][k, 1] = np.nan
    clean = _drop(sc, ~(cam1 & np.isin(frames, [0, 1, 2, 3, 4])))
    pd, pc = _problem(dirty, [1, 0]), _problem(clean, [1, 0])
    rd, rc = pd.estimate_start(), pc.estimate_start()
    vd = pd.start_views()
    sd, sc_ = pd.get_state(want_cost=False), pc.get_state(want_cost=False)
    pd.close(); pc.close()
    kinds = {(int(f), int(c)): int(kd) for f, c, kd in zip(vd["frame"], vd["camera"], vd["kind"])}
    assert [kinds[(f, 1)] for f in (0, 1, 2, 3)] == [0, 0, 0, 0] and (4, 1) not in kinds
    assert kinds[(5, 1)] == kinds[(6, 1)] == 2 and all(kinds[(f, 0)] == 2 for f in range(7))
    assert (rd["views_invalid"], rd["views_valid"], rd["views_general"]) == (4, 9, 9) and rc["views_invalid"] == 0 and rc["views_valid"] == 9
    assert rd["frames_unplaced"] == 0 and rd["cameras_unplaced"] == 0 and list(rd["parent"]) == [-1, 0]
    for a, b in zip(sd[:4], sc_[:4]):
        assert a.tobytes() == b.tobytes()


# ---- 4. stages C and F ------------------------------------------------------------------------------------------------------
def _rot(axis, deg):
    return ref._exp(np.asarray(axis, dtype=np.float64) * np.deg2rad(deg))


def _rig_case(name):
    """(scene, frozen flags, caller's camera poses (R, t) or None)"""
    rng = np.random.default_rng(41)
    F = 6
    frame_R = [ref.random_rotation(rng, 0.5) for _ in range(F)]
    frame_t = [rng.uniform(-0.5, 0.5, 3) for _ in range(F)]
    if name == "half_turns":   # cameras within 1 degree of 180 degrees about x, y and z from the root: q and -q both occur
        cam_R = [np.eye(3), _rot([1, 0, 0], 179.95), _rot([0, 1, 0], 180.03), _rot([0, 0, 1], 179.98)]
        vis = np.ones((F, 4), dtype=bool)
        frozen = [1, 0, 0, 0]
    elif name == "through_a_third":   # camera 2 never shares a frame with the root 0; it is reached through camera 1
        cam_R = [_rot([0, 1, 0], 20), _rot([1, 0, 0], 30), _rot([0, 0, 1], -40)]
        vis = np.array([[1, 1, 0], [1, 1, 0], [1, 0, 0], [0, 1, 1], [0, 1, 1], [1, 1, 0]], dtype=bool)
        frozen = [1, 0, 0]   # a frozen root with a pose that is not the identity
    elif name == "disconnected":      # camera 2 shares no frame with anyone, frame 5 is seen by nobody
        cam_R = [np.eye(3), _rot([0, 1, 0], 15), _rot([1, 1, 0], 25)]
        vis = np.array([[1, 1, 0], [1, 1, 0], [0, 0, 1], [1, 1, 0], [0, 0, 1], [0, 0, 0]], dtype=bool)
        frozen = [1, 0, 0]
    else:                             # no frozen camera: the root (camera 1: most views) goes to the identity
        assert name == "no_frozen"
        cam_R = [_rot([0, 1, 0], 10), np.eye(3), _rot([1, 0, 0], -20)]
        vis = np.array([[1, 1, 1], [0, 1, 1], [1, 1, 0], [1, 1, 1], [0, 1, 1], [1, 1, 1]], dtype=bool)
        frozen = [0, 0, 0]
    cam_t = [rng.uniform(-0.3, 0.3, 3) for _ in cam_R]
    if name == "no_frozen":
        cam_t[1] = np.zeros(3)
    sc = ref.plant_rig(cam_R, cam_t, frame_R, frame_t, vis, 9, seed=42, noise=1e-3)
    return sc, frozen, vis


@pytest.mark.parametrize("name", ["half_turns", "through_a_third", "disconnected", "no_frozen"])
def test_camera_and_frame_poses_match_the_reference_means(name, monkeypatch):
    sc, frozen, vis = _rig_case(name)
    C, F = sc["n_cams"], len(sc["frame_offsets"]) - 1
    rng = np.random.default_rng(43)
    # the caller's poses: the planted ones for frozen cameras, arbitrary (and unnormalised) ones elsewhere -- those must survive
    # bit for bit where nothing is estimated
    cq = np.stack([ref.R_to_quat(R) for R in sc["cam_R"]]) * rng.uniform(0.5, 2.0, (C, 1))
    ct = sc["cam_t"] + np.where(np.asarray(frozen, dtype=bool)[:, None], 0.0, rng.normal(size=(C, 3)))
    fq, ft = rng.normal(size=(F, 4)), rng.normal(size=(F, 3))
    results = []
    for waves in (None, 2, 4, 2):
        if waves is None:
            monkeypatch.delenv("CC_RIG_SWEEP_WG_WAVES", raising=False)
        else:
            monkeypatch.setenv("CC_RIG_SWEEP_WG_WAVES", str(waves))
        p = _problem(sc, frozen)
        rep = p.estimate_start(cq, ct, fq, ft)
        if waves is None:
            again = p.estimate_start(cq, ct, fq, ft)   # a second call on the same handle
            assert {k: (v.tolist() if k == "parent" else v) for k, v in again.items()} == {k: (v.tolist() if k == "parent" else v) for k, v in rep.items()}
        results.append((rep, p.start_views(), p.get_state(want_cost=False)))
        p.close()
    rep, got, state = results[0]
    for _, g2, s2 in results[1:]:
        assert all(a.tobytes() == b.tobytes() for a, b in zip(state[:4], s2[:4]))
        assert all(got[k].tobytes() == g2[k].tobytes() for k in got)
    # stages T, C and F of the reference on the DEVICE's view results: the means themselves, without the views' own deviation
    vl = [(int(f), int(c), int(k), ref.quat_to_R(q) if k else None, t, m)
          for f, c, k, q, t, m in zip(got["frame"], got["camera"], got["kind"], got["q"], got["t"], got["rms2"])]
    rq, rt, rfq, rft, rrep = ref.poses_from_views(C, F, vl, frozen, cq, ct, fq, ft)
    assert rep["root_camera"] == rrep["root_camera"] and list(rep["parent"]) == rrep["parent"]
    assert bool(rep["root_at_identity"]) == rrep["root_at_identity"]
    assert (rep["cameras_placed"], rep["cameras_unplaced"], rep["frames_placed"], rep["frames_unplaced"]) == \
        (rrep["cameras_placed"], rrep["cameras_unplaced"], rrep["frames_placed"], rrep["frames_unplaced"])
    bound_r, bound_t, _, _ = _route_yardstick(_views(sc))
    gq, gt, gfq, gft = state[:4]
    worst = 0.0
    for a, b, ta, tb in list(zip(gq, rq, gt, rt)) + list(zip(gfq, rfq, gft, rft)):
        worst = max(worst, ref.rot_angle(ref.quat_to_R(a), ref.quat_to_R(b)) / bound_r, np.linalg.norm(ta - tb) / bound_t)
    print(f"{name}: device means vs reference means, worst fraction of the bound ({bound_r:.2e} rad, {bound_t:.2e}) {worst:.1e}")
    assert worst <= 1.0
    # ... and the planted poses are what comes out, to the noise: 1e-3 in the image over >= 9 points a view
    placed_c = [c for c in range(C) if frozen[c] or rep["parent"][c] >= 0 or c == rep["root_camera"]]
    for c in placed_c:
        ident = rep["root_at_identity"] and c == rep["root_camera"]
        Rc = ref.quat_to_R(gq[c])
        assert ref.rot_angle(Rc, np.eye(3) if ident else sc["cam_R"][c]) < 2e-2
    if name == "through_a_third":
        assert list(rep["parent"]) == [-1, 0, 1] and rep["root_camera"] == 0
    if name == "disconnected":
        assert rep["cameras_unplaced"] == 1 and rep["frames_unplaced"] == 3   # (frames 2 and 4 are seen by the unplaced camera only)
        assert gq[2].tobytes() == cq[2].tobytes() and gt[2].tobytes() == ct[2].tobytes()
        for f in (2, 4, 5):
            assert gfq[f].tobytes() == fq[f].tobytes() and gft[f].tobytes() == ft[f].tobytes()
    if name == "no_frozen":
        assert rep["root_camera"] == 1 and rep["root_at_identity"] == 1
        assert gq[1].tolist() == [1.0, 0.0, 0.0, 0.0] and gt[1].tolist() == [0.0, 0.0, 0.0]
    if name in ("half_turns", "through_a_third"):   # frozen root: the caller's pose, bit for bit
        assert gq[0].tobytes() == cq[0].tobytes() and gt[0].tobytes() == ct[0].tobytes()
    if name == "half_turns":   # both signs occur among the relative quaternions the means were taken over
        w = []   # w of the relative quaternion whose axis component is positive: sign of the antisymmetric part about that axis
        for f in range(F):
            v = {c: k for k, (ff, c) in enumerate(zip(got["frame"], got["camera"])) if ff == f}
            for c, (i, j) in ((1, (2, 1)), (2, (0, 2)), (3, (1, 0))):
                Rr = ref.quat_to_R(got["q"][v[c]]) @ ref.quat_to_R(got["q"][v[0]]).T
                w.append(Rr[i, j] - Rr[j, i])
        assert min(w) < 0 < max(w) and max(abs(x) for x in w) < 0.1, w


def test_a_noisy_view_moves_the_frame_mean_by_its_weight_only():
    """All cameras frozen at the planted poses, so a frame's pose is the mean over its three views alone. One view has
    sqrt(1000) times the image noise of the others: its rms^2 is ~1000 x theirs. With it the frame's translation is
    t_without + w / (W + w) (t_view - t_without) exactly, w = 1 / rms^2 the view's weight and W the others' total."""
    rng = np.random.default_rng(51)
    cam_R = [np.eye(3), _rot([0, 1, 0], 12), _rot([1, 0, 0], -9)]
    cam_t = [rng.uniform(-0.3, 0.3, 3) for _ in cam_R]
    frame_R, frame_t = [ref.random_rotation(rng, 0.4) for _ in range(3)], [rng.uniform(-0.5, 0.5, 3) for _ in range(3)]
    sc = ref.plant_rig(cam_R, cam_t, frame_R, frame_t, np.ones((3, 3), dtype=bool), 12, seed=52, noise=1e-3,
                       view_noise={(1, 2): 1e-3 * np.sqrt(1000.0)})
    frames = np.repeat(np.arange(3), np.diff(sc["frame_offsets"]))
    without = _drop(sc, ~((sc["obs_cam"] == 2) & (frames == 1)))
    cq = np.stack([ref.R_to_quat(R) for R in cam_R])
    out = []
    for s in (sc, without):
        p = _problem(s, [1, 1, 1])
        p.estimate_start(cq, np.stack(cam_t))
        out.append((p.start_views(), p.get_state(want_cost=False)))
        p.close()
    (v, st), (_, st0) = out
    k = [i for i, (f, c) in enumerate(zip(v["frame"], v["camera"])) if f == 1]
    rms2 = v["rms2"][k]
    assert 300 < rms2[2] / rms2[:2].mean() < 3000, rms2
    w, W = 1.0 / rms2[2], (1.0 / rms2[:2]).sum()
    t_view = cam_R[2].T @ (v["t"][k[2]] - cam_t[2])
    moved, allowed = np.linalg.norm(st[3][1] - st0[3][1]), w / (W + w) * np.linalg.norm(t_view - st0[3][1])
    print(f"rms^2 ratio {rms2[2] / rms2[:2].mean():.0f}, weight share {w / (W + w):.2e}: moved {moved:.3e}, allowed {allowed:.3e}")
    assert moved <= allowed * (1 + 1e-9) and moved >= allowed * (1 - 1e-6)
    for f in (0, 2):   # the other frames do not know about it
        assert st[2][f].tobytes() == st0[2][f].tobytes() and st[3][f].tobytes() == st0[3][f].tobytes()


# ---- 5. end to end ----------------------------------------------------------------------------------------------------------
TIGHT = dict(max_iterations=1000, function_tolerance=1e-15, gradient_tolerance=1e-13, parameter_tolerance=1e-14)


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2], SHAPES[6]], ids=lambda s: "%dx%dx%d_seed%d" % s)
def test_start_then_solve_ends_at_the_oracles_minimum(shape, monkeypatch):
    # Bits are compared in the three-kernel form: a small rig's default is the lean persistent solve, which may give up for want
    # of residency and be run again in the three-kernel form -- same minimum, other last bits (cc_rig_solver_status). The default
    # form is held against the oracle at the end.
    monkeypatch.setenv("CC_RIG_PERSIST", "0")
    C, F, M, seed = shape
    sc = po.rig_scenario(C, F, M, seed=seed)
    sc["n_cams"] = C
    cq0, ct0 = po.affine_to_qt(sc["cam_T"])
    fq0, ft0 = po.affine_to_qt(sc["frame_T"])
    want = po.rig_solve(C, sc["frame_offsets"], sc["obs_cam"], sc["obs_world"], sc["obs_uv"], sc["world_xyz"], cq0, ct0,
                        sc["cam_frozen"], fq0, ft0, options=po.default_options(**TIGHT))
    p = _problem(sc, sc["cam_frozen"])
    rep = p.estimate_start(cq0, ct0)   # (the frames from the identity: every one of them is placed)
    assert rep["cameras_unplaced"] == 0 and rep["frames_unplaced"] == 0 and rep["views_invalid"] == 0
    start = p.get_state(want_cost=True)
    cost0 = p.eval()
    # the handle's state is what set_state with the read-back poses gives
    p2 = _problem(sc, sc["cam_frozen"])
    p2.set_state(*start[:4])
    s2 = p2.get_state(want_cost=True)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(start, s2)) and p2.eval() == cost0
    summary = p.solve(capi.default_options(**TIGHT))
    end = p.get_state(want_cost=False)
    s2sum = p2.solve(capi.default_options(**TIGHT))
    end2 = p2.get_state(want_cost=False)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(end[:4], end2[:4])) and summary["iterations"] == s2sum["iterations"]
    p.reset()   # ... and reset returns to the start
    back = p.get_state(want_cost=True)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(start, back))
    p.close(); p2.close()
    ca, cb = want[5]["final_cost"], summary["final_cost"]
    dt = np.abs(want[1] - end[1]).max()
    dr = max(ref.rot_angle(ref.quat_to_R(want[0][c]), ref.quat_to_R(end[0][c])) for c in range(C))
    print(f"{shape}: start cost {cost0:.3e}; oracle {ca:.9e} ({want[5]['iterations']} it) vs start + solve {cb:.9e} ({summary['iterations']} it): "
          f"rel {abs(ca - cb) / ca:.2e}, cam_t {dt:.2e}, cam_R {dr:.2e}")
    assert abs(ca - cb) <= COST_REL * ca and dt <= CAM_T_ABS and dr <= CAM_R_ABS
    # the one-shot call is start then solve
    one = capi.rig_estimate(C, sc["frame_offsets"], sc["obs_cam"], sc["obs_world"], sc["obs_uv"], sc["world_xyz"], sc["cam_frozen"],
                            cam_q=cq0, cam_t=ct0, options=capi.default_options(**TIGHT))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(one[:4], end[:4])) and one[5]["iterations"] == summary["iterations"]
    # the default form of the solver from the same start
    monkeypatch.delenv("CC_RIG_PERSIST")
    p = _problem(sc, sc["cam_frozen"])
    p.estimate_start(cq0, ct0)
    sd = p.solve(capi.default_options(**TIGHT))
    endd = p.get_state(want_cost=False)
    p.close()
    dt = np.abs(want[1] - endd[1]).max()
    dr = max(ref.rot_angle(ref.quat_to_R(want[0][c]), ref.quat_to_R(endd[0][c])) for c in range(C))
    print(f"{shape}, default form: rel {abs(ca - sd['final_cost']) / ca:.2e}, cam_t {dt:.2e}, cam_R {dr:.2e}")
    assert abs(ca - sd["final_cost"]) <= COST_REL * ca and dt <= CAM_T_ABS and dr <= CAM_R_ABS


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------
def _refused(p, *a):
    with pytest.raises(capi.CcError) as e:
        p.estimate_start(*a)
    assert "cc error %d" % CC_ERR_STATE in str(e.value)


def test_refusals_leave_the_handle_as_it_was():
    sc = po.rig_scenario(2, 10, 6, seed=3)
    sc["n_cams"] = 2
    cq0, ct0 = po.affine_to_qt(sc["cam_T"])
    fq0, ft0 = po.affine_to_qt(sc["frame_T"])
    ref_p = _problem(sc, sc["cam_frozen"])
    ref_p.set_state(cq0, ct0, fq0, ft0)
    want_sum = ref_p.solve()
    want = ref_p.get_state(want_cost=False)
    ref_p.close()
    # a handle with an exchange attached (a single rank is a valid, degenerate exchange)
    p = _problem(sc, sc["cam_frozen"])
    p.set_state(cq0, ct0, fq0, ft0)
    p.exchange_attach(0, [p.exchange_export()])
    before = p.get_state(want_cost=False)
    _refused(p, cq0, ct0, fq0, ft0)
    with pytest.raises(capi.CcError):
        p.start_views()
    after = p.get_state(want_cost=False)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(before[:4], after[:4]))
    got_sum = p.solve()
    got = p.get_state(want_cost=False)
    p.close()
    assert got_sum["iterations"] == want_sum["iterations"] and all(np.allclose(a, b, rtol=0, atol=1e-9) for a, b in zip(want[:4], got[:4]))
    # a handle with intrinsics: pixel observations. Next to a handle that never saw the refused call
    K = np.array([500.0, 500.0, 320.0, 240.0, 0, 0, 0, 0, 0])
    uv_px = (sc["obs_uv"].reshape(-1, 2) * K[:2] + K[2:4]).astype(np.float32)
    ends = []
    for refuse in (True, False):
        pk = capi.RigProblem(2, sc["frame_offsets"], sc["obs_cam"], sc["obs_world"], uv_px, sc["world_xyz"], sc["cam_frozen"],
                             with_intrinsics=True)
        pk.set_intrinsics(K)
        pk.set_state(cq0, ct0, fq0, ft0)
        before = pk.get_state(want_cost=False)
        if refuse:
            _refused(pk)
            after = pk.get_state(want_cost=False)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(before[:4], after[:4]))
        it = pk.solve()["iterations"]
        ends.append((it, pk.get_state(want_cost=False), pk.get_intrinsics()))
        pk.close()
    assert ends[0][0] == ends[1][0] and ends[0][2].tobytes() == ends[1][2].tobytes()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(ends[0][1][:4], ends[1][1][:4]))
    # no observation at all
    empty = dict(sc, frame_offsets=np.zeros(11, dtype=np.int64), obs_cam=sc["obs_cam"][:0], obs_world=sc["obs_world"][:0], obs_uv=sc["obs_uv"][:0])
    try:
        pe = _problem(empty, sc["cam_frozen"])
    except capi.CcError:
        return   # (the library does not make a handle of an empty problem at all)
    _refused(pe)
    pe.close()
