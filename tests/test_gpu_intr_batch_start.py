"""GPU: the batched fisheye focal-length start (cc_intrinsics_batch_estimate_start_fisheye, cc_intrinsics_batch_start_scores,
cc_intrinsics_batch_estimate_start, the four-argument Calibrator::EstimateMany; k_intrb_start_extent / _view / _pick in
camera_calibrator_amd/csrc/cc_intr_start_batch.hip) against the numpy reference of the start applied problem by problem
(tests/intr_start_ref.start), against the single handle, and against itself in other batches. Every test calls one of the new
entry points and fails on a library without them."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

from camera_calibrator_amd import capi
from tests import intr_start_ref as ref
from tests import rig_start_ref as rs
from tests.test_intr_start_ref_cpu import COST_REL, INTR_REL, ROT_ABS, T_ABS, distances, scene_of, truth_solve

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "camera_calibrator_amd"))
pytestmark = pytest.mark.gpu
FISH = capi.MODEL_FISHEYE
CC_ERR_BAD_ARGUMENT, CC_ERR_STATE = -1, -5
TIGHT = dict(max_iterations=1000, function_tolerance=1e-15, gradient_tolerance=1e-13, parameter_tolerance=1e-14)
NAMES = ("ragged", "85deg_seed6", "95deg_seed3")   # views of 4 .. 144 points; 6 x 25; 12 x 36


def _bits(*arrays):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)


def _prob(c, uv=None):
    return (c["off"], c["uv"] if uv is None else uv, c["xyz"])


def _base():
    return [_prob(scene_of(n)) for n in NAMES]


def _rc(fn):
    try:
        fn()
    except capi.CcError as e:
        return int(str(e).split()[2].rstrip(":"))
    return 0


def _run(problems, **options):
    """One batched start on a fresh handle: per problem (intr [9], q, t, report, f, score, qualified)."""
    h = capi.IntrinsicsBatch(problems)
    h.set_model(FISH)
    intr, q, t, reports = h.estimate_start_fisheye(**options)
    f, score, qualified = h.start_scores()
    qs, ts = h._split(q, 4), h._split(t, 3)
    h.close()
    return [dict(intr=intr[p], q=qs[p], t=ts[p], report=reports[p], f=f[p], score=score[p], qualified=qualified[p]) for p in range(len(problems))]


def _single(problem, **options):
    p = capi.IntrinsicsProblem(*problem)
    p.set_model(FISH)
    intr, q, t, report = p.estimate_start_fisheye(**options)
    f, score, qualified = p.start_scores()
    p.close()
    return dict(intr=intr, q=q, t=t, report=report, f=f, score=score, qualified=qualified)


def _same(a, b):
    return a["report"] == b["report"] and _bits(a["intr"], a["q"], a["t"], a["f"], a["score"], a["qualified"]) == _bits(b["intr"], b["q"], b["t"], b["f"], b["score"], b["qualified"])


@functools.lru_cache(maxsize=None)
def _ref_start(name, route="svd", **options):
    c = _named(name)
    return ref.start(c["off"], c["uv"], c["xyz"], route=route, **options)


def _named(name):
    if name == "pairs":
        return ref.pairs_scene()
    if name == "85deg_seed6_nan":
        c = scene_of("85deg_seed6")
        uv = c["uv"].copy()
        uv[int(np.argmax(uv[:, 0])), 1] = np.nan   # the pixel that would set the box's right edge
        return dict(c, uv=uv)
    return scene_of(name)


def _exact(g, a):
    """The quantities without a rounding of their own: centre, r_max, every f_j, the picked index, the report and intr9."""
    assert g["report"] == a["report"], (g["report"], a["report"])
    assert _bits(g["report"]["centre"][0], g["report"]["centre"][1], g["report"]["r_max"]) == _bits(a["centre"][0], a["centre"][1], a["r_max"])
    assert _bits(g["f"]) == _bits(a["f"]) and _bits(g["intr"]) == _bits(a["intr"]) and list(g["qualified"]) == list(a["qualified"])
    assert g["report"]["best_candidate"] == a["best"]


# ---- 1. the exact quantities --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["clean", "nan_pixel", "centre"])
def test_exact_quantities_are_the_references_bits_per_problem(case):
    """Centre, r_max (min, max and one unfused fp64 expression: no rounding of the kernel's own), the candidates, the pick, the
    report and intr9 of every problem of the B = 3 batch: with a NaN pixel on the box's edge in the middle problem (left out of
    its box and r_max; its view has no pose), and about a centre the caller gives (applied to every problem)."""
    names = list(NAMES)
    options = {}
    if case == "nan_pixel":
        names[1] = "85deg_seed6_nan"
    if case == "centre":
        options = dict(centre=(801.25, 498.5))
    got = _run([_prob(_named(n)) for n in names], **options)
    for n, g in zip(names, got):
        _exact(g, _ref_start(n, **options))
    if case == "nan_pixel":
        assert [g["report"]["views_invalid"] for g in got] == [0, 1, 0]
        clean = _ref_start("85deg_seed6")
        assert got[1]["report"]["r_max"] != clean["r_max"] or got[1]["report"]["centre"] != tuple(clean["centre"])   # (the pixel did set the box)
    if case == "centre":
        assert all(g["report"]["centre"] == (801.25, 498.5) for g in got)


# ---- 2. a problem's bits do not depend on the batch ----------------------------------------------------------------------------
@pytest.mark.parametrize("search_views", [0, 5])
def test_a_problems_outputs_are_the_same_alone_in_the_batch_and_in_the_reversed_batch(search_views):
    """Every output -- poses (the records), scores, qualified, report, intr9 -- np.array_equal between a batch of one, the batch of
    three and the batch reversed. search_views = 5: views 0 2 4 7 9 of the 12-view problem, 5 of the ragged problem's 6."""
    base = _base()
    batch = _run(base, search_views=search_views)
    rev = _run(base[::-1], search_views=search_views)[::-1]
    for p, prob in enumerate(base):
        alone = _run([prob], search_views=search_views)[0]
        assert _same(alone, batch[p]) and _same(alone, rev[p]), (NAMES[p], search_views)
    want = [(6, 6), (6, 6), (12, 12)] if search_views == 0 else [(6, 5), (6, 5), (12, 5)]
    assert [(g["report"]["views"], g["report"]["views_searched"]) for g in batch] == want
    if search_views == 5:
        assert ref.searched(12, 5) == [0, 2, 4, 7, 9] and batch[2]["report"] == _ref_start("95deg_seed3", search_views=5)["report"]
        assert batch[0]["report"] == _ref_start("ragged", search_views=5)["report"]


# ---- 3. against the single handle and the reference ---------------------------------------------------------------------------
def _bounds(a, b):
    """16 x the reference's own SVD-to-Gram distance, floor 1e-12: rotation, translation, relative score (the rule of DESIGN 4.18 /
    4.19, recomputed here from the reference's two routes on the poses at the winner)."""
    dr = max(rs.rot_angle(rs.quat_to_R(x), rs.quat_to_R(y)) for x, y in zip(a["q"], b["q"]))
    dt = float(np.max(np.linalg.norm(a["t"] - b["t"], axis=1)))
    ds = float(np.max(np.abs(a["score"] - b["score"]) / np.abs(a["score"])))
    return max(16 * dr, 1e-12), max(16 * dt, 1e-12), max(16 * ds, 1e-12)


def _pose_distance(g, a):
    dr = max(rs.rot_angle(rs.quat_to_R(x), rs.quat_to_R(y)) for x, y in zip(g["q"], a["q"]))
    dt = float(np.max(np.linalg.norm(g["t"] - a["t"], axis=1)))
    ds = float(np.max(np.abs(g["score"] - a["score"]) / np.abs(a["score"])))
    return dr, dt, ds


def test_the_batch_against_the_single_handle_and_the_reference():
    """Batch of three: the rectangular-board pairs scene (the translation can be compared: intr_start_ref.pairs_scene says why),
    about its centre, next to the two square-grid scenes. Exact quantities and views_invalid: bit-equal to the single handle on
    every problem. Poses and scores of the pairs scene: within 16 x the reference's SVD-to-Gram distance (floor 1e-12) of the
    single handle AND of the reference. Whether the batch is in fact bit-equal to the single handle is printed, not asserted: the
    two view kernels are compiled from the same lines, what the compiler makes of them is its decision."""
    pairs = ref.pairs_scene()
    options = dict(centre=tuple(pairs["centre"]), search_views=0)
    problems = [_prob(scene_of("85deg_seed6")), _prob(pairs), _prob(scene_of("95deg_seed3"))]
    got = _run(problems, **options)
    singles = [_single(p, **options) for p in problems]
    equal = []
    for g, s in zip(got, singles):
        assert g["report"] == s["report"] and _bits(g["f"], g["intr"], g["qualified"]) == _bits(s["f"], s["intr"], s["qualified"])
        equal.append(_same(g, s))
    print(f"batch bit-equal to the single handle (poses, scores, everything): {equal}")
    a, b = _ref_start("pairs", **options), _ref_start("pairs", route="gram", **options)
    _exact(got[1], a)
    bound_r, bound_t, bound_s = _bounds(a, b)
    for what, other in (("single handle", singles[1]), ("reference", a)):
        dr, dt, ds = _pose_distance(got[1], other)
        print(f"pairs scene, batch vs {what}: rotation {dr:.2e} ({dr / bound_r:.3f} of bound), translation {dt:.2e} ({dt / bound_t:.3f}), "
              f"scores {ds:.2e} ({ds / bound_s:.3f})")
        assert dr <= bound_r and dt <= bound_t and ds <= bound_s, what


# ---- 4. invalid views and failures ---------------------------------------------------------------------------------------------
def _dirty():
    """85deg_seed6 with a collinear view, a 3-point view and a NaN-pixel view between its own (tests/test_gpu_intr_start.py builds
    the same problem for the single handle)."""
    c = scene_of("85deg_seed6")
    off, uv, xyz = c["off"], c["uv"], c["xyz"]
    view = lambda f: (uv[off[f]:off[f + 1]], xyz[off[f]:off[f + 1]])
    line = np.stack([np.linspace(-0.3, 0.3, 7), np.linspace(-0.1, 0.2, 7), np.zeros(7)], axis=1).astype(np.float32)
    nan_uv = view(2)[0].copy()
    nan_uv[3, 0] = np.nan
    parts = [view(0), (view(1)[0][:7], line), view(1), (view(3)[0][:3], view(3)[1][:3]), view(2), (nan_uv, view(2)[1]), view(3), view(4), view(5)]
    d_off = np.concatenate([[0], np.cumsum([len(a) for a, _ in parts])]).astype(np.int64)
    return (d_off, np.concatenate([a for a, _ in parts]), np.concatenate([b for _, b in parts])), [0, 2, 4, 6, 7, 8], [1, 3, 5]


def test_invalid_views_are_counted_in_their_problem_and_leave_the_other_problems_alone():
    centre = (900.0, 600.0)   # (given: the added pixels must not move it)
    dirty, keep, bad = _dirty()
    base = _base()
    clean = _run(base, centre=centre, search_views=0)
    got = _run([base[0], dirty, base[2]], centre=centre, search_views=0)
    assert _same(got[0], clean[0]) and _same(got[2], clean[2])
    d, c = got[1], clean[1]
    assert (d["report"]["views_invalid"], d["report"]["views"], c["report"]["views_invalid"]) == (3, 9, 0)
    assert d["report"]["best_candidate"] == c["report"]["best_candidate"] and d["report"]["candidates_qualified"] == 24 and d["report"]["r_max"] == c["report"]["r_max"]
    assert _bits(d["q"][keep], d["t"][keep], d["intr"]) == _bits(c["q"], c["t"], c["intr"])
    assert d["q"][bad].tolist() == [[1.0, 0.0, 0.0, 0.0]] * 3 and not d["t"][bad].any()
    # the one-shot call names problem and view (the view by its index within the problem)
    with pytest.raises(capi.CcError, match="problem 1: view 1 has no pose") as e:
        capi.intrinsics_batch_estimate([base[0], dirty, base[2]], model=FISH, start="fisheye", start_options=dict(centre=centre))
    assert str(e.value).startswith(f"cc error {CC_ERR_BAD_ARGUMENT}:")


def test_a_problem_without_a_winner_fails_the_call_fills_every_report_and_writes_nothing_else():
    """No candidate qualifies only when every score is non-finite: a problem's own pixels cannot do that (float32 pixels give a
    finite r_max; a problem without a finite pixel has r_max = 0, f = 0, every view invalid for every candidate, score 0 and
    candidate 0 wins with views_invalid = F). A centre so far off that the squared distance overflows does: r_max = inf, every
    f_j = inf, every score inf * 0 = NaN. The single handle returns CC_ERR_STATE for it -- asserted first, it is the single
    path's way to that return -- and the centre belongs to the whole batch, so every problem is marked; the message names the
    first. Every report is filled and the caller's arrays keep what they held."""
    far = (1e200, 1e200)
    base = _base()
    p = capi.IntrinsicsProblem(*base[1])
    p.set_model(FISH)
    assert _rc(lambda: p.estimate_start_fisheye(centre=far)) == CC_ERR_STATE
    p.close()
    h = capi.IntrinsicsBatch(base)
    h.set_model(FISH)
    lib = capi.lib()
    o = capi.intr_start_options(centre=far)
    intr, q, t = np.full((3, 9), 7.0), np.full((h.n_frames, 4), 7.0), np.full((h.n_frames, 3), 7.0)
    r = (capi.IntrStartReport * 3)()
    rc = lib.cc_intrinsics_batch_estimate_start_fisheye(h._h, C.byref(o), capi._p(intr, C.c_double), capi._p(q, C.c_double), capi._p(t, C.c_double), r)
    msg = lib.cc_last_error().decode()
    assert rc == CC_ERR_STATE and "problem 0" in msg, (rc, msg)
    assert np.all(intr == 7.0) and np.all(q == 7.0) and np.all(t == 7.0)
    assert [(r[i].best_candidate, r[i].candidates_qualified, r[i].views, r[i].views_searched, r[i].views_invalid) for i in range(3)] == [(-1, 0, 6, 6, 0), (-1, 0, 6, 6, 0), (-1, 0, 12, 12, 0)]
    assert all((r[i].centre[0], r[i].centre[1]) == far and r[i].r_max == np.inf and r[i].focal == 0.0 for i in range(3))
    f, score, qualified = h.start_scores()   # (the search ran: its scores say why nothing qualified)
    assert f.shape == (3, 24) and np.all(np.isinf(f)) and np.all(np.isnan(score)) and not qualified.any()
    with pytest.raises(capi.CcError, match="problem 0") as e:   # the Python wrapper keeps the reports for the caller
        h.estimate_start_fisheye(centre=far)
    assert str(e.value).startswith(f"cc error {CC_ERR_STATE}:") and [x["best_candidate"] for x in h.last_start_reports] == [-1, -1, -1]
    good = h.estimate_start_fisheye()   # the handle is as good as new
    assert [x["best_candidate"] for x in good[3]] == [g["report"]["best_candidate"] for g in _run(base)]
    h.close()
    with pytest.raises(capi.CcError, match="problem 0") as e:
        capi.intrinsics_batch_estimate(base, model=FISH, start="fisheye", start_options=dict(centre=far))
    assert str(e.value).startswith(f"cc error {CC_ERR_BAD_ARGUMENT}:")


# ---- 5. many problems ----------------------------------------------------------------------------------------------------------
def test_seventy_problems_hold_the_bits_of_each_problem_alone():
    """70 problems of 3 views of 9 points, cut from one scene (72 views of a 3 x 3 board, problem p its views p, p + 1, p + 2): more
    problems than a wave has lanes, 70 pick workgroups. Three of them against their own batch of one."""
    c = ref.scene(72, 3, 0.3, 0.40, 60.0, 11)
    off = c["off"]
    problems = []
    for p in range(70):
        lo, hi = int(off[p]), int(off[p + 3])
        problems.append((off[p:p + 4] - off[p], c["uv"][lo:hi], c["xyz"][lo:hi]))
    got = _run(problems)
    assert len(got) == 70 and all(g["report"]["views"] == 3 and g["report"]["views_searched"] == 3 for g in got)
    assert all(g["report"]["best_candidate"] >= 0 for g in got)
    for p in (0, 37, 69):
        assert _same(_run([problems[p]])[0], got[p]), p
    assert len({g["report"]["focal"] for g in got}) > 10   # (the problems are not copies of one another)


# ---- 6. end to end -------------------------------------------------------------------------------------------------------------
def test_one_shot_batch_from_the_search_ends_at_the_references_minimum():
    """capi.intrinsics_batch_estimate(model=fisheye, start="fisheye") on the B = 3 batch at the tight tolerances against the CPU
    reference's solve from the generator's poses, per problem: the bounds of DESIGN 4.19's end-to-end table x 10
    (tests/test_intr_start_ref_cpu.py). Iterations within 1 of the single path's one-shot. On the seed-6 scene the batch's Zhang
    start ends at more than 100 x that cost (the wrong basin of DESIGN 4.19)."""
    base = _base()
    opt = capi.default_options(**TIGHT)
    K, intr, qs, ts, ss = capi.intrinsics_batch_estimate(base, model=FISH, start="fisheye", options=opt)
    for p, name in enumerate(NAMES):
        want = truth_solve(name)
        d = distances(want, (intr[p], qs[p], ts[p], ss[p]))
        _, _, _, _, s1 = capi.intrinsics_estimate(*base[p], model=FISH, start="fisheye", options=opt)
        rep = _ref_start(name)["report"]
        assert K[p].tolist() == [[np.float32(rep["focal"]), 0, np.float32(rep["centre"][0])], [0, np.float32(rep["focal"]), np.float32(rep["centre"][1])], [0, 0, 1]]
        print(f"{name}: {ss[p]['iterations']} it (single one-shot {s1['iterations']}, reference {want[3]['iterations']}); cost rel {d[0]:.2e} ({d[0] / COST_REL:.3f} of bound), "
              f"rotation {d[1]:.2e} ({d[1] / ROT_ABS:.3f}), translation {d[2]:.2e} ({d[2] / T_ABS:.3f}), intrinsics {d[3]:.2e} ({d[3] / INTR_REL:.3f})")
        assert d[0] <= COST_REL and d[1] <= ROT_ABS and d[2] <= T_ABS and d[3] <= INTR_REL
        assert abs(ss[p]["iterations"] - s1["iterations"]) <= 1
    _, _, _, _, sz = capi.intrinsics_batch_estimate(base, model=FISH, start="zhang", options=opt)
    print(f"85deg_seed6: final cost {ss[1]['final_cost']:.6e} from the search, {sz[1]['final_cost']:.6e} from Zhang ({sz[1]['iterations']} it)")
    assert sz[1]["final_cost"] > 100 * ss[1]["final_cost"]


def test_without_a_start_the_call_returns_the_model_calls_bits():
    base = _base()
    a = capi.intrinsics_batch_estimate(base, model=FISH)
    poff, foff, uv, xyz = capi._batch_layout(base)
    B, F = 3, int(poff[-1])
    for start in ("zhang", None):
        b = capi.intrinsics_batch_estimate(base, model=FISH, start=start)
        assert _bits(a[0], a[1], *a[2], *a[3]) == _bits(b[0], b[1], *b[2], *b[3]) and [s["iterations"] for s in a[4]] == [s["iterations"] for s in b[4]]
    K, intr, q, t = np.zeros((B, 9), dtype=np.float32), np.zeros((B, 9)), np.zeros((F, 4)), np.zeros((F, 3))
    opt = capi.default_options()
    ss, _logs = capi._batch_summaries(B, 16)
    capi._check(capi.lib().cc_intrinsics_batch_estimate_start(C.byref(opt), C.c_int32(0), C.c_int64(B), capi._p(poff, C.c_int64), capi._p(foff, C.c_int64),
                                                               capi._p(uv, C.c_float), capi._p(xyz, C.c_float), None, None, capi._p(K, C.c_float),
                                                               capi._p(intr, C.c_double), capi._p(q, C.c_double), capi._p(t, C.c_double), ss, None,
                                                               C.c_int32(FISH), None))
    assert _bits(K.reshape(B, 3, 3), intr, q, t) == _bits(a[0], a[1], np.concatenate(a[2]), np.concatenate(a[3]))
    assert [ss[p].iterations for p in range(B)] == [s["iterations"] for s in a[4]] and [ss[p].final_cost for p in range(B)] == [s["final_cost"] for s in a[4]]


# ---- 7. class ------------------------------------------------------------------------------------------------------------------
def _views(problem):
    off, uv, xyz = problem
    F = len(off) - 1
    return [uv[off[f]:off[f + 1]] for f in range(F)], [xyz[off[f]:off[f + 1]] for f in range(F)]


def _class_state(cal):
    Kc = cal.GetK()
    return np.concatenate([[Kc[0, 0], Kc[1, 1], Kc[0, 2], Kc[1, 2]], cal.GetDistortion()]).astype(np.float32)


def _calibrators(pc, n):
    cs = [pc.Calibrator(1600, 1000) for _ in range(n)]
    for c in cs:
        c.SetCameraModel(pc.CameraModel.Fisheye)
    return cs


def test_the_four_argument_estimate_many_follows_the_one_shot_and_sets_each_focal():
    import pycalibrator as pc
    base = _base()
    img, world = [_views(p)[0] for p in base], [_views(p)[1] for p in base]
    _, intr, _, _, ss = capi.intrinsics_batch_estimate(base, model=FISH, start="fisheye")   # (the class's options: the defaults)
    cs = _calibrators(pc, 3)
    pc.EstimateMany(cs, img, world, pc.Start.FisheyeFocalSearch)
    for p, cal in enumerate(cs):
        got, want = _class_state(cal), intr[p][:8].astype(np.float32)
        assert np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64)).max() <= 1, (p, got, want)
        assert cal.LastStatus() == 0 and cal.LastIterations() == ss[p]["iterations"]
        assert cal.LastStartFocal() == float(np.float32(_ref_start(NAMES[p])["report"]["focal"])) and cal.GetStart() == pc.Start.Zhang
    # Start.Zhang in the four-argument form is the three-argument call
    a, b = _calibrators(pc, 3), _calibrators(pc, 3)
    pc.EstimateMany(a, img, world)
    pc.EstimateMany(b, img, world, pc.Start.Zhang)
    for x, y in zip(a, b):
        assert _bits(_class_state(x)) == _bits(_class_state(y)) and x.LastIterations() == y.LastIterations() and y.LastStartFocal() == 0.0


# ---- 8. reuse ------------------------------------------------------------------------------------------------------------------
def test_a_second_start_and_a_solve_behind_a_start_give_a_fresh_handles_bits():
    base = _base()
    opt = capi.default_options(**TIGHT)
    fresh = _run(base)
    h = capi.IntrinsicsBatch(base)
    h.set_model(FISH)
    h.estimate_start_fisheye(candidates=5, search_views=2)   # (another layout of the scratch first)
    intr, q, t, reports = h.estimate_start_fisheye()
    f, score, qualified = h.start_scores()
    assert reports == [g["report"] for g in fresh] and _bits(intr, q, t) == _bits(*[g["intr"] for g in fresh], *[g["q"] for g in fresh], *[g["t"] for g in fresh])
    assert _bits(f, score, qualified) == _bits(np.stack([g["f"] for g in fresh]), np.stack([g["score"] for g in fresh]), np.stack([g["qualified"] for g in fresh]))
    h.set_state(intr, q, t)
    s1 = h.solve(opt)
    st1 = h.get_state()
    h.close()
    g = capi.IntrinsicsBatch(base)   # a handle that never ran the start before its solve
    g.set_model(FISH)
    g.set_state(intr, q, t)
    s2 = g.solve(opt)
    st2 = g.get_state()
    g.close()
    assert _bits(st1[0], *st1[1], *st1[2]) == _bits(st2[0], *st2[1], *st2[2])
    assert [s["iterations"] for s in s1] == [s["iterations"] for s in s2] and [s["final_cost"] for s in s1] == [s["final_cost"] for s in s2]
