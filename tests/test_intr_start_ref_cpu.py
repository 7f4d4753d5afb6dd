"""CPU: the reference of the fisheye focal-length start (tests/intr_start_ref.py) against itself -- its scenes, its two routes
to the null vector, the yardstick of the solve that follows it, and the scenes where Zhang's start fails. No GPU, no library
call: what tests/test_gpu_intr_start.py holds the kernels to is measured here (DESIGN 4.19 has the tables)."""
import functools

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import fisheye_ref as fr
from tests import intr_start_ref as ref
from tests import rig_start_ref as rs

# (F, side, half, dist, max_dir, seed) of intr_start_ref.scene; ("ragged",): intr_start_ref.ragged_scene, views of 4 .. 144 points
SCENES = {
    "ragged": ("ragged",),
    "75deg_seed2": (10, 7, 0.3, 0.40, 75.0, 2),
    "85deg_seed6": (6, 5, 0.3, 0.40, 85.0, 6),
    "95deg_seed3": (12, 6, 0.25, 0.35, 95.0, 3),
    "85deg_seed8": (10, 7, 0.3, 0.40, 85.0, 8),
}
# largest angle off the axis [deg] and share of the observations beyond 90 degrees, as the generator reports them
GEOMETRY = {"ragged": (76.4, 0.0), "75deg_seed2": (120.0, 0.037), "85deg_seed6": (113.4, 0.053), "95deg_seed3": (134.6, 0.185),
            "85deg_seed8": (123.0, 0.116)}
ZHANG_FAILS = ("75deg_seed2", "85deg_seed6")

# The yardstick: lm_solve at the tight tolerances from the focal-length start against the same solve from the generator's poses
# (true fx fy px py, k = 0). All ten solves stop on the parameter test. Measured with this reference (the test prints it):
#   scene         focal  candidate  margin   iterations  cost (relative)  rotation (rad)  translation  intrinsics
#   ragged        554.1  8          0.5 %    9 / 10      6.74e-15         1.32e-14        5.16e-15     1.09e-13
#   75deg_seed2   533.5  14         8.3 %    10 / 10     3.33e-15         1.70e-14        6.51e-15     3.66e-14
#   85deg_seed6   528.5  12         4.8 %    10 / 11     6.04e-14         1.50e-15        3.00e-15     7.58e-15
#   95deg_seed3   531.3  17         4.3 %    10 / 11     1.30e-14         4.08e-15        5.00e-16     4.99e-15
#   85deg_seed8   550.5  15         3.8 %    10 / 11     1.80e-14         4.58e-16        2.22e-16     9.16e-16
# (intrinsics: |difference| / max(|slot|, 1), largest slot). The bounds of the end-to-end GPU test: the largest figure of each
# column x 10, for the stopping rule's slack, as DESIGN 4.15 and 4.16 do.
COST_REL, ROT_ABS, T_ABS, INTR_REL = 6.04e-13, 1.70e-13, 6.51e-14, 1.09e-12


def tight_options():
    return po.default_options(max_iterations=1000, function_tolerance=1e-15, gradient_tolerance=1e-13, parameter_tolerance=1e-14)


def scene_of(name):
    key = SCENES[name]
    return ref.ragged_scene() if key[0] == "ragged" else ref.scene(*key)


def problem_of(c):
    return fr.Problem(fr.fisheye_model, c["off"], c["uv"], c["xyz"], 0.0, fr.K8_HELD)


@functools.lru_cache(maxsize=None)
def truth_solve(name, tight=True):
    """lm_solve from the generator's poses, true fx fy px py, k = 0: (intr, q, t, summary)."""
    c = scene_of(name)
    return fr.lm_solve(problem_of(c), c["intr0_true"], c["q_true"], c["t_true"], tight_options() if tight else po.default_options())


@functools.lru_cache(maxsize=None)
def start_of(name, route="svd"):
    return ref.scene_start(SCENES[name], route=route)


def distances(a, b):
    """(relative cost difference, largest rotation [rad], largest translation difference, largest intrinsics difference relative to
    max(|slot|, 1)) between two (intr, q, t, summary) results."""
    ca, cb = a[3]["final_cost"], b[3]["final_cost"]
    dr = max(rs.rot_angle(rs.quat_to_R(p), rs.quat_to_R(q)) for p, q in zip(np.reshape(a[1], (-1, 4)), np.reshape(b[1], (-1, 4))))
    dt = float(np.abs(np.reshape(a[2], (-1, 3)) - np.reshape(b[2], (-1, 3))).max())
    ka, kb = np.asarray(a[0], dtype=np.float64), np.asarray(b[0], dtype=np.float64)
    return abs(ca - cb) / ca, dr, dt, float((np.abs(ka - kb) / np.maximum(np.abs(ka), 1.0)).max())


def margin(s):
    order = np.sort(s["score"][s["qualified"] == 1])
    return float((order[1] - order[0]) / order[0])


@pytest.mark.parametrize("name", sorted(SCENES))
def test_scene_geometry_and_the_conditions_on_a_test_scene(name):
    """The generator's largest angle and share beyond 90 degrees; every view valid, every candidate qualified, and the winner
    ahead of the runner-up by more than 1e-3 relative: the picked index is not a coin toss."""
    c, s = scene_of(name), start_of(name)
    assert c["max_angle_deg"] == pytest.approx(GEOMETRY[name][0], abs=0.05) and c["beyond_90"] == pytest.approx(GEOMETRY[name][1], abs=5e-4)
    assert c["uv"].dtype == np.float32 and c["xyz"].dtype == np.float32
    assert s["report"]["views_invalid"] == 0 and s["report"]["candidates_qualified"] == 24 and s["report"]["views_searched"] == len(c["off"]) - 1
    assert margin(s) > 1e-3, margin(s)


def test_two_scenes_have_5_to_20_percent_beyond_90_degrees_and_the_ragged_one_its_counts():
    assert sum(0.05 <= GEOMETRY[n][1] <= 0.20 for n in SCENES) >= 2
    assert tuple(np.diff(ref.ragged_scene()["off"])) == (4, 9, 25, 64, 65, 144)


@pytest.mark.parametrize("name", ["ragged", "85deg_seed6"])
def test_both_routes_to_the_null_vector_pick_the_same_candidate(name):
    a, b = start_of(name, "svd"), start_of(name, "gram")
    assert a["best"] == b["best"] and np.array_equal(a["qualified"], b["qualified"])
    assert np.allclose(a["score"], b["score"], rtol=1e-6)
    assert a["report"]["focal"] == b["report"]["focal"] and a["report"]["centre"] == b["report"]["centre"]


@pytest.mark.parametrize("name", sorted(SCENES))
def test_yardstick_solve_from_the_focal_search_ends_where_the_generators_poses_end(name):
    s = start_of(name)
    a = truth_solve(name)
    b = fr.lm_solve(problem_of(scene_of(name)), s["intr"], s["q"], s["t"], tight_options())
    d = distances(a, b)
    print(f"{name}: f {s['report']['focal']:.1f} (candidate {s['best']}, margin {100 * margin(s):.1f} %); {a[3]['iterations']} / {b[3]['iterations']} it, "
          f"{a[3]['termination']} / {b[3]['termination']}; cost rel {d[0]:.2e}, rotation {d[1]:.2e}, translation {d[2]:.2e}, intrinsics {d[3]:.2e}")
    assert a[3]["termination"] == b[3]["termination"]
    assert d[0] <= COST_REL and d[1] <= ROT_ABS and d[2] <= T_ABS and d[3] <= INTR_REL


@pytest.mark.parametrize("name", ZHANG_FAILS)
def test_zhang_start_ends_in_a_wrong_basin_where_the_focal_search_ends_on_the_minimum(name):
    """Default options. Zhang's pinhole K and poses with k = 0 end at more than 100 x the cost that the generator's poses reach;
    the focal-length start ends on it, in that solve's iterations + 1 at most."""
    c = scene_of(name)
    a = truth_solve(name, tight=False)
    K, qz, tz = po.zhang_init(c["off"], c["uv"], c["xyz"])
    z = fr.lm_solve(problem_of(c), np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2], 0, 0, 0, 0, 0], dtype=np.float64), qz.astype(np.float64),
                    tz.astype(np.float64), po.default_options())
    s = start_of(name)
    b = fr.lm_solve(problem_of(c), s["intr"], s["q"], s["t"], po.default_options())
    print(f"{name}: generator's poses {a[3]['iterations']} it {a[3]['final_cost']:.6g}; Zhang fx {K[0, 0]:.0f}, {z[3]['iterations']} it {z[3]['final_cost']:.6g} "
          f"(fx {z[0][0]:.0f}); focal search f {s['report']['focal']:.0f}, {b[3]['iterations']} it {b[3]['final_cost']:.6g}")
    assert z[3]["final_cost"] > 100 * a[3]["final_cost"]
    assert b[3]["final_cost"] == pytest.approx(a[3]["final_cost"], rel=1e-6) and b[3]["iterations"] <= a[3]["iterations"] + 1


def test_closed_form_routes_differ_by_this_much_on_the_pair_scene():
    """The SVD-to-Gram distance of the reference on the (view, candidate) pairs of the GPU test, refine_iterations = 0: the kernel
    (Gram route) is held to 16 x it there. Printed for DESIGN 4.19."""
    c = ref.pairs_scene()
    for C in (1, 2, 24):
        a = ref.start(c["off"], c["uv"], c["xyz"], centre=c["centre"], candidates=C, search_views=0, refine_iterations=0, route="svd")
        b = ref.start(c["off"], c["uv"], c["xyz"], centre=c["centre"], candidates=C, search_views=0, refine_iterations=0, route="gram")
        dr = dt = 0.0
        for key, (kind, R, t, cost) in a["pairs"].items():
            kb, Rb, tb, _ = b["pairs"][key]
            assert kind == kb and kind == (ref.GENERAL if key[1] >= 6 else ref.PLANAR)
            dr, dt = max(dr, rs.rot_angle(R, Rb)), max(dt, float(np.linalg.norm(t - tb)))
        ds = float(np.max(np.abs(a["score"] - b["score"]) / np.abs(a["score"])))
        print(f"C = {C}: {len(a['pairs'])} pairs, SVD vs Gram {dr:.2e} rad / {dt:.2e} m, scores {ds:.2e} relative")
        assert a["best"] == b["best"]
    # the pixel moved onto the centre has the bearing (0, 0, 1) exactly
    i = int(c["off"][3]) + 30
    assert np.array_equal(ref.bearings(c["uv"][i], c["centre"], 500.0)[0], [0.0, 0.0, 1.0])


def test_pick_rules():
    f = np.array([3.0, 2.0, 1.0])
    kinds = np.array([[1, 0, 1], [1, 0, 1], [1, 0, 0]])          # view 1 is invalid for every candidate; candidate 2 loses view 2
    costs = np.array([[1.0, 0.0, 1.0], [2.0, 0.0, 2.5], [0.1, 0.0, 0.0]])
    best, score, qualified = ref.pick(f, kinds, costs)
    assert list(qualified) == [1, 1, 0] and list(score) == [18.0, 18.0, pytest.approx(0.1)] and best == 0   # the tie goes to the lowest index
    assert ref.pick(f, np.zeros((3, 2), dtype=int), np.zeros((3, 2)))[0] == 0   # (no view has a pose anywhere: nothing disqualifies)
    assert ref.searched(12, 5) == [0, 2, 4, 7, 9] and ref.searched(12, 0) == list(range(12)) and ref.searched(3, 32) == [0, 1, 2]
    assert np.allclose(ref.candidates(3.0, 0.3, 3.0, 1), [10.0]) and np.allclose(ref.candidates(3.0, 0.3, 3.0, 2), [10.0, 1.0])
