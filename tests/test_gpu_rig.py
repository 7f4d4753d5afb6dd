"""Parity of the HIP rig path (cc_rig_*, through the C ABI) against the CPU oracle.
Scenario: src/test_extrinsics_calibrator.cpp:48-134 at several sizes. Tolerances (round 5) at the MEASURED floor of the path
with its approximate arithmetic in (1 / z from the hardware estimate + two Newton steps, Huber tail from refined v_rsq_f64,
pivots and quaternion norms through rsqrt_pos) -- profiles/r05/rig_deviation.jsonl (scripts/rig_deviation.py: seven shapes up to
BASELINE configs[3] with 1.6 - 22 % of the blocks in the Huber tail, default build and -DCC_RIG_EXACT_DIV -DCC_RIG_EXACT_HUBER
side by side -- the two builds deviate alike, i.e. what is left is the order of the sums): identical iteration count and
accept / reject sequence; per-iteration costs <= 2e-12 relative (asserted 1e-10); converged poses <= 7e-15 (asserted 1e-11; were
1e-9); per-observation costs <= 3.3e-10 relative (asserted 1e-9: three times the floor); final cost <= 3e-14 (asserted 1e-12)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from camera_calibrator_amd import capi
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

TIGHT = dict(function_tolerance=1e-15, gradient_tolerance=1e-13, parameter_tolerance=1e-14, max_iterations=200)


def _inputs(sc):
    cq, ct = po.affine_to_qt(sc["cam_T"])
    fq, ft = po.affine_to_qt(sc["frame_T"])
    return cq, ct, fq, ft


def _both(sc, n_cams, huber_a=capi.HUBER_A, frozen=None, **kw):
    cq, ct, fq, ft = _inputs(sc)
    frozen = sc["cam_frozen"] if frozen is None else frozen
    args = (n_cams, sc["frame_offsets"], sc["obs_cam"], sc["obs_world"], sc["obs_uv"], sc["world_xyz"], cq, ct, frozen, fq, ft)
    g = capi.rig_optimize(*args, huber_a=huber_a, options=capi.default_options(max_iterations=1000, **kw))
    o = po.rig_solve(*args, huber_a=huber_a, options=po.default_options(max_iterations=1000, **kw))
    return g, o


def _assert_same(g, o, atol=1e-11):
    assert g[5]["iterations"] == o[5]["iterations"] and g[5]["termination"] == o[5]["termination"]
    assert [l["accepted"] for l in g[5]["log"]] == [l["accepted"] for l in o[5]["log"]]
    assert np.allclose([l["cost"] for l in g[5]["log"]], [l["cost"] for l in o[5]["log"]], rtol=1e-10)
    for k in range(4):
        assert np.abs(g[k] - o[k]).max() < atol
    assert np.allclose(g[4], o[4], rtol=1e-9, atol=1e-18), np.abs(g[4] / np.maximum(o[4], 1e-300) - 1).max()
    assert np.isclose(g[5]["final_cost"], o[5]["final_cost"], rtol=1e-12)


def _noise_floor_step(log):
    """Step norm of the first iteration of a tight solve whose cost change is below the rounding of the cost sum (1e-13
    relative): from there on which steps are accepted depends on the order of the sums, and every implementation ends within
    that step of the minimiser -- on its own iterate (tests/test_golden.py::_rigk_noise_floor, same bound)."""
    for l in log:
        if abs(l["cost_change"]) < 1e-13 * l["cost"]:
            return float(l["step_norm"])
    return None


@pytest.mark.parametrize("cams,frames,pts", [(2, 50, 4), (2, 1000, 4), (4, 40, 30), (3, 20, 300), (8, 25, 70)])
def test_rig_default_options_match_oracle(cams, frames, pts):
    sc = po.rig_scenario(cams, frames, pts)
    g, o = _both(sc, cams)
    _assert_same(g, o)
    assert np.array_equal(g[0][0], o[0][0]) and np.array_equal(g[1][0], o[1][0])   # frozen camera untouched


@pytest.mark.parametrize("waves", [1, 2, 4])
@pytest.mark.parametrize("cams,frames,pts", [(3, 30, 150), (5, 12, 70)])
def test_rig_sweep_workgroup_sizes_give_the_same_solve(monkeypatch, waves, cams, frames, pts):
    """The poses-only sweep runs with 1, 2 or 4 waves per (frame, camera) group depending on the problem's shape
    (cc_rig.hip, rig_create_impl); every variant must match the oracle, whatever the heuristic would pick."""
    monkeypatch.setenv("CC_RIG_SWEEP_WG_WAVES", str(waves))
    sc = po.rig_scenario(cams, frames, pts)
    g, o = _both(sc, cams)
    _assert_same(g, o)


def test_rig_converged_minimiser_and_golden():
    import os
    gld = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rig_2x50x4.npz"))
    g = capi.rig_optimize(2, gld["frame_offsets"], gld["obs_cam"], gld["obs_world"], gld["obs_uv"], gld["world_xyz"],
                          gld["cam_q0"], gld["cam_t0"], gld["cam_frozen"], gld["frame_q0"], gld["frame_t0"],
                          options=capi.default_options(max_iterations=1000, function_tolerance=1e-15,
                                                       gradient_tolerance=1e-13, parameter_tolerance=1e-14))
    assert np.isclose(g[5]["final_cost"], float(gld["final_cost"]), rtol=1e-10)
    assert np.abs(g[1] - gld["cam_t"]).max() < 1e-9 and np.abs(g[0] - gld["cam_q"]).max() < 1e-9
    assert np.abs(g[3] - gld["frame_t"]).max() < 1e-8
    assert np.allclose(g[4], gld["obs_cost"], rtol=1e-5, atol=1e-13)  # frames with 8 observations for 6 dof: residual-level sensitivity at the flat minimum
    # float write-back of the camera transform (extrinsics_calibrator.cpp:228-256)
    assert np.abs(po.qt_to_affine(g[0], g[1]) - gld["cam_T_out"]).max() <= 1.2e-7


def test_rig_huber_off_equals_l2():
    sc = po.rig_scenario(2, 30, 4)
    g, o = _both(sc, 2, huber_a=1e6)
    _assert_same(g, o)


@pytest.mark.parametrize("waves,pts", [(None, 6), (1, 90), (2, 90), (4, 90)])
def test_rig_ragged_visibility_unobserved_camera_and_empty_frame(monkeypatch, waves, pts):
    """(with the sweep's workgroup size forced: groups of ragged size, more than one 64-observation chunk)"""
    if waves is not None:
        monkeypatch.setenv("CC_RIG_SWEEP_WG_WAVES", str(waves))
    sc = po.rig_scenario(3, 20, pts)
    rng = np.random.default_rng(0)
    keep = (sc["obs_cam"] != 2) & (rng.uniform(size=len(sc["obs_cam"])) > 0.3)   # camera 2 sees nothing; random drop-outs
    off0 = sc["frame_offsets"]
    keep[off0[7]:off0[8]] = False                                               # frame 7 has no observation
    counts = [np.count_nonzero(keep[off0[f]:off0[f + 1]]) for f in range(20)]
    sc2 = dict(sc, obs_cam=sc["obs_cam"][keep], obs_world=sc["obs_world"][keep], obs_uv=sc["obs_uv"][keep],
               frame_offsets=np.concatenate([[0], np.cumsum(counts)]).astype(np.int64))
    g, o = _both(sc2, 3)
    _assert_same(g, o)
    cq, ct, fq, ft = _inputs(sc)
    assert np.array_equal(g[0][2], cq[2]) and np.array_equal(g[2][7], fq[7]) and np.array_equal(g[3][7], ft[7])


def test_rig_handle_api_reset_and_determinism():
    sc = po.rig_scenario(2, 60, 4)
    cq, ct, fq, ft = _inputs(sc)
    prob = capi.RigProblem(2, sc["frame_offsets"], sc["obs_cam"], sc["obs_world"], sc["obs_uv"], sc["world_xyz"], sc["cam_frozen"])
    prob.set_state(cq, ct, fq, ft)
    c0 = prob.eval()
    s1 = prob.solve(); r1 = prob.get_state()
    prob.reset()
    assert prob.eval() == c0
    s2 = prob.solve(); r2 = prob.get_state()
    prob.close()
    assert s1["final_cost"] == s2["final_cost"] and all(np.array_equal(a, b) for a, b in zip(r1, r2))
    assert np.isclose(s1["initial_cost"], c0, rtol=1e-12) and np.isclose(r1[4].sum(), s1["final_cost"], rtol=1e-12)


def test_rig_rccl_path_with_a_single_rank_communicator():
    """The multi-GPU launch sequence of the rig path (reduce -> all-reduce -> solve ... stats -> all-reduce
    -> init/decide) with a 1-rank RCCL communicator must reproduce the single-GPU solve."""
    sc = po.rig_scenario(3, 40, 6)
    cq, ct, fq, ft = _inputs(sc)
    prob = capi.RigProblem(3, sc["frame_offsets"], sc["obs_cam"], sc["obs_world"], sc["obs_uv"], sc["world_xyz"], sc["cam_frozen"])
    prob.set_state(cq, ct, fq, ft)
    s0 = prob.solve(); r0 = prob.get_state()
    prob.comm_init(capi.comm_get_unique_id(), 0, 1)
    prob.reset()
    s1 = prob.solve(); r1 = prob.get_state()
    prob.close()
    assert s1["iterations"] == s0["iterations"] and s1["termination"] == s0["termination"]
    assert np.allclose([l["cost"] for l in s1["log"]], [l["cost"] for l in s0["log"]], rtol=1e-12)
    for a, b in zip(r0, r1):
        assert np.allclose(a, b, rtol=1e-12, atol=1e-14)


def test_rig_c4_full_size_matches_oracle():
    """BASELINE.json configs[3] (4 cameras x 400 frames x 300 points, 480k observations) against the
    oracle: same trajectory, same minimiser (the oracle needs ~2 s for it)."""
    sc = po.rig_scenario(4, 400, 300)
    g, o = _both(sc, 4)
    _assert_same(g, o)


def test_rig_c5_full_size_against_the_committed_oracle_result_and_properties():
    """BASELINE.json configs[4] (8 cameras x 2000 frames x 500 points, 8M observations). The oracle needs
    a minute for it, so its answer is a committed fixture (tests/golden/make_rig_c5.py): same trajectory,
    same minimiser. Plus size-independent properties: the frozen camera is untouched, the per-observation
    costs add up to the reported cost, a second solve from the solution is a fixed point.
    (With the reference's tolerances this scenario stops at cost 450.27 with only camera 1 back at the
    planted rig; the oracle does exactly the same.)"""
    import os
    gld = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rig_c5_oracle.npz"))
    C_ = int(gld["cams"])
    sc = po.rig_scenario(C_, int(gld["frames"]), int(gld["pts"]))
    cq, ct, fq, ft = _inputs(sc)
    prob = capi.RigProblem(C_, sc["frame_offsets"], sc["obs_cam"], sc["obs_world"], sc["obs_uv"], sc["world_xyz"], sc["cam_frozen"])
    prob.set_state(cq, ct, fq, ft)
    s1 = prob.solve(capi.default_options(max_iterations=1000))
    r1 = prob.get_state()
    assert s1["termination"] == str(gld["termination"]) and s1["iterations"] == int(gld["iterations"])
    assert [l["accepted"] for l in s1["log"]] == list(gld["accepted"])
    # (tolerances at the measured floor of this very configuration against the live oracle, profiles/r05/rig_deviation.jsonl: costs
    # of 8 M-term sums 5.7e-11, poses <= 1e-13, per-observation costs 2e-9; were 1e-9 / 1e-9 / 1e-7)
    assert np.allclose([l["cost"] for l in s1["log"]], gld["costs"], rtol=2e-10)
    assert np.isclose(s1["initial_cost"], float(gld["initial_cost"]), rtol=1e-10)
    assert np.isclose(s1["final_cost"], float(gld["final_cost"]), rtol=1e-10)
    assert np.abs(r1[0] - gld["cam_q"]).max() < 1e-11 and np.abs(r1[1] - gld["cam_t"]).max() < 1e-11
    pick = gld["frame_pick"]
    assert np.abs(r1[2][pick] - gld["frame_q"]).max() < 1e-11 and np.abs(r1[3][pick] - gld["frame_t"]).max() < 1e-11
    assert np.allclose(r1[4][:64], gld["obs_cost_head"], rtol=1e-8, atol=1e-14)
    assert np.isclose(r1[4].sum(), float(gld["obs_cost_sum"]), rtol=1e-10)
    # properties
    assert np.array_equal(r1[0][0], cq[0]) and np.array_equal(r1[1][0], ct[0])
    assert np.isclose(r1[4].sum(), s1["final_cost"], rtol=1e-10) and r1[4].shape == (8_000_000,)
    prob.set_state(r1[0], r1[1], r1[2], r1[3])
    s2 = prob.solve(capi.default_options(max_iterations=1000))
    r2 = prob.get_state()
    prob.close()
    assert s2["iterations"] <= 2 and s2["final_cost"] <= s1["final_cost"] * (1 + 1e-9)
    assert np.abs(r2[1] - r1[1]).max() < 1e-6


def test_rig_many_cameras_only_optimised_ones_cost_columns():
    """The reference takes any number of cameras (extrinsics_calibrator.cpp:9-17). Here only observed, non-frozen
    cameras own columns: 16 observed cameras solve (90 shared coordinates), and so does the state the reference's
    own test leaves behind -- Serialize -> Parse into the same object doubles the cameras (Parse does not clear
    them, extrinsics_calibrator.cpp:348-351): ids C..2C-1 are unobserved duplicates, the copy of camera 0 frozen."""
    sc = po.rig_scenario(16, 30, 12)
    g, o = _both(sc, 16)
    _assert_same(g, o)
    sc = po.rig_scenario(6, 40, 10)
    cq, ct, fq, ft = _inputs(sc)
    cq2, ct2 = np.concatenate([cq, cq]), np.concatenate([ct, ct])
    frozen2 = np.concatenate([sc["cam_frozen"], sc["cam_frozen"]])
    args = (12, sc["frame_offsets"], sc["obs_cam"], sc["obs_world"], sc["obs_uv"], sc["world_xyz"], cq2, ct2, frozen2, fq, ft)
    g = capi.rig_optimize(*args, options=capi.default_options(max_iterations=1000))
    o = po.rig_solve(*args, options=po.default_options(max_iterations=1000))
    _assert_same(g, o)
    assert np.array_equal(g[0][6:], cq) and np.array_equal(g[1][6:], ct)            # the duplicates never move
    g6, _ = _both(sc, 6)
    assert np.abs(g[1][:6] - g6[1]).max() < 1e-12 and g[5]["iterations"] == g6[5]["iterations"]
    # 200 idle cameras around two live ones
    sc = po.rig_scenario(2, 25, 8)
    cq, ct, fq, ft = _inputs(sc)
    pad_q, pad_t = np.tile([1.0, 0, 0, 0], (200, 1)), np.zeros((200, 3))
    args = (202, sc["frame_offsets"], sc["obs_cam"] * np.uint32(201), sc["obs_world"], sc["obs_uv"], sc["world_xyz"],
            np.concatenate([cq[:1], pad_q, cq[1:]]), np.concatenate([ct[:1], pad_t, ct[1:]]),
            np.concatenate([[1], np.zeros(201, dtype=np.uint8)]).astype(np.uint8), fq, ft)
    g = capi.rig_optimize(*args, options=capi.default_options(max_iterations=1000))
    o = po.rig_solve(*args, options=po.default_options(max_iterations=1000))
    _assert_same(g, o)


def test_rig_twenty_two_cameras_take_the_large_elimination_variant():
    """22 observed cameras (21 optimised: 126 shared coordinates, the limit is 127) carry 594 direct-sum entries, more
    than the small-register variant of the elimination holds: the variant with LDS accumulators runs (cc_rig.hip,
    k_rig_elim<HK, 24>), the factorisation works on two rows per lane (S > 64)."""
    sc = po.rig_scenario(22, 24, 10)
    g, o = _both(sc, 22)
    _assert_same(g, o)


@pytest.mark.parametrize("cams", [12, 13, 18, 21])
def test_reduced_systems_between_65_and_127_coordinates_at_the_edges_of_the_panel_loop(cams):
    """Round 6: the factorisation of 65 .. 127 shared coordinates runs its eight-column panels with look-ahead (the next panel's
    tile column first, then the panel on wave 0 next to the rest of the trailing update) and its backward substitution in two
    phases (rows >= 64, then rows < 64). Sizes chosen for the loop's edges: 12 cameras = 66 coordinates (eight full panels and a
    last one of two columns, two rows beyond 64), 13 = 72 (nine panels exactly), 18 = 102 (six columns in the last panel, a
    partial block of the upper phase), 21 = 120 (fifteen panels exactly). Same bar as every other rig test."""
    sc = po.rig_scenario(cams, 20, 10)
    g, o = _both(sc, cams)
    _assert_same(g, o)


@pytest.mark.parametrize("cams", [6, 7, 9, 10, 11])
def test_reduced_systems_of_30_to_60_coordinates_at_both_ends_of_the_four_column_factorisation(cams):
    """6 (cams - 1) shared coordinates through chol_block4 (24 < S <= 63, cc_rig_dev.hpp): 6 cameras = 30, the first size
    after the register-row solve (two 16-row tile rows, a last block of two columns); 7 = 36 and 9 = 48 (three tile rows:
    48 + the right-hand side's row opens the fourth); 10 = 54 and 11 = 60, the top of the routine for this handle (four tile
    rows, ten tiles over three waves, the last block full). The oracle on these: FUNCTION tolerance after 4 to 10
    iterations, one rejected step each. Same bar as every other rig test."""
    sc = po.rig_scenario(cams, 12, 8)
    g, o = _both(sc, cams)
    _assert_same(g, o)


def test_rig_kernel_profile_of_a_solve():
    sc = po.rig_scenario(3, 40, 20)
    cq, ct, fq, ft = _inputs(sc)
    prob = capi.RigProblem(3, sc["frame_offsets"], sc["obs_cam"], sc["obs_world"], sc["obs_uv"], sc["world_xyz"], sc["cam_frozen"])
    prob.set_state(cq, ct, fq, ft)
    s0 = prob.solve()
    prob.reset()
    s1 = prob.solve(capi.default_options(max_iterations=1000, profile_kernels=1))
    prob.close()
    # (the profiled solve runs the three-kernel form, the first one the persistent kernel: the partial rows are added in
    # another order)
    assert s1["iterations"] == s0["iterations"] and np.isclose(s1["final_cost"], s0["final_cost"], rtol=1e-12)
    # (launches of a chunk that follow the terminating iteration return at once but are still counted)
    assert s1["kernel_launches"]["sweep"] >= s1["iterations"] + 1 and s1["kernel_ms"]["sweep"] > 0 and s1["kernel_ms"]["elim"] > 0


@pytest.mark.parametrize("cams,frames,pts", [(3, 24, 8), (4, 60, 40)])
def test_rig_huber_active_at_the_minimiser_matches_oracle(cams, frames, pts):
    """Planted outliers (tests/helpers.py rig_outlier_case): > 5 % of the residual blocks sit in the linear tail of the
    Huber loss at the solution, so loss scaling and corrector (extrinsics_calibrator.cpp:175-176) shape the fixed point
    itself. The oracle's fixed point for the (3, 24, 8) case is pinned independently on the CPU
    (tests/test_oracle_rig_huber.py: numpy restatement of the objective, vanishing gradient, scipy finds nothing
    lower); here the HIP path must follow the oracle through the same trajectory, default and tight options."""
    from tests.helpers import rig_outlier_case
    sc = rig_outlier_case(cams, frames, pts)
    args = (cams, sc["frame_offsets"], sc["obs_cam"], sc["obs_world"], sc["obs_uv"], sc["world_xyz"],
            sc["cam_q0"], sc["cam_t0"], sc["cam_frozen"], sc["frame_q0"], sc["frame_t0"])
    a = capi.HUBER_A

    def tail_ok(g):
        tail = g[4] > 0.5 * a * a * (1 + 1e-9)          # 1/2 rho(s) > 1/2 a^2  <=>  s > a^2
        assert tail.mean() > 0.05 and tail[sc["outlier"]].mean() > 0.9
        assert np.isclose(g[4].sum(), g[5]["final_cost"], rtol=1e-12)

    # the reference's options (extrinsics_calibrator.cpp:206-213): the whole trajectory
    g = capi.rig_optimize(*args, huber_a=a, options=capi.default_options(max_iterations=1000))
    o = po.rig_solve(*args, huber_a=a, options=po.default_options(max_iterations=1000))
    _assert_same(g, o)
    tail_ok(g)
    # converged to the rounding floor: the minimiser itself. (How many iterations the last digits of the cost take, and
    # which tolerance fires, is rounding noise there -- the sweep's 1/z is within an ulp or two of the oracle's division,
    # and a residual a hair from the kink |r| = a may sit on either side -- so the trajectory is not compared.)
    kw = dict(TIGHT, function_tolerance=1e-16, max_iterations=500)
    g = capi.rig_optimize(*args, huber_a=a, options=capi.default_options(**kw))
    o = po.rig_solve(*args, huber_a=a, options=po.default_options(**kw))
    assert g[5]["termination"] in ("FUNCTION", "GRADIENT", "PARAMETER")
    # the iterate: within the step at which the oracle's cost changes drop into the rounding of the cost sum -- the bound the data
    # gives (measured: poses 9e-16 .. 1.6e-11 against floors 6e-9 .. 5e-8, profiles/r05/rig_deviation.jsonl), not 1e-6 / 1e-4
    floor = _noise_floor_step(o[5]["log"])
    assert floor is not None and 1e-10 < floor < 1e-6, floor
    assert np.isclose(g[5]["final_cost"], o[5]["final_cost"], rtol=1e-13)
    for k in range(4):
        assert np.abs(g[k] - o[k]).max() < floor, (k, np.abs(g[k] - o[k]).max(), floor)
    # per-observation costs 1/2 rho(|r|^2), |r| <= 0.06 here: d cost <= |r| |J| |d x| -- below the floor itself
    assert np.abs(g[4] - o[4]).max() < floor
    tail_ok(g)


@pytest.mark.parametrize("cams,frames,pts", [(23, 30, 6), (32, 24, 10), (40, 12, 8)])
def test_rigs_with_more_than_21_optimised_cameras_match_the_oracle(cams, frames, pts):
    """The reference takes any number of cameras (extrinsics_calibrator.cpp:9-17). Beyond 21 optimised ones the reduced
    system has more than 127 coordinates and the plain kernels take over (k_rig_elim_big, k_rig_solve_big; DESIGN.md
    section 4): 22 optimised cameras = 132 coordinates, 31 = 186 (packed triangle in LDS), 39 = 234 (reduced system in
    global memory). Same bar as every other rig test."""
    sc = po.rig_scenario(cams, frames, pts)
    g, o = _both(sc, cams)
    _assert_same(g, o)
    assert np.array_equal(g[0][0], o[0][0]) and np.array_equal(g[1][0], o[1][0])   # frozen camera untouched
    g, o = _both(sc, cams, **{k: v for k, v in TIGHT.items() if k != "max_iterations"})
    assert np.isclose(g[5]["final_cost"], o[5]["final_cost"], rtol=1e-12)
    bound = _noise_floor_step(o[5]["log"]) or 1e-8   # (measured at 23 cameras: 1e-15 against a floor of 4e-9; was 1e-8)
    for k in range(4):
        assert np.abs(g[k] - o[k]).max() < bound


def test_more_than_255_shared_coordinates_are_refused_loudly():
    sc = po.rig_scenario(44, 6, 6)     # 43 optimised cameras = 258 coordinates
    cq, ct = po.affine_to_qt(sc["cam_T"])
    fq, ft = po.affine_to_qt(sc["frame_T"])
    with pytest.raises(capi.CcError, match="at most 255"):
        capi.rig_optimize(44, sc["frame_offsets"], sc["obs_cam"], sc["obs_world"], sc["obs_uv"], sc["world_xyz"], cq, ct, sc["cam_frozen"], fq, ft)


@pytest.mark.skipif(os.environ.get("CC_RIG_FORCE_BIG", "0") != "0", reason="already running on the plain kernels")
def test_plain_kernels_pass_the_rig_suites_on_problems_the_tuned_kernels_solve():
    """CC_RIG_FORCE_BIG=1 sends every single-GPU rig problem through k_rig_elim_big / k_rig_solve_big: both rig suites (poses,
    robust loss, held cameras, shared and per-camera intrinsics, held intrinsics) must pass on them too. The multi-GPU
    tests are left out (the plain kernels refuse an exchange)."""
    env = dict(os.environ, CC_RIG_FORCE_BIG="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_rig.py", "tests/test_gpu_rigk.py", "-q", "-m", "gpu", "-x",
                        "-k", "not rccl and not exchange and not plain_kernels and not every_form and not rerun and not ranks", "-p", "no:cacheprovider"],
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]


@pytest.mark.parametrize("seed", list(range(12)))
def test_random_small_rigs_match_the_oracle(seed):
    """Random small rigs -- 1 to 4 cameras, 1 to 70 frames (1, 2 or 4 of them per workgroup of the lean persistent kernel,
    a last workgroup that is not full), 1 to 90 points, random drop-outs, sometimes a camera that sees nothing, an empty
    frame, a second frozen camera, the robust loss on or off -- against the oracle: same trajectory, same minimiser."""
    rng = np.random.default_rng(1000 + seed)
    cams = int(rng.integers(1, 5))
    frames = int(rng.integers(1, 71))
    pts = int(rng.integers(1, 91))
    sc = po.rig_scenario(cams, frames, pts)
    keep = rng.uniform(size=len(sc["obs_cam"])) > rng.choice([0.0, 0.2, 0.5])
    if cams >= 3 and rng.uniform() < 0.4:
        keep &= sc["obs_cam"] != cams - 1                       # the last camera sees nothing
    off0 = sc["frame_offsets"]
    if frames >= 3 and rng.uniform() < 0.5:
        f_empty = int(rng.integers(0, frames))
        keep[off0[f_empty]:off0[f_empty + 1]] = False           # a frame without observations
    if not keep.any():
        keep[0] = True
    counts = [np.count_nonzero(keep[off0[f]:off0[f + 1]]) for f in range(frames)]
    sc2 = dict(sc, obs_cam=sc["obs_cam"][keep], obs_world=sc["obs_world"][keep], obs_uv=sc["obs_uv"][keep],
               frame_offsets=np.concatenate([[0], np.cumsum(counts)]).astype(np.int64))
    frozen = np.array(sc["cam_frozen"], dtype=np.uint8).copy()
    if cams >= 3 and rng.uniform() < 0.3:
        frozen[1] = 1
    huber = capi.HUBER_A if rng.uniform() < 0.7 else 1e6
    g, o = _both(sc2, cams, huber_a=huber, frozen=frozen)
    _assert_same(g, o)


def test_small_rig_among_more_cameras_than_it_observes():
    """Seven cameras, four of them observed: the lean persistent form takes it (its limits count OBSERVED cameras), and the
    control workgroup's broadcast carries the records of all seven (the slot it lands in once held four)."""
    sc = po.rig_scenario(7, 24, 12)
    keep = sc["obs_cam"] < 4
    off0 = sc["frame_offsets"]
    counts = [np.count_nonzero(keep[off0[f]:off0[f + 1]]) for f in range(24)]
    sc2 = dict(sc, obs_cam=sc["obs_cam"][keep], obs_world=sc["obs_world"][keep], obs_uv=sc["obs_uv"][keep],
               frame_offsets=np.concatenate([[0], np.cumsum(counts)]).astype(np.int64))
    if not any(os.environ.get(k) for k in ("CC_RIG_PERSIST", "CC_RIG_FORCE_BIG")):
        prob = capi.RigProblem(7, sc2["frame_offsets"], sc2["obs_cam"], sc2["obs_world"], sc2["obs_uv"], sc2["world_xyz"], sc2["cam_frozen"])
        assert prob.solver_form() == 2
        prob.close()
    g, o = _both(sc2, 7)
    _assert_same(g, o)
    cq, ct, fq, ft = _inputs(sc)
    assert all(np.array_equal(g[0][c], cq[c]) and np.array_equal(g[1][c], ct[c]) for c in (4, 5, 6))   # unobserved: untouched


def test_rig_with_no_camera_held_constant_runs_the_lean_form_at_24_shared_coordinates():
    """Four cameras, none frozen: 24 shared coordinates, the most the lean persistent form takes. The problem has a gauge
    freedom (the damping makes every step well defined); the trajectory is compared with the oracle's over the first
    iterations, where both are far from the flat directions' noise."""
    sc = po.rig_scenario(4, 30, 20)
    frozen = np.zeros(4, dtype=np.uint8)
    cq, ct, fq, ft = _inputs(sc)
    prob = capi.RigProblem(4, sc["frame_offsets"], sc["obs_cam"], sc["obs_world"], sc["obs_uv"], sc["world_xyz"], frozen)
    if not any(os.environ.get(k) for k in ("CC_RIG_PERSIST", "CC_RIG_FORCE_BIG")):
        assert prob.solver_form() == 2
    prob.close()
    g, o = _both(sc, 4, frozen=frozen)
    n = min(6, len(g[5]["log"]), len(o[5]["log"]))
    assert [l["accepted"] for l in g[5]["log"][:n]] == [l["accepted"] for l in o[5]["log"][:n]]
    assert np.allclose([l["cost"] for l in g[5]["log"][:n]], [l["cost"] for l in o[5]["log"][:n]], rtol=1e-8)
    assert np.isclose(g[5]["final_cost"], o[5]["final_cost"], rtol=1e-6)


def test_four_frame_lean_workers_on_a_four_camera_rig_when_forced(monkeypatch):
    """Four frames per workgroup x four groups per frame = sixteen waves a worker: the shape the default rule no longer picks
    (round 6) stays correct when CC_RIG_PERSIST=1 asks for it."""
    if os.environ.get("CC_RIG_FORCE_BIG"):
        pytest.skip("the plain large-rig kernels are forced in this environment")
    monkeypatch.setenv("CC_RIG_PERSIST", "1")
    sc = po.rig_scenario(4, 600, 12)
    prob = capi.RigProblem(4, sc["frame_offsets"], sc["obs_cam"], sc["obs_world"], sc["obs_uv"], sc["world_xyz"], sc["cam_frozen"])
    assert prob.solver_form() == 2
    prob.close()
    g, o = _both(sc, 4)
    _assert_same(g, o)


def _form_of(cams, frames, pts, env):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from camera_calibrator_amd import capi\nfrom oracle import pyoracle as po\n"
            "sc = po.rig_scenario(%d, %d, %d)\n"
            "p = capi.RigProblem(%d, sc['frame_offsets'], sc['obs_cam'], sc['obs_world'], sc['obs_uv'], sc['world_xyz'], sc['cam_frozen'])\n"
            "print('form', p.solver_form())\n") % (root, cams, frames, pts, cams)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return int(r.stdout.split("form")[1].split()[0])


_NESTED = any(os.environ.get(k) for k in ("CC_RIG_PERSIST", "CC_RIG_FORCE_BIG"))


@pytest.mark.skipif(_NESTED, reason="a forced solver form is already in the environment")
def test_the_rig_suite_in_every_form_of_the_solver():
    """A small rig (at most 4 observed cameras, 24 shared coordinates, ~1020 frames) is solved by ONE launch of the lean
    persistent kernel (k_rig_persist_w + k_rig_persist_ctl) by default -- which is what every other test in this file then
    exercises. CC_RIG_PERSIST=0: the three kernels per LM iteration on everything. The rig suite again, in that form.
    (Round 3's third form, the glued persistent kernel behind CC_RIG_PERSIST=1, is gone: CC_RIG_PERSIST=1 is the default.)"""
    env = dict(os.environ, CC_RIG_PERSIST="0")
    assert _form_of(3, 40, 20, dict(os.environ)) == 2
    assert _form_of(3, 40, 20, dict(os.environ, CC_RIG_PERSIST="1")) == 2
    assert _form_of(3, 40, 20, env) == 0
    assert _form_of(8, 30, 10, dict(os.environ)) == 0      # 42 shared coordinates: not the lean form's
    # round 6: where the lean form FITS but does not PAY (four frames per workgroup -- more than 510 frames -- unless the rig has two
    # observed cameras and a handful of points per frame: profiles/r06/lean_vs_three_kernel_grid.txt) the three kernels run by
    # default; CC_RIG_PERSIST=1 still forces the lean form wherever it fits (and the suite below solves 2 x 1000 x 4 with it)
    assert _form_of(4, 800, 12, dict(os.environ)) == 0
    assert _form_of(4, 800, 12, dict(os.environ, CC_RIG_PERSIST="1")) == 2
    assert _form_of(4, 500, 12, dict(os.environ)) == 2
    assert _form_of(2, 1000, 4, dict(os.environ)) == 2
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_rig.py", "-q", "-m", "gpu", "-x",
                        "-k", "not rccl and not exchange and not plain_kernels and not every_form and not ranks and not rerun", "-p", "no:cacheprovider"],
                       cwd=root, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]


@pytest.mark.skipif(_NESTED, reason="a forced solver form is already in the environment")
def test_lean_persistent_solve_that_cannot_get_its_grid_is_rerun_in_the_three_kernel_form():
    """The lean persistent form needs its workers AND the control workgroup's launch resident at once. When a wait inside
    it gives up (42 ms for the control to appear at all, 1.3 s afterwards) nothing has been written back -- frame poses return
    to global memory only at the end of a solve that did not fail, the cameras of the starting point were put aside -- and
    cc_rig_solve runs the solve again, three kernels per iteration. A give-up in the first round demotes the handle the
    second time in a row (a host thread that lost its time slice between the two launches says nothing about the device).
    Forced by not launching the control workgroup (CC_RIG_PERSIST_TEST_NO_CONTROL, read once per process: a process of its own)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    # Round 6: what a give-up says is remembered per DEVICE as well (persist_device_try, cc_common.hpp: the solves after it are
    # turned away from the lean form for a window -- here 1 solve / 0 ms, doubling -- and one solve then probes again), so the
    # sequence below alternates: give-up, turned away, probe.
    code = ("import sys, time; sys.path.insert(0, %r)\n"
            "import numpy as np\nimport ctypes as C\nfrom camera_calibrator_amd import capi\nfrom oracle import pyoracle as po\n"
            "sc = po.rig_scenario(3, 40, 20)\n"
            "cq, ct = po.affine_to_qt(sc['cam_T']); fq, ft = po.affine_to_qt(sc['frame_T'])\n"
            "args = (3, sc['frame_offsets'], sc['obs_cam'], sc['obs_world'], sc['obs_uv'], sc['world_xyz'])\n"
            "o = po.rig_solve(*args, cq, ct, sc['cam_frozen'], fq, ft, options=po.default_options(max_iterations=1000))\n"
            # a ONE-SHOT call destroys its handle before it returns -- its caller asks cc_last_call_solver_status (round 5, ADVICE)
            "t0 = time.time(); r = capi.rig_optimize(*args, cq, ct, sc['cam_frozen'], fq, ft); dt = time.time() - t0\n"
            "assert 0.03 < dt < 1.0, dt\n"
            "form, reruns, note = C.c_int32(-1), C.c_int32(-1), C.create_string_buffer(640)\n"
            "assert capi.lib().cc_last_call_solver_status(C.byref(form), C.byref(reruns), note, 640) == 0\n"
            "assert (form.value, reruns.value) == (0, 1) and b'NEVER RAN' in note.value and b'three kernels' in note.value, (form.value, reruns.value, note.value)\n"
            "assert r[5]['iterations'] == o[5]['iterations'] and all(np.abs(r[k] - o[k]).max() < 1e-9 for k in range(4))\n"
            # a handle: its first solve falls into the device's window (no lean launch, no wait, no rerun) ...
            "p = capi.RigProblem(*args, sc['cam_frozen'])\n"
            "p.set_state(cq, ct, fq, ft)\n"
            "assert p.solver_form() == 2\n"
            "t0 = time.time(); s = p.solve(); dt = time.time() - t0\n"
            "assert dt < 0.03 and p.solver_status()[:2] == (2, 0), (dt, p.solver_status())\n"
            "g = p.get_state()\n"
            "assert s['iterations'] == o[5]['iterations'] and s['termination'] == o[5]['termination']\n"
            "assert all(np.abs(g[k] - o[k]).max() < 1e-9 for k in range(4))\n"
            "assert all(np.abs(r[k] - g[k]).max() < 1e-11 for k in range(4))\n"
            # ... its second probes the lean form, gives up in the first round (strike one: the handle would try again) and is rerun
            "p.set_state(cq, ct, fq, ft)\n"
            "t0 = time.time(); s1 = p.solve(); dt = time.time() - t0\n"
            "assert 0.03 < dt < 1.0, dt\n"
            "form, reruns, note = p.solver_status()\n"
            "assert (form, reruns) == (2, 1) and 'NEVER RAN' in note and 'three kernels' in note and 'again next time' in note, (form, reruns, note)\n"
            "assert s1['iterations'] == s['iterations'] and s1['final_cost'] == s['final_cost']\n"
            # ... the window is two solves now; the probe after it is strike two: the handle stays on the three-kernel form
            "for k in range(3):\n"
            "    p.set_state(cq, ct, fq, ft)\n"
            "    s2 = p.solve()\n"
            "    assert p.solver_status()[1] == (2 if k == 2 else 1), (k, p.solver_status())\n"
            "    assert s2['iterations'] == s['iterations'] and s2['final_cost'] == s['final_cost']\n"
            "form, reruns, note = p.solver_status()\n"
            "assert (form, reruns) == (0, 2) and 'stays on that form' in note, (form, reruns, note)\n"
            "s3 = p.solve(); assert s3['iterations'] <= 2 and p.solver_status()[1] == 2\n"
            "print('rerun ok', dt)\n") % root
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, CC_RIG_PERSIST_TEST_NO_CONTROL="1", CC_PERSIST_BACKOFF_CALLS="1",
                                                              CC_PERSIST_BACKOFF_MS="0"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "rerun ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


@pytest.mark.parametrize("cams,frames,pts,ragged", [(2, 50, 4, False), (4, 40, 30, True), (8, 2200, 70, False)])
def test_frame_by_frame_records_give_the_bits_of_the_flat_arrays(cams, frames, pts, ragged):
    """cc_rig_optimize_frames (what ExtrinsicsCalibrator::Optimize calls on one device: its per-frame lists of sightings read in
    place, the costs written back into them) against cc_rig_optimize on the flattened arrays: same regrouping, same bits --
    also with frames that lost observations (some empty) and with enough observations for several host threads."""
    sc = po.rig_scenario(cams, frames, pts)
    cq, ct, fq, ft = _inputs(sc)
    off, cam, world, uv = sc["frame_offsets"], sc["obs_cam"], sc["obs_world"], sc["obs_uv"]
    if ragged:
        rng = np.random.default_rng(3)
        keep = rng.random(len(cam)) < 0.8
        keep[off[5]:off[6]] = False          # an empty frame
        counts = np.array([keep[off[f]:off[f + 1]].sum() for f in range(frames)])
        off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        cam, world, uv = cam[keep], world[keep], np.asarray(uv).reshape(-1, 2)[keep]
    args = (cams, off, cam, world, uv, sc["world_xyz"], cq, ct, sc["cam_frozen"], fq, ft)
    opts = capi.default_options(max_iterations=30)
    a = capi.rig_optimize(*args, options=opts)
    b = capi.rig_optimize_frames(*args, options=opts)
    assert a[5]["iterations"] == b[5]["iterations"] and a[5]["final_cost"] == b[5]["final_cost"]
    for k in range(5):
        assert np.array_equal(a[k], b[k])


@pytest.mark.parametrize("camera_dtype,world_dtype", [(np.uint32, np.uint64), (np.uint64, np.uint32), (np.uint32, np.uint32)])
def test_frame_by_frame_columns_give_the_bits_of_the_flat_arrays(camera_dtype, world_dtype):
    """cc_rig_optimize_columns (round 5: what ExtrinsicsCalibrator::Optimize calls on one device -- per frame one array of camera
    ids, one of point ids, one of image points, one of costs) against cc_rig_optimize on the flattened arrays, ids 4 or 8 bytes
    wide, with frames that lost observations (one of them empty: NULL column entries)."""
    sc = po.rig_scenario(4, 40, 30)
    cq, ct, fq, ft = _inputs(sc)
    off, cam, world, uv = sc["frame_offsets"], sc["obs_cam"], sc["obs_world"], sc["obs_uv"]
    rng = np.random.default_rng(5)
    keep = rng.random(len(cam)) < 0.8
    keep[off[7]:off[8]] = False
    counts = np.array([keep[off[f]:off[f + 1]].sum() for f in range(40)])
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    cam, world, uv = cam[keep], world[keep], np.asarray(uv).reshape(-1, 2)[keep]
    args = (4, off, cam, world, uv, sc["world_xyz"], cq, ct, sc["cam_frozen"], fq, ft)
    opts = capi.default_options(max_iterations=30)
    a = capi.rig_optimize(*args, options=opts)
    b = capi.rig_optimize_columns(*args, options=opts, camera_dtype=camera_dtype, world_dtype=world_dtype)
    assert a[5]["iterations"] == b[5]["iterations"] and a[5]["final_cost"] == b[5]["final_cost"]
    for k in range(5):
        assert np.array_equal(a[k], b[k])
    c = capi.rig_optimize_columns(*args, options=opts, want_cost=False)     # (no cost column: nothing written, same poses)
    assert c[4] is None and all(np.array_equal(a[k], c[k]) for k in range(4))


def test_columns_that_do_not_make_sense_are_refused():
    sc = po.rig_scenario(2, 10, 4)
    cq, ct, fq, ft = _inputs(sc)
    args = (2, sc["frame_offsets"], sc["obs_cam"], sc["obs_world"], sc["obs_uv"], sc["world_xyz"], cq, ct, sc["cam_frozen"], fq, ft)
    with pytest.raises(capi.CcError, match="not 4 or 8 bytes wide"):
        capi.rig_optimize_columns(*args, camera_dtype=np.uint16)
    cam = sc["obs_cam"].copy()
    cam[17] = 9
    with pytest.raises(capi.CcError, match="observation 17: camera id out of range"):
        capi.rig_optimize_columns(2, sc["frame_offsets"], cam, *args[3:])


def test_frame_by_frame_records_with_a_bad_id_are_refused():
    sc = po.rig_scenario(2, 10, 4)
    cq, ct, fq, ft = _inputs(sc)
    cam = sc["obs_cam"].copy()
    cam[17] = 9
    with pytest.raises(capi.CcError, match="observation 17: camera id out of range"):
        capi.rig_optimize_frames(2, sc["frame_offsets"], cam, sc["obs_world"], sc["obs_uv"], sc["world_xyz"], cq, ct, sc["cam_frozen"], fq, ft)


def test_releasing_the_caches_between_calls_changes_nothing():
    """cc_release_caches hands the pooled device blocks, the arena and the pinned staging block back; the next call allocates
    again and gives the same bits (also for the intrinsics path, which keeps its arena in the same cache)."""
    sc = po.rig_scenario(3, 30, 20)
    cq, ct, fq, ft = _inputs(sc)
    args = (3, sc["frame_offsets"], sc["obs_cam"], sc["obs_world"], sc["obs_uv"], sc["world_xyz"], cq, ct, sc["cam_frozen"], fq, ft)
    a = capi.rig_optimize(*args)
    off, uv, xyz = capi.make_intrinsics_problem(12, 40)
    e0 = capi.intrinsics_estimate(off, uv, xyz)
    capi.release_caches()
    capi.release_caches()          # (nothing left: a no-op)
    b = capi.rig_optimize(*args)
    e1 = capi.intrinsics_estimate(off, uv, xyz, views=True)
    for k in range(5):
        assert np.array_equal(a[k], b[k])
    assert np.array_equal(e0[1], e1[1]) and np.array_equal(e0[2], e1[2])


def test_one_shot_calls_from_two_host_threads_at_once():
    """The process-wide caches behind the one-shot calls (pinned staging block, device block pool, permutation storage, streams)
    are handed to one owner at a time: host threads calling cc_rig_optimize / cc_rig_optimize_frames / cc_intrinsics_estimate
    concurrently get the results of the same calls made one after the other -- the intrinsics path bit for bit; the rig path to
    the rounding by which its two solver forms differ, because a lean persistent solve whose control launch got stuck behind
    another thread's device-wide wait is rerun with three kernels per iteration (42 ms late, not 1.3 s)."""
    import threading
    scs = [po.rig_scenario(3, 60, 40), po.rig_scenario(4, 45, 25)]
    args = []
    for sc, cams in zip(scs, (3, 4)):
        cq, ct, fq, ft = _inputs(sc)
        args.append((cams, sc["frame_offsets"], sc["obs_cam"], sc["obs_world"], sc["obs_uv"], sc["world_xyz"], cq, ct, sc["cam_frozen"], fq, ft))
    off, uv, xyz = capi.make_intrinsics_problem(30, 80)
    ref = [capi.rig_optimize(*args[0]), capi.rig_optimize_frames(*args[1]), capi.intrinsics_estimate(off, uv, xyz, views=True)]
    out = [[None] * 4 for _ in range(3)]
    err = []

    def work(which):
        try:
            for rep in range(4):
                if which == 0:
                    out[0][rep] = capi.rig_optimize(*args[0])
                elif which == 1:
                    out[1][rep] = capi.rig_optimize_frames(*args[1])
                else:
                    out[2][rep] = capi.intrinsics_estimate(off, uv, xyz, views=True)
        except Exception as e:   # (reported below: an exception in a thread would otherwise pass silently)
            err.append(repr(e))

    th = [threading.Thread(target=work, args=(w,)) for w in range(3)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not err, err
    for w in range(3):
        for rep in range(4):
            got = out[w][rep]
            n = 5 if w < 2 else 4
            for k in range(n):
                if w == 2:
                    assert np.array_equal(np.asarray(got[k]), np.asarray(ref[w][k])), (w, rep, k)
                else:
                    assert np.allclose(np.asarray(got[k]), np.asarray(ref[w][k]), rtol=1e-9, atol=1e-12), (w, rep, k)
