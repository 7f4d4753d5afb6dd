"""A pixel model per camera on the rig solve with intrinsics (cc_rigk_set_camera_model), the part that needs no GPU: the CPU
reference the GPU tests lean on (tests/rigk_mixed_ref.py) is pinned -- with one model for all cameras it IS
tests/rigk_fisheye_ref.py's problem, bit for bit; the rows of a camera are its model's; its minimum is scipy's; every shape the
GPU tests use takes the same decisions in two precisions and ends at the noise."""
import numpy as np
import pytest
from scipy.optimize import least_squares

from oracle import pyoracle as po
from tests import fisheye_ref as fr
from tests import rigk_fisheye_ref as rr
from tests import rigk_mixed_ref as mr
from tests.helpers import TIGHT, quat_plus


@pytest.mark.parametrize("kind", ["R", "F"])
def test_one_model_for_all_cameras_is_the_homogeneous_problem_bit_for_bit(kind):
    """3 x 8 x 12, masks and the loss on: rows, evaluation blocks and the whole solve of the subclass with models = [m, m, m]
    against rigk_fisheye_ref.problem(model=m, per_camera=True) on the same data."""
    k = mr.mixed_rig_case(3, 8, 12, kind * 3)
    masks = np.array([1 << 5, 0, 1 << 7], dtype=np.uint32)
    Pm = mr.problem(k, huber_a=1.5, const_masks=masks)
    Ph = rr.problem(k, model=mr.MODELS[kind], huber_a=1.5, per_camera=True, const_masks=masks)
    assert np.array_equal(Pm.masks, Ph.masks) and np.array_equal(Pm.fixed, Ph.fixed)
    st = (k["intr0"], k["cam_q0"], k["cam_t0"], k["frame_q0"], k["frame_t0"])
    for a, b in zip(Pm.rows(st), Ph.rows(st)):
        assert np.array_equal(a, b)
    opt = po.default_options(max_iterations=50)
    g, o = mr.solve_case(k, Pm, options=opt), rr.solve_case(k, Ph, options=opt)
    assert g[6]["iterations"] >= 3
    for a in range(6):
        assert np.array_equal(g[a], o[a])
    assert g[6] == o[6]


def test_the_rows_of_a_camera_are_its_models_rows():
    """On `percam` (kinds FRF) at the start: the rows of camera c equal those of the homogeneous problem of kinds[c]'s model on
    the same data, and differ from the other model's."""
    k, pk, _ = mr.gpu_case("percam")
    P = mr.problem(k, **pk)
    st = (k["intr0"], k["cam_q0"], k["cam_t0"], k["frame_q0"], k["frame_t0"])
    r, J = P.rows(st)
    hom = {x: rr.problem(k, model=mr.MODELS[x], per_camera=True).rows(st) for x in "RF"}
    for c, x in enumerate(k["kinds"]):
        idx = P.by_cam[c]
        other = "F" if x == "R" else "R"
        assert np.array_equal(r[idx], hom[x][0][idx]) and np.array_equal(J[idx], hom[x][1][idx])
        assert not np.array_equal(r[idx], hom[other][0][idx])
    assert [bool(m & fr.K8_HELD) for m in P.masks] == [True, True, True]     # (camera 1's bit 8 comes from PC_MASKS)
    assert [bool(m & fr.K8_HELD) for m in mr.problem(mr.gpu_case("rf")[0]).masks] == [False, True]


def test_mixed_rig_minimiser_matches_scipy():
    """tests/test_rigk_fisheye_cpu.py's check on `rf`, to its bound: the same minimum from the same start (k3 and k4 of the fisheye
    camera, and p1 p2 k3 of the radial-tangential one, held: on 240 noisy points per camera they are not determined to the digits
    compared), cost 1e-9 relative, fx fy px py 1e-6 relative."""
    k, _, _ = mr.gpu_case("rf")
    masks = np.array([(1 << 6) | (1 << 7) | (1 << 8), (1 << 6) | (1 << 7)], dtype=np.uint32)
    P = mr.problem(k, const_masks=masks)
    g = mr.solve_case(k, P, options=po.default_options(**TIGHT))
    F, free = 12, np.arange(6)

    def state(p):
        intr = k["intr0"].copy()
        intr[0, free], intr[1, free] = p[0:6], p[6:12]
        cq, ct = k["cam_q0"].copy(), k["cam_t0"].copy()
        cq[1], ct[1] = quat_plus(cq[1], p[12:15]), ct[1] + p[15:18]
        d = p[18:].reshape(F, 6)
        fq = np.array([quat_plus(k["frame_q0"][f], d[f, :3]) for f in range(F)])
        return (intr, cq, ct, fq, k["frame_t0"] + d[:, 3:])

    x0 = np.concatenate([k["intr0"][0, free], k["intr0"][1, free], np.zeros(6 + 6 * F)])
    sol = least_squares(lambda p: P.rows(state(p))[0].ravel(), x0, method="trf", x_scale="jac", ftol=1e-15, xtol=1e-15, gtol=1e-15, max_nfev=400)
    cost = 0.5 * float(np.sum(sol.fun ** 2))
    print("reference %.12g, scipy %.12g" % (g[6]["final_cost"], cost))
    assert abs(g[6]["final_cost"] - cost) <= 1e-9 * cost
    assert np.abs(g[0][0, :4] / sol.x[0:4] - 1).max() <= 1e-6 and np.abs(g[0][1, :4] / sol.x[6:10] - 1).max() <= 1e-6


@pytest.mark.parametrize("name", mr.GPU_CASES)
def test_every_gpu_shape_has_a_stable_trajectory_and_ends_at_the_noise(name):
    """The reference takes the same accept / valid sequence in float64 and in np.longdouble, with exactly one rejected step, and
    ends FUNCTION (ng1024 too, inside its six iterations); without displaced pixels the final RMS is below 0.45 px (noise 0.3 px per
    coordinate: 0.42 px)."""
    k, pk, _ = mr.gpu_case(name)
    s, sl = mr.gpu_reference(name)[6], mr.gpu_reference(name, np.longdouble)[6]
    print("%s: %d iterations, %s, rms %.3f px" % (name, s["iterations"], s["termination"], np.sqrt(2 * s["final_cost"] / len(k["obs_cam"]))))
    assert s["termination"] == sl["termination"] and s["iterations"] == sl["iterations"] and s["iterations"] >= 3
    assert [(l["accepted"], l["valid"]) for l in s["log"]] == [(l["accepted"], l["valid"]) for l in sl["log"]]
    assert np.allclose([l["cost"] for l in s["log"]], [l["cost"] for l in sl["log"]], rtol=1e-9)
    assert sum(1 for l in s["log"] if not l["accepted"]) == 1
    assert s["termination"] == "FUNCTION"
    if name != "percam":
        assert np.sqrt(2 * s["final_cost"] / len(k["obs_cam"])) < 0.45
