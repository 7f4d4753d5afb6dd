"""Fisheye camera model of the rig solve with intrinsics (cc_rigk_set_model), the part that needs no GPU: the CPU reference the
GPU tests lean on (tests/rigk_fisheye_ref.py) is pinned -- its LM restatement against the rig-with-intrinsics oracle with the
pinhole model plugged in, its fisheye rows against the 50-digit model, its minimum against scipy, its stability in two
precisions on every shape the GPU tests use, the scenario generator's wide shape and what the model buys there."""
import numpy as np
import pytest
from scipy.optimize import least_squares

from camera_calibrator_amd.harness import rigk_case
from oracle import pyoracle as po
from tests import fisheye_ref as fr
from tests import rigk_fisheye_ref as rr
from tests.helpers import TIGHT, quat_plus


def _oracle(k, per_camera, masks, huber_a, iters):
    a = (k["cams"], k["frame_offsets"], k["obs_cam"], k["obs_world"], k["obs_uv_pix"], k["world_xyz"], k["intr0"], k["cam_q0"],
         k["cam_t0"], k["cam_frozen"], k["frame_q0"], k["frame_t0"])
    if per_camera:
        return po.rigk_solve_per_camera(*a, const_masks=masks, huber_a=huber_a, options=po.default_options(max_iterations=iters))
    return po.rigk_solve(*a, const_mask=int(masks), huber_a=huber_a, options=po.default_options(max_iterations=iters))


# Largest deviations of the restatement from the oracle, measured with this file (printed by the test), shared / per camera:
# logged costs 3.1e-14 / 1.1e-14 relative; focal lengths and principal point 8.9e-16 / 1.1e-15 relative; distortion 4.0e-14 /
# 7.9e-15; poses 5.3e-16 / 6.3e-16; per-observation costs 3.3e-13 / 6.4e-13 absolute. Asserted at ten times the larger measured
# value, rounded up to a power of ten (fisheye_ref.lm_solve reached 2e-13 / 3e-13 in the same exercise).
PIN_COST_REL, PIN_INTR_REL, PIN_DIST_ABS, PIN_STATE_ABS, PIN_OBS_ABS = 1e-12, 1e-13, 1e-12, 1e-14, 1e-11


@pytest.mark.parametrize("shape,per_camera,masks,huber_a,iters", [
    ((2, 10, 8), False, 0, 0.0, 200),
    ((3, 12, 20), True, np.array([(1 << 8) | (1 << 5), 0, 1 << 8], dtype=np.uint32), 1.5, 300)])
def test_the_restated_lm_with_the_pinhole_model_reproduces_the_oracle(shape, per_camera, masks, huber_a, iters):
    k = rigk_case(*shape, per_camera=per_camera)
    P = rr.problem(k, model=fr.pinhole_model, huber_a=huber_a, per_camera=per_camera, const_masks=masks)
    g = rr.solve_case(k, P, options=po.default_options(max_iterations=iters))
    o = _oracle(k, per_camera, masks, huber_a, iters)
    sg, so = g[6], o[6]
    assert sg["termination"] == so["termination"] and sg["iterations"] == so["iterations"] and sg["iterations"] >= 4
    assert [l["accepted"] for l in sg["log"]] == [l["accepted"] for l in so["log"]]
    assert [l["valid"] for l in sg["log"]] == [l["valid"] for l in so["log"]]
    cost_dev = max(abs(a["cost"] / b["cost"] - 1) for a, b in zip(sg["log"], so["log"]))
    gi, oi = np.atleast_2d(g[0]), np.atleast_2d(o[0])
    intr_dev, dist_dev = np.abs(gi[:, :4] / oi[:, :4] - 1).max(), np.abs(gi[:, 4:] - oi[:, 4:]).max()
    pose_dev = max(np.abs(g[a] - o[a]).max() for a in range(1, 5))
    obs_dev = np.abs(g[5] - o[5]).max()
    print("measured: costs %.2g, intrinsics %.2g rel, distortion %.2g, poses %.2g, per-observation costs %.2g" % (cost_dev, intr_dev, dist_dev, pose_dev, obs_dev))
    assert cost_dev <= PIN_COST_REL and intr_dev <= PIN_INTR_REL and dist_dev <= PIN_DIST_ABS and pose_dev <= PIN_STATE_ABS
    assert obs_dev <= PIN_OBS_ABS
    # its per-observation rows are pyoracle.rigk_residual's (at the start)
    st = (np.asarray(k["intr0"], dtype=np.float64).reshape(-1, 9), k["cam_q0"], k["cam_t0"], k["frame_q0"], k["frame_t0"])
    r, J = P.rows(st)
    for i in range(0, len(P.cam), 7):
        c, f = P.cam[i], P.frame[i]
        ro, Jo = po.rigk_residual(st[0][P.kset(c)], st[3][f], st[4][f], st[1][c], st[2][c], P.X[i].astype(np.float64), P.uv[i].astype(np.float64))
        Jo = np.asarray(Jo).reshape(2, 21)
        assert np.abs(r[i] - ro).max() <= 1e-9 and np.abs(J[i] - Jo).max() <= 1e-12 * np.abs(Jo).max()


def _mp_checks(P, st, picks):
    worst = 0.0
    r, J = P.rows(st)
    for i in picks:
        c, f = P.cam[i], P.frame[i]
        X, uv = P.X[i].astype(np.float64), P.uv[i].astype(np.float64)
        rm, Jm = rr.mp_rig_residual(st[0][P.kset(c)], st[1][c], st[2][c], st[3][f], st[4][f], X, uv)
        assert np.all(np.isfinite(r[i])) and np.all(np.isfinite(J[i]))
        # residuals are differences of ~1e3 px numbers: an ulp of those
        assert np.abs(r[i] - rm).max() <= 1e-12 * 1e3
        for row in range(2):
            dev = np.abs(J[i, row] - Jm[row]).max() / np.abs(Jm[row]).max()
            worst = max(worst, dev)
            assert dev <= 1e-12, (i, row, dev)
        # ... and the single-camera 50-digit model at the composed pose (R_c R_f, R_c t_f + t_c). The pose is composed in
        # np.longdouble and rounded to float64: <= an ulp of a metre-sized coordinate, times fx / zc ~ 1e3 px / m -- 1e-12 px;
        # asserted at 1e-10 px
        ld = np.longdouble
        qc, qf = np.asarray(st[1][c], dtype=ld), np.asarray(st[3][f], dtype=ld)
        q = np.array([qc[0] * qf[0] - qc[1:] @ qf[1:], *(qc[0] * qf[1:] + qf[0] * qc[1:] + np.cross(qc[1:], qf[1:]))])
        t = rr._rot(qc) @ np.asarray(st[4][f], dtype=ld) + np.asarray(st[2][c], dtype=ld)
        rs, _ = fr.mp_residual(st[0][P.kset(c)], q.astype(np.float64), t.astype(np.float64), X, uv)
        assert np.abs(rs - rm).max() <= 1e-10
    return worst


def test_fisheye_rows_match_the_50_digit_model_through_both_poses():
    """All 21 columns (camera pose 6, frame pose 6, intrinsics 9) against central differences at 50 digits through Plus, 1e-12 of
    the row's largest entry: on the axis (rho / zc = 0, 1e-9, 1e-6, 1e-3, a point behind the camera; identity poses) and at the
    start of the shared case (general poses, points up to 54 degrees off the axis)."""
    k = rr.axis_case()
    P = rr.problem(k)
    st = (k["intr0"].reshape(1, 9), k["cam_q0"], k["cam_t0"], k["frame_q0"], k["frame_t0"])
    w1 = _mp_checks(P, st, range(5))
    k, pk, _ = rr.gpu_case("shared")
    P = rr.problem(k, **pk)
    st = (rr.TRUE_INTR.reshape(1, 9), k["cam_q0"], k["cam_t0"], k["frame_q0"], k["frame_t0"])
    w2 = _mp_checks(P, st, range(0, len(P.cam), 53))
    print("largest column deviation / row maximum: axis %.2g, general %.2g" % (w1, w2))


def test_fisheye_rig_minimiser_matches_scipy():
    """tests/test_fisheye_cpu.py's check for the rig: the same minimum from the same start (k3 and k4 held: on 192 noisy points
    they are not determined to the digits compared), cost 1e-9 relative, fx fy px py 1e-6 relative."""
    k = rr.fisheye_rig_case(2, 6, 16)
    mask = (1 << 6) | (1 << 7)
    P = rr.problem(k, const_masks=mask)
    g = rr.solve_case(k, P, options=po.default_options(**TIGHT))
    F, free = 6, np.arange(6)

    def state(p):
        intr = k["intr0"].copy()
        intr[free] = p[:6]
        cq, ct = k["cam_q0"].copy(), k["cam_t0"].copy()
        cq[1], ct[1] = quat_plus(cq[1], p[6:9]), ct[1] + p[9:12]
        d = p[12:].reshape(F, 6)
        fq = np.array([quat_plus(k["frame_q0"][f], d[f, :3]) for f in range(F)])
        return (intr.reshape(1, 9), cq, ct, fq, k["frame_t0"] + d[:, 3:])

    sol = least_squares(lambda p: P.rows(state(p))[0].ravel(), np.concatenate([k["intr0"][free], np.zeros(6 + 6 * F)]), method="trf",
                        x_scale="jac", ftol=1e-15, xtol=1e-15, gtol=1e-15, max_nfev=400)
    cost = 0.5 * float(np.sum(sol.fun ** 2))
    assert abs(g[6]["final_cost"] - cost) <= 1e-9 * cost
    assert np.abs(g[0][:4] / sol.x[:4] - 1).max() <= 1e-6


@pytest.mark.parametrize("name", rr.GPU_CASES + ("wide",))
def test_every_gpu_shape_has_a_stable_trajectory(name):
    """The reference takes the same accept / valid sequence in float64 and in np.longdouble: a decision of the GPU solve that differs
    from the reference's is then a difference of the code, not of a coin toss in the last bits."""
    s, sl = rr.gpu_reference(name)[6], rr.gpu_reference(name, np.longdouble)[6]
    assert s["termination"] == sl["termination"] and s["iterations"] == sl["iterations"] and s["iterations"] >= 3
    assert [(l["accepted"], l["valid"]) for l in s["log"]] == [(l["accepted"], l["valid"]) for l in sl["log"]]
    assert np.allclose([l["cost"] for l in s["log"]], [l["cost"] for l in sl["log"]], rtol=1e-9)


def test_the_wide_shape_is_beyond_60_degrees_and_only_the_fisheye_model_fits_it():
    """What the model buys (profiles/r14/rigk_fisheye_fit_study.txt): on pixels of a fisheye lens with points up to 76 degrees off
    the axis the fisheye rig fit ends at the noise (sub-pixel RMS), the radial-tangential rig fit from the same start several
    pixels above it."""
    k, _, _ = rr.gpu_case("wide")
    n = len(k["obs_cam"])
    assert k["max_angle_deg"] > 60.0
    rms_f = np.sqrt(2 * rr.gpu_reference("wide")[6]["final_cost"] / n)
    o = _oracle(k, False, 0, 0.0, 200)
    rms_r = np.sqrt(2 * o[6]["final_cost"] / n)
    print("fisheye %.3f px, radial-tangential %.3f px, largest angle %.1f degrees" % (rms_f, rms_r, k["max_angle_deg"]))
    assert rms_f < 0.5 and rms_r > rms_f + 3.0


def test_the_committed_gram_fixture_belongs_to_the_scenarios():
    """tests/golden/rigk_fisheye_gram.npz (50-digit rows, tests/golden/make_rigk_fisheye_gram.py) against the reference's own rows
    in np.longdouble: the same pixels, the same Gram to 1e-13 of its largest entry (both are far more accurate than the 1e-12
    the GPU test asks of the kernel; this guards against a fixture left behind by a change of the scenarios)."""
    import os
    gld = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rigk_fisheye_gram.npz"))
    for k, keys in ((rr.gpu_case("ragged")[0], {0: "_0", 3: "_3", 5: "_5"}), (rr.axis_case(), {0: ""})):
        P = rr.problem(k)
        st = tuple(np.asarray(a, dtype=np.longdouble) for a in (k["intr0"].reshape(1, 9), k["cam_q0"], k["cam_t0"], k["frame_q0"], k["frame_t0"]))
        r, J = P.rows(st, np.longdouble)
        off, cam = np.asarray(k["frame_offsets"]), np.asarray(k["obs_cam"])
        groups = [np.nonzero(cam[off[f]:off[f + 1]] == c)[0] + off[f] for f in range(len(off) - 1) for c in np.unique(cam[off[f]:off[f + 1]])]
        tag = "ragged" if len(groups) > 1 else "axis"
        for gi, sfx in keys.items():
            idx = groups[gi]
            assert np.array_equal(gld[tag + "_uv" + sfx], k["obs_uv_pix"][idx])
            X = np.concatenate([J[idx][:, :, 0:6], r[idx][:, :, None], J[idx][:, :, 12:21]], axis=2).reshape(-1, 16)
            want = gld[tag + "_gram" + sfx]
            assert np.abs((X.T @ X).astype(np.float64) - want).max() <= 1e-13 * np.abs(want).max()
