"""Calibrator.EstimateMany over fisheye calibrators (SetCameraModel(Fisheye) on every one: the batch has one model) through
pycalibrator: each calibrator ends at the C-ABI one-shot result (cc_intrinsics_batch_estimate_model) written back as float32,
with its own held coefficient and its own loss; a radial-tangential EstimateMany still ends where it did; Distort / Undistort
of a calibrator calibrated this way go through the fisheye point kernels."""
import os
import sys

import mpmath as mp
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "camera_calibrator_amd"))
pytestmark = pytest.mark.gpu

from camera_calibrator_amd import capi  # noqa: E402
from tests import fisheye_ref as fr  # noqa: E402

FISH = capi.MODEL_FISHEYE
_cache = {}


def _frames(c):
    off, uv, xyz = c["off"], c["uv"], c["xyz"]
    return [uv[off[f]:off[f + 1]] for f in range(len(off) - 1)], [xyz[off[f]:off[f + 1]] for f in range(len(off) - 1)]


def _model(c):
    K = c.GetK()
    return np.concatenate([[K[0, 0], K[1, 1], K[0, 2], K[1, 2]], c.GetDistortion()]).astype(np.float32)


def _ulps(got, want):
    return np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))


def _cases():
    """8x40 with displaced observations (its calibrator has the loss), fov140 (k3 held), 3x12."""
    return [fr.displaced(fr.case("8x40")), fr.case("fov140"), fr.case("3x12")]


def _calibrated():
    """The three calibrators after one EstimateMany: computed once, never modified."""
    if "many" not in _cache:
        import pycalibrator as pc
        many = [pc.Calibrator(1600, 1000) for _ in range(3)]
        for c in many:
            c.SetCameraModel(pc.CameraModel.Fisheye)
        many[0].SetHuberLoss(1.0)
        many[1].ForceDistortionToConstant(2)
        cams = [_frames(c) for c in _cases()]
        pc.EstimateMany(many, [img for img, _ in cams], [world for _, world in cams])
        _cache["many"] = many
    return _cache["many"]


def test_estimate_many_over_fisheye_calibrators_is_the_c_abi_one_shot():
    many = _calibrated()
    cases = _cases()
    _, intr, _, _, ss = capi.intrinsics_batch_estimate([(c["off"], c["uv"], c["xyz"]) for c in cases], const_mask=[0, 1 << 6, 0],
                                                       huber_a=[1.0, 0.0, 0.0], model=FISH)
    for p, c in enumerate(many):
        assert c.LastStatus() == 0 and c.LastSolverForm() == 0 and c.LastSolverReruns() == 0
        assert len(c.GetDistortion()) == 4 and intr[p][8] == 0.0
        assert c.LastIterations() == ss[p]["iterations"] > 0 and c.LastFinalCost() == ss[p]["final_cost"]
        got, want = _model(c), intr[p][:8].astype(np.float32)
        print("camera", p, "ulp", _ulps(got, want), "fx", got[0], "iterations", c.LastIterations())
        assert _ulps(got, want).max() <= 1
    assert many[1].GetDistortion()[2] == 0.0 and many[0].GetDistortion()[2] != 0.0          # k3 held in the second camera only
    # the loss was that calibrator's own: without it the displaced observations pull the fit elsewhere
    _, plain, _, _, _ = capi.intrinsics_batch_estimate([(c["off"], c["uv"], c["xyz"]) for c in cases], const_mask=[0, 1 << 6, 0], model=FISH)
    assert abs(plain[0][0] - intr[0][0]) > 1e-3 and np.array_equal(plain[1], intr[1]) and np.array_equal(plain[2], intr[2])


def test_a_radial_tangential_estimate_many_ends_where_it_did():
    """The 20 x 88 fixture of tests/golden/c1_intrinsics.npz: EstimateMany over radial-tangential calibrators takes the symbol
    and launches the kernels it took before (their gfx950 text is unchanged: profiles/r13/batch_fisheye_identity.txt), so it is
    the C-ABI batch estimate written back as float32 BIT FOR BIT, and a separate Estimate() to +-1 ulp as in
    tests/test_gpu_pycalibrator_batch.py."""
    import pycalibrator as pc
    g = np.load(os.path.join(ROOT, "tests", "golden", "c1_intrinsics.npz"))
    case = dict(off=g["off"], uv=g["uv"], xyz=g["xyz"])
    img, world = _frames(case)
    many = [pc.Calibrator(1600, 1000), pc.Calibrator(1600, 1000)]
    many[1].ForceDistortionToConstant(4)
    pc.EstimateMany(many, [img, img], [world, world])
    _, intr, _, _, ss = capi.intrinsics_batch_estimate([(case["off"], case["uv"], case["xyz"])] * 2, const_mask=[0, 1 << 8])
    for p, c in enumerate(many):
        assert c.LastStatus() == 0 and c.LastSolverForm() == 0 and len(c.GetDistortion()) == 5
        assert c.LastIterations() == ss[p]["iterations"] > 0 and c.LastFinalCost() == ss[p]["final_cost"]
        assert np.array_equal(_model(c), intr[p].astype(np.float32))
        one = pc.Calibrator(1600, 1000)
        if p == 1:
            one.ForceDistortionToConstant(4)
        one.Estimate(img, world)
        assert one.LastIterations() == c.LastIterations()
        got, want = _model(c), _model(one)
        coarse = np.spacing(np.abs(want)).astype(np.float64) >= 1e-9
        assert np.all(_ulps(got, want)[coarse] <= 1) and np.all(np.abs(got.astype(np.float64) - want.astype(np.float64))[~coarse] <= 1e-9)
    assert many[1].GetDistortion()[4] == 0.0 and many[0].GetDistortion()[4] != 0.0


def _distort_reference(K, d4, xy):
    """Pixels of the normalised points xy from the 50-digit model of tests/fisheye_ref.py (the point (x, y, 1) seen from the
    origin), rounded to float32."""
    intr = np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2], d4[0], d4[1], d4[2], d4[3], 0.0], dtype=np.float64)
    X = np.concatenate([xy.astype(np.float64), np.ones((len(xy), 1))], axis=1)
    return fr.mp_project(intr, np.array([1.0, 0, 0, 0]), np.zeros(3), X).astype(np.float32)


def _undistort_reference(K, d4, uv):
    """The inverse at 50 digits: the root theta of theta_d(theta) = |((u, v) - p) / f|, then tan(theta) along that direction."""
    out = np.zeros(uv.shape)
    with mp.workdps(50):
        k = [mp.mpf(float(v)) for v in d4]
        fx, fy, px, py = (mp.mpf(float(K[i, j])) for i, j in ((0, 0), (1, 1), (0, 2), (1, 2)))
        theta_d = lambda th: th * (1 + th**2 * (k[0] + th**2 * (k[1] + th**2 * (k[2] + th**2 * k[3]))))
        for i, (u, v) in enumerate(uv):
            a, b = (mp.mpf(float(u)) - px) / fx, (mp.mpf(float(v)) - py) / fy
            td = mp.sqrt(a * a + b * b)
            th = mp.findroot(lambda t: theta_d(t) - td, td, tol=mp.mpf(10) ** -45)
            assert 0 <= th < mp.pi / 2
            out[i] = float(a * mp.tan(th) / td), float(b * mp.tan(th) / td)
    return out.astype(np.float32)


def _assert_within_one_ulp(got, want):
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    print("max error in ulps", float(np.max(err / np.spacing(np.abs(want)).astype(np.float64))))
    assert np.all(err <= np.spacing(np.abs(want)).astype(np.float64))


def test_distort_and_undistort_of_a_batch_calibrated_fisheye_calibrator():
    """A round trip of 5 points through the calibrated model of the 140 degree camera, each leg +-1 float32 ulp of the 50-digit
    value (the point kernels compute in double: only the final rounding can differ)."""
    c = _calibrated()[1]
    K, d4 = np.array(c.GetK(), dtype=np.float32), np.array(c.GetDistortion(), dtype=np.float32)
    xy = np.array([[0.1, -0.2], [0.8, 0.3], [-1.2, 0.9], [0.02, 0.01], [-0.5, -1.5]], dtype=np.float32)
    uv = np.array(c.Distort([p for p in xy]), dtype=np.float32)
    back = np.array(c.Undistort([p for p in uv]), dtype=np.float32)
    assert np.array_equal(uv, capi.distort(K, d4, xy, model=FISH)) and np.array_equal(back, capi.undistort(K, d4, uv, model=FISH))
    assert not np.array_equal(uv, capi.distort(K, np.append(d4, np.float32(0)), xy))          # (not the radial-tangential kernels)
    _assert_within_one_ulp(uv, _distort_reference(K, d4, xy))
    _assert_within_one_ulp(back, _undistort_reference(K, d4, uv))    # (from the pixels the GPU returned: what Undistort was given)
    r = np.hypot(xy[:, 0], xy[:, 1]).astype(np.float64)
    assert np.all(np.abs(back.astype(np.float64) - xy.astype(np.float64)).max(axis=1) <= 4e-7 * (1 + r * r) + 2.0**-23 * r)
