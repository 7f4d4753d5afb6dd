"""Calibrator.SetHuberLoss (an extension: the reference's Optimize sets no loss function) through pycalibrator: Estimate,
Optimize and EstimateMany honour it, several devices refuse it, and switching it off gives an untouched calibrator's results."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "camera_calibrator_amd"))
pytestmark = pytest.mark.gpu

from camera_calibrator_amd import capi  # noqa: E402
from tests import huber_ref as hr  # noqa: E402


def _frames(c):
    off, uv, xyz = c["off"], c["uv"], c["xyz"]
    return [uv[off[f]:off[f + 1]] for f in range(len(off) - 1)], [xyz[off[f]:off[f + 1]] for f in range(len(off) - 1)]


def _model(c):
    K = c.GetK()
    return np.concatenate([[K[0, 0], K[1, 1], K[0, 2], K[1, 2]], c.GetDistortion()]).astype(np.float32)


def _assert_float32_close(got, want):
    """Float32 write-backs of fp64 results: identical or +-1 ulp where float32 is the coarser, 1e-9 absolute where it is finer
    (the tolerance of tests/test_gpu_pycalibrator_batch.py)."""
    got, want = np.asarray(got, dtype=np.float32).ravel(), np.asarray(want, dtype=np.float32).ravel()
    ulp = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
    coarse = np.spacing(np.abs(want)).astype(np.float64) >= 1e-9
    print("ulp", ulp, "abs", np.abs(got.astype(np.float64) - want.astype(np.float64)))
    assert np.all(ulp[coarse] <= 1), ulp
    assert np.all(np.abs(got.astype(np.float64) - want.astype(np.float64))[~coarse] <= 1e-9)


def test_estimate_with_the_loss_is_the_c_abi_estimate():
    import pycalibrator as pc
    case = hr.dirty_case("8x40")
    img, world = _frames(case)
    c = pc.Calibrator(1600, 1000)
    assert c.GetHuberLoss() == 0.0
    c.SetHuberLoss(1.0)
    assert c.GetHuberLoss() == 1.0
    c.Estimate(img, world)
    assert c.LastStatus() == 0 and c.LastSolverForm() == 0 and c.LastSolverReruns() == 0
    _, intr, _, _, s = capi.intrinsics_estimate(case["off"], case["uv"], case["xyz"], huber_a=1.0)
    assert c.LastIterations() == s["iterations"] > 0
    got, want = _model(c), intr.astype(np.float32)
    ulp = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
    print("ulp", ulp)
    assert ulp.max() <= 1
    # and it is the robust answer, not the plain one: fx within 1 px of the fixture's 1000 where the sum of squares ends 5 px off
    plain = pc.Calibrator(1600, 1000)
    plain.Estimate(img, world)
    assert abs(c.GetK()[0, 0] - 1000.0) < 1.0 < abs(plain.GetK()[0, 0] - 1000.0)
    # Optimize from the same start takes the same loss
    K0, q0, t0 = capi.zhang_init(case["off"], case["uv"], case["xyz"])
    o = pc.Calibrator(1600, 1000)
    o.SetK(K0)
    o.SetHuberLoss(1.0)
    o.Optimize(img, world, [q for q in q0], [t for t in t0])
    assert o.LastStatus() == 0 and o.LastSolverForm() == 0 and o.LastIterations() == c.LastIterations()
    assert np.array_equal(_model(o), _model(c))


def test_estimate_many_with_a_loss_per_calibrator_equals_their_own_estimates():
    import pycalibrator as pc
    cases = [hr.dirty_case("5x30"), hr.dirty_case("8x40"), hr.dirty_case("ragged")]
    losses = [1.0, 2.0, 0.0]

    def make(i):
        c = pc.Calibrator(1600, 1000)
        c.SetHuberLoss(losses[i])
        return c

    many = [make(i) for i in range(3)]
    pc.EstimateMany(many, [_frames(c)[0] for c in cases], [_frames(c)[1] for c in cases])
    for i, case in enumerate(cases):
        one = make(i)
        one.Estimate(*_frames(case))
        assert many[i].LastStatus() == 0 and one.LastStatus() == 0
        assert many[i].LastIterations() == one.LastIterations() > 0
        assert np.isclose(many[i].LastFinalCost(), one.LastFinalCost(), rtol=1e-9)
        assert many[i].LastSolverForm() == 0 and many[i].LastSolverReruns() == 0
        _assert_float32_close(many[i].GetK(), one.GetK())
        _assert_float32_close(many[i].GetDistortion(), one.GetDistortion())
        assert many[i].GetHuberLoss() == losses[i]


def test_several_devices_refuse_the_loss_and_switching_it_off_restores_the_plain_results():
    import pycalibrator as pc
    case = hr.dirty_case("8x40")
    img, world = _frames(case)
    untouched = pc.Calibrator(1600, 1000)
    untouched.Estimate(img, world)
    c = pc.Calibrator(1600, 1000)
    c.SetHuberLoss(1.0)
    c.SetDevices([0, 0])
    with pytest.raises(ValueError, match="one device"):
        c.Estimate(img, world)
    K0, q0, t0 = capi.zhang_init(case["off"], case["uv"], case["xyz"])
    with pytest.raises(ValueError, match="one device"):
        c.Optimize(img, world, [q for q in q0], [t for t in t0])
    assert np.array_equal(c.GetK(), np.eye(3, dtype=np.float32))   # nothing was touched
    c.SetDevice(0)
    c.SetHuberLoss(0)
    c.Estimate(img, world)
    assert c.LastStatus() == 0 and c.LastIterations() == untouched.LastIterations()
    assert c.LastSolverForm() == untouched.LastSolverForm()
    assert np.array_equal(c.GetK(), untouched.GetK()) and np.array_equal(c.GetDistortion(), untouched.GetDistortion())
