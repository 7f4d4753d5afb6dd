"""The fisheye camera model of the BATCHED intrinsics solve (cc_intrinsics_batch_set_model, k_intrb_sweep_fisheye,
cc_intrinsics_batch_estimate_model, Calibrator::EstimateMany over fisheye calibrators), the part that needs no GPU: the new
kernel's register table, refusals before any device call, the Python keywords' routing, the class surface, and the
preconditions of tests/test_gpu_intr_batch_fisheye.py checked on the CPU reference alone (tests/fisheye_ref.py)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from camera_calibrator_amd import capi
from oracle import pyoracle as po
from tests import fisheye_ref as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARGUMENT, NO_DEVICE = -1, -2
FISH = capi.MODEL_FISHEYE
K4_HELD = 1 << 7

# The five-problem batch of the GPU tests: (shape, constant mask). Shared with tests/test_gpu_intr_batch_fisheye.py.
BATCH5 = [("ragged", 0), ("3x12", 0), ("8x40", 0), ("fov140", 0), ("3x12", K4_HELD)]
# Every (shape, threshold, mask, min_relative_decrease, displaced) the GPU file holds to the numpy LM that
# tests/test_fisheye_cpu.py::SOLVE_CASES does not already cover: the problem with k4 held, and 3x12 under the raised
# min_relative_decrease of the rejected-step test (the options belong to the whole batch, so it runs under it next to 8x40).
NEW_SOLVE_CASES = [("3x12", 0.0, K4_HELD, None, False), ("3x12", 0.0, 0, 1.01, False)]


def _pycalibrator():
    sys.path.insert(0, os.path.join(ROOT, "camera_calibrator_amd"))
    import pycalibrator as pc   # (the project's own module: a binding that does not import is a failure, not a skip)
    return pc


# ---- register table ----------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_the_new_unit_holds_one_kernel_that_neither_spills_nor_uses_scratch():
    """Three waves per SIMD (168 vector registers at most), as k_intr_sweep_fisheye: the library's atan2 in the loop. The two
    radial-tangential batch units keep their kernel sets."""
    from tests.test_kernel_budgets import _table
    t = _table("cc_intrinsics_batch_fisheye.hip")
    assert set(t) == {"cc::k_intrb_sweep_fisheye"}, sorted(t)
    k = t["cc::k_intrb_sweep_fisheye"]
    print("k_intrb_sweep_fisheye", k)
    assert k["vspill"] == 0 and k["sspill"] == 0 and k["scratch"] == 0 and k["vgpr"] <= 168, k
    assert set(_table("cc_intrinsics_batch.hip")) == {"cc::k_intrb_sweep", "cc::k_intrb_step", "cc::k_intrb_begin"}
    assert set(_table("cc_intrinsics_batch_huber.hip")) == {"cc::k_intrb_sweep_huber"}


# ---- refusals without a device -------------------------------------------------------------------------------------------------
def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None


def _tiny():
    """A well-formed one-problem batch, 3 frames x 4 points of zeros."""
    poff, foff = np.array([0, 3], dtype=np.int64), np.arange(4, dtype=np.int64) * 4
    return poff, foff, np.zeros((12, 2), np.float32), np.zeros((12, 3), np.float32)


def test_bad_arguments_are_refused_before_any_device_call():
    lib = capi.lib()
    err = lambda: lib.cc_last_error().decode()
    model = C.c_int32(-5)
    assert lib.cc_intrinsics_batch_set_model(None, C.c_int32(FISH)) == BAD_ARGUMENT and "NULL" in err()
    assert lib.cc_intrinsics_batch_set_model(None, C.c_int32(7)) == BAD_ARGUMENT
    assert lib.cc_intrinsics_batch_get_model(None, C.byref(model)) == BAD_ARGUMENT and model.value == -5
    poff, foff, uv, xyz = _tiny()
    intr, q, t = np.zeros(9), np.zeros((3, 4)), np.zeros((3, 3))
    opt = capi.default_options()
    ip, fp = C.POINTER(C.c_int64), C.POINTER(C.c_float)
    args = lambda i=intr: (C.byref(opt), C.c_int32(0), C.c_int64(1), poff.ctypes.data_as(ip), foff.ctypes.data_as(ip), uv.ctypes.data_as(fp),
                           xyz.ctypes.data_as(fp), None, None, None, _dp(i), _dp(q), _dp(t), None)
    nan = np.array([float("nan")])
    # (a well-formed call on device 0 would come back with CC_ERR_NO_DEVICE here, or run where there is a device)
    assert lib.cc_intrinsics_batch_estimate_model(*args(), None, C.c_int32(7)) == BAD_ARGUMENT and "unknown model" in err()
    assert lib.cc_intrinsics_batch_estimate_model(*args(), None, C.c_int32(-1)) == BAD_ARGUMENT and "unknown model" in err()
    assert lib.cc_intrinsics_batch_estimate_model(*args(), _dp(nan), C.c_int32(FISH)) == BAD_ARGUMENT and "NaN" in err()
    assert lib.cc_intrinsics_batch_estimate_model(*args(i=None), None, C.c_int32(FISH)) == BAD_ARGUMENT
    short = np.arange(4, dtype=np.int64) * 3    # 3 points a frame: the Zhang precondition, whatever the model
    a = list(args())
    a[4] = short.ctypes.data_as(ip)
    assert lib.cc_intrinsics_batch_estimate_model(*a, None, C.c_int32(FISH)) == BAD_ARGUMENT and "fewer than 4" in err()


@pytest.mark.skipif(capi.device_count() > 0, reason="only meaningful without a GPU")
def test_the_new_one_shot_form_reports_a_missing_device():
    lib = capi.lib()
    poff, foff, uv, xyz = _tiny()
    intr, q, t = np.zeros(9), np.zeros((3, 4)), np.zeros((3, 3))
    opt = capi.default_options()
    ip, fp = C.POINTER(C.c_int64), C.POINTER(C.c_float)
    rc = lib.cc_intrinsics_batch_estimate_model(C.byref(opt), C.c_int32(0), C.c_int64(1), poff.ctypes.data_as(ip), foff.ctypes.data_as(ip),
                                                uv.ctypes.data_as(fp), xyz.ctypes.data_as(fp), None, None, None, _dp(intr), _dp(q), _dp(t), None,
                                                None, C.c_int32(FISH))
    assert rc == NO_DEVICE


def test_python_keywords_route_to_the_old_symbols_when_off(monkeypatch):
    """model = 0 must take the symbols it takes today; MODEL_FISHEYE the new ones (device -1: refused by the library)."""
    calls = []

    class Spy:
        def __init__(self, lib):
            self._lib = lib

        def __getattr__(self, name):
            calls.append(name)
            return getattr(self._lib, name)

    spy = Spy(capi.lib())
    monkeypatch.setattr(capi, "lib", lambda: spy)
    _, foff, uv, xyz = _tiny()
    probs = [(foff, uv, xyz)]
    q, t = [np.tile([1.0, 0, 0, 0], (3, 1))], [np.zeros((3, 3))]
    new = lambda: [n for n in calls if "model" in n]
    for fn in (lambda: capi.intrinsics_batch_estimate(probs, model=0, device=-1),
               lambda: capi.intrinsics_batch_estimate(probs, model=0, huber_a=[1.0], device=-1),
               lambda: capi.intrinsics_batch_optimize(probs, np.zeros((1, 9)), q, t, model=0, device=-1)):
        with pytest.raises(capi.CcError):
            fn()
    assert not new(), calls
    assert [n for n in calls if n.startswith("cc_intrinsics_batch")] == ["cc_intrinsics_batch_estimate", "cc_intrinsics_batch_estimate_huber",
                                                                        "cc_intrinsics_batch_optimize"], calls
    del calls[:]
    for fn in (lambda: capi.intrinsics_batch_estimate(probs, model=FISH, device=-1),
               lambda: capi.intrinsics_batch_estimate(probs, model=FISH, huber_a=[1.0], distortion5=np.zeros((1, 4)), device=-1)):
        with pytest.raises(capi.CcError):
            fn()
    assert [n for n in calls if n.startswith("cc_intrinsics_batch")] == ["cc_intrinsics_batch_estimate_model"] * 2, calls
    with pytest.raises(capi.CcError):   # the handle route of the one-shot optimise: refused where the handle is created
        capi.intrinsics_batch_optimize(probs, np.zeros((1, 9)), q, t, model=FISH, device=-1)
    assert calls[-2:] == ["cc_intrinsics_batch_create", "cc_last_error"], calls
    assert hasattr(capi.IntrinsicsBatch, "set_model") and hasattr(capi.IntrinsicsBatch, "get_model")


# ---- class, without a device ---------------------------------------------------------------------------------------------------
def _class_views(F=3, pts=4):
    return [np.zeros((pts, 2), np.float32) for _ in range(F)], [np.zeros((pts, 3), np.float32) for _ in range(F)]


def test_class_refuses_a_mixture_of_models_and_says_why():
    pc = _pycalibrator()
    px, w = _class_views()
    for first_fisheye in (False, True):
        a, b = pc.Calibrator(1600, 1000), pc.Calibrator(1600, 1000)
        (a if first_fisheye else b).SetCameraModel(pc.CameraModel.Fisheye)
        a.SetDevice(-1)
        with pytest.raises(ValueError, match="fisheye") as e:
            pc.EstimateMany([a, b], [px, px], [w, w])
        assert "one model" in str(e.value)


def test_class_takes_a_batch_of_fisheye_calibrators_to_the_library():
    """The class-level test that fails without the feature: with ALL calibrators fisheye EstimateMany is no ValueError any more.
    It reaches the library, whose answer without a usable device is a RuntimeError (device -1: CC_ERR_NO_DEVICE on a machine
    without a GPU, CC_ERR_BAD_ARGUMENT for the device number on one with)."""
    pc = _pycalibrator()
    px, w = _class_views()
    cs = [pc.Calibrator(1600, 1000) for _ in range(3)]
    for c in cs:
        c.SetCameraModel(pc.CameraModel.Fisheye)
    cs[0].SetDevice(-1)
    cs[1].ForceDistortionToConstant(2)
    cs[2].SetHuberLoss(1.0)
    with pytest.raises(RuntimeError, match="device"):
        pc.EstimateMany(cs, [px] * 3, [w] * 3)
    assert all(len(c.GetDistortion()) == 4 for c in cs)


@pytest.mark.skipif(capi.device_count() > 0, reason="only meaningful without a GPU")
def test_class_reports_the_missing_device_with_default_settings():
    pc = _pycalibrator()
    px, w = _class_views()
    cs = [pc.Calibrator(1600, 1000) for _ in range(2)]
    for c in cs:
        c.SetCameraModel(pc.CameraModel.Fisheye)
    with pytest.raises(RuntimeError, match="no HIP device"):
        pc.EstimateMany(cs, [px] * 2, [w] * 2)
    assert cs[0].LastStatus() == NO_DEVICE


# ---- preconditions of the GPU tests, on the reference alone --------------------------------------------------------------------
def test_the_batch_of_five_does_not_end_in_one_round():
    """"A finished problem stays untouched while the others iterate" is exercised only if the problems of the batch stop after
    different numbers of iterations."""
    its = [fr.reference_solution(name, 0.0, mask)[3]["iterations"] for name, mask in BATCH5]
    print("iterations of the five problems", its)
    assert len(set(its)) >= 2, its


@pytest.mark.parametrize("name,a,mask,mrd,dirty", NEW_SOLVE_CASES)
def test_reference_is_stable_on_the_combinations_the_batch_tests_add(name, a, mask, mrd, dirty):
    """As tests/test_fisheye_cpu.py::test_reference_is_stable_on_every_shape_the_gpu_tests_use: float64 and np.longdouble take the
    same accept / valid sequence, iteration count and termination."""
    c = fr.displaced(fr.case(name)) if dirty else fr.case(name)
    o = po.default_options() if mrd is None else po.default_options(min_relative_decrease=mrd)
    P = fr.Problem(fr.fisheye_model, c["off"], c["uv"], c["xyz"], a, mask | fr.K8_HELD)
    i64, _, _, s64 = fr.reference_solution(name, a, mask, mrd, dirty)
    _, _, _, sl = fr.lm_solve(P, c["intr0"], c["q0"], c["t0"], o, dtype=np.longdouble)
    assert s64["iterations"] == sl["iterations"] and s64["termination"] == sl["termination"]
    assert [l["accepted"] for l in s64["log"]] == [l["accepted"] for l in sl["log"]]
    assert [l["valid"] for l in s64["log"]] == [l["valid"] for l in sl["log"]]
    assert np.allclose([l["cost"] for l in s64["log"]], [l["cost"] for l in sl["log"]], rtol=1e-10, atol=0)
    assert s64["iterations"] > 0
    if mask & K4_HELD:
        assert i64[7] == 0.0                         # k4 stays where it started
    if mrd is not None:
        assert 0 in [l["accepted"] for l in s64["log"]][:-1], "the raised threshold must reject a step"


def test_the_loss_per_problem_combinations_are_covered_by_the_existing_stability_test():
    """a = [1, 0, 1, 0, 0] over BATCH5: the two problems with the loss are (ragged, 1 px, displaced) and (8x40, 1 px, displaced),
    the rejected-step run is (8x40, min_relative_decrease 1.01) -- all in tests/test_fisheye_cpu.py::SOLVE_CASES."""
    from tests.test_fisheye_cpu import SOLVE_CASES
    need = [(BATCH5[0][0], 1.0, 0, None, True), (BATCH5[2][0], 1.0, 0, None, True), ("8x40", 0.0, 0, 1.01, False), ("3x12", 0.0, 0, 1.01, False)]
    need += [(name, 0.0, mask, None, False) for name, mask in BATCH5]
    for n in need:
        assert n in SOLVE_CASES or n in NEW_SOLVE_CASES, n
