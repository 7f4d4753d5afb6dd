"""Huber loss of the single-camera intrinsics solve, the part that needs no GPU: the CPU reference the GPU tests lean on is
pinned against the plain intrinsics oracle, bad arguments to the new entry points are refused before any device call, the
class surface carries the setting, and the new kernels neither spill nor use scratch."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from camera_calibrator_amd import capi
from oracle import pyoracle as po
from tests import huber_ref as hr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARGUMENT = -1


@pytest.mark.parametrize("shape", ["8x40", "5x30"])
def test_one_frozen_camera_rig_oracle_is_the_intrinsics_oracle_with_the_loss_off(shape):
    """oc_rigk_solve with one camera frozen at the identity and no loss against oc_intrinsics_solve: same iterations and
    termination, costs and intrinsics 1e-12 relative (measured 2e-13 and 2e-15). Pins the reference of the GPU tests."""
    c = hr.dirty_case(shape)
    ir, qr, tr, _, sr = hr.oracle_solve(c, 0.0)
    io, qo, to, so = po.intrinsics_solve(c["off"], c["uv"], c["xyz"], c["intr0"], c["q0"], c["t0"])
    assert sr["iterations"] == so["iterations"] and sr["termination"] == so["termination"]
    assert [l["accepted"] for l in sr["log"]] == [l["accepted"] for l in so["log"]]
    cr, co = np.array([l["cost"] for l in sr["log"]]), np.array([l["cost"] for l in so["log"]])
    assert np.abs(cr - co).max() <= 1e-12 * np.abs(co).max() and np.allclose(cr, co, rtol=1e-12, atol=0)
    assert np.allclose(ir, io, rtol=1e-12, atol=1e-12 * np.abs(io).max())
    assert np.abs(qr - qo).max() < 1e-12 and np.abs(tr - to).max() < 1e-12


@pytest.mark.parametrize("shape", list(hr.SHAPES))
def test_the_oracle_takes_the_iterations_the_gpu_tests_expect(shape):
    """a = 1.0, default options, free and with k3 frozen: the table in tests/huber_ref.py; every solve ends on FUNCTION, between
    5 % and 20 % of the observations end in the tail, and the loss brings fx at least twice as close to the fixture's 1000 as
    the plain sum of squares does (measured factors 37, 7, 14)."""
    for mask, want in zip((0, hr.K3_FROZEN), hr.ORACLE_ITERATIONS[shape]):
        intr, _, _, cost, s = hr.oracle_solution(shape, 1.0, mask)
        assert s["iterations"] == want and s["termination"] == "FUNCTION", (shape, mask, s["iterations"], s["termination"])
        assert 0.05 <= (cost > 0.5).mean() <= 0.20
    fx_huber, fx_l2 = hr.oracle_solution(shape, 1.0)[0][0], hr.oracle_solution(shape, 1e6)[0][0]
    assert 2.0 * abs(fx_huber - 1000.0) <= abs(fx_l2 - 1000.0), (fx_huber, fx_l2)


def test_reference_blocks_reduce_to_the_plain_blocks_without_a_tail():
    c = hr.dirty_case("5x30")
    cost_o, blocks_o = po.intrinsics_blocks(c["off"], c["uv"], c["xyz"], c["intr0"], c["q0"], c["t0"])
    cost_r, blocks_r = hr.huber_blocks(c, c["intr0"], c["q0"], c["t0"], 1e6)
    assert np.isclose(cost_r, cost_o, rtol=1e-13) and np.abs(blocks_r - blocks_o).max() <= 1e-12 * np.abs(blocks_o).max()
    cost_h, blocks_h = hr.huber_blocks(c, c["intr0"], c["q0"], c["t0"], 1.0)
    assert cost_h < 0.5 * cost_o and np.abs(blocks_h).max() < np.abs(blocks_o).max()


def _views(F=3, pts=4):
    uv = [np.zeros((pts, 2), np.float32) for _ in range(F)]
    xyz = [np.zeros((pts, 3), np.float32) for _ in range(F)]
    fp = C.POINTER(C.c_float)
    return ((fp * F)(*[a.ctypes.data_as(fp) for a in uv]), (fp * F)(*[a.ctypes.data_as(fp) for a in xyz]),
            np.full(F, pts, dtype=np.int64), (uv, xyz))


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None


def test_bad_arguments_are_refused_before_any_device_call():
    lib = capi.lib()
    err = lambda: lib.cc_last_error().decode()
    out = np.zeros(4)
    assert lib.cc_intrinsics_set_huber(None, C.c_double(1.0)) == BAD_ARGUMENT and "NULL" in err()
    assert lib.cc_intrinsics_set_huber(None, C.c_double(float("nan"))) == BAD_ARGUMENT
    assert lib.cc_intrinsics_obs_cost(None, _dp(out)) == BAD_ARGUMENT and "NULL" in err()
    assert lib.cc_intrinsics_batch_set_huber(None, _dp(out)) == BAD_ARGUMENT and "NULL" in err()
    # the one-shot forms: NaN and NULL arrays, with everything else in order
    F = 3
    uvv, xyzv, counts, _keep = _views(F)
    intr, q, t = np.zeros(9), np.zeros((F, 4)), np.zeros((F, 3))
    q[:, 0] = 1.0
    opt = capi.default_options()
    cnt = counts.ctypes.data_as(C.POINTER(C.c_int64))
    nan, one = C.c_double(float("nan")), C.c_double(1.0)
    args = lambda uv=uvv, i=intr: (C.byref(opt), C.c_int32(0), C.c_int64(F), uv, xyzv, cnt, _dp(i), C.c_uint32(0), _dp(q), _dp(t), None)
    assert lib.cc_intrinsics_optimize_views_huber(*args(), nan) == BAD_ARGUMENT and "NaN" in err()
    assert lib.cc_intrinsics_optimize_views_huber(*args(uv=None), one) == BAD_ARGUMENT
    assert lib.cc_intrinsics_optimize_views_huber(*args(i=None), one) == BAD_ARGUMENT
    eargs = lambda uv=uvv, i=intr: (C.byref(opt), C.c_int32(0), C.c_int64(F), uv, xyzv, cnt, None, C.c_uint32(0), None, _dp(i), _dp(q), _dp(t), None)
    assert lib.cc_intrinsics_estimate_views_huber(*eargs(), nan) == BAD_ARGUMENT and "NaN" in err()
    assert lib.cc_intrinsics_estimate_views_huber(*eargs(uv=None), one) == BAD_ARGUMENT
    assert lib.cc_intrinsics_estimate_views_huber(*eargs(i=None), one) == BAD_ARGUMENT
    # the batched one-shot form: two problems of three frames of four points
    poff = np.array([0, 3, 6], dtype=np.int64)
    foff = np.arange(7, dtype=np.int64) * 4
    uv, xyz = np.zeros((24, 2), np.float32), np.zeros((24, 3), np.float32)
    bintr, bq, bt = np.zeros((2, 9)), np.zeros((6, 4)), np.zeros((6, 3))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
    fpp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    bargs = lambda i=bintr, fo=foff: (C.byref(opt), C.c_int32(0), C.c_int64(2), ip(poff), ip(fo) if fo is not None else None, fpp(uv), fpp(xyz),
                                      None, None, None, _dp(i), _dp(bq), _dp(bt), None)
    assert lib.cc_intrinsics_batch_estimate_huber(*bargs(), _dp(np.array([1.0, float("nan")]))) == BAD_ARGUMENT and "NaN" in err()
    assert lib.cc_intrinsics_batch_estimate_huber(*bargs(i=None), _dp(np.array([1.0, 2.0]))) == BAD_ARGUMENT
    assert lib.cc_intrinsics_batch_estimate_huber(*bargs(fo=None), _dp(np.array([1.0, 2.0]))) == BAD_ARGUMENT


def test_python_keywords_route_to_the_old_symbols_when_off(monkeypatch):
    """huber_a = 0 / None must not touch the new one-shot symbols (the existing entry points keep their bits by construction)."""
    calls = []

    class Spy:
        def __init__(self, lib):
            self._lib = lib

        def __getattr__(self, name):
            calls.append(name)
            return getattr(self._lib, name)

    spy = Spy(capi.lib())
    monkeypatch.setattr(capi, "lib", lambda: spy)
    off = np.arange(4, dtype=np.int64) * 4
    uv, xyz = np.zeros((12, 2), np.float32), np.zeros((12, 3), np.float32)
    q, t = np.tile([1.0, 0, 0, 0], (3, 1)), np.zeros((3, 3))
    for fn in (lambda: capi.intrinsics_optimize(off, uv, xyz, np.zeros(9), q, t, huber_a=0.0, device=-1),
               lambda: capi.intrinsics_estimate(off, uv, xyz, huber_a=0.0, device=-1),
               lambda: capi.intrinsics_batch_estimate([(off, uv, xyz)], huber_a=None, device=-1)):
        with pytest.raises(capi.CcError):
            fn()
    assert not any(n.endswith("_huber") for n in calls), calls
    del calls[:]
    for fn in (lambda: capi.intrinsics_optimize(off, uv, xyz, np.zeros(9), q, t, huber_a=1.0, device=-1),
               lambda: capi.intrinsics_estimate(off, uv, xyz, huber_a=1.0, device=-1),
               lambda: capi.intrinsics_batch_estimate([(off, uv, xyz)], huber_a=[1.0], device=-1)):
        with pytest.raises(capi.CcError):
            fn()
    assert [n for n in calls if n.endswith("_huber")] == ["cc_intrinsics_optimize_views_huber", "cc_intrinsics_estimate_views_huber",
                                                           "cc_intrinsics_batch_estimate_huber"], calls


def test_pybind_module_exposes_the_loss_and_it_is_off_by_default():
    sys.path.insert(0, os.path.join(ROOT, "camera_calibrator_amd"))
    import pycalibrator as pc   # (the project's own module: a binding that does not import is a failure, not a skip)
    c = pc.Calibrator(1600, 1000)
    assert hasattr(c, "SetHuberLoss") and hasattr(c, "GetHuberLoss")
    assert c.GetHuberLoss() == 0.0
    c.SetHuberLoss(1.5)
    assert c.GetHuberLoss() == 1.5
    c.SetHuberLoss(-2.0)
    assert c.GetHuberLoss() == 0.0
    with pytest.raises(ValueError):
        c.SetHuberLoss(float("nan"))


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_the_new_kernels_neither_spill_nor_use_scratch():
    """In the manner of tests/test_kernel_budgets.py (whose per-session table of cc_intrinsics.hip is shared). The robust sweeps
    keep __launch_bounds__(256, 4): at most 128 VGPRs is four waves per SIMD, and they must get there without spilling."""
    from tests.test_kernel_budgets import _table
    t = _table("cc_intrinsics.hip")
    for k in ("cc::k_intr_sweep_huber", "cc::k_intr_obs_cost"):
        assert t[k]["vspill"] == 0 and t[k]["scratch"] == 0, (k, t[k])
    assert t["cc::k_intr_sweep_huber"]["vgpr"] <= 128, t["cc::k_intr_sweep_huber"]
    t = _table("cc_intrinsics_batch_huber.hip")   # (a translation unit of its own: cc_intrinsics_batch.hip keeps its three kernels)
    assert set(t) == {"cc::k_intrb_sweep_huber"}, sorted(t)
    k = "cc::k_intrb_sweep_huber"
    assert t[k]["vspill"] == 0 and t[k]["scratch"] == 0 and t[k]["vgpr"] <= 128, (k, t[k])
