"""The batched intrinsics solve without a GPU: the entry points fail loudly when there is no device (no CPU fallback), bad
arguments are refused before any device call, and the two kernels keep their register allocation (scripts/kernel_regs.py
cross-compiles the translation unit for gfx950 and reads the code object's metadata)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from camera_calibrator_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _problem(frames=3, pts=4):
    off = np.arange(frames + 1, dtype=np.int64) * pts
    return off, np.zeros((frames * pts, 2), np.float32), np.zeros((frames * pts, 3), np.float32)


def _raw(name, poff, foff, uv, xyz, B=None, out=True):
    """The three entry points that take a batch's arrays, called with exactly these pointers; returns (status, message)."""
    lib = capi.lib()
    B = (len(poff) - 1) if B is None else B
    F = int(poff[-1]) if poff is not None and len(poff) else 0
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t)) if a is not None else None
    poff = np.ascontiguousarray(poff, dtype=np.int64) if poff is not None else None
    foff = np.ascontiguousarray(foff, dtype=np.int64) if foff is not None else None
    intr, q, t = np.zeros((max(B, 1), 9)), np.zeros((max(F, 1), 4)), np.zeros((max(F, 1), 3))
    q[:, 0] = 1.0
    opt = capi.default_options()
    if name == "create":
        h = C.c_void_p()
        rc = lib.cc_intrinsics_batch_create(C.c_int32(0), C.c_int64(B), p(poff, C.c_int64), p(foff, C.c_int64), p(uv, C.c_float),
                                            p(xyz, C.c_float), C.byref(h) if out else None)
        assert not h.value or rc == 0
        if h.value:
            lib.cc_intrinsics_batch_destroy(h)
    elif name == "optimize":
        rc = lib.cc_intrinsics_batch_optimize(C.byref(opt), C.c_int32(0), C.c_int64(B), p(poff, C.c_int64), p(foff, C.c_int64),
                                              p(uv, C.c_float), p(xyz, C.c_float), p(intr, C.c_double) if out else None, None,
                                              p(q, C.c_double), p(t, C.c_double), None)
    else:
        rc = lib.cc_intrinsics_batch_estimate(C.byref(opt), C.c_int32(0), C.c_int64(B), p(poff, C.c_int64), p(foff, C.c_int64),
                                              p(uv, C.c_float), p(xyz, C.c_float), None, None, None, p(intr, C.c_double) if out else None,
                                              p(q, C.c_double), p(t, C.c_double), None)
    return rc, lib.cc_last_error().decode()


ENTRY_POINTS = ["create", "optimize", "estimate"]
BAD_ARGUMENT, NO_DEVICE = -1, -2


@pytest.mark.skipif(capi.device_count() > 0, reason="only meaningful without a GPU")
@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_entry_points_report_the_missing_device(name):
    off, uv, xyz = _problem()
    foff = np.concatenate([off, off[1:] + off[-1]])
    rc, msg = _raw(name, [0, 3, 6], foff, np.concatenate([uv, uv]), np.concatenate([xyz, xyz]))
    assert rc == NO_DEVICE and "no HIP device" in msg, (rc, msg)


@pytest.mark.skipif(capi.device_count() > 0, reason="only meaningful without a GPU")
def test_python_surface_raises_without_a_device():
    off, uv, xyz = _problem()
    with pytest.raises(capi.CcError, match="no HIP device|no CPU fallback"):
        capi.IntrinsicsBatch([(off, uv, xyz), (off, uv, xyz)])
    with pytest.raises(capi.CcError, match="no HIP device|no CPU fallback"):
        capi.intrinsics_batch_optimize([(off, uv, xyz)], np.zeros((1, 9)), [np.tile([1.0, 0, 0, 0], (3, 1))], [np.zeros((3, 3))])
    with pytest.raises(capi.CcError, match="no HIP device|no CPU fallback"):
        capi.intrinsics_batch_estimate([(off, uv, xyz)])


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_bad_arguments_are_refused_before_any_device_call(name):
    """BAD_ARGUMENT on a machine without a device too: the checks come first."""
    off, uv, xyz = _problem()
    foff2 = np.concatenate([off, off[1:] + off[-1]])
    uv2, xyz2 = np.concatenate([uv, uv]), np.concatenate([xyz, xyz])
    cases = {
        "no problems": dict(poff=[0], foff=[0], uv=uv, xyz=xyz, B=0),
        "negative count": dict(poff=[0, 3], foff=off, uv=uv, xyz=xyz, B=-1),
        "a problem without frames": dict(poff=[0, 3, 3, 6], foff=foff2, uv=uv2, xyz=xyz2),
        "problem offsets decrease": dict(poff=[0, 4, 3, 6], foff=foff2, uv=uv2, xyz=xyz2),
        "problem offsets start late": dict(poff=[1, 3], foff=off, uv=uv, xyz=xyz),
        "frame offsets decrease": dict(poff=[0, 3], foff=[0, 8, 4, 12], uv=uv, xyz=xyz),
        "frame offsets start late": dict(poff=[0, 3], foff=[4, 8, 12, 16], uv=uv, xyz=xyz),
        "problem offsets NULL": dict(poff=None, foff=off, uv=uv, xyz=xyz, B=1),
        "frame offsets NULL": dict(poff=[0, 3], foff=None, uv=uv, xyz=xyz),
        "uv NULL": dict(poff=[0, 3], foff=off, uv=None, xyz=xyz),
        "xyz NULL": dict(poff=[0, 3], foff=off, uv=uv, xyz=None),
        "output NULL": dict(poff=[0, 3], foff=off, uv=uv, xyz=xyz, out=False),
    }
    for label, kw in cases.items():
        rc, msg = _raw(name, **kw)
        assert rc == BAD_ARGUMENT and msg, (label, rc, msg)
    if name == "estimate":   # Zhang's preconditions, per problem
        rc, msg = _raw(name, [0, 2], off[:3], uv, xyz)
        assert rc == BAD_ARGUMENT and "fewer than 3 frames" in msg
        rc, msg = _raw(name, [0, 3], [0, 4, 7, 11], uv, xyz)
        assert rc == BAD_ARGUMENT and "fewer than 4 points" in msg


def test_handle_calls_refuse_a_null_handle():
    lib = capi.lib()
    x = np.zeros(16)
    px = x.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.cc_intrinsics_batch_set_state(None, px, None, px, px) == BAD_ARGUMENT
    assert lib.cc_intrinsics_batch_get_state(None, px, px, px) == BAD_ARGUMENT
    assert lib.cc_intrinsics_batch_solve(None, None, None) == BAD_ARGUMENT
    lib.cc_intrinsics_batch_destroy(None)   # a no-op


def test_batch_layout_of_the_python_binding():
    a, b = _problem(3, 4), _problem(2, 5)
    poff, foff, uv, xyz = capi._batch_layout([a, b])
    assert poff.tolist() == [0, 3, 5] and foff.tolist() == [0, 4, 8, 12, 17, 22]
    assert uv.shape == (22, 2) and xyz.shape == (22, 3) and uv.dtype == np.float32


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_batch_kernels_keep_their_register_allocation():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "kernel_regs.py"),
                        os.path.join(ROOT, "camera_calibrator_amd", "csrc", "cc_intrinsics_batch.hip")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    t = {}
    for line in r.stdout.splitlines()[1:]:
        m = re.match(r"(\S.*?)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)$", line)
        if m:
            t[m.group(1)] = dict(zip(("vgpr", "agpr", "sgpr", "vspill", "sspill", "scratch", "lds"), map(int, m.groups()[1:])))
    assert set(t) == {"cc::k_intrb_sweep", "cc::k_intrb_step", "cc::k_intrb_begin"}, sorted(t)
    sweep, step = t["cc::k_intrb_sweep"], t["cc::k_intrb_step"]
    # the sweep runs four waves per SIMD (128 registers) and must not touch scratch: a spill there is traffic in the main loop
    assert sweep["vgpr"] == 124 and sweep["vspill"] == 0 and sweep["sspill"] == 0 and sweep["scratch"] == 0, sweep
    # the step is one 256-thread workgroup per problem (one wave per SIMD): what the built kernel has, as k_intr_decide_elim
    assert step["vgpr"] == 273 and step["vspill"] <= 18 and step["scratch"] <= 112, step
