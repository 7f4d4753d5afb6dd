"""GPU: the class surface of the rig start -- pycalibrator.ExtrinsicsCalibrator.EstimateInitialPoses / Estimate /
LastStartReport (csrc/extrinsics_calibrator.cpp over cc_rig_estimate_start). Optimize() on its own is what it was: the existing
class-surface tests (tests/test_gpu_pycalibrator.py, tests/test_gpu_dropin_cpp.py) run it on the existing fixtures unchanged."""
import os
import sys

import numpy as np
import pytest

from camera_calibrator_amd import capi
from oracle import pyoracle as po

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "camera_calibrator_amd"))
pytestmark = pytest.mark.gpu
CC_ERR_STATE = -5
C, F, M, SEED = 3, 20, 12, 1


def _build(sc, at_identity):
    import pycalibrator as pc
    e = pc.ExtrinsicsCalibrator()
    e.SetVerbose(False)
    eye = np.eye(4, dtype=np.float32)
    for c in range(C):
        e.AddCameraTRig(eye if at_identity else sc["cam_T"][c].reshape(4, 4).T, freeze=(c == 0))
    for f in range(F):
        e.AddObservationFrame(eye if at_identity else sc["frame_T"][f].reshape(4, 4).T)
    k = 0
    for f in range(F):
        for p in range(M):
            w = e.AddWorldPoint(f, sc["world_xyz"][f * M + p])
            for c in range(C):
                assert sc["obs_cam"][k] == c and sc["obs_world"][k] == w
                e.AddObservation(c, w, sc["obs_uv"][k])
                k += 1
    return e


def test_estimate_from_identity_poses_reaches_the_cost_of_optimize_from_the_scenarios():
    sc = po.rig_scenario(C, F, M, seed=SEED)
    a = _build(sc, at_identity=False)
    a.Optimize()
    b = _build(sc, at_identity=True)
    b.Estimate()
    assert a.LastStatus() == 0 and b.LastStatus() == 0
    rep = b.LastStartReport()
    assert rep["views_valid"] == C * F and rep["views_invalid"] == 0 and rep["cameras_unplaced"] == 0 and rep["frames_unplaced"] == 0
    assert rep["root_camera"] == 0 and not rep["root_at_identity"] and rep["parent"] == [-1, 0, 0]
    # Both solves stop by Ceres' default function tolerance, 1e-6 of the cost per iteration: each ends within a few 1e-6 of
    # the minimum's cost (the frozen camera at the identity instead of its pose only renames the rig frame), so 1e-5 apart
    # at the most
    ca, cb = a.LastFinalCost(), b.LastFinalCost()
    print(f"Optimize from the scenario's poses {ca:.9e} ({a.LastIterations()} it), Estimate from identities {cb:.9e} ({b.LastIterations()} it)")
    assert abs(ca - cb) <= 1e-5 * ca
    assert np.array_equal(b.GetCameraTRig(0), np.eye(4, dtype=np.float32))   # frozen: as it was added


def test_estimate_initial_poses_stores_what_the_c_abi_computes():
    sc = po.rig_scenario(C, F, M, seed=SEED)
    e = _build(sc, at_identity=True)
    e.EstimateInitialPoses()
    assert e.LastStatus() == 0
    p = capi.RigProblem(C, sc["frame_offsets"], sc["obs_cam"], sc["obs_world"], sc["obs_uv"], sc["world_xyz"], sc["cam_frozen"])
    rep = p.estimate_start()
    cq, ct, fq, ft, _ = p.get_state(want_cost=False)
    p.close()
    got = e.LastStartReport()
    assert got["parent"] == list(rep["parent"]) and all(got[k] == rep[k] for k in rep if k != "parent")
    want_c, want_f = po.qt_to_affine(cq, ct), po.qt_to_affine(fq, ft)   # fp64 pose -> float 4 x 4, as the class stores it
    for c in range(C):
        assert np.abs(e.GetCameraTRig(c).T.reshape(-1) - want_c[c]).max() <= 1e-6
    for f in range(F):
        assert np.abs(e.GetObservationFrame(f).T.reshape(-1) - want_f[f]).max() <= 1e-6 * max(1.0, np.abs(want_f[f]).max())
    # several devices: refused, nothing changes
    before = [e.GetCameraTRig(c) for c in range(C)] + [e.GetObservationFrame(f) for f in range(F)]
    e.SetDevices([0, 1])
    e.EstimateInitialPoses()
    assert e.LastStatus() == CC_ERR_STATE
    after = [e.GetCameraTRig(c) for c in range(C)] + [e.GetObservationFrame(f) for f in range(F)]
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
