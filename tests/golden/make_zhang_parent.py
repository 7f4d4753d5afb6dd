"""Outputs K, q, t and H of cc_zhang_init recorded on the GPU from PARENT_COMMIT: the state before the four kernels and their
device helpers moved, text unchanged, from cc_zhang.hip into cc_zhang_dev.hpp so that the probe library can
launch them one at a time. The move changes no arithmetic, so the branch must reproduce these numbers BIT FOR BIT
(tests/test_gpu_zhang.py, which names the one quaternion that the fix of k_zhang_poses' second attempt moved by one float32
unit). Two inputs: the ragged 12-frame generator problem of test_gpu_zhang.py, and the 12-frame planted
problem of tests/zhang_ref.py in millimetres with fx != fy, whose inputs are stored too. Run once, on a GPU, on a build of
PARENT_COMMIT:
    python tests/golden/make_zhang_parent.py      -> tests/golden/zhang_parent.npz
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PARENT_COMMIT = "86f38db"   # "k_intr_persist: end of a solve as tagged words, without L2 write-back"
RAGGED = [4, 9, 64, 65, 300, 5, 257, 128, 77, 500, 31, 1000]


def make_inputs():
    sys.path.insert(0, ROOT)
    from oracle import pyoracle as po
    from tests import zhang_ref as zr
    off, uv, xyz = po.make_intrinsics_problem(len(RAGGED), RAGGED)
    sc = zr.golden_planted_problem()
    return {"ragged": (off, uv, xyz), "planted": (sc["off"], sc["uv"], sc["xyz"])}


def run_all(inputs):
    sys.path.insert(0, ROOT)
    from camera_calibrator_amd import capi
    out = {}
    for name, (off, uv, xyz) in inputs.items():
        K, q, t, H = capi.zhang_init(off, uv, xyz, want_homographies=True)
        out[name + "_K"], out[name + "_q"], out[name + "_t"], out[name + "_H"] = K, q, t, H
    return out


if __name__ == "__main__":
    inputs = make_inputs()
    res = run_all(inputs)
    for k, v in res.items():
        assert np.all(np.isfinite(v)), k
    off, uv, xyz = inputs["planted"]
    dst = os.environ.get("ZHANG_PARENT_OUT", os.path.join(os.path.dirname(os.path.abspath(__file__)), "zhang_parent.npz"))
    np.savez_compressed(dst, parent_commit=PARENT_COMMIT, in_planted_off=off, in_planted_uv=uv, in_planted_xyz=xyz, **res)
    print("wrote", dst, os.path.getsize(dst), "bytes")
