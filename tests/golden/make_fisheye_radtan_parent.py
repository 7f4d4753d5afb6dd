"""Results of a radial-tangential Calibrator (pycalibrator) on the 8 x 40 fixture, recorded on the GPU from PARENT_COMMIT: the
state before the fisheye camera model went through the class, the C ABI and the point kernels' translation
unit. The model is off by default, so a Calibrator that never calls SetCameraModel must reproduce these numbers BIT FOR BIT
(tests/test_gpu_pycalibrator_fisheye.py). Run once, on a GPU, on a build of PARENT_COMMIT:
    python tests/golden/make_fisheye_radtan_parent.py      -> tests/golden/fisheye_radtan_parent.npz
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PARENT_COMMIT = "1eabca1"   # "Huber loss for the intrinsics solve: single, batched, class surface"


def run_all(inputs):
    """{name: array}: Estimate free and with k3 held, Estimate with the Huber loss (the two-kernel form), Optimize from the Zhang
    start, Distort / Undistort with the estimated model."""
    sys.path.insert(0, os.path.join(ROOT, "camera_calibrator_amd"))
    import pycalibrator as pc
    off, uv, xyz = inputs["off"], inputs["uv"], inputs["xyz"]
    img = [uv[off[f]:off[f + 1]] for f in range(len(off) - 1)]
    world = [xyz[off[f]:off[f + 1]] for f in range(len(off) - 1)]
    out = {}

    def record(tag, c):
        assert c.LastStatus() == 0
        out[tag + "_K"], out[tag + "_dist"] = np.array(c.GetK()), np.array(c.GetDistortion())
        out[tag + "_iterations"], out[tag + "_form"] = np.int64(c.LastIterations()), np.int64(c.LastSolverForm())
        out[tag + "_cost"] = np.float64(c.LastFinalCost())

    c = pc.Calibrator(1600, 1000)
    c.Estimate(img, world)
    record("free", c)
    out["distort"] = np.array(c.Distort([p for p in inputs["xy"]]))
    out["undistort"] = np.array(c.Undistort([p for p in out["distort"]]))
    h = pc.Calibrator(1600, 1000)
    h.ForceDistortionToConstant(4)
    h.Estimate(img, world)
    record("k3_held", h)
    r = pc.Calibrator(1600, 1000)
    r.SetHuberLoss(1.0)
    r.Estimate(img, world)
    record("huber", r)
    o = pc.Calibrator(1600, 1000)
    o.SetK(inputs["K0"])
    o.Optimize(img, world, [q for q in inputs["q0"]], [t for t in inputs["t0"]])
    record("optimize", o)
    return out


def make_inputs():
    sys.path.insert(0, ROOT)
    from oracle import pyoracle as po
    off, uv, xyz = po.make_intrinsics_problem(8, 40)
    K0, q0, t0 = po.zhang_init(off, uv, xyz)
    rng = np.random.default_rng(7)
    xy = rng.uniform(-0.6, 0.45, size=(257, 2)).astype(np.float32)
    return dict(off=off, uv=uv, xyz=xyz, xy=xy, K0=K0.astype(np.float32), q0=q0.astype(np.float32), t0=t0.astype(np.float32))


if __name__ == "__main__":
    inputs = make_inputs()
    res = run_all(inputs)
    for k, v in res.items():
        assert np.all(np.isfinite(v)), k
    print({k: (int(v) if k.endswith(("iterations", "form")) else None) for k, v in res.items() if k.endswith(("iterations", "form"))})
    dst = os.environ.get("FISHEYE_RADTAN_OUT", os.path.join(os.path.dirname(os.path.abspath(__file__)), "fisheye_radtan_parent.npz"))
    np.savez_compressed(dst, parent_commit=PARENT_COMMIT, **{"in_" + k: v for k, v in inputs.items()}, **res)
    print("wrote", dst, os.path.getsize(dst), "bytes")
