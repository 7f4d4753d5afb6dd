"""tests/zhang_ref.py on its own (no GPU, no library): the reference that tests/test_gpu_zhang_stages.py holds the kernels of
Zhang's initialisation against must itself recover a planted truth, reach every branch the pose-stage test claims to reach,
and count exactly.

Measured (float32 rounding of the pixels is the only error on a noise-free scene): K to at most 6.2e-7 relative, R to 5.7e-7,
t / distance to 8.6e-7, against the bounds of 2e-6 asserted below. Census of the 360 pose-stage inputs by quaternion branch:
trace 86, x 90, y 94, z 90."""
import collections

import numpy as np
import pytest
from mpmath import mp, mpf

from tests import zhang_ref as zr


@pytest.mark.parametrize("units", list(zr.UNITS))
@pytest.mark.parametrize("camera", list(zr.CAMERAS))
def test_reference_recovers_the_planted_camera_and_poses(camera, units):
    sc = zr.noise_free_scene(camera, units)
    F = len(sc["off"]) - 1
    Hs = np.array([zr.homography_f32(*zr.frame(sc, f)) for f in range(F)])
    alpha, beta, u0, v0 = (float(v) for v in zr.k_from_b(Hs))
    K = sc["K"]
    errK = max(abs(alpha - K[0, 0]) / K[0, 0], abs(beta - K[1, 1]) / K[1, 1], abs(u0 - K[0, 2]) / K[0, 0], abs(v0 - K[1, 2]) / K[0, 0])
    K32 = np.array([[alpha, 0, u0], [0, beta, v0], [0, 0, 1]], dtype=np.float32)
    errR = errt = 0.0
    for f in range(F):
        p = zr.front_pose(Hs[f], K32)
        errR = max(errR, np.abs(p["R"] - sc["R"][f]).max())
        errt = max(errt, np.abs(p["t"] - sc["t"][f]).max() / sc["distance"])
    print(f"[zhang-ref] {camera} {units}: K {errK:.2e} relative, R {errR:.2e}, t / distance {errt:.2e}")
    assert errK <= 2e-6 and errR <= 2e-6 and errt <= 2e-6, (errK, errR, errt)


def test_census_every_quaternion_branch_is_reached_by_the_pose_stage_inputs():
    inputs, refs = zr.pose_stage_inputs(), zr.pose_references("census")
    count = collections.Counter(r["branch"] for r in refs)
    print("[zhang-ref] pose-stage inputs by quaternion branch:", dict(count))
    for b in zr.BRANCHES:
        assert count[b] >= 10, count
    # every pose comes once as H and once as -H
    Hs = {H.tobytes() for _, _, H, _ in inputs}
    for _, _, H, _ in inputs:
        assert (-H).tobytes() in Hs
    # and the truth of every one has t_z > 0 in exactly one of the two
    for r in refs:
        assert r["t"][2] > 0


def test_exact_gram_agrees_with_fdot_on_floats_and_with_integers_on_integers():
    rng = np.random.default_rng(5)
    sc = zr.noisy_scene("large", "millimetres")
    A = zr.dlt_rows(*zr.frame(sc, 3))
    G, S = zr.exact_gram(A)
    old = mp.dps
    mp.dps = 80    # the products have 48 bits each and the sums span ~60 bits of exponent: 80 digits hold all of it
    try:
        for i in range(9):
            for j in range(9):
                want = mp.fdot([mpf(float(v)) for v in A[:, i]], [mpf(float(v)) for v in A[:, j]])
                wabs = mp.fdot([abs(mpf(float(v))) for v in A[:, i]], [abs(mpf(float(v))) for v in A[:, j]])
                assert mpf(G[i, j].numerator) / mpf(G[i, j].denominator) == want
                assert mpf(S[i, j].numerator) / mpf(S[i, j].denominator) == wabs
    finally:
        mp.dps = old
    M = rng.integers(-64, 65, size=(1026, 9))
    G, S = zr.exact_gram(M.astype(np.float64))
    want = M.astype(np.int64).T @ M.astype(np.int64)
    assert all(G[i, j] == int(want[i, j]) for i in range(9) for j in range(9))
    wabs = np.abs(M).astype(np.int64).T @ np.abs(M).astype(np.int64)
    assert all(S[i, j] == int(wabs[i, j]) for i in range(9) for j in range(9))


def test_dlt_rows_take_their_products_in_float32():
    xyz = np.array([[0.1, 0.7, 0.0]], dtype=np.float32)
    uv = np.array([[1234.567, 89.0123]], dtype=np.float32)
    A = zr.dlt_rows(xyz, uv)
    x1, y1, x2, y2 = xyz[0, 0], xyz[0, 1], uv[0, 0], uv[0, 1]
    assert A[0].tolist() == [0, 0, 0, -float(x1), -float(y1), -1.0, float(np.float32(x1 * y2)), float(np.float32(y1 * y2)), float(y2)]
    assert A[1].tolist() == [float(x1), float(y1), 1.0, 0, 0, 0, -float(np.float32(x1 * x2)), -float(np.float32(y1 * x2)), -float(x2)]
    assert float(np.float32(x1 * x2)) != float(x1) * float(x2)    # (the float product is a rounding, not the double one)
