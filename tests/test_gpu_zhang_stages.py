"""The four kernels of Zhang's initialisation (cc_zhang_dev.hpp) and the two helpers they inline, each stage on its own through
the probe library (tests/cpp/dev_probe.hip, tests/dev_probe.py), against tests/zhang_ref.py: exact integers and Fractions for
the Gram, mpmath at 50 digits for the eigenvectors, K and the poses. Neither the oracle nor the code under test is the
reference; the oracle appears once, as the yardstick of what float32 arithmetic can deliver at the pose stage. u = 2^-53.

Every bound comes from the arithmetic or from the contract written in cc_zhang_dev.hpp (the homography is kept as float32, so
its eigenvector must be good to 2^-24), none from the results; each test prints its worst case (`pytest -s`).

Measured on an MI355X:

    0.033 of the bound      (2n + 8) u Σ|a||b| per entry    k_zhang_gram, planted and generator frames: largest error / bound
    1.21e-8                 2^-24 = 5.96e-8                 smallest_eigvec<9>, worst sine to the 50-digit eigenvector (four-point
                                                            frames; planted frames 4.50e-10, 30-point generator frames 3.49e-12)
    2.09e-15                2^-24                           smallest_eigvec<6>, worst sine (F = 3, 4, 5, 300)
    1.7 u                   16 u                            | |x| - 1 | of both (the restatement's 1.7 u; the device 1.3 u)
    3.05e-8                 2^-22 = 2.38e-7                 k_zhang_k against k_from_b, worst of alpha, beta (relative), u0, v0 (/ alpha)
    q 4.62e-8, t 2.01e-7    2 e_ref + 2^-22                 k_zhang_poses: worst q error and worst t error / |t|; the oracle's e_ref on
                                                            the same inputs: q 4.62e-8, t 1.73e-7
    q 3.94e-8, t 1.42e-7    2 e_ref + 2^-22                 the same on skewed columns (polar factor); oracle q 3.94e-8, t 1.15e-7
    0.126, 0.086            32 u, 32 u |S|                  jacobi_eigen<3>: orthogonality, reconstruction, as fractions of the bound

What these tests found: k_zhang_poses returned quaternions one float32 unit apart for H and -H (x180/4, s = +-1000). Its
two-attempt loop was unrolled into two copies whose multiplications and additions the compiler fused differently; the kernel
now negates r0, r1 and t, which is exact, and runs one copy of the arithmetic. A numpy restatement of the kernels with the
x-pivot or the y-pivot branch of the quaternion step taken out fails test_poses_on_every_quaternion_branch_and_for_both_signs_of_h
(q errors of 7e-7 and 1.6e-6 against an allowance of 2.4e-7).
"""
import functools
from fractions import Fraction

import numpy as np
import pytest
from mpmath import mp, mpf

from oracle import pyoracle as po
from tests import dev_probe as dp
from tests import zhang_ref as zr

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
F32_EPS = 2.0 ** -24


def _report(what, text):
    print(f"[zhang-stages] {what}: {text}")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _pack(frames):
    """[(xyz, uv)] -> off, uv, xyz of one launch."""
    off = np.concatenate([[0], np.cumsum([len(x) for x, _ in frames])]).astype(np.int64)
    return off, np.concatenate([u for _, u in frames]).astype(np.float32), np.concatenate([x for x, _ in frames]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _generator_frames(count, pts):
    off, uv, xyz = po.make_intrinsics_problem(count, pts)
    return tuple((xyz[off[f]:off[f + 1]], uv[off[f]:off[f + 1]]) for f in range(count))


@functools.lru_cache(maxsize=None)
def _planted_frames():
    """Four frames (one of each base rotation) of every camera, unit set and noise level: 48 frames of 48 points."""
    out = []
    for cam in zr.CAMERAS:
        for units in zr.UNITS:
            for sc in (zr.noise_free_scene(cam, units), zr.noisy_scene(cam, units)):
                out += [zr.frame(sc, f) for f in range(4)]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _float_frames():
    return _planted_frames() + _generator_frames(6, 30)


@functools.lru_cache(maxsize=None)
def _exact_grams(which):
    frames = {"float": _float_frames, "four": lambda: _generator_frames(6, 4)}[which]()
    return tuple(zr.exact_gram(zr.dlt_rows(x, u)) for x, u in frames)


# ---------------------------------------------------------------------------------------------------------------------
# k_zhang_gram
# ---------------------------------------------------------------------------------------------------------------------
INT_SIZES = [4, 5, 63, 64, 65, 255, 256, 257, 513]


def test_gram_exact_on_integers_zero_padding_and_symmetric():
    """Integer coordinates |v| <= 64: every product is at most 2^12 (exact in float32), every partial sum stays below 2^34
    (exact in double in any order), so the 9 x 9 block IS the integer product, for every pass count and tail length."""
    rng = np.random.default_rng(31)
    frames = []
    for n in INT_SIZES:
        xyz = np.zeros((n, 3), dtype=np.float32)
        xyz[:, :2] = rng.integers(-64, 65, size=(n, 2))
        frames.append((xyz, rng.integers(-64, 65, size=(n, 2)).astype(np.float32)))
    got = dp.zhang_gram(*_pack(frames))
    for f, (xyz, uv) in enumerate(frames):
        A = zr.dlt_rows(xyz, uv).astype(np.int64)
        want = A.T @ A
        assert np.abs(want).max() < 2 ** 34
        assert np.array_equal(got[f, :9, :9], want.astype(np.float64)), (INT_SIZES[f], got[f, :9, :9] - want)
        assert not np.any(got[f, 9:, :]) and not np.any(got[f, :, 9:]), INT_SIZES[f]
        assert _same_bits(got[f], got[f].T.copy()), INT_SIZES[f]


def test_gram_of_floats_within_the_summation_bound_of_the_exact_gram():
    """The operands are floats and their float products are kept as floats, so each product of two operands is exact in double:
    the only error is that of summing 2n of them, in whatever order (the accumulators, the two halves, the four waves), and
    (2n + 8) u Σ|a||b| bounds any order."""
    frames, exact = _float_frames(), _exact_grams("float")
    got = dp.zhang_gram(*_pack(frames))
    worst = 0.0
    for f, ((xyz, _), (G, S)) in enumerate(zip(frames, exact)):
        n = len(xyz)
        assert np.all(np.isfinite(got[f]))
        for i in range(9):
            for j in range(9):
                err = abs(Fraction(float(got[f, i, j])) - G[i, j])
                bound = (2 * n + 8) * Fraction(U) * S[i, j]
                if S[i, j] == 0:
                    assert got[f, i, j] == 0.0
                    continue
                worst = max(worst, float(err / bound))
                assert err <= bound, (f, i, j, float(err), float(bound))
        assert not np.any(got[f, 9:, :]) and not np.any(got[f, :, 9:])
    _report("Gram of floats, largest error / bound", f"{worst:.3f}")


def test_gram_of_a_frame_does_not_depend_on_its_neighbours():
    gen = _generator_frames(6, 30)
    planted = _planted_frames()
    big = po.make_intrinsics_problem(1, 300)
    X = (big[2], big[1])                       # two passes, a tail of 44
    others = [gen[0], planted[5], gen[3], planted[17], _generator_frames(6, 4)[1]]
    first = dp.zhang_gram(*_pack([X] + others))
    middle = dp.zhang_gram(*_pack(others[:2] + [X] + others[2:]))
    last = dp.zhang_gram(*_pack(others + [X]))
    assert _same_bits(first[0], middle[2]) and _same_bits(first[0], last[5])
    assert _same_bits(first[1:], last[:5])
    # a NaN pixel in X poisons X's block and nothing else
    Xn = (X[0], X[1].copy())
    Xn[1][257, 0] = np.nan
    bad = dp.zhang_gram(*_pack(others[:2] + [Xn] + others[2:]))
    assert not np.all(np.isfinite(bad[2]))
    keep = [0, 1, 3, 4, 5]
    assert _same_bits(bad[keep], middle[keep])


# ---------------------------------------------------------------------------------------------------------------------
# smallest_eigvec<9>, smallest_eigvec<6>, k_zhang_eig9
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _eig9_cases():
    """(matrices [n][9][9] of doubles: exact_gram rounded, so that the stage sees exactly what the reference sees; labels)."""
    mats = [zr.to_double(G) for G, _ in _exact_grams("float")] + [zr.to_double(G) for G, _ in _exact_grams("four")]
    labels = ["planted"] * len(_planted_frames()) + ["generator 30"] * 6 + ["four points"] * 6
    return np.array(mats), labels


def _check_eigvecs(A, labels):
    got = dp.smallest_eigvec(A)
    worst, worst_norm = {}, 0.0
    for a, x, lab in zip(A, got, labels):
        assert np.all(np.isfinite(x)), lab
        sine = zr.sine_to(x, zr.smallest_eigvec_mp(a))
        worst[lab] = max(worst.get(lab, 0.0), sine)
        nrm = abs(mp.sqrt(sum(mpf(float(v)) ** 2 for v in x)) - 1)
        worst_norm = max(worst_norm, float(nrm))
        assert sine <= F32_EPS, (lab, sine)
        assert nrm <= 16 * U, (lab, float(nrm))
    return got, worst, worst_norm


def test_smallest_eigvec9_is_as_good_as_the_float32_it_is_stored_in():
    A, labels = _eig9_cases()
    _, worst, worst_norm = _check_eigvecs(A, labels)
    _report("smallest_eigvec<9>, worst sine to the 50-digit eigenvector",
            ", ".join(f"{k} {v:.2e}" for k, v in worst.items()) + f"; | |x| - 1 | <= {worst_norm / U:.1f} u")


def test_smallest_eigvec6_on_the_k_systems_of_planted_homographies():
    Hs = zr.many_homographies()
    Fs = [3, 4, 5, 300]
    A = np.array([zr.mp_to_double(zr.k_system_mp(Hs[:F])) for F in Fs])
    _, worst, worst_norm = _check_eigvecs(A, [f"F = {F}" for F in Fs])
    _report("smallest_eigvec<6>, worst sine", ", ".join(f"{k} {v:.2e}" for k, v in worst.items()) + f"; | |x| - 1 | <= {worst_norm / U:.1f} u")


def test_eig9_kernel_stores_the_float32_rounding_of_smallest_eigvec():
    A, _ = _eig9_cases()
    gram = np.zeros((len(A), 16, 16))
    gram[:, :9, :9] = A
    H = dp.zhang_eig9(gram)
    x = dp.smallest_eigvec(A)
    assert _same_bits(H.reshape(-1, 9), x.astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------------
# k_zhang_k
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [3, 4, 5, 12, 257, 300])
def test_k_from_reference_homographies_matches_the_closed_form_at_50_digits(F):
    """(257 and 300 cross the kernel's stride of 256 frames per thread.) Four float32 units in the last place on a result that
    is stored as float32."""
    Hs = zr.many_homographies()[:F]
    K = dp.zhang_k(Hs).astype(np.float64)
    alpha, beta, u0, v0 = (float(v) for v in zr.k_from_b(Hs))
    errs = [abs(K[0, 0] - alpha) / alpha, abs(K[1, 1] - beta) / beta, abs(K[0, 2] - u0) / alpha, abs(K[1, 2] - v0) / alpha]
    _report(f"k_zhang_k, F = {F}", "errors of alpha, beta (relative), u0, v0 (/ alpha): " + " ".join(f"{e:.2e}" for e in errs))
    assert np.all(np.isfinite(K))
    assert max(errs[:2]) <= 2.0 ** -22 and max(errs[2:]) <= 2.0 ** -22, errs
    assert K[0, 1] == 0.0 and K[1, 0] == 0.0 and K[2, 0] == 0.0 and K[2, 1] == 0.0 and K[2, 2] == 1.0


# ---------------------------------------------------------------------------------------------------------------------
# k_zhang_poses
# ---------------------------------------------------------------------------------------------------------------------
def _inv3f(m):
    """The oracle's inv3f: cofactors in float32."""
    m = np.asarray(m, dtype=np.float32).ravel()
    c00, c01, c02 = m[4] * m[8] - m[5] * m[7], m[5] * m[6] - m[3] * m[8], m[3] * m[7] - m[4] * m[6]
    d = np.float32(1.0) / (m[0] * c00 + m[1] * c01 + m[2] * c02)
    return np.array([c00 * d, (m[2] * m[7] - m[1] * m[8]) * d, (m[1] * m[5] - m[2] * m[4]) * d,
                     c01 * d, (m[0] * m[8] - m[2] * m[6]) * d, (m[2] * m[3] - m[0] * m[5]) * d,
                     c02 * d, (m[1] * m[6] - m[0] * m[7]) * d, (m[0] * m[4] - m[1] * m[3]) * d], dtype=np.float32).reshape(3, 3)


def _quat_eigen(R):
    """The oracle's mat_to_quat (Eigen's rule) in double on a float32 rotation, stored as float32."""
    m = np.asarray(R, dtype=np.float64).ravel()
    q = np.zeros(4)
    t = m[0] + m[4] + m[8]
    if t > 0:
        t = np.sqrt(t + 1.0)
        q[0] = 0.5 * t
        t = 0.5 / t
        q[1], q[2], q[3] = (m[7] - m[5]) * t, (m[2] - m[6]) * t, (m[3] - m[1]) * t
    else:
        i = 0
        if m[4] > m[0]:
            i = 1
        if m[8] > m[i * 4]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = np.sqrt(m[i * 4] - m[j * 4] - m[k * 4] + 1.0)
        q[1 + i] = 0.5 * t
        t = 0.5 / t
        q[0] = (m[k * 3 + j] - m[j * 3 + k]) * t
        q[1 + j] = (m[j * 3 + i] + m[i * 3 + j]) * t
        q[1 + k] = (m[k * 3 + i] + m[i * 3 + k]) * t
    return q.astype(np.float32)


def _oracle_pose(K, H):
    """po.recover_extrinsics with the oracle's own retry on t_z < 0 (oc_zhang_init), then its quaternion."""
    Ki = _inv3f(K)
    R, t = po.recover_extrinsics(Ki, H)
    if t[2] < 0:
        R, t = po.recover_extrinsics(Ki, -np.asarray(H, dtype=np.float32))
    return _quat_eigen(R), t


def _quat_err(q, ref):
    q = np.asarray(q, dtype=np.float64)
    return min(np.abs(q - ref).max(), np.abs(q + ref).max())


def _check_poses(inputs, refs, what):
    """The kernel may err by 2 e_ref + 2^-22 (t: 2^-22 |t|), e_ref the error of the oracle's float32 route on the same input
    against the 50-digit pose: both work in float32, in different operation orders."""
    q_all, t_all = np.zeros((len(inputs), 4), dtype=np.float32), np.zeros((len(inputs), 3), dtype=np.float32)
    for K in zr.CAMERAS.values():          # one launch per camera
        K32 = K.astype(np.float32)
        idx = [n for n, (_, Kn, _, _) in enumerate(inputs) if np.array_equal(Kn, K32)]
        q, t = dp.zhang_poses(np.array([inputs[n][2] for n in idx]), K32)
        q_all[idx], t_all[idx] = q, t
    worst = dict(q=0.0, q_ref=0.0, t=0.0, t_ref=0.0)
    for n, ((label, K, H, _), ref) in enumerate(zip(inputs, refs)):
        assert np.all(np.isfinite(q_all[n])) and np.all(np.isfinite(t_all[n])), label
        qo, to = _oracle_pose(K, H)
        tn = np.linalg.norm(ref["t"])
        eq, eq_ref = _quat_err(q_all[n], ref["q"]), _quat_err(qo, ref["q"])
        et, et_ref = np.abs(t_all[n].astype(np.float64) - ref["t"]).max(), np.abs(to.astype(np.float64) - ref["t"]).max()
        worst = dict(q=max(worst["q"], eq), q_ref=max(worst["q_ref"], eq_ref), t=max(worst["t"], et / tn), t_ref=max(worst["t_ref"], et_ref / tn))
        assert t_all[n, 2] >= 0, label
        assert eq <= 2 * eq_ref + 2.0 ** -22, (label, eq, eq_ref)
        assert et <= 2 * et_ref + 2.0 ** -22 * tn, (label, et, et_ref)
    _report(what, f"worst q error {worst['q']:.2e} (oracle {worst['q_ref']:.2e}), worst t error / |t| {worst['t']:.2e} (oracle {worst['t_ref']:.2e})")
    return q_all, t_all


def test_poses_on_every_quaternion_branch_and_for_both_signs_of_h():
    """All four branches of the matrix-to-quaternion step (tests/test_zhang_ref_cpu.py counts them), exact half turns (w = 0),
    the three-way tie of 120 degrees about (1,1,1), the seams trace = 0 and R00 = R11 from both sides; s = +-1, +-1e-3, +-1e3."""
    inputs, refs = zr.pose_stage_inputs(), zr.pose_references("census")
    q, t = _check_poses(inputs, refs, "k_zhang_poses")
    # H and -H are the same homography: the same bits come back (the inputs list s and -s next to each other)
    for n in range(0, len(inputs), 2):
        assert np.array_equal(inputs[n][2], -inputs[n + 1][2])
        assert _same_bits(q[n], q[n + 1]) and _same_bits(t[n], t[n + 1]), inputs[n][0]


def test_poses_of_skewed_columns_are_the_polar_factor():
    _check_poses(zr.skewed_inputs(), zr.pose_references("skewed"), "k_zhang_poses, skewed columns")


# ---------------------------------------------------------------------------------------------------------------------
# jacobi_eigen<3>
# ---------------------------------------------------------------------------------------------------------------------
def test_jacobi_eigen3_orthogonal_and_reconstructs_its_input():
    S = [np.eye(3), np.diag([3.0, 1.0, 2.0]), np.diag([1e-3, 1.0, 1e3]),       # no rotation at all: every pair takes the skip path
         np.array([[2.0, 1.0, 0.5], [1.0, 2.0, 0.25], [0.5, 0.25, 2.0]]),     # equal diagonal: theta = 0 in the first rotation
         np.array([[1.0, 0.5, 0.0], [0.5, 1.0, 0.0], [0.0, 0.0, 1.0]])]        # theta = 0 and two pairs skipped
    for _, K, H, _ in zr.skewed_inputs():                                      # R^T R of columns that are not orthonormal
        h = np.linalg.inv(K.astype(np.float64)) @ H.astype(np.float64)
        r0, r1 = h[:, 0] / np.linalg.norm(h[:, 0]), h[:, 1] / np.linalg.norm(h[:, 0])
        R = np.column_stack([r0, r1, np.cross(r0, r1)])
        S.append(R.T @ R)
    S = np.array(S)
    S = (S + S.transpose(0, 2, 1)) / 2
    lam, V = dp.jacobi_eigen3(S)
    worst_o = worst_r = 0.0
    for s, l, v in zip(S, lam, V):
        assert np.all(np.isfinite(l)) and np.all(np.isfinite(v))
        Vm, Sm = zr.to_mp(v), zr.to_mp(s)
        D = mp.diag([mpf(float(x)) for x in l])
        orth = Vm.T * Vm - mp.eye(3)
        rec = Vm * D * Vm.T - Sm
        eo = max(abs(orth[i, j]) for i in range(3) for j in range(3))
        er = max(abs(rec[i, j]) for i in range(3) for j in range(3)) / mpf(float(np.linalg.norm(s, 2)))
        worst_o, worst_r = max(worst_o, float(eo)), max(worst_r, float(er))
        assert eo <= 32 * U and er <= 32 * U, (s, float(eo), float(er))
    _report("jacobi_eigen<3>, largest error / (32 u)", f"orthogonality {worst_o / (32 * U):.3f}, reconstruction {worst_r / (32 * U):.3f}")
