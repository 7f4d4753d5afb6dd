"""A reference for Zhang's initialisation (cc_zhang.hip, cc_zhang_dev.hpp) that is neither the oracle nor the code under test:
plain numpy float64, Python integers / Fraction where a result is exact, mpmath at 50 digits elsewhere. Nothing here imports
the library. Used by tests/test_zhang_ref_cpu.py, tests/test_gpu_zhang_stages.py, tests/test_gpu_zhang.py and
tests/golden/make_zhang_parent.py.

The stages, as the reference has them (geometry.cpp:70-203, calibrator.cpp:47-66):
    dlt_rows -> exact_gram -> smallest_eigvec_mp        the homography of one frame
    k_from_b                                            K from the homographies (Zhang's closed form, zero skew)
    pose_from_h                                         RecoverExtrinsics + FixRotationMatrix + Quaternionf(R), for H and -H
"""
import functools
import math
from fractions import Fraction

import numpy as np
from mpmath import mp, mpf

mp.dps = 50

FIXTURE_K = np.array([[1000, 0, 800], [0, 1000, 500], [0, 0, 1]], dtype=np.float64)
SMALL_K = np.array([[420, 0, 331], [0, 415, 236], [0, 0, 1]], dtype=np.float64)
LARGE_K = np.array([[3500, 0, 1900], [0, 3480, 1100], [0, 0, 1]], dtype=np.float64)
CAMERAS = {"fixture": FIXTURE_K, "small": SMALL_K, "large": LARGE_K}
UNITS = {"metres": (0.03, 0.5), "millimetres": (30.0, 500.0)}   # name -> (pitch, distance)
NOISES = (0.0, 0.3)

BASE_ROTATIONS = {
    "identity": np.diag([1.0, 1.0, 1.0]),
    "x180": np.diag([1.0, -1.0, -1.0]),    # board y up against image y down: the common convention of real data
    "y180": np.diag([-1.0, 1.0, -1.0]),
    "z180": np.diag([-1.0, -1.0, 1.0]),
}
ALL_BASES = tuple(BASE_ROTATIONS.values())

BOARD_COLS, BOARD_ROWS = 8, 6


def rodrigues(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * Kx + (1.0 - math.cos(angle)) * (Kx @ Kx)


def board(pitch):
    """The 8 x 6 board: float32 world points, z = 0, the origin at one corner."""
    ix, iy = np.meshgrid(np.arange(BOARD_COLS), np.arange(BOARD_ROWS))
    xyz = np.zeros((BOARD_COLS * BOARD_ROWS, 3), dtype=np.float32)
    xyz[:, 0] = (ix.ravel() * np.float64(pitch)).astype(np.float32)
    xyz[:, 1] = (iy.ravel() * np.float64(pitch)).astype(np.float32)
    return xyz


def random_tilt(rng, max_deg=35.0):
    return rodrigues(rng.normal(size=3), math.radians(rng.uniform(0.0, max_deg)))


def planted_scene(rng, K, base_rotations, frames, pitch, distance, noise):
    """`frames` views of the board by a pinhole camera K with known poses: the truth a Zhang initialisation must return.

    Per frame R = (a random tilt of at most 35 degrees) x base_rotations[f mod len]; t puts the board's centre 0.8 to 1.5 x
    `distance` ahead of the camera with up to 0.1 x `distance` of sideways offset. Pixels: the pinhole model in float64 plus
    uniform noise of +-`noise` px, rounded to float32. Returns a dict: off, uv, xyz (the inputs of cc_zhang_init), K, R [F,3,3],
    t [F,3] (the truth), distance.

    Precondition, asserted here from the truth: every board point has positive depth AND t_z > 0, i.e. the world origin
    itself lies in front of the camera. A homography is defined up to sign; the kernel and the oracle both pick between H and
    -H by the sign of t_z (the depth of the world ORIGIN, not of the board), which is the port's own rule -- the reference
    makes no choice. A board whose origin lies far off the board and behind the camera plane therefore comes back mirrored
    from both (an origin 1.2 m from a 0.2 m board does it). That rule is not under test here: the origin is a corner of the
    board, and the scenes stay clear of it.
    """
    K = np.asarray(K, dtype=np.float64)
    xyz1 = board(pitch)
    X = xyz1.astype(np.float64)
    centre = np.array([(BOARD_COLS - 1) * pitch / 2.0, (BOARD_ROWS - 1) * pitch / 2.0, 0.0])
    Rs, ts, uvs = [], [], []
    for f in range(frames):
        R = random_tilt(rng) @ np.asarray(base_rotations[f % len(base_rotations)], dtype=np.float64)
        target = np.array([rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1), rng.uniform(0.8, 1.5)]) * distance
        t = target - R @ centre
        P = X @ R.T + t
        assert np.all(P[:, 2] > 0.0) and t[2] > 0.0, "planted_scene: the board or the world origin is behind the camera"
        p = P @ K.T
        uv = p[:, :2] / p[:, 2:3] + noise * rng.uniform(-1.0, 1.0, size=(len(X), 2))
        Rs.append(R), ts.append(t), uvs.append(uv.astype(np.float32))
    n = len(xyz1)
    return dict(off=np.arange(frames + 1, dtype=np.int64) * n, uv=np.concatenate(uvs), xyz=np.tile(xyz1, (frames, 1)),
                K=K, R=np.array(Rs), t=np.array(ts), distance=float(distance))


def frame(scene, f):
    """(xyz, uv) of frame f."""
    a, b = int(scene["off"][f]), int(scene["off"][f + 1])
    return scene["xyz"][a:b], scene["uv"][a:b]


def golden_planted_problem():
    """The 12-frame planted problem of tests/golden/zhang_parent.npz: millimetres, fx != fy, all four base rotations."""
    pitch, distance = UNITS["millimetres"]
    return planted_scene(np.random.default_rng(2024), LARGE_K, ALL_BASES, 12, pitch, distance, 0.3)


# ---------------------------------------------------------------------------------------------------------------------
# homography
# ---------------------------------------------------------------------------------------------------------------------
def dlt_rows(xyz, uv):
    """The 2n x 9 DLT rows of geometry.cpp:79-97 as float64, the products of two coordinates taken in float32 as the
    reference, the oracle and the kernel take them (p1 = world x, y; p2 = pixel)."""
    xyz, uv = np.asarray(xyz, dtype=np.float32), np.asarray(uv, dtype=np.float32)
    x1, y1, x2, y2 = xyz[:, 0], xyz[:, 1], uv[:, 0], uv[:, 1]
    n = len(x1)
    A = np.zeros((2 * n, 9), dtype=np.float64)
    one = np.float32(1.0)
    A[0::2, 3], A[0::2, 4], A[0::2, 5] = -x1, -y1, -one
    A[0::2, 6], A[0::2, 7], A[0::2, 8] = (x1 * y2).astype(np.float32), (y1 * y2).astype(np.float32), y2
    A[1::2, 0], A[1::2, 1], A[1::2, 2] = x1, y1, one
    A[1::2, 6], A[1::2, 7], A[1::2, 8] = (-x1 * x2).astype(np.float32), (-y1 * x2).astype(np.float32), -x2
    return A


def _as_integers(A):
    """Finite doubles A -> (object array of Python ints M, int e) with A = M / 2^e exactly."""
    flat = [float(v).as_integer_ratio() for v in np.asarray(A, dtype=np.float64).ravel()]
    den = max(d for _, d in flat)
    M = np.array([n * (den // d) for n, d in flat], dtype=object).reshape(np.shape(A))
    return M, den


def exact_gram(A):
    """A^T A of a matrix of doubles, exactly: -> (G, S), k x k object arrays of Fraction with G[i][j] = sum_r A[r][i] A[r][j]
    and S[i][j] = sum_r |A[r][i]| |A[r][j]| (the scale of any summation-error bound)."""
    M, den = _as_integers(A)
    Mabs = np.array([abs(v) for v in M.ravel()], dtype=object).reshape(M.shape)
    Gi, Si = M.T.dot(M), Mabs.T.dot(Mabs)
    k = M.shape[1]
    G, S = np.empty((k, k), dtype=object), np.empty((k, k), dtype=object)
    for i in range(k):
        for j in range(k):
            G[i, j], S[i, j] = Fraction(int(Gi[i, j]), den * den), Fraction(int(Si[i, j]), den * den)
    return G, S


def to_double(G):
    """Object array of Fraction -> float64, every entry correctly rounded."""
    return np.array([float(v) for v in np.asarray(G, dtype=object).ravel()], dtype=np.float64).reshape(np.shape(G))


def _mpf(v):
    if isinstance(v, Fraction):
        return mpf(v.numerator) / mpf(v.denominator)
    return mpf(float(v)) if not isinstance(v, mpf) else v


def to_mp(A):
    A = np.asarray(A, dtype=object)
    return mp.matrix([[_mpf(A[i, j]) for j in range(A.shape[1])] for i in range(A.shape[0])])


def smallest_eigvec_mp(A):
    """Unit eigenvector (list of mpf) of the smallest eigenvalue of a symmetric matrix (doubles, Fractions or mpf), mp.eigsy at
    50 digits; sign: the largest component positive."""
    M = A if isinstance(A, mp.matrix) else to_mp(A)
    E, Q = mp.eigsy(M)
    k = min(range(len(E)), key=lambda i: E[i])
    x = [Q[i, k] for i in range(M.rows)]
    nrm = mp.sqrt(sum(v * v for v in x))
    big = max(x, key=abs)
    s = -1 if big < 0 else 1
    return [s * v / nrm for v in x]


def sine_to(x, ref):
    """Sine of the angle between a vector of doubles and a reference of mpf (50 digits: no cancellation to speak of)."""
    xm = [mpf(float(v)) for v in x]
    nx = mp.sqrt(sum(v * v for v in xm))
    nr = mp.sqrt(sum(v * v for v in ref))
    c = sum(a * b for a, b in zip(xm, ref)) / (nx * nr)
    d = [a / nx - (1 if c >= 0 else -1) * b / nr for a, b in zip(xm, ref)]   # |d| = 2 sin(angle / 2)
    h = mp.sqrt(sum(v * v for v in d)) / 2
    return float(2 * h * mp.sqrt(1 - h * h))


def homography_mp(xyz, uv):
    """The reference homography of one frame: 9 mpf, unit norm (sign: largest component positive)."""
    G, _ = exact_gram(dlt_rows(xyz, uv))
    return smallest_eigvec_mp(G)


def homography_f32(xyz, uv):
    return np.array([float(v) for v in homography_mp(xyz, uv)], dtype=np.float64).astype(np.float32).reshape(3, 3)


# ---------------------------------------------------------------------------------------------------------------------
# K
# ---------------------------------------------------------------------------------------------------------------------
def _vij(H, i, j):
    return [H[0][i] * H[0][j], H[0][i] * H[1][j] + H[1][i] * H[0][j], H[1][i] * H[1][j],
            H[2][i] * H[0][j] + H[0][i] * H[2][j], H[2][i] * H[1][j] + H[1][i] * H[2][j], H[2][i] * H[2][j]]


def k_system_mp(Hs):
    """The 6 x 6 normal matrix V^T V of Zhang's V b = 0 (geometry.cpp:123-152, the zero-skew row weighted with the number of
    frames included) from float32 homographies, as an mp.matrix."""
    Hs = np.asarray(Hs, dtype=np.float32).reshape(-1, 3, 3)
    A = mp.zeros(6, 6)
    for Hf in Hs:
        H = [[mpf(float(Hf[r, c])) for c in range(3)] for r in range(3)]
        a, b0, b1 = _vij(H, 0, 1), _vij(H, 0, 0), _vij(H, 1, 1)
        r2 = [x - y for x, y in zip(b0, b1)]
        for i in range(6):
            for j in range(i, 6):
                A[i, j] += a[i] * a[j] + r2[i] * r2[j]
    A[1, 1] += mpf(len(Hs)) ** 2
    for i in range(6):
        for j in range(i):
            A[i, j] = A[j, i]
    return A


def mp_to_double(M):
    return np.array([[float(M[i, j]) for j in range(M.cols)] for i in range(M.rows)], dtype=np.float64)


def k_from_b(Hs):
    """(alpha, beta, u0, v0) as mpf: Zhang's closed form (skew forced to zero, geometry.cpp:157-171) evaluated from a 50-digit
    eigenvector of the 6 x 6 system of the float32 homographies Hs."""
    B11, B12, B22, B13, B23, B33 = smallest_eigvec_mp(k_system_mp(Hs))
    den = B11 * B22 - B12 * B12
    v0 = (B12 * B13 - B11 * B23) / den
    lam = B33 - (B13 * B13 + v0 * (B12 * B13 - B11 * B23)) / B11
    alpha, beta = mp.sqrt(lam / B11), mp.sqrt(lam * B11 / den)
    u0 = -B13 * alpha * alpha / lam
    return alpha, beta, u0, v0


# ---------------------------------------------------------------------------------------------------------------------
# poses
# ---------------------------------------------------------------------------------------------------------------------
BRANCHES = ("trace", "x", "y", "z")


def quat_eigen_mp(R):
    """Eigen's Quaternion(Matrix3) rule on a 3 x 3 of mpf -> ([w, x, y, z], the branch it took)."""
    tr = R[0][0] + R[1][1] + R[2][2]
    q = [mpf(0)] * 4
    if tr > 0:
        s = mp.sqrt(tr + 1)
        q[0] = s / 2
        s = mpf(1) / (2 * s)
        q[1], q[2], q[3] = (R[2][1] - R[1][2]) * s, (R[0][2] - R[2][0]) * s, (R[1][0] - R[0][1]) * s
        return q, "trace"
    i = 0
    if R[1][1] > R[0][0]:
        i = 1
    if R[2][2] > R[i][i]:
        i = 2
    j = (i + 1) % 3
    k = (j + 1) % 3
    s = mp.sqrt(R[i][i] - R[j][j] - R[k][k] + 1)
    q[1 + i] = s / 2
    s = mpf(1) / (2 * s)
    q[0] = (R[k][j] - R[j][k]) * s
    q[1 + j] = (R[j][i] + R[i][j]) * s
    q[1 + k] = (R[k][i] + R[i][k]) * s
    return q, BRANCHES[1 + i]


def _pose_of(Ki, H):
    h = [[sum(Ki[r, k] * H[k][c] for k in range(3)) for c in range(3)] for r in range(3)]   # K^-1 H
    l = 1 / mp.sqrt(sum(h[r][0] ** 2 for r in range(3)))
    r0, r1, t = [l * h[r][0] for r in range(3)], [l * h[r][1] for r in range(3)], [l * h[r][2] for r in range(3)]
    r2 = [r0[1] * r1[2] - r0[2] * r1[1], r0[2] * r1[0] - r0[0] * r1[2], r0[0] * r1[1] - r0[1] * r1[0]]
    R = mp.matrix([[r0[r], r1[r], r2[r]] for r in range(3)])
    U, _, V = mp.svd_r(R)                      # R = U diag(S) V: the polar factor (FixRotationMatrix) is U V
    P = U * V
    Rp = [[P[r, c] for c in range(3)] for r in range(3)]
    q, branch = quat_eigen_mp(Rp)
    return dict(R=np.array([[float(v) for v in row] for row in Rp]), t=np.array([float(v) for v in t]),
                q=np.array([float(v) for v in q]), branch=branch)


def pose_from_h(H, K):
    """RecoverExtrinsics (geometry.cpp:179-203) and the quaternion of calibrator.cpp:63 at 50 digits, from a float32 homography
    and a float32 K: -> (pose of H, pose of -H), each a dict R (the exact polar factor), t, q (w x y z), branch (which of
    Eigen's four matrix-to-quaternion branches the exact rotation takes). Which of the two is the camera's is the caller's
    to say (the port: the one with t_z >= 0)."""
    Km = mp.matrix([[mpf(float(v)) for v in row] for row in np.asarray(K, dtype=np.float32).reshape(3, 3)])
    Ki = Km ** -1
    Hm = [[mpf(float(v)) for v in row] for row in np.asarray(H, dtype=np.float32).reshape(3, 3)]
    Hn = [[-v for v in row] for row in Hm]
    return _pose_of(Ki, Hm), _pose_of(Ki, Hn)


def front_pose(H, K):
    """The pose of the pair pose_from_h returns that has t_z > 0."""
    a, b = pose_from_h(H, K)
    assert (a["t"][2] > 0) != (b["t"][2] > 0)
    return a if a["t"][2] > 0 else b


def h_from_pose(K, R, t, s=1.0):
    """s K [r0 r1 t] in float64, rounded to float32."""
    M = np.column_stack([R[:, 0], R[:, 1], t])
    return (s * (np.asarray(K, dtype=np.float64) @ M)).astype(np.float32)


def _rot_with_trace(tr, axis):
    """Rotation about `axis` whose trace is tr = 1 + 2 cos(angle)."""
    return rodrigues(axis, math.acos((tr - 1.0) / 2.0))


POSE_SCALES = (1.0, -1.0, 1e-3, -1e-3, 1e3, -1e3)


@functools.lru_cache(maxsize=None)
def pose_stage_rotations():
    """[(label, R)]: the rotations of the pose-stage test. Twelve random tilts of each base rotation (the census: identity ->
    trace branch, 180 degrees about x / y / z -> that pivot), the exact half turns (trace -1, w = 0), 120 degrees about
    (1,1,1)/sqrt(3) (trace 0, all three diagonal entries tie), and rotations a few float32 units to either side of trace = 0
    and of R00 = R11."""
    rng = np.random.default_rng(77)
    out = []
    for name, B in BASE_ROTATIONS.items():
        for i in range(12):
            out.append((f"{name}/{i}", random_tilt(rng) @ B))
    for name in ("x180", "y180", "z180"):
        out.append((f"exact {name}", BASE_ROTATIONS[name].copy()))
    out.append(("120 about 111", rodrigues([1, 1, 1], 2.0 * math.pi / 3.0)))
    for k in (-3, -1, 1, 3):
        # trace = k float32 units of 1 away from 0, about a skew axis (no two diagonal entries equal)
        out.append((f"trace 0 {k:+d} ulp", _rot_with_trace(k * 2.0 ** -23, [0.3, -0.5, 0.8])))
        # about (1,1,c): R00 = R11 exactly for every angle; tipping the axis by a few units of 2^-23 splits them either way
        out.append((f"R00 = R11 {k:+d} ulp", rodrigues([1.0 + k * 2.0 ** -22, 1.0, 0.2], math.radians(170.0))))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def pose_stage_inputs():
    """[(label, K float32 3x3, H float32 3x3, distance)]: H = s K [r0 r1 t] for every rotation of pose_stage_rotations and
    every s of POSE_SCALES (so each pose comes once as H and once as -H), cameras and units taking turns, t with t_z > 0."""
    rng = np.random.default_rng(78)
    cams, units = list(CAMERAS.values()), list(UNITS.values())
    out = []
    for n, (label, R) in enumerate(pose_stage_rotations()):
        K = cams[n % 3]
        distance = units[(n // 3) % 2][1]
        t = np.array([rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1), rng.uniform(0.8, 1.5)]) * distance
        for s in POSE_SCALES:
            out.append((f"{label} s={s:g}", K.astype(np.float32), h_from_pose(K, R, t, s), distance))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def skewed_inputs():
    """[(label, K, H, distance)] whose recovered columns are not orthonormal: |r1| / |r0| from 0.9 to 1.1 and an angle between
    them of 85 to 95 degrees. FixRotationMatrix must return the polar factor of [r0 r1 r0 x r1]."""
    rng = np.random.default_rng(79)
    cams = list(CAMERAS.values())
    out = []
    n = 0
    for ratio in (0.9, 0.97, 1.0, 1.04, 1.1):
        for deg in (85.0, 88.0, 90.0, 93.0, 95.0):
            B = list(BASE_ROTATIONS.values())[n % 4]
            R = random_tilt(rng) @ B
            a = math.radians(deg)
            c0 = R[:, 0]
            c1 = ratio * (math.cos(a) * R[:, 0] + math.sin(a) * R[:, 1])
            t = np.array([rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1), rng.uniform(0.8, 1.5)]) * 0.5
            K = cams[n % 3]
            M = np.column_stack([c0, c1, t])
            out.append((f"ratio {ratio} angle {deg}", K.astype(np.float32), (K @ M).astype(np.float32), 0.5))
            n += 1
    return tuple(out)


@functools.lru_cache(maxsize=None)
def pose_references(which="census"):
    """front_pose of every input of pose_stage_inputs ("census") or skewed_inputs ("skewed"), computed once."""
    inputs = pose_stage_inputs() if which == "census" else skewed_inputs()
    return tuple(front_pose(H, K) for _, K, H, _ in inputs)


# ---------------------------------------------------------------------------------------------------------------------
# shared, computed once
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def noise_free_scene(camera, units, frames=12):
    pitch, distance = UNITS[units]
    seed = 100 + 10 * list(CAMERAS).index(camera) + list(UNITS).index(units)
    return planted_scene(np.random.default_rng(seed), CAMERAS[camera], ALL_BASES, frames, pitch, distance, 0.0)


@functools.lru_cache(maxsize=None)
def noisy_scene(camera, units, frames=12):
    pitch, distance = UNITS[units]
    seed = 200 + 10 * list(CAMERAS).index(camera) + list(UNITS).index(units)
    return planted_scene(np.random.default_rng(seed), CAMERAS[camera], ALL_BASES, frames, pitch, distance, 0.3)


@functools.lru_cache(maxsize=None)
def many_homographies():
    """300 reference homographies (float32, [300,3,3]) of one noise-free planted scene of the fixture camera: the K stage's input
    (F = 3, 4, 5, 12, 257, 300 are its prefixes)."""
    pitch, distance = UNITS["metres"]
    sc = planted_scene(np.random.default_rng(300), FIXTURE_K, ALL_BASES, 300, pitch, distance, 0.0)
    return np.array([homography_f32(*frame(sc, f)) for f in range(300)])
