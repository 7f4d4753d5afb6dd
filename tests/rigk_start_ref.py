"""CPU reference of the pixel start of a rig problem with intrinsics (cc_rigk_estimate_start): the inverse of both pixel models
at 50 digits (mpmath), then the start's own reference (tests/rig_start_ref.py) on the points rounded to float32. Shares no code
with the kernel. A helper module, not a test (tests/test_rigk_start_ref_cpu.py, tests/test_gpu_rigk_start.py).

  radial-tangential (slots fx fy px py k1 k2 p1 p2 k3, the map of SURVEY Appendix A): the root on the sheet of the map that
      holds the axis. The distorted point is approached from the axis in RADTAN_STAGES equal stages, each solved by Newton's
      method from the stage before to a residual of 1e-40; the map's (symmetric) Jacobian must stay positive definite at every
      iterate. An iterate on or beyond the fold of the map, or a stage that does not converge: the search from the distorted
      point has no root to reach, NaN, NaN. (Plain Newton from the distorted point itself, at 50 digits, crosses the fold of
      a barrel map and lands on a root of another sheet, on the far side of the axis.)
  fisheye (slots fx fy px py k1 k2 k3 k4 -): theta_d(theta) = theta (1 + k1 theta^2 + .. + k4 theta^8) = |distorted point|. The
      zeros of the slope inside (0, pi/2) -- roots of a quartic in theta^2 -- cut [0, pi/2] into pieces on which theta_d is
      monotone; the root is taken from the first piece whose ends have theta_d - |distorted point| on both sides of zero,
      that is the smallest root in [0, pi/2). None: NaN, NaN. The axis maps to itself. Point = distorted point x
      tan(theta) / theta_d.
  both: a non-finite pixel, a zero or non-finite fx or fy: NaN, NaN.
Pixels may be floats or mpmath numbers (the round-trip test hands over 50-digit pixels: next to a principal point of 800 a
float64 pixel resolves 1e-13 px, which is 2e-7 of a point 1e-9 off the axis)."""
import mpmath as mp
import numpy as np

from tests import rig_start_ref as rs

RADTAN, FISHEYE = 0, 1
DPS = 50
RADTAN_STAGES = 8


def radtan_map(k, x, y):
    """Appendix A's distortion map on normalised coordinates, in whatever arithmetic its arguments carry."""
    k1, k2, p1, p2, k3 = k[4], k[5], k[6], k[7], k[8]
    r2 = x * x + y * y
    m = 1 + r2 * (k1 + r2 * (k2 + r2 * k3))
    return x * m + 2 * p1 * x * y + p2 * (r2 + 2 * x * x), y * m + 2 * p2 * x * y + p1 * (r2 + 2 * y * y)


def radtan_pixel(k, x, y):
    xd, yd = radtan_map(k, x, y)
    return k[0] * xd + k[2], k[1] * yd + k[3]


def fisheye_theta_d(k, th):
    w = th * th
    return th * (1 + w * (k[4] + w * (k[5] + w * (k[6] + w * k[7]))))


def fisheye_pixel(k, x, y):
    """The fisheye projection of the normalised point (x, y, 1) (tests/rigk_fisheye_ref._mp_pixel at the identity pose)."""
    rho = mp.sqrt(x * x + y * y)
    if rho == 0:
        return k[0] * x + k[2], k[1] * y + k[3]
    s = fisheye_theta_d(k, mp.atan(rho)) / rho
    return k[0] * x * s + k[2], k[1] * y * s + k[3]


def _radtan_root(k, xd, yd):
    k1, k2, p1, p2, k3 = k[4], k[5], k[6], k[7], k[8]
    x = y = mp.mpf(0)
    tiny = mp.mpf(10) ** (-40) * (1 + abs(xd) + abs(yd))
    for stage in range(1, RADTAN_STAGES + 1):
        gx, gy = xd * stage / RADTAN_STAGES, yd * stage / RADTAN_STAGES
        for _ in range(60):
            r2 = x * x + y * y
            m = 1 + r2 * (k1 + r2 * (k2 + r2 * k3))
            mpr = k1 + 2 * k2 * r2 + 3 * k3 * r2 * r2
            j00 = m + 2 * mpr * x * x + 2 * p1 * y + 6 * p2 * x
            j01 = 2 * mpr * x * y + 2 * p1 * x + 2 * p2 * y
            j11 = m + 2 * mpr * y * y + 2 * p2 * x + 6 * p1 * y
            det = j00 * j11 - j01 * j01
            if not (det > 0 and j00 + j11 > 0):   # the fold of the map, or beyond it
                return None
            a, b = radtan_map(k, x, y)
            r0, r1 = a - gx, b - gy
            if mp.sqrt(r0 * r0 + r1 * r1) <= tiny:
                break
            x, y = x - (j11 * r0 - j01 * r1) / det, y - (j00 * r1 - j01 * r0) / det
        else:
            return None
    return x, y


def _fisheye_theta(k, td):
    half_pi = mp.pi / 2
    # slope = 1 + 3 k1 w + 5 k2 w^2 + 7 k3 w^3 + 9 k4 w^4, w = theta^2
    coeffs = [9 * k[7], 7 * k[6], 5 * k[5], 3 * k[4], mp.mpf(1)]
    while len(coeffs) > 1 and coeffs[0] == 0:
        coeffs = coeffs[1:]
    cuts = []
    if len(coeffs) > 1:
        for w in mp.polyroots(coeffs, maxsteps=500, extraprec=200):
            if abs(mp.im(w)) <= mp.mpf(10) ** (-30) * (1 + abs(w)) and mp.re(w) > 0:
                th = mp.sqrt(mp.re(w))
                if th < half_pi:
                    cuts.append(th)
    ends = [mp.mpf(0)] + sorted(cuts) + [half_pi]
    f = lambda th: fisheye_theta_d(k, th) - td
    for a, b in zip(ends[:-1], ends[1:]):
        fa, fb = f(a), f(b)
        if fa == 0:
            return a
        if (fa < 0) != (fb < 0) and fb != 0:
            lo, hi = (a, b) if fa < 0 else (b, a)   # f(lo) < 0 < f(hi)
            for _ in range(4 * DPS):
                mid = (lo + hi) / 2
                if f(mid) < 0:
                    lo = mid
                else:
                    hi = mid
            return (lo + hi) / 2
        if fb == 0 and b < half_pi:
            return b
    return None


def unproject(model, intr, uv_px):
    """[n, 2] float64 normalised points of the pixels uv_px [n, 2] under `model` with the nine slots intr; NaN, NaN: no point."""
    pts = np.asarray(uv_px, dtype=object).reshape(-1, 2)
    out = np.full((len(pts), 2), np.nan)
    intr = np.asarray(intr, dtype=np.float64)
    if not (np.isfinite(intr[0]) and np.isfinite(intr[1]) and intr[0] != 0 and intr[1] != 0):
        return out
    with mp.workdps(DPS):
        k = [mp.mpf(float(v)) for v in intr]
        if not all(mp.isfinite(v) for v in k):
            return out
        for i, (u, v) in enumerate(pts):
            u, v = mp.mpf(u) if isinstance(u, mp.mpf) else mp.mpf(float(u)), mp.mpf(v) if isinstance(v, mp.mpf) else mp.mpf(float(v))
            if not (mp.isfinite(u) and mp.isfinite(v)):
                continue
            xd, yd = (u - k[2]) / k[0], (v - k[3]) / k[1]
            if model == FISHEYE:
                td = mp.sqrt(xd * xd + yd * yd)
                if td == 0:
                    out[i] = float(xd), float(yd)
                    continue
                th = _fisheye_theta(k, td)
                if th is not None:
                    s = mp.tan(th) / td
                    out[i] = float(xd * s), float(yd * s)
            else:
                root = _radtan_root(k, xd, yd)
                if root is not None:
                    out[i] = float(root[0]), float(root[1])
    return out


def normalised_points(model, intr, obs_cam, obs_uv_pix):
    """unproject of every observation with its camera's set (intr [9] shared, or [C, 9] per camera), rounded to float32 -- what
    cc_rigk_start_points returns."""
    intr = np.asarray(intr, dtype=np.float64)
    uv = np.asarray(obs_uv_pix, dtype=np.float32).reshape(-1, 2)
    cam = np.asarray(obs_cam, dtype=np.int64)
    out = np.full(uv.shape, np.nan, dtype=np.float32)
    if intr.ndim == 1:
        return unproject(model, intr, uv).astype(np.float32)
    for c in np.unique(cam):
        out[cam == c] = unproject(model, intr[c], uv[cam == c]).astype(np.float32)
    return out


def start_from_pixels(model, intr, n_cams, frame_offsets, obs_cam, obs_world, obs_uv_pix, world_xyz, frozen, **kw):
    """unproject, rounding to float32, rig_start_ref.start (its keywords: the caller's poses, refine, iterations, route).
    Returns start's tuple with the float32 points appended."""
    pts = normalised_points(model, intr, obs_cam, obs_uv_pix)
    return rs.start(n_cams, frame_offsets, obs_cam, obs_world, pts, world_xyz, frozen, **kw) + (pts,)
