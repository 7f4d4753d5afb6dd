"""CPU reference of the fisheye focal-length start (cc_intrinsics_estimate_start_fisheye), written in numpy from the method's
description in include/cc_solver.h and DESIGN 4.19, on the per-view reference of the bearing start
(tests/rigk_bearing_ref.view_closed_form / refine_lm). Shares no code with the kernels. A helper module, not a test
(tests/test_intr_start_ref_cpu.py, tests/test_gpu_intr_start.py, scripts/intr_start_fit_study.py).

  extent        centre: the caller's when both coordinates are finite, else the midpoint of the bounding box of the finite pixels;
                r_max: the largest distance of a finite pixel from it (float64 from the float32 pixels)
  candidates    theta_j = theta_lo + j (theta_hi - theta_lo) / (C - 1), f_j = r_max / theta_j (C = 1: theta_lo)
  searched      floor(k F / S), k = 0 .. S - 1; every view when S is 0 or >= F
  bearings      d = uv - c, theta = |d| / f, b = (sin theta d / |d|, cos theta) in float64; the centre pixel is (0, 0, 1)
  pair          one (view, candidate): closed form, `refine_iterations` LM steps on the chord, cost = sum |p / |p| - b|^2
  start         S_j = f_j^2 sum_v cost_{j,v} in index order; a candidate that cannot place a view some candidate places is
                disqualified; the smallest S_j wins, the lowest index on ties; then every view's pose at the winner
  scene         boards round a fisheye lens, as a surround-view camera is calibrated (fisheye_ref.TRUE_INTR)
"""
import functools

import numpy as np

from tests import fisheye_ref as fr
from tests import rig_start_ref as rs
from tests import rigk_bearing_ref as br

INVALID, PLANAR, GENERAL = rs.INVALID, rs.PLANAR, rs.GENERAL
DEFAULTS = dict(centre=None, theta_lo=0.3, theta_hi=3.0, candidates=24, search_views=32, refine_iterations=3)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the steps
# ---------------------------------------------------------------------------------------------------------------------------
def extent(uv, centre=None):
    """(centre [2] float64, r_max) of the float32 pixels uv [n, 2]."""
    uv = np.asarray(uv, dtype=np.float32).reshape(-1, 2)
    ok = np.isfinite(uv[:, 0]) & np.isfinite(uv[:, 1])
    p = uv[ok].astype(np.float64)
    if centre is not None and np.all(np.isfinite(centre)):
        c = np.asarray(centre, dtype=np.float64)
    elif len(p):
        c = 0.5 * (p.min(axis=0) + p.max(axis=0))
    else:
        c = np.full(2, np.nan)
    d = p - c
    r = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    return c, float(r.max()) if len(r) else 0.0


def candidates(r_max, theta_lo=0.3, theta_hi=3.0, C=24):
    j = np.arange(C, dtype=np.float64)
    th = np.full(C, theta_lo) if C == 1 else theta_lo + (j * (theta_hi - theta_lo)) / (C - 1)
    return r_max / th


def searched(F, S):
    return list(range(F)) if S <= 0 or S >= F else [(k * F) // S for k in range(S)]


def bearings(uv, c, f):
    """[n, 3] float64 unit bearings of the float32 pixels through the equidistant lens r = f theta about c."""
    d = np.asarray(uv, dtype=np.float32).reshape(-1, 2).astype(np.float64) - c
    r = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    th = r / f
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(r > 0, np.sin(th) / r, 0.0)
    return np.stack([s * d[:, 0], s * d[:, 1], np.where(r > 0, np.cos(th), 1.0)], axis=1)


def chord_cost(R, t, X, b):
    r = br.residuals(R, t, X, b)
    return float(r @ r)


def pair(X, uv, c, f, refine_iterations=3, route="svd", refine="lm"):
    """(kind, R, t, cost) of one view through one candidate; (INVALID, None, None, 0.0) when it has no pose.
    refine: "lm" (the specified steps) or "converged" (scipy's least_squares on the same chord)."""
    X = np.asarray(X, dtype=np.float64)
    if not (np.isfinite(f) and f > 0 and np.all(np.isfinite(c))):
        return INVALID, None, None, 0.0
    b = bearings(uv, c, f)
    kind, R, t = br.view_closed_form(X, b, route)
    if kind == INVALID:
        return INVALID, None, None, 0.0
    if refine == "converged":
        R, t = br.refine_converged(R, t, X, b)
    elif refine_iterations:
        R, t = br.refine_lm(R, t, X, b, refine_iterations)
    cost = chord_cost(R, t, X, b)
    if not (np.isfinite(cost) and np.all(np.isfinite(t))):
        return INVALID, None, None, 0.0
    return kind, R, t, cost


def pick(f, kinds, costs):
    """(best index or -1, score [C], qualified [C]) from kinds / costs [C][S]."""
    kinds, costs = np.asarray(kinds), np.asarray(costs, dtype=np.float64)
    C, S = kinds.shape
    inv = (kinds == INVALID) | ~np.isfinite(costs)
    all_inv = inv.all(axis=0)
    score, qualified = np.zeros(C), np.zeros(C, dtype=np.int32)
    for j in range(C):
        total = 0.0
        for k in range(S):   # (index order: the sum the kernel makes)
            if not inv[j, k]:
                total += costs[j, k]
        score[j] = f[j] * f[j] * total
        qualified[j] = int(not np.any(inv[j] & ~all_inv) and np.isfinite(score[j]))
    best = -1
    for j in range(C):
        if qualified[j] and (best < 0 or score[j] < score[best]):
            best = j
    return best, score, qualified


def start(off, uv, xyz, centre=None, theta_lo=0.3, theta_hi=3.0, candidates=24, search_views=32, refine_iterations=3, route="svd"):
    """The whole start. Returns a dict: intr [9], q [F, 4], t [F, 3], kind [F], report (the fields of cc_intr_start_report),
    f / score / qualified [C], pairs {(j, k): (kind, R, t, cost)} of the search (k: position in the searched list)."""
    off = np.asarray(off, dtype=np.int64)
    uv = np.asarray(uv, dtype=np.float32).reshape(-1, 2)
    xyz = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
    F = len(off) - 1
    c, r_max = extent(uv, centre)
    f = globals()["candidates"](r_max, theta_lo, theta_hi, candidates)
    views = searched(F, search_views)
    sl = lambda v: slice(int(off[v]), int(off[v + 1]))
    pairs = {(j, k): pair(xyz[sl(v)], uv[sl(v)], c, f[j], refine_iterations, route) for j in range(candidates) for k, v in enumerate(views)}
    kinds = [[pairs[j, k][0] for k in range(len(views))] for j in range(candidates)]
    costs = [[pairs[j, k][3] for k in range(len(views))] for j in range(candidates)]
    best, score, qualified = pick(f, kinds, costs)
    out = dict(f=f, score=score, qualified=qualified, pairs=pairs, searched=views, best=best, centre=c, r_max=r_max)
    if best < 0:
        return out
    q, t, kind = np.tile([1.0, 0.0, 0.0, 0.0], (F, 1)), np.zeros((F, 3)), np.zeros(F, dtype=np.int32)
    where = {v: k for k, v in enumerate(views)}
    for v in range(F):
        rec = pairs[best, where[v]] if v in where else pair(xyz[sl(v)], uv[sl(v)], c, f[best], refine_iterations, route)
        kind[v] = rec[0]
        if rec[0] != INVALID:
            q[v], t[v] = rs.R_to_quat(rec[1]), rec[2]
    out.update(intr=np.array([f[best], f[best], c[0], c[1], 0, 0, 0, 0, 0], dtype=np.float64), q=q, t=t, kind=kind,
               report=dict(centre=(float(c[0]), float(c[1])), r_max=r_max, focal=float(f[best]), best_candidate=best,
                           candidates_qualified=int(qualified.sum()), views=F, views_searched=len(views), views_invalid=int((kind == INVALID).sum())))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# 2. scenes: boards round the lens
# ---------------------------------------------------------------------------------------------------------------------------
def _grid(side, half):
    g = np.linspace(-half, half, side)
    gx, gy = np.meshgrid(g, g)
    return np.stack([gx.ravel(), gy.ravel(), np.zeros(side * side)], axis=1).astype(np.float32)


def _scene(boards, dist, max_dir_deg, seed, sigma):
    """One camera with fisheye_ref.TRUE_INTR. Frame 0's board centre lies on the axis; every other centre lies U(0, max_dir) off
    it at azimuth U(0, 2 pi) and distance dist U(0.9, 1.2). Board frame: z the line of sight, x = normalise(z x (0.3, 0.5, 0.8)),
    y = z x x, then rotated by exp(w), w ~ U(-0.35, 0.35)^3. Pixels: the fisheye projection + N(0, sigma) px, float32."""
    rng = np.random.default_rng(seed)
    intr = fr.TRUE_INTR
    off, uv, xyz, qs, ts, ang = [0], [], [], [], [], []
    for i, X in enumerate(boards):
        a = 0.0 if i == 0 else np.deg2rad(rng.uniform(0.0, max_dir_deg))
        az, d = rng.uniform(0.0, 2 * np.pi), dist * rng.uniform(0.9, 1.2)
        z = np.array([np.sin(a) * np.cos(az), np.sin(a) * np.sin(az), np.cos(a)])
        x = np.cross(z, [0.3, 0.5, 0.8])
        x /= np.linalg.norm(x)
        R = rs._exp(rng.uniform(-0.35, 0.35, 3)) @ np.stack([x, np.cross(z, x), z], axis=1)
        t = d * z
        p = X.astype(np.float64) @ R.T + t
        px = br.fisheye_pixels(intr, p) + sigma * rng.normal(size=(len(X), 2))
        uv.append(px.astype(np.float32)); xyz.append(X); qs.append(rs.R_to_quat(R)); ts.append(t)
        off.append(off[-1] + len(X))
        ang.append(np.degrees(np.arctan2(np.hypot(p[:, 0], p[:, 1]), p[:, 2])))
    ang = np.concatenate(ang)
    intr0 = np.array([intr[0], intr[1], intr[2], intr[3], 0, 0, 0, 0, 0], dtype=np.float64)
    return dict(off=np.array(off, dtype=np.int64), uv=np.concatenate(uv), xyz=np.concatenate(xyz), q_true=np.array(qs), t_true=np.array(ts),
                intr_true=intr.copy(), intr0_true=intr0, max_angle_deg=float(ang.max()), beyond_90=float(np.mean(ang > 90.0)))


@functools.lru_cache(maxsize=None)
def scene(F, side, half, dist, max_dir_deg, seed, sigma=0.3):
    """F boards of side x side float32 points in [-half, half]^2. intr0_true: the true fx fy px py with k = 0 -- with q_true, t_true
    `the generator's poses`, the start the yardstick solves begin from."""
    return _scene([_grid(side, half)] * F, dist, max_dir_deg, seed, sigma)


RAGGED = (4, 9, 25, 64, 65, 144)   # a minimal view, less than a wave, one wave, one more, three passes


@functools.lru_cache(maxsize=None)
def ragged_scene(counts=RAGGED, half=0.3, dist=0.45, max_dir_deg=40.0, seed=1, sigma=0.3):
    """The same with view i holding the first counts[i] points of the smallest square grid that has them."""
    return _scene([fr._board(n, half) for n in counts], dist, max_dir_deg, seed, sigma)


@functools.lru_cache(maxsize=None)
def pairs_scene(half=0.3, dist=0.45, max_dir_deg=40.0, seed=1, sigma=0.3):
    """The ragged counts on RECTANGULAR boards (y scaled by 0.8) plus two general (non-planar) views of 6 and 65 points,
    U(-half, half)^3 about their centre: every shape of view the pair kernel has a path for. Pixel 30 of the 64-point view is
    moved onto a float32 centre, `centre`.
    Rectangular, because a record can only be compared between two implementations where the closed form is defined: the
    homography is scaled by the length of its first column IN THE BOARD'S EIGEN-BASIS, and with a focal length that is off its
    two columns differ in length, so the translation depends on the in-plane basis (0.1 - 0.7 m on these views at theta_lo; the
    rotation does not). A square grid has two equal in-plane eigenvalues: its basis is whatever the eigen-solver returns, Jacobi
    on the device, LAPACK here. With distinct eigenvalues the basis is fixed up to signs, which the length does not see."""
    rng = np.random.default_rng([seed, 99])
    clouds = [rng.uniform(-half, half, (n, 3)).astype(np.float32) for n in (6, 65)]
    boards = [(fr._board(n, half) * np.array([1.0, 0.8, 1.0], dtype=np.float32)).astype(np.float32) for n in RAGGED]
    c = _scene(boards + clouds, dist, max_dir_deg, seed, sigma)
    centre = np.array([805.0, 495.0], dtype=np.float32)
    uv = c["uv"].copy()
    uv[int(c["off"][3]) + 30] = centre
    return dict(c, uv=uv, centre=centre.astype(np.float64))


@functools.lru_cache(maxsize=None)
def scene_start(key, **options):
    """start() on a scene named by its constructor's arguments (("ragged",) + arguments: ragged_scene), once per process."""
    c = ragged_scene(*key[1:]) if key[0] == "ragged" else scene(*key)
    return start(c["off"], c["uv"], c["xyz"], **options)
