"""CPU references of the fisheye (Kannala-Brandt) camera model tests (tests/test_fisheye_cpu.py, tests/test_gpu_intr_fisheye.py,
tests/test_gpu_pycalibrator_fisheye.py). Shares no code with the kernels. A helper module, not a test.

  1. The model in mpmath at 50 digits: theta = atan2(rho, zc), theta_d = theta (1 + k1 theta^2 + .. + k4 theta^8),
     u = fx theta_d xc / rho + px, v alike; the Jacobian by sympy differentiation through QuaternionManifold::Plus linearised at
     0, as tests/test_oracle_model.py does for the pinhole model. On the axis itself (rho == 0, a 0 / 0 of the formula) the
     point is moved by 1e-30 of a unit along x: value and derivatives are continuous there, the shift is 20 digits below
     anything the tests resolve. Gram blocks are summed in np.longdouble, as in tests/huber_ref.py.
  2. A dense-normal-equations numpy LM for the single-camera problem: oracle.cpp's run_lm restated (Jacobi scaling computed
     once, the LM diagonal clamped, Ceres' non-monotonic step evaluator with its window of 5, the radius rules, Ceres'
     gradient max-norm || x - Plus(x, -g) ||, the parameter / function tolerance tests before acceptance, max iterations before
     the gradient tolerance) with a pluggable observation model and Ceres' HuberLoss Corrector. It runs in the dtype it is
     given: float64 and np.longdouble. The pinhole model plugged in reproduces pyoracle.intrinsics_solve
     (tests/test_fisheye_cpu.py), which validates the restatement independently of the fisheye model.
  3. Data: planar boards projected with the mpmath model, optional Gaussian noise from a fixed seed, rounded to float32.
Everything is computed once per process; callers must not modify what they get."""
import functools

import mpmath as mp
import numpy as np
import sympy as sp

from oracle import pyoracle as po
from tests.rig_inner_ref import pose_grad_max, quat_plus

DBL_MAX = np.finfo(np.float64).max
RAGGED = (5, 63, 64, 65, 257, 300)
K8_HELD = 1 << 8          # slot 8 is unused by the model: always held
TERM = po.TERMINATION


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the model at 50 digits
# ---------------------------------------------------------------------------------------------------------------------------
def _rot(q):
    w, x, y, z = q
    n = sp.sqrt(w * w + x * x + y * y + z * z)
    w, x, y, z = w / n, x / n, y / n, z / n
    return sp.Matrix([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                      [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                      [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _qmul(a, b):
    return [a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
            a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
            a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1],
            a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]]


@functools.lru_cache(maxsize=None)
def _symbolic():
    """(residual-and-Jacobian function, camera-point function), both on mpmath numbers. Arguments: fx fy px py k1 k2 k3 k4,
    q (4, any norm), t (3), X (3), uv (2). J: 2 x 14 over [fx fy px py k1 k2 k3 k4 | rot tangent (3) | t (3)]."""
    k = sp.symbols("fx fy px py k1 k2 k3 k4")
    q = sp.symbols("qw qx qy qz")
    t = sp.symbols("tx ty tz")
    X = sp.symbols("X Y Z")
    uv = sp.symbols("u v")
    d = sp.symbols("d1 d2 d3")
    fx, fy, px, py, k1, k2, k3, k4 = k
    xc = _rot(_qmul([sp.Integer(1), d[0], d[1], d[2]], list(q))) * sp.Matrix(X) + sp.Matrix(t)   # Plus linearised at delta = 0
    rho = sp.sqrt(xc[0] ** 2 + xc[1] ** 2)
    th = sp.atan2(rho, xc[2])
    thd = th * (1 + k1 * th**2 + k2 * th**4 + k3 * th**6 + k4 * th**8)
    res = sp.Matrix([fx * thd * xc[0] / rho + px - uv[0], fy * thd * xc[1] / rho + py - uv[1]])
    zero = {d[0]: 0, d[1]: 0, d[2]: 0}
    J = res.jacobian(list(k) + list(d) + list(t)).subs(zero)
    args = list(k) + list(q) + list(t) + list(X) + list(uv)
    cam = (_rot(list(q)) * sp.Matrix(X) + sp.Matrix(t))
    return sp.lambdify(args, [res.subs(zero), J], modules="mpmath", cse=True), sp.lambdify(args, list(cam), modules="mpmath")


def mp_residual(intr, q, t, X, uv):
    """(r [2], J [2][15]) of one observation as float64, evaluated at 50 digits from the float64 / float32 inputs as they are.
    intr: 9 slots (slot 8 ignored; its column is zero)."""
    with mp.workdps(50):
        fn, cam = _symbolic()
        a = [mp.mpf(float(v)) for v in list(intr[:8]) + list(q) + list(t) + list(X) + list(uv)]
        c = cam(*a)
        if c[0] == 0 and c[1] == 0:   # the axis itself: the limit (see the module's text)
            a[12] = a[12] + mp.mpf("1e-30")
        r, J = fn(*a)
        out = np.zeros((2, 15))
        for i in range(2):
            for j in range(8):
                out[i, j] = float(J[i, j])
            for j in range(6):
                out[i, 9 + j] = float(J[i, 8 + j])
        return np.array([float(r[0]), float(r[1])]), out


def mp_project(intr, q, t, X):
    """Pixel coordinates [n][2] of the points X [n][3] at 50 digits (returned as float64)."""
    z = np.zeros(2)
    return np.array([mp_residual(intr, q, t, x, z)[0] for x in np.asarray(X)])


def mp_rows(off, uv, xyz, intr, q, t):
    """(r [N][2], J [N][2][15]) of every observation of a problem from the mpmath model."""
    n = int(off[-1])
    r, J = np.zeros((n, 2)), np.zeros((n, 2, 15))
    for f in range(len(off) - 1):
        for i in range(int(off[f]), int(off[f + 1])):
            r[i], J[i] = mp_residual(intr, q[f], t[f], xyz[i], uv[i])
    return r, J


def huber_weights(s, a):
    """(rho, sqrt(rho')) of ceres::HuberLoss(a) at s = |r|^2, elementwise in s's dtype (a <= 0 or inf: no tail)."""
    one = s.dtype.type(1)
    if not a > 0 or np.isinf(a):
        return s.copy(), np.ones_like(s)
    al = s.dtype.type(a)
    tail = s > al * al
    root = np.sqrt(np.where(tail, s, one))
    return np.where(tail, 2 * al * root - al * al, s), np.where(tail, np.sqrt(al / root), one)


def blocks_from_rows(off, r, J, a=0.0, const_mask=K8_HELD):
    """(cost, blocks [F][16][16], per-observation cost [N]) in np.longdouble from rows (r, J): [J r]^T [J r] per frame with the
    Huber Corrector's weight on the rows; rows and columns of held coordinates are zero, as the sweep leaves them."""
    F = len(off) - 1
    rl, Jl = r.astype(np.longdouble), J.astype(np.longdouble)
    rho, w = huber_weights((rl**2).sum(axis=1), a)
    rows = np.concatenate([Jl, rl[:, :, None]], axis=2) * w[:, None, None]
    blocks = np.zeros((F, 16, 16), dtype=np.longdouble)
    for f in range(F):
        v = rows[int(off[f]):int(off[f + 1])].reshape(-1, 16)
        blocks[f] = v.T @ v
    held = [j for j in range(9) if const_mask & (1 << j)]
    blocks[:, held, :] = 0
    blocks[:, :, held] = 0
    return float(rho.sum() / 2), blocks.astype(np.float64), (rho / 2).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. observation models in numpy (any float dtype) and the dense LM
# ---------------------------------------------------------------------------------------------------------------------------
def _rotation(q):
    w, x, y, z = q / np.sqrt(q @ q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _pose_columns(J, a, bu, bv):
    """Columns 9..14 of the two rows from b = d r / d (camera point): rotation tangent 2 (a x b) (d x_cam / d delta = -2 [R X]_x),
    translation b."""
    J[:, 0, 9:12] = 2 * np.cross(a, bu)
    J[:, 1, 9:12] = 2 * np.cross(a, bv)
    J[:, 0, 12:15] = bu
    J[:, 1, 12:15] = bv


def fisheye_model(intr, q, t, X, uv):
    """(r [n][2], J [n][2][15]) of one frame's observations, in intr's dtype. Slots fx fy px py k1 k2 k3 k4 -."""
    dt = intr.dtype
    n = len(X)
    a = X.astype(dt) @ _rotation(q).T
    xc, yc, zc = (a + t).T
    rho2 = xc * xc + yc * yc
    rho = np.sqrt(rho2)
    th = np.arctan2(rho, zc)
    on = rho2 > 0
    safe = np.where(on, rho, dt.type(1))
    cx, cy = np.where(on, xc / safe, 0), np.where(on, yc / safe, 0)
    e = np.where(on, th / safe, 1 / zc)
    w = th * th
    fx, fy, px, py, k1, k2, k3, k4 = intr[:8]
    P = 1 + w * (k1 + w * (k2 + w * (k3 + w * k4)))
    Q = 1 + w * (3 * k1 + w * (5 * k2 + w * (7 * k3 + w * 9 * k4)))
    g = e * P
    qz = Q / (rho2 + zc * zc)
    D = qz * zc - g
    xd, yd = th * cx * P, th * cy * P
    r = np.stack([fx * xd + px - uv[:, 0].astype(dt), fy * yd + py - uv[:, 1].astype(dt)], axis=1)
    J = np.zeros((n, 2, 15), dtype=dt)
    J[:, 0, 0], J[:, 0, 2], J[:, 1, 1], J[:, 1, 3] = xd, 1, yd, 1
    for j in range(4):
        J[:, 0, 4 + j] = fx * th * cx * w ** (j + 1)
        J[:, 1, 4 + j] = fy * th * cy * w ** (j + 1)
    dxy = D * cx * cy
    bu = fx * np.stack([g + D * cx * cx, dxy, -qz * xc], axis=1)
    bv = fy * np.stack([dxy, g + D * cy * cy, -qz * yc], axis=1)
    _pose_columns(J, a, bu, bv)
    return r, J


def pinhole_model(intr, q, t, X, uv):
    """The reference's pinhole + radial-tangential model (calibrator.cpp:70-95), slots fx fy px py k1 k2 p1 p2 k3."""
    dt = intr.dtype
    n = len(X)
    a = X.astype(dt) @ _rotation(q).T
    xc, yc, zc = (a + t).T
    iz = 1 / zc
    x, y = xc * iz, yc * iz
    fx, fy, px, py, k1, k2, p1, p2, k3 = intr
    r2 = x * x + y * y
    r4, r6 = r2 * r2, r2 * r2 * r2
    m = 1 + k1 * r2 + k2 * r4 + k3 * r6
    xd = x * m + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * m + 2 * p2 * x * y + p1 * (r2 + 2 * y * y)
    r = np.stack([fx * xd + px - uv[:, 0].astype(dt), fy * yd + py - uv[:, 1].astype(dt)], axis=1)
    J = np.zeros((n, 2, 15), dtype=dt)
    J[:, 0, 0], J[:, 0, 2], J[:, 1, 1], J[:, 1, 3] = xd, 1, yd, 1
    J[:, 0, 4], J[:, 0, 5], J[:, 0, 6], J[:, 0, 7], J[:, 0, 8] = fx * x * r2, fx * x * r4, fx * 2 * x * y, fx * (r2 + 2 * x * x), fx * x * r6
    J[:, 1, 4], J[:, 1, 5], J[:, 1, 6], J[:, 1, 7], J[:, 1, 8] = fy * y * r2, fy * y * r4, fy * (r2 + 2 * y * y), fy * 2 * x * y, fy * y * r6
    mp_ = k1 + 2 * k2 * r2 + 3 * k3 * r4
    dxx = m + 2 * mp_ * x * x + 2 * p1 * y + 6 * p2 * x
    dxy = 2 * mp_ * x * y + 2 * p1 * x + 2 * p2 * y
    dyy = m + 2 * mp_ * y * y + 2 * p2 * x + 6 * p1 * y
    bu = (fx * iz)[:, None] * np.stack([dxx, dxy, -(dxx * x + dxy * y)], axis=1)
    bv = (fy * iz)[:, None] * np.stack([dxy, dyy, -(dxy * x + dyy * y)], axis=1)
    _pose_columns(J, a, bu, bv)
    return r, J


def _cholesky_solve(A, b):
    """x with A x = b by a Cholesky factorisation in A's dtype; None when A is not positive definite."""
    n = len(b)
    L = np.zeros_like(A)
    for j in range(n):
        d = A[j, j] - L[j, :j] @ L[j, :j]
        if not d > 0 or not np.isfinite(d):
            return None
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    y = np.zeros_like(b)
    for i in range(n):
        y[i] = (b[i] - L[i, :i] @ y[:i]) / L[i, i]
    x = np.zeros_like(b)
    for i in range(n - 1, -1, -1):
        x[i] = (y[i] - L[i + 1:, i] @ x[i + 1:]) / L[i, i]
    return x


class Problem:
    """off / uv / xyz of a single-camera problem with an observation model and a Huber threshold (0: none)."""

    def __init__(self, model, off, uv, xyz, huber_a=0.0, const_mask=0):
        self.model, self.off = model, np.asarray(off, dtype=np.int64)
        self.uv, self.xyz = np.asarray(uv, dtype=np.float32).reshape(-1, 2), np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
        self.F, self.a, self.mask = len(self.off) - 1, float(huber_a), int(const_mask)

    def rows(self, intr, q, t):
        """Per frame (r [n][2], J [n][2][15]), rho [n], weight [n]."""
        out = []
        for f in range(self.F):
            s = slice(int(self.off[f]), int(self.off[f + 1]))
            r, J = self.model(intr, q[f], t[f], self.xyz[s], self.uv[s])
            rho, w = huber_weights((r * r).sum(axis=1), self.a)
            out.append((r, J, rho, w))
        return out

    def cost(self, intr, q, t):
        c = intr.dtype.type(0)
        for r, J, rho, w in self.rows(intr, q, t):
            c = c + rho.sum() / 2
        return c

    def eval(self, intr, q, t):
        """(cost, gradient [9 + 6 F], Gauss-Newton matrix) over [intrinsics | frame 0 rot t | frame 1 ...]; rows and columns of
        held intrinsics are zero."""
        n = 9 + 6 * self.F
        dt = intr.dtype
        H, g, c = np.zeros((n, n), dtype=dt), np.zeros(n, dtype=dt), dt.type(0)
        for f, (r, J, rho, w) in enumerate(self.rows(intr, q, t)):
            c = c + rho.sum() / 2
            Jw = (J * w[:, None, None]).reshape(-1, 15)
            rw = (r * w[:, None]).reshape(-1)
            idx = np.r_[0:9, 9 + 6 * f:15 + 6 * f]
            H[np.ix_(idx, idx)] += Jw.T @ Jw
            g[idx] += Jw.T @ rw
        for j in range(9):
            if self.mask & (1 << j):
                H[j, :] = 0
                H[:, j] = 0
                g[j] = 0
        return c, g, H


def _opt(o, name):
    return o[name] if isinstance(o, dict) else getattr(o, name)


def lm_solve(problem, intr0, q0, t0, options=None, dtype=np.float64):
    """oracle.cpp's run_lm on the dense normal equations, in `dtype`. Returns (intr, q, t, summary) with summary as
    pyoracle.intrinsics_solve gives it (iterations, termination, initial_cost, final_cost, log)."""
    o = options if options is not None else po.default_options()
    P = problem
    F = P.F
    intr = np.asarray(intr0, dtype=dtype).copy()
    q = np.asarray(q0, dtype=dtype).reshape(F, 4).copy()
    t = np.asarray(t0, dtype=dtype).reshape(F, 3).copy()
    n = 9 + 6 * F
    held = np.array([bool(P.mask & (1 << j)) for j in range(9)] + [False] * (6 * F))
    x_cost, g, H = P.eval(intr, q, t)
    sc = 1 / (1 + np.sqrt(np.diag(H))) if _opt(o, "jacobi_scaling") else np.ones(n, dtype=dtype)
    maxn = _opt(o, "max_consecutive_nonmonotonic_steps") if _opt(o, "use_nonmonotonic_steps") else 0
    ev = dict(minimum=x_cost, current=x_cost, reference=x_cost, candidate=x_cost, acc_ref=dtype(0), acc_cand=dtype(0), nonmono=0)
    radius, decrease, initial_cost = dtype(_opt(o, "initial_radius")), dtype(2), x_cost

    def x_norm(intr, q, t):
        return np.sqrt((intr * intr).sum() + (q * q).sum() + (t * t).sum())

    def grad_max(q, g):
        m = max(abs(g[j]) for j in range(9) if not held[j]) if not held[:9].all() else dtype(0)
        for f in range(F):
            m = max(m, pose_grad_max(q[f], g[9 + 6 * f:15 + 6 * f]))
        return m

    xn, gmax = x_norm(intr, q, t), grad_max(q, g)
    n_invalid = iters = n_success = 0
    term, log = 0, []
    lo, hi = dtype(_opt(o, "min_lm_diagonal")), dtype(_opt(o, "max_lm_diagonal"))
    if gmax <= _opt(o, "gradient_tolerance"):
        term = 1
    while term == 0 and iters < _opt(o, "max_iterations"):
        if radius < _opt(o, "min_radius"):
            term = 5
            break
        iters += 1
        A = H * np.outer(sc, sc)
        A = A + np.diag(np.clip(np.diag(A), lo, hi) / radius)
        b = g * sc
        A[held, :] = 0
        A[:, held] = 0
        A[held, held] = 1
        b[held] = 0
        dy = _cholesky_solve(A, b)
        ok = dy is not None and bool(np.all(np.isfinite(dy)))
        mcc = dtype(0)
        if ok:
            delta = -dy * sc
            mcc = -(delta @ (g + (H @ delta) / 2))
            ok = bool(np.isfinite(mcc)) and mcc > 0
        if not ok:
            n_invalid += 1
            radius = radius / decrease
            decrease = decrease * 2
            log.append(dict(cost=float(x_cost), cost_change=0.0, model_cost_change=float(mcc), relative_decrease=0.0, step_norm=0.0, accepted=0, valid=0))
            if n_invalid >= _opt(o, "max_consecutive_invalid_steps"):
                term = 4
                break
            continue
        n_invalid = 0
        ci = intr + delta[:9]
        cq = np.array([quat_plus(q[f], delta[9 + 6 * f:12 + 6 * f]) for f in range(F)], dtype=dtype)
        ct = t + delta[9:].reshape(F, 6)[:, 3:]
        step_norm = np.sqrt(((ci - intr) ** 2).sum() + ((cq - q) ** 2).sum() + ((ct - t) ** 2).sum())
        cand_cost, gc, Hc = P.eval(ci, cq, ct)
        if not np.isfinite(cand_cost):
            cand_cost = dtype(DBL_MAX)
        cost_change = x_cost - cand_cost
        if step_norm <= _opt(o, "parameter_tolerance") * (xn + _opt(o, "parameter_tolerance")):
            term = 2
            log.append(dict(cost=float(x_cost), cost_change=float(cost_change), model_cost_change=float(mcc), relative_decrease=0.0, step_norm=float(step_norm), accepted=0, valid=1))
            break
        if abs(cost_change) <= _opt(o, "function_tolerance") * x_cost:
            term = 3
            log.append(dict(cost=float(x_cost), cost_change=float(cost_change), model_cost_change=float(mcc), relative_decrease=0.0, step_norm=float(step_norm), accepted=0, valid=1))
            break
        if not cand_cost < DBL_MAX:
            quality = dtype(-DBL_MAX)
        else:
            quality = max((ev["current"] - cand_cost) / mcc, (ev["reference"] - cand_cost) / (ev["acc_ref"] + mcc))
        if quality > _opt(o, "min_relative_decrease"):
            intr, q, t, g, H, x_cost = ci, cq, ct, gc, Hc, cand_cost
            xn, gmax = x_norm(intr, q, t), grad_max(q, g)
            q3 = 2 * quality - 1
            radius = min(dtype(_opt(o, "max_radius")), radius / max(dtype(1) / 3, 1 - q3 * q3 * q3))
            decrease = dtype(2)
            ev["current"] = cand_cost
            ev["acc_cand"] = ev["acc_cand"] + mcc
            ev["acc_ref"] = ev["acc_ref"] + mcc
            if ev["current"] < ev["minimum"]:
                ev["minimum"], ev["nonmono"], ev["candidate"], ev["acc_cand"] = ev["current"], 0, ev["current"], dtype(0)
            else:
                ev["nonmono"] += 1
                if ev["current"] > ev["candidate"]:
                    ev["candidate"], ev["acc_cand"] = ev["current"], dtype(0)
            if ev["nonmono"] == maxn:
                ev["reference"], ev["acc_ref"] = ev["candidate"], ev["acc_cand"]
            n_success += 1
            log.append(dict(cost=float(x_cost), cost_change=float(cost_change), model_cost_change=float(mcc), relative_decrease=float(quality), step_norm=float(step_norm), accepted=1, valid=1))
            if iters < _opt(o, "max_iterations") and gmax <= _opt(o, "gradient_tolerance"):
                term = 1
                break
        else:
            radius = radius / decrease
            decrease = decrease * 2
            log.append(dict(cost=float(x_cost), cost_change=float(cost_change), model_cost_change=float(mcc), relative_decrease=float(quality), step_norm=float(step_norm), accepted=0, valid=1))
    summary = dict(iterations=iters, successful_steps=n_success, termination=TERM[term], initial_cost=float(initial_cost),
                   final_cost=float(x_cost), log=log)
    return intr.astype(np.float64), q.astype(np.float64), t.astype(np.float64), summary


# ---------------------------------------------------------------------------------------------------------------------------
# 3. data
# ---------------------------------------------------------------------------------------------------------------------------
TRUE_INTR = np.array([620.0, 615.0, 805.0, 495.0, -0.035, 0.004, -0.0009, 0.0001, 0.0])
# name: (points per frame, board half-size [m], board distance [m], tilt [rad], noise sigma [px])
SHAPES = {
    "ragged": (list(RAGGED), 0.30, 0.45, 0.35, 0.3),
    "8x40": ([40] * 8, 0.30, 0.45, 0.35, 0.3),
    "3x12": ([12] * 3, 0.30, 0.45, 0.35, 0.3),
    "fov140": ([48] * 6, 0.29, 0.22, 0.30, 0.3),    # a 140 degree field of view: corners out to 70 degrees off the axis
}


def _board(n, half):
    side = int(np.ceil(np.sqrt(n)))
    gx, gy = np.meshgrid(np.linspace(-half, half, side), np.linspace(-half, half, side))
    return np.stack([gx.ravel()[:n], gy.ravel()[:n], np.zeros(n)], axis=1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(name, noise=True):
    """dict(off, uv, xyz, q_true, t_true, intr_true, intr0, q0, t0, theta_max): the shape's fisheye data with its Zhang
    (pinhole) start and k = 0."""
    counts, half, dist, tilt, sigma = SHAPES[name]
    return make_case(counts, half, dist, tilt, sigma if noise else 0.0)


def make_case(counts, half, dist, tilt, sigma, seed=11):
    """The data of case() for any geometry: len(counts) boards of half-size `half` at about `dist`, tilted by up to `tilt`."""
    noise = sigma > 0
    rng = np.random.default_rng(seed)
    F = len(counts)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    uv, xyz, qs, ts = [], [], [], []
    for f in range(F):
        ang = rng.uniform(-tilt, tilt, size=3) * np.array([1.0, 1.0, 0.3])
        qf = quat_plus(np.array([1.0, 0.0, 0.0, 0.0]), ang / 2)
        tf = np.array([rng.uniform(-0.05, 0.05), rng.uniform(-0.05, 0.05), dist * rng.uniform(0.9, 1.2)])
        X = _board(counts[f], half)
        p = mp_project(TRUE_INTR, qf, tf, X)
        if noise:
            p = p + rng.normal(scale=sigma, size=p.shape)
        uv.append(p.astype(np.float32)); xyz.append(X); qs.append(qf); ts.append(tf)
    uv, xyz = np.concatenate(uv), np.concatenate(xyz)
    K, q0, t0 = po.zhang_init(off, uv, xyz)
    intr0 = np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2], 0, 0, 0, 0, 0], dtype=np.float64)
    th = []
    for f in range(F):
        c = xyz[off[f]:off[f + 1]].astype(np.float64) @ _rotation(qs[f]).T + ts[f]
        th.append(np.arctan2(np.hypot(c[:, 0], c[:, 1]), c[:, 2]).max())
    return dict(off=off, uv=uv, xyz=xyz, q_true=np.array(qs), t_true=np.array(ts), intr_true=TRUE_INTR.copy(), intr0=intr0,
                q0=q0.astype(np.float64), t0=t0.astype(np.float64), theta_max=float(max(th)))


def displaced(c, frac=0.10, seed=3):
    """The case with `frac` of the observations displaced by +-U(5, 30) px per coordinate (tests/huber_ref.py's outliers)."""
    rng = np.random.default_rng(seed)
    n = len(c["uv"])
    idx = rng.choice(n, max(1, int(n * frac)), replace=False)
    uv = c["uv"].astype(np.float64)
    uv[idx] += rng.uniform(5.0, 30.0, size=(len(idx), 2)) * rng.choice([-1.0, 1.0], size=(len(idx), 2))
    return dict(c, uv=uv.astype(np.float32))


@functools.lru_cache(maxsize=None)
def reference_solution(name, huber_a=0.0, const_mask=0, min_relative_decrease=None, dirty=False):
    """lm_solve in float64 on the named case from its own start (fisheye model, slot 8 held), once per process."""
    c = case(name)
    if dirty:
        c = displaced(c)
    o = po.default_options() if min_relative_decrease is None else po.default_options(min_relative_decrease=min_relative_decrease)
    P = Problem(fisheye_model, c["off"], c["uv"], c["xyz"], huber_a, const_mask | K8_HELD)
    return lm_solve(P, c["intr0"], c["q0"], c["t0"], o)


def assert_solve_matches(summary, state, ref_summary, ref_state):
    """The intrinsics-path tolerances of DESIGN 2: iterations, termination and the accepted / valid flags equal, logged costs
    1e-9 relative, fx fy px py 1e-9 relative, k1..k4 1e-9 absolute, poses 1e-9."""
    s, so = summary, ref_summary
    assert s["iterations"] == so["iterations"] and s["termination"] == so["termination"], (s["iterations"], s["termination"], so["iterations"], so["termination"])
    assert [l["accepted"] for l in s["log"]] == [l["accepted"] for l in so["log"]]
    assert [l["valid"] for l in s["log"]] == [l["valid"] for l in so["log"]]
    assert np.allclose([l["cost"] for l in s["log"]], [l["cost"] for l in so["log"]], rtol=1e-9, atol=0)
    (ig, qg, tg), (io, qo, to) = state, ref_state
    assert np.allclose(ig[:4], io[:4], rtol=1e-9, atol=0) and np.allclose(ig[4:], io[4:], rtol=0, atol=1e-9), (ig, io)
    assert np.abs(np.reshape(qg, (-1, 4)) - np.reshape(qo, (-1, 4))).max() < 1e-9
    assert np.abs(np.reshape(tg, (-1, 3)) - np.reshape(to, (-1, 3))).max() < 1e-9
