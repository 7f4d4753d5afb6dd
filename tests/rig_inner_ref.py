"""numpy restatement of ONE inner pass of Ceres' inner iterations (CoordinateDescentMinimizer) on the rig problem, poses only
(cc_rig_inner_pass, camera_calibrator_amd/csrc/cc_rig_inner.hip). Semantics restated from Ceres 2.x; parity with Ceres is
unpinned.

Blocks are visited group by group -- every camera's t_cr, every camera's q_cr, every frame's t_rw, every frame's q_rw -- and
each is minimised with the others held, over the residuals that touch it, by a trust-region LM with Ceres' default
Solver::Options (monotonic steps, 50 iterations, tolerances 1e-6 / 1e-10 / 1e-8, radius 1e4, LM diagonal in [1e-6, 1e32],
Jacobi scaling taken at the first iteration, 5 invalid steps at most). Residuals and 2 x 12 tangent Jacobians come from
pyoracle.rig_residual (columns: camera rotation, camera translation, frame rotation, frame translation); the Huber loss is
applied with Ceres' Corrector (rho'' <= 0: residual and Jacobian scaled by sqrt(rho')). The step solves the 3 x 3 normal
equations by Cholesky, as the kernels do (Ceres uses DENSE_QR: the same step up to rounding). A helper module, not a test."""
import numpy as np

from oracle import pyoracle as po

DBL_MAX = np.finfo(np.float64).max
OPTS = dict(max_iterations=50, function_tolerance=1e-6, gradient_tolerance=1e-10, parameter_tolerance=1e-8,
            initial_radius=1e4, max_radius=1e16, min_radius=1e-32, min_relative_decrease=1e-3, min_lm_diagonal=1e-6,
            max_lm_diagonal=1e32, max_consecutive_invalid_steps=5)
GROUPS = ("t_cr", "q_cr", "t_rw", "q_rw")
_COLS = {"q_cr": slice(0, 3), "t_cr": slice(3, 6), "q_rw": slice(6, 9), "t_rw": slice(9, 12)}

# terminations (cc_solver.h)
NO_CONVERGENCE, GRADIENT, PARAMETER, FUNCTION, INVALID_STEPS, MIN_RADIUS = 0, 1, 2, 3, 4, 5


def quat_plus(x, d):
    """ceres::QuaternionManifold::Plus: [cos |d|, sin |d| / |d| d] * x."""
    n = np.sqrt(d @ d)
    if n == 0.0:
        return x.copy()
    a0, s = np.cos(n), np.sin(n) / n
    a1, a2, a3 = s * d
    return np.array([a0 * x[0] - a1 * x[1] - a2 * x[2] - a3 * x[3],
                     a0 * x[1] + a1 * x[0] + a2 * x[3] - a3 * x[2],
                     a0 * x[2] - a1 * x[3] + a2 * x[0] + a3 * x[1],
                     a0 * x[3] + a1 * x[2] - a2 * x[1] + a3 * x[0]])


def quat_grad_max(q, g):
    """|| q - Plus(q, -g) ||_inf without the cancellation (the kernels' pose_grad_proj_max rule: tangent max-norm for |g| >= 1/4)."""
    n2 = g @ g
    if not n2 < 0.0625:
        return np.abs(g).max()
    c1 = n2 * (1 / 2 + n2 * (-1 / 24 + n2 * (1 / 720 + n2 * (-1 / 40320 + n2 * (1 / 3628800 + n2 * (-1 / 479001600 + n2 * (
        1 / 87178291200.0 + n2 * (-1 / 20922789888000.0))))))))
    s = 1.0 + n2 * (-1 / 6 + n2 * (1 / 120 + n2 * (-1 / 5040 + n2 * (1 / 362880 + n2 * (-1 / 39916800 + n2 * (
        1 / 6227020800.0 + n2 * (-1 / 1307674368000.0 + n2 * (1 / 355687428096000.0))))))))
    w, v = q[0], q[1:]
    dw = c1 * w - s * (g @ v)
    dv = c1 * v + s * (w * g + np.cross(g, v))
    return max(abs(dw), np.abs(dv).max())


class RigData:
    """The rig problem as the caller hands it to cc_rig_create (frame-grouped observations)."""

    def __init__(self, n_cams, frame_offsets, obs_cam, obs_world, obs_uv, world_xyz, cam_frozen, huber_a):
        self.C, self.off = int(n_cams), np.asarray(frame_offsets, dtype=np.int64)
        self.F = len(self.off) - 1
        self.cam = np.asarray(obs_cam, dtype=np.int64)
        self.X = np.asarray(world_xyz, dtype=np.float32).reshape(-1, 3)[np.asarray(obs_world, dtype=np.int64)].astype(np.float64)
        self.uv = np.asarray(obs_uv, dtype=np.float32).reshape(-1, 2).astype(np.float64)
        self.frame = np.repeat(np.arange(self.F), np.diff(self.off))
        self.huber_a = float(huber_a)
        seen = np.zeros(self.C, dtype=bool)
        seen[self.cam] = True
        self.cam_block = seen & (np.asarray(cam_frozen) == 0)        # optimised cameras
        self.frame_block = np.diff(self.off) > 0                      # frames with observations

    def obs_of(self, kind, i):
        return np.nonzero(self.cam == i)[0] if kind.endswith("cr") else np.arange(self.off[i], self.off[i + 1])


def block_eval(d, state, kind, i, x):
    """Cost, tangent gradient and Gram of block (kind, i) at value x, the other blocks from `state`."""
    cq, ct, fq, ft = (a.copy() for a in state)
    {"q_cr": cq, "t_cr": ct, "q_rw": fq, "t_rw": ft}[kind][i] = x
    cols = _COLS[kind]
    cost, g, A = 0.0, np.zeros(3), np.zeros((3, 3))
    a = d.huber_a
    for k in d.obs_of(kind, i):
        c, f = d.cam[k], d.frame[k]
        r, J = po.rig_residual(fq[f], ft[f], cq[c], ct[c], d.X[k], d.uv[k])
        s = r @ r
        if s > a * a:    # ceres::HuberLoss + Corrector (rho'' < 0): scale by sqrt(rho')
            rn = np.sqrt(s)
            rho, sr = 2.0 * a * rn - a * a, np.sqrt(a / rn)
        else:
            rho, sr = s, 1.0
        cost += 0.5 * rho
        Jb, rs = sr * J[:, cols], sr * r
        g += Jb.T @ rs
        A += Jb.T @ Jb
    return cost, g, A


class Ctl:
    """The fields of the LM state machine (cc_common.hpp LmCtl) a monotonic solve uses."""

    def __init__(self, cost, x_norm, o):
        self.x_cost = self.current_cost = self.reference_cost = self.candidate_cost = self.minimum_cost = cost
        self.x_norm, self.radius, self.decrease_factor = x_norm, o["initial_radius"], 2.0
        self.acc_ref = self.acc_cand = 0.0
        self.iter = self.n_success = self.n_invalid = 0
        self.done, self.term = False, NO_CONVERGENCE


def lm_decide(st, o, valid, cand_cost, mcc, step2, xn2_cand):
    """lm_trial + lm_apply (cc_common.hpp) for monotonic steps. Returns True when the candidate was accepted."""
    st.iter += 1
    accepted = False
    valid = valid and mcc > 0.0 and np.isfinite(mcc)
    if not valid:
        st.n_invalid += 1
        st.radius /= st.decrease_factor
        st.decrease_factor *= 2.0
        if st.n_invalid >= o["max_consecutive_invalid_steps"]:
            st.done, st.term = True, INVALID_STEPS
    else:
        st.n_invalid = 0
        step_norm = np.sqrt(step2)
        if not np.isfinite(cand_cost):
            cand_cost = DBL_MAX
        cost_change = st.x_cost - cand_cost
        if step_norm <= o["parameter_tolerance"] * (st.x_norm + o["parameter_tolerance"]):
            st.done, st.term = True, PARAMETER
        elif abs(cost_change) <= o["function_tolerance"] * st.x_cost:
            st.done, st.term = True, FUNCTION
        else:
            if not cand_cost < DBL_MAX:
                quality = -DBL_MAX
            else:
                quality = max((st.current_cost - cand_cost) / mcc, (st.reference_cost - cand_cost) / (st.acc_ref + mcc))
            if quality > o["min_relative_decrease"]:
                accepted = True
                st.x_cost, st.x_norm = cand_cost, np.sqrt(xn2_cand)
                q3 = 2.0 * quality - 1.0
                st.radius = min(o["max_radius"], st.radius / max(1.0 / 3.0, 1.0 - q3 ** 3))
                st.decrease_factor = 2.0
                st.current_cost = cand_cost
                st.acc_cand += mcc
                st.acc_ref += mcc
                if st.current_cost < st.minimum_cost:
                    st.minimum_cost = st.current_cost
                    st.candidate_cost, st.acc_cand = st.current_cost, 0.0
                elif st.current_cost > st.candidate_cost:
                    st.candidate_cost, st.acc_cand = st.current_cost, 0.0
                st.reference_cost, st.acc_ref = st.candidate_cost, st.acc_cand   # (monotonic: every accepted step)
                st.n_success += 1
            else:
                st.radius /= st.decrease_factor
                st.decrease_factor *= 2.0
    if not st.done and st.iter >= o["max_iterations"]:
        st.done, st.term = True, NO_CONVERGENCE
    return accepted


def _gmax(kind, x, g):
    return quat_grad_max(x, g) if kind.startswith("q") else np.abs(g).max()


def mini_solve(d, state, kind, i, o=OPTS):
    """One block's LM with the other blocks held. Returns (x, iterations, termination, gradient max-norm at x)."""
    x = {"q_cr": state[0], "t_cr": state[1], "q_rw": state[2], "t_rw": state[3]}[kind][i].copy()
    cost, g, A = block_eval(d, state, kind, i, x)
    st = Ctl(cost, np.sqrt(x @ x), o)
    sc = 1.0 / (1.0 + np.sqrt(np.diag(A)))
    gmax = _gmax(kind, x, g)
    if gmax <= o["gradient_tolerance"]:
        return x, 0, GRADIENT, gmax
    while True:
        As = A * np.outer(sc, sc)
        gs = g * sc
        M = As + np.diag(np.clip(np.diag(As), o["min_lm_diagonal"], o["max_lm_diagonal"]) / st.radius)
        try:
            L = np.linalg.cholesky(M)
            dy = -np.linalg.solve(L.T, np.linalg.solve(L, gs))
            ok = bool(np.all(np.isfinite(dy)))
        except np.linalg.LinAlgError:
            dy, ok = np.zeros(3), False
        qm = dy @ (gs + 0.5 * (As @ dy))
        delta = dy * sc
        xc = quat_plus(x, delta) if kind.startswith("q") else x + delta
        valid = ok and -qm > 0.0 and np.isfinite(qm)
        cc, gc, Ac = block_eval(d, state, kind, i, xc) if valid else (st.x_cost, None, None)
        if lm_decide(st, o, valid, cc, -qm, (xc - x) @ (xc - x), xc @ xc):
            x, g, A = xc, gc, Ac
            gmax = _gmax(kind, x, g)
            if not st.done:
                if gmax <= o["gradient_tolerance"]:
                    st.done, st.term = True, GRADIENT
                elif st.radius < o["min_radius"]:
                    st.done, st.term = True, MIN_RADIUS
        elif not st.done and st.radius < o["min_radius"]:
            st.done, st.term = True, MIN_RADIUS
        if st.done:
            return x, st.iter, st.term, gmax


def total_cost(d, state):
    cq, ct, fq, ft = state
    a, cost = d.huber_a, 0.0
    for k in range(len(d.cam)):
        c, f = d.cam[k], d.frame[k]
        r, _ = po.rig_residual(fq[f], ft[f], cq[c], ct[c], d.X[k], d.uv[k], want_jacobian=False)
        s = r @ r
        cost += 0.5 * ((2.0 * a * np.sqrt(s) - a * a) if s > a * a else s)
    return cost


def inner_pass(d, cam_q, cam_t, frame_q, frame_t, o=OPTS):
    """One pass from the given state. Returns (cam_q, cam_t, frame_q, frame_t, mini_iterations[4], per-block records):
    records[kind] = list of (block, iterations, termination, gradient max-norm at its end)."""
    state = [np.array(a, dtype=np.float64).copy() for a in (cam_q, cam_t, frame_q, frame_t)]
    where = {"q_cr": 0, "t_cr": 1, "q_rw": 2, "t_rw": 3}
    its, records = [], {}
    for kind in GROUPS:
        blocks = np.nonzero(d.cam_block if kind.endswith("cr") else d.frame_block)[0]
        new, recs = {}, []
        for i in blocks:   # (independent inside a group: every block sees the state at the group's start)
            x, n, term, gmax = mini_solve(d, state, kind, i, o)
            new[i] = x
            recs.append((int(i), n, term, gmax))
        for i, x in new.items():
            state[where[kind]][i] = x
        its.append(max([r[1] for r in recs], default=0))
        records[kind] = recs
    return (*state, its, records)


# ---------------------------------------------------------------------------------------------------------------------------
# The outer rig LM (cc_rig_solve / pyoracle.rig_solve) on dense normal equations, with Ceres' inner iterations as an option
# (TrustRegionMinimizer::DoInnerIterationsIfNeeded, IsStepSuccessful). For problems of up to ~200 unknowns.
# ---------------------------------------------------------------------------------------------------------------------------
RIG_OPTS = dict(OPTS, max_iterations=1000, use_nonmonotonic_steps=1, max_consecutive_nonmonotonic_steps=5)
TERM_NAMES = po.TERMINATION


def pose_grad_max(q, g6):
    """pose_grad_proj_max (cc_common.hpp): Ceres' || x - Plus(x, -g) ||_inf of one pose block [q t] with g = [g_rot g_t]."""
    g6 = np.asarray(g6)
    gt = np.abs(g6[3:]).max()
    if not g6[:3] @ g6[:3] < 0.0625:
        return max(gt, np.abs(g6[:3]).max())
    return max(gt, quat_grad_max(q, g6[:3]))


def _unknowns(d):
    cams = [int(c) for c in np.nonzero(d.cam_block)[0]]
    frames = [int(f) for f in np.nonzero(d.frame_block)[0]]
    return cams, frames


def full_eval(d, state, cams, frames):
    """Total cost, gradient and Gram over the unknowns (optimised cameras, then active frames, 6 tangent columns each)."""
    cq, ct, fq, ft = state
    ci = {c: k for k, c in enumerate(cams)}
    fi = {f: len(cams) + k for k, f in enumerate(frames)}
    n = 6 * (len(cams) + len(frames))
    H, g, cost, a = np.zeros((n, n)), np.zeros(n), 0.0, d.huber_a
    for k in range(len(d.cam)):
        c, f = d.cam[k], d.frame[k]
        r, J = po.rig_residual(fq[f], ft[f], cq[c], ct[c], d.X[k], d.uv[k])
        s = r @ r
        if s > a * a:
            rn = np.sqrt(s)
            rho, sr = 2.0 * a * rn - a * a, np.sqrt(a / rn)
        else:
            rho, sr = s, 1.0
        cost += 0.5 * rho
        Jf = np.zeros((2, n))
        if c in ci:
            Jf[:, 6 * ci[c]:6 * ci[c] + 6] = sr * J[:, 0:6]
        Jf[:, 6 * fi[f]:6 * fi[f] + 6] = sr * J[:, 6:12]
        g += Jf.T @ (sr * r)
        H += Jf.T @ Jf
    return cost, g, H


def _plus(state, cams, frames, delta):
    cq, ct, fq, ft = (a.copy() for a in state)
    for k, c in enumerate(cams):
        cq[c] = quat_plus(state[0][c], delta[6 * k:6 * k + 3])
        ct[c] = state[1][c] + delta[6 * k + 3:6 * k + 6]
    for k, f in enumerate(frames):
        j = 6 * (len(cams) + k)
        fq[f] = quat_plus(state[2][f], delta[j:j + 3])
        ft[f] = state[3][f] + delta[j + 3:j + 6]
    return [cq, ct, fq, ft]


def _ambient(state, cams, frames):
    cq, ct, fq, ft = state
    return np.concatenate([np.concatenate([cq[c], ct[c]]) for c in cams] + [np.concatenate([fq[f], ft[f]]) for f in frames])


def _grad_max(state, cams, frames, g):
    m = 0.0
    for k, c in enumerate(cams):
        m = max(m, pose_grad_max(state[0][c], g[6 * k:6 * k + 6]))
    for k, f in enumerate(frames):
        j = 6 * (len(cams) + k)
        m = max(m, pose_grad_max(state[2][f], g[j:j + 6]))
    return m


def rig_solve(d, cam_q, cam_t, frame_q, frame_t, o=RIG_OPTS, inner=False, inner_tolerance=1e-3):
    """Returns (cam_q, cam_t, frame_q, frame_t, summary): summary has iterations, termination (name), initial_cost, final_cost,
    log (cost, cost_change, model_cost_change, relative_decrease, step_norm, accepted, valid per iteration) and, with inner
    iterations, passes / useful_passes / enabled_at_end / cost_removed (cc_rig_inner_status)."""
    state = [np.array(a, dtype=np.float64).copy() for a in (cam_q, cam_t, frame_q, frame_t)]
    cams, frames = _unknowns(d)
    x_cost, g, H = full_eval(d, state, cams, frames)
    sc = 1.0 / (1.0 + np.sqrt(np.diag(H)))
    maxn = o["max_consecutive_nonmonotonic_steps"] if o["use_nonmonotonic_steps"] else 0
    ev = dict(minimum=x_cost, current=x_cost, reference=x_cost, candidate=x_cost, acc_ref=0.0, acc_cand=0.0, nonmono=0)
    radius, decrease, initial_cost = o["initial_radius"], 2.0, x_cost
    xn = np.linalg.norm(_ambient(state, cams, frames))
    gmax = _grad_max(state, cams, frames, g)
    n_invalid = iters = 0
    term, log = NO_CONVERGENCE, []
    enabled = inner
    stats = dict(passes=0, useful_passes=0, cost_removed=0.0)
    if gmax <= o["gradient_tolerance"]:
        term = GRADIENT
    while term == NO_CONVERGENCE and iters < o["max_iterations"]:
        if radius < o["min_radius"]:
            term = MIN_RADIUS
            break
        iters += 1
        A = H * np.outer(sc, sc)
        A = A + np.diag(np.clip(np.diag(A), o["min_lm_diagonal"], o["max_lm_diagonal"]) / radius)
        try:
            dy = -np.linalg.solve(A, g * sc)
            ok = bool(np.all(np.isfinite(dy)))
        except np.linalg.LinAlgError:
            dy, ok = np.zeros_like(g), False
        delta = dy * sc
        mcc = -(delta @ (g + 0.5 * (H @ delta))) if ok else 0.0
        if not (ok and np.isfinite(mcc) and mcc > 0.0):
            n_invalid += 1
            radius /= decrease
            decrease *= 2.0
            log.append(dict(cost=x_cost, cost_change=0.0, model_cost_change=mcc, relative_decrease=0.0, step_norm=0.0, accepted=0, valid=0))
            if n_invalid >= o["max_consecutive_invalid_steps"]:
                term = INVALID_STEPS
            continue
        n_invalid = 0
        cand = _plus(state, cams, frames, delta)
        cand_cost = total_cost(d, cand)
        if not np.isfinite(cand_cost):
            cand_cost = DBL_MAX
        useful = False
        if enabled and cand_cost < DBL_MAX:    # DoInnerIterationsIfNeeded
            cq, ct, fq, ft, _, _ = inner_pass(d, *cand)
            cand_in = [cq, ct, fq, ft]
            c_in = total_cost(d, cand_in)
            mcc += cand_cost - c_in
            useful = c_in < x_cost
            enabled = 1.0 - c_in / cand_cost > inner_tolerance
            stats["passes"] += 1
            stats["useful_passes"] += int(useful)
            stats["cost_removed"] += cand_cost - c_in
            cand, cand_cost = cand_in, c_in
        step_norm = np.linalg.norm(_ambient(cand, cams, frames) - _ambient(state, cams, frames))
        cost_change = x_cost - cand_cost
        if step_norm <= o["parameter_tolerance"] * (xn + o["parameter_tolerance"]):
            term = PARAMETER
            log.append(dict(cost=x_cost, cost_change=cost_change, model_cost_change=mcc, relative_decrease=0.0, step_norm=step_norm, accepted=0, valid=1))
            break
        if abs(cost_change) <= o["function_tolerance"] * x_cost:
            term = FUNCTION
            log.append(dict(cost=x_cost, cost_change=cost_change, model_cost_change=mcc, relative_decrease=0.0, step_norm=step_norm, accepted=0, valid=1))
            break
        if not cand_cost < DBL_MAX:
            quality = -DBL_MAX
        else:
            quality = max((ev["current"] - cand_cost) / mcc, (ev["reference"] - cand_cost) / (ev["acc_ref"] + mcc))
        if useful or quality > o["min_relative_decrease"]:
            state, x_cost = cand, cand_cost
            x_cost, g, H = full_eval(d, state, cams, frames)
            x_cost = cand_cost
            xn = np.linalg.norm(_ambient(state, cams, frames))
            gmax = _grad_max(state, cams, frames, g)
            q3 = 2.0 * quality - 1.0
            radius = min(o["max_radius"], radius / max(1.0 / 3.0, 1.0 - q3 ** 3))
            decrease = 2.0
            ev["current"] = cand_cost
            ev["acc_cand"] += mcc
            ev["acc_ref"] += mcc
            if ev["current"] < ev["minimum"]:
                ev["minimum"], ev["nonmono"], ev["candidate"], ev["acc_cand"] = ev["current"], 0, ev["current"], 0.0
            else:
                ev["nonmono"] += 1
                if ev["current"] > ev["candidate"]:
                    ev["candidate"], ev["acc_cand"] = ev["current"], 0.0
            if ev["nonmono"] == maxn:
                ev["reference"], ev["acc_ref"] = ev["candidate"], ev["acc_cand"]
            log.append(dict(cost=x_cost, cost_change=cost_change, model_cost_change=mcc, relative_decrease=quality, step_norm=step_norm, accepted=1, valid=1))
            if iters < o["max_iterations"] and gmax <= o["gradient_tolerance"]:
                term = GRADIENT
                break
        else:
            radius /= decrease
            decrease *= 2.0
            log.append(dict(cost=x_cost, cost_change=cost_change, model_cost_change=mcc, relative_decrease=quality, step_norm=step_norm, accepted=0, valid=1))
    summary = dict(iterations=iters, termination=TERM_NAMES[term], initial_cost=initial_cost, final_cost=x_cost, log=log,
                   enabled_at_end=int(enabled), **stats)
    return (*state, summary)
