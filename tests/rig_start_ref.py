"""Numpy restatement of the rig start (cc_rig_estimate_start), independent of the kernels: written from the method's
description in include/cc_solver.h and DESIGN 4.15, sharing no code with csrc/.

A pose (R, t) maps x_cam = R X + t; a camera's pose is camera_T_rig, a frame's rig_T_world, a view's their product
(x_cam = R_cr (R_rw X + t_rw) + t_cr). Quaternions are (w, x, y, z).

    view_closed_form   stage V: null vectors by np.linalg.svd of the row matrix (route="svd"), or by eigh of its Gram matrix
                       (route="gram": the route the kernel takes; kept as a yardstick for how far the two routes differ)
    refine_lm          stage R as specified: at most `iterations` damped steps
    refine_converged   stage R run to convergence by scipy.optimize.least_squares
    tree               stage T
    mean_pose          the weighted mean of stages C and F
    start              the whole start of a problem in the layout of cc_rig_create
    plant_scene        scenes with exact planted poses: general clouds or boards anywhere in the world, metres or millimetres
"""
import numpy as np

PLANAR_TOL = 1e-3
INVALID, PLANAR, GENERAL = 0, 1, 2


def quat_to_R(q):
    w, x, y, z = np.asarray(q, dtype=np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def R_to_quat(R):
    """Through the symmetric 4 x 4 matrix whose top eigenvector is the quaternion (Bar-Itzhack): no case distinction."""
    K = np.array([[R[0, 0] + R[1, 1] + R[2, 2], R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]],
                  [0, R[0, 0] - R[1, 1] - R[2, 2], R[0, 1] + R[1, 0], R[0, 2] + R[2, 0]],
                  [0, 0, R[1, 1] - R[0, 0] - R[2, 2], R[1, 2] + R[2, 1]],
                  [0, 0, 0, R[2, 2] - R[0, 0] - R[1, 1]]]) / 3.0
    K = K + np.triu(K, 1).T
    q = np.linalg.eigh(K)[1][:, -1]
    return q if q[0] >= 0 else -q


def nearest_rotation(M):
    U, _, Vt = np.linalg.svd(M)
    return U @ Vt


def rot_angle(Ra, Rb):
    # |Ra - Rb|_F = 2 sqrt(2) sin(angle / 2): exact, and keeps small angles (the arccos of the trace loses them below 1e-8)
    return float(2.0 * np.arcsin(min(1.0, np.linalg.norm(Ra - Rb) / (2.0 * np.sqrt(2.0)))))


def _null(A, route):
    if route == "svd":
        return np.linalg.svd(A)[2][-1]
    return np.linalg.eigh(A.T @ A)[1][:, 0]


def classify(X):
    """kind of a view from its world points alone, and centroid, rms radius, eigen-basis (ascending)."""
    X = np.asarray(X, dtype=np.float64)
    n = len(X)
    if n < 4 or not np.all(np.isfinite(X)):
        return INVALID, None, None, None
    c = X.mean(axis=0)
    d = X - c
    s = np.sqrt((d * d).sum() / n)
    if not s > 0:
        return INVALID, None, None, None
    lam, E = np.linalg.eigh(d.T @ d / (n * s * s))
    lam = np.maximum(lam, 0.0)
    if not lam[2] > 0 or np.sqrt(lam[1] / lam[2]) < PLANAR_TOL:
        return INVALID, None, None, None
    kind = PLANAR if np.sqrt(lam[0] / lam[1]) < PLANAR_TOL else GENERAL
    if kind == GENERAL and n < 6:
        return INVALID, None, None, None
    return kind, c, s, E


def view_closed_form(X, uv, route="svd"):
    """(kind, R, t) of one view; R, t None for an invalid view."""
    X, uv = np.asarray(X, dtype=np.float64), np.asarray(uv, dtype=np.float64)
    if not np.all(np.isfinite(uv)):
        return INVALID, None, None
    kind, c, s, E = classify(X)
    if kind == INVALID:
        return INVALID, None, None
    u, v = uv[:, 0], uv[:, 1]
    n = len(X)
    if kind == PLANAR:
        B = np.stack([E[:, 2], E[:, 1], np.cross(E[:, 2], E[:, 1])], axis=1)
        y = (X - c) @ B / s
        Y = np.stack([y[:, 0], y[:, 1], np.ones(n)], axis=1)
        Z = np.zeros((n, 3))
        A = np.concatenate([np.concatenate([Y, Z, -u[:, None] * Y], axis=1), np.concatenate([Z, Y, -v[:, None] * Y], axis=1)])
        H = _null(A, route).reshape(3, 3)
        H = H / np.linalg.norm(H[:, 0])
        if H[2, 2] < 0:
            H = -H
        Rp = nearest_rotation(np.stack([H[:, 0], H[:, 1], np.cross(H[:, 0], H[:, 1])], axis=1))
        tp = H[:, 2]
    else:
        B = np.eye(3)
        y = (X - c) / s
        Y = np.concatenate([y, np.ones((n, 1))], axis=1)
        Z = np.zeros((n, 4))
        A = np.concatenate([np.concatenate([Y, Z, -u[:, None] * Y], axis=1), np.concatenate([Z, Y, -v[:, None] * Y], axis=1)])
        P = _null(A, route).reshape(3, 4)
        P = P / np.cbrt(np.linalg.det(P[:, :3]))
        Rp = nearest_rotation(P[:, :3])
        tp = P[:, 3]
    R = Rp @ B.T
    return kind, R, s * tp - R @ c


def residuals(R, t, X, uv):
    p = np.asarray(X, dtype=np.float64) @ R.T + t
    return (p[:, :2] / p[:, 2:3] - np.asarray(uv, dtype=np.float64)).ravel(), p[:, 2]


def rms2(R, t, X, uv):
    r, _ = residuals(R, t, X, uv)
    return float(r @ r / len(r))


def _exp(w):
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-8:
        return np.eye(3) + K + 0.5 * K @ K
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * K @ K


def _jacobian(R, t, X):
    p = np.asarray(X, dtype=np.float64) @ R.T
    xc = p + t
    iz = 1.0 / xc[:, 2]
    x, y = xc[:, 0] * iz, xc[:, 1] * iz
    n = len(p)
    J = np.zeros((n, 2, 6))
    for i in range(n):
        Bm = np.array([[iz[i], 0, -x[i] * iz[i]], [0, iz[i], -y[i] * iz[i]]])
        px = np.array([[0, -p[i, 2], p[i, 1]], [p[i, 2], 0, -p[i, 0]], [-p[i, 1], p[i, 0], 0]])
        J[i, :, :3] = -Bm @ px
        J[i, :, 3:] = Bm
    return J.reshape(2 * n, 6)


def refine_lm(R, t, X, uv, iterations=10):
    """The specified refinement: update R <- exp(w) R, t <- t + d; damping lambda diag(H) from 1e-4, x 0.1 on acceptance,
    x 10 on rejection; a step is accepted when the cost drops, is finite and every depth stays positive."""
    lam = 1e-4
    r, _ = residuals(R, t, X, uv)
    cost = r @ r
    for _ in range(iterations):
        J = _jacobian(R, t, X)
        H, g = J.T @ J, J.T @ r
        try:
            d = np.linalg.solve(H + lam * np.diag(np.diag(H)), -g)
        except np.linalg.LinAlgError:
            lam *= 10
            continue
        Rn, tn = _exp(d[:3]) @ R, t + d[3:]
        rn, z = residuals(Rn, tn, X, uv)
        cn = rn @ rn
        if np.isfinite(cn) and cn < cost and np.all(z > 0):
            R, t, r, cost, lam = Rn, tn, rn, cn, lam * 0.1
        else:
            lam *= 10
    return R, t


def refine_converged(R, t, X, uv):
    from scipy.optimize import least_squares

    def f(p):
        return residuals(_exp(p[:3]) @ R, t + p[3:], X, uv)[0]
    s = least_squares(f, np.zeros(6), method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=2000)
    return _exp(s.x[:3]) @ R, t + s.x[3:]


def tree(covis, frozen):
    """(root, root_at_identity, parent[C], placed[C], order) from the table of co-visible valid views."""
    covis = np.asarray(covis)
    C = len(covis)
    frozen = np.asarray(frozen, dtype=bool)
    nv = np.diag(covis)
    cand = [c for c in range(C) if frozen[c] and nv[c] > 0] or [c for c in range(C) if nv[c] > 0]
    parent, placed, order = [-1] * C, [bool(f) for f in frozen], []
    if not cand:
        return -1, False, parent, placed, order
    root = max(cand, key=lambda c: (nv[c], -c))
    placed[root] = True
    while True:
        pairs = [(covis[u, p], -u, -p) for u in range(C) if not placed[u] for p in range(C) if placed[p] and covis[u, p] > 0]
        if not pairs:
            break
        _, u, p = max(pairs)
        placed[-u], parent[-u] = True, -p
        order.append(-u)
    return root, not frozen[root], parent, placed, order


def mean_pose(weights, Rs, ts):
    """Weighted mean of poses: rotation = top eigenvector of sum w q q^T, translation = weighted mean."""
    w = np.asarray(weights, dtype=np.float64)
    Q = np.stack([R_to_quat(R) for R in Rs])
    M = (Q * w[:, None]).T @ Q / w.sum()
    q = np.linalg.eigh(M)[1][:, -1]
    q = q if q[0] >= 0 else -q
    return q, (np.asarray(ts) * w[:, None]).sum(axis=0) / w.sum()


def views_of(frame_offsets, obs_cam, obs_world, obs_uv, world_xyz):
    """[(frame, camera, X, uv)] in (frame, camera) order -- the order of cc_rig_start_views."""
    out = []
    world_xyz = np.asarray(world_xyz, dtype=np.float32).reshape(-1, 3)
    obs_uv = np.asarray(obs_uv, dtype=np.float32).reshape(-1, 2)
    for f in range(len(frame_offsets) - 1):
        a, b = int(frame_offsets[f]), int(frame_offsets[f + 1])
        for c in sorted(set(int(x) for x in obs_cam[a:b])):
            k = a + np.nonzero(np.asarray(obs_cam[a:b]) == c)[0]
            out.append((f, c, world_xyz[np.asarray(obs_world)[k].astype(np.int64)].astype(np.float64), obs_uv[k].astype(np.float64)))
    return out


def poses_from_views(n_cams, n_frames, view_list, frozen, cam_q=None, cam_t=None, frame_q=None, frame_t=None):
    """Stages T, C and F from per-view results: view_list = [(frame, camera, kind, R, t, rms2)]."""
    C, F = n_cams, n_frames
    cq = np.tile([1.0, 0, 0, 0], (C, 1)) if cam_q is None else np.array(cam_q, dtype=np.float64).reshape(C, 4)
    ct = np.zeros((C, 3)) if cam_t is None else np.array(cam_t, dtype=np.float64).reshape(C, 3)
    fq = np.tile([1.0, 0, 0, 0], (F, 1)) if frame_q is None else np.array(frame_q, dtype=np.float64).reshape(F, 4)
    ft = np.zeros((F, 3)) if frame_t is None else np.array(frame_t, dtype=np.float64).reshape(F, 3)
    valid = {(f, c): (R, t, m) for f, c, kind, R, t, m in view_list if kind != INVALID}
    covis = np.zeros((C, C), dtype=np.int64)
    for (f, a) in valid:
        for b in range(C):
            if (f, b) in valid:
                covis[a, b] += 1
    root, at_identity, parent, placed, order = tree(covis, frozen)
    if root >= 0 and at_identity:
        cq[root], ct[root] = [1.0, 0, 0, 0], 0.0
    for c in order:
        p = parent[c]
        frames = [f for f in range(F) if (f, c) in valid and (f, p) in valid]
        Rs, ts, ws = [], [], []
        for f in frames:
            Rc, tc, mc = valid[(f, c)]
            Rp, tp, mp = valid[(f, p)]
            Rr = Rc @ Rp.T
            Rs.append(Rr); ts.append(tc - Rr @ tp); ws.append(1.0 / (mc + mp + 1e-30))
        q, t = mean_pose(ws, Rs, ts)
        Rr, Rpar = quat_to_R(q), quat_to_R(cq[p])
        cq[c], ct[c] = R_to_quat(Rr @ Rpar), Rr @ ct[p] + t
    frames_placed = 0
    for f in range(F):
        Rs, ts, ws = [], [], []
        for c in range(C):
            if placed[c] and (f, c) in valid:
                Rv, tv, m = valid[(f, c)]
                Rc = quat_to_R(cq[c])
                Rs.append(Rc.T @ Rv); ts.append(Rc.T @ (tv - ct[c])); ws.append(1.0 / (m + 1e-30))
        if ws:
            fq[f], ft[f] = mean_pose(ws, Rs, ts)
            frames_placed += 1
    report = dict(root_camera=root, root_at_identity=at_identity, parent=parent, cameras_placed=sum(placed),
                  cameras_unplaced=C - sum(placed), frames_placed=frames_placed, frames_unplaced=F - frames_placed)
    return cq, ct, fq, ft, report


def start(n_cams, frame_offsets, obs_cam, obs_world, obs_uv, world_xyz, frozen, cam_q=None, cam_t=None, frame_q=None, frame_t=None,
          refine="lm", iterations=10, route="svd"):
    """The whole start. refine: "lm" (the specified steps), "converged" (least_squares) or None (closed form)."""
    vl = []
    for f, c, X, uv in views_of(frame_offsets, obs_cam, obs_world, obs_uv, world_xyz):
        kind, R, t = view_closed_form(X, uv, route)
        if kind != INVALID:
            if refine == "lm":
                R, t = refine_lm(R, t, X, uv, iterations)
            elif refine == "converged":
                R, t = refine_converged(R, t, X, uv)
            m = rms2(R, t, X, uv)
            if not np.isfinite(m):
                kind = INVALID
        vl.append((f, c, kind, R, t, m if kind != INVALID else 0.0))
    cq, ct, fq, ft, report = poses_from_views(n_cams, len(frame_offsets) - 1, vl, frozen, cam_q, cam_t, frame_q, frame_t)
    kinds = [v[2] for v in vl]
    report.update(views_planar=kinds.count(PLANAR), views_general=kinds.count(GENERAL), views_invalid=kinds.count(INVALID),
                  views_valid=len(kinds) - kinds.count(INVALID))
    return cq, ct, fq, ft, report, vl


def random_rotation(rng, max_angle=np.pi):
    a = rng.normal(size=3)
    return _exp(a / np.linalg.norm(a) * rng.uniform(0, max_angle))


def plant_scene(n_cams, n_frames, n_points, seed=0, planar=False, unit=1.0, noise=0.0, board=None, on_z0=False):
    """A rig scene with exact planted poses, in the layout of cc_rig_create.

    Every frame has its own world points: a general cloud, or (planar) a board rotated and shifted anywhere in the world --
    board=(nx, ny) for a grid, else n_points random points on it; on_z0 leaves the board on the plane z = 0 about the origin. unit scales the world (1e3: millimetres). The cameras sit
    within 0.3 units of the rig origin turned by up to 0.4 rad, the rig stands about 4 units in front of the points. Inputs
    are rounded to float32 like the real ones; the planted poses are returned in float64 and are exact for the unrounded data.
    """
    rng = np.random.default_rng(seed)
    cam_R = [random_rotation(rng, 0.4) for _ in range(n_cams)]
    cam_t = [rng.uniform(-0.3, 0.3, 3) * unit for _ in range(n_cams)]
    world, off, ocam, oworld, ouv, fR, ft = [], [0], [], [], [], [], []
    for f in range(n_frames):
        if planar:
            if board:
                gx, gy = np.meshgrid(np.arange(board[0]), np.arange(board[1]))
                P2 = np.stack([gx.ravel() * 0.25, gy.ravel() * 0.25], axis=1) - [0.25 * (board[0] - 1) / 2, 0.25 * (board[1] - 1) / 2]
            else:
                P2 = rng.uniform(-0.8, 0.8, (n_points, 2))
            Rb, shift = (np.eye(3), np.zeros(3)) if on_z0 else (random_rotation(rng), rng.uniform(-3, 3, 3))
            X = (np.concatenate([P2, np.zeros((len(P2), 1))], axis=1) @ Rb.T + shift) * unit
        else:
            X = (rng.uniform(-0.8, 0.8, (n_points, 3)) + rng.uniform(-3, 3, 3)) * unit
        X = X.astype(np.float32).astype(np.float64)
        # rig pose: the points' centroid lands about 4 units down the rig's z axis; a board faces the rig within ~35 degrees
        Rf = random_rotation(rng, 0.6) @ Rb.T if planar else random_rotation(rng, 0.8)
        tf = np.array([0, 0, 4.0 * unit]) + rng.uniform(-0.3, 0.3, 3) * unit - Rf @ X.mean(axis=0)
        base = sum(len(w) for w in world)
        world.append(X)
        fR.append(Rf); ft.append(tf)
        for c in range(n_cams):
            xc = (X @ Rf.T + tf) @ cam_R[c].T + cam_t[c]
            assert np.all(xc[:, 2] > 0.5 * unit)
            uv = xc[:, :2] / xc[:, 2:3] + noise * rng.normal(size=(len(X), 2))
            ocam += [c] * len(X); oworld += list(range(base, base + len(X))); ouv.append(uv)
        off.append(len(ocam))
    return dict(n_cams=n_cams, frame_offsets=np.array(off, dtype=np.int64), obs_cam=np.array(ocam, dtype=np.uint32),
                obs_world=np.array(oworld, dtype=np.uint64), obs_uv=np.concatenate(ouv).astype(np.float32),
                world_xyz=np.concatenate(world).astype(np.float32), cam_R=np.stack(cam_R), cam_t=np.stack(cam_t),
                frame_R=np.stack(fR), frame_t=np.stack(ft))


def plant_rig(cam_R, cam_t, frame_R, frame_t, visible, n_points, seed=0, noise=0.0, view_noise=None):
    """Views planted for GIVEN poses, any poses: every (frame, camera) with visible[f][c] gets its own n_points world points,
    drawn in front of that camera (depth 3 .. 5) and carried back into the world through the planted poses, so cameras may
    look anywhere (rotations of 180 degrees between them included). view_noise = {(f, c): sigma} overrides the image noise of
    single views. Layout of cc_rig_create; world points are float32 numbers, image points rounded to float32."""
    rng = np.random.default_rng(seed)
    C, F = len(cam_R), len(frame_R)
    world, off, ocam, oworld, ouv = [], [0], [], [], []
    nw = 0
    for f in range(F):
        for c in range(C):
            if not visible[f][c]:
                continue
            xc = np.concatenate([rng.uniform(-0.8, 0.8, (n_points, 2)), rng.uniform(3, 5, (n_points, 1))], axis=1)
            X = ((xc - cam_t[c]) @ cam_R[c] - frame_t[f]) @ frame_R[f]
            X = X.astype(np.float32).astype(np.float64)
            p = (X @ frame_R[f].T + frame_t[f]) @ cam_R[c].T + cam_t[c]
            sigma = (view_noise or {}).get((f, c), noise)
            ouv.append(p[:, :2] / p[:, 2:3] + sigma * rng.normal(size=(n_points, 2)))
            world.append(X)
            ocam += [c] * n_points; oworld += list(range(nw, nw + n_points))
            nw += n_points
        off.append(len(ocam))
    return dict(n_cams=C, frame_offsets=np.array(off, dtype=np.int64), obs_cam=np.array(ocam, dtype=np.uint32),
                obs_world=np.array(oworld, dtype=np.uint64), obs_uv=np.concatenate(ouv).astype(np.float32),
                world_xyz=np.concatenate(world).astype(np.float32), cam_R=np.asarray(cam_R), cam_t=np.asarray(cam_t),
                frame_R=np.asarray(frame_R), frame_t=np.asarray(frame_t))


def merge_scenes(scenes):
    """Scenes of the same cameras one after the other: their frames, their world points renumbered."""
    off, nw, out = [0], 0, dict(n_cams=scenes[0]["n_cams"])
    for s in scenes:
        off += list(off[-1] + np.asarray(s["frame_offsets"][1:]))
    out["frame_offsets"] = np.array(off, dtype=np.int64)
    out["obs_cam"] = np.concatenate([s["obs_cam"] for s in scenes])
    ow = []
    for s in scenes:
        ow.append(s["obs_world"] + np.uint64(nw))
        nw += len(s["world_xyz"])
    out["obs_world"] = np.concatenate(ow)
    out["obs_uv"] = np.concatenate([s["obs_uv"] for s in scenes])
    out["world_xyz"] = np.concatenate([s["world_xyz"] for s in scenes])
    return out
