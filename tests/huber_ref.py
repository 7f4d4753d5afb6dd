"""Shared inputs and CPU references of the Huber-loss tests of the single-camera intrinsics solve (tests/test_huber_cpu.py,
tests/test_gpu_intr_huber*.py).

Inputs: the fixture generator's problem with 10 % of the observations displaced by +-U(5, 30) px per coordinate
(default_rng(3)), started from the Zhang initialisation of the SAME dirty data with zero distortion.

References, both from the CPU oracle as it stands:
  * the solve: oc_rigk_solve with ONE camera frozen at the identity and huber_a in pixels is the single-camera problem
    (tests/test_huber_cpu.py pins it against oc_intrinsics_solve with the loss off); it also returns the per-observation costs;
  * the blocks: po.intrinsics_residual per observation (2 x 15 J and r), the two rows scaled by sqrt(rho'), [J r]^T [J r] summed
    in np.longdouble; the cost is 1/2 sum rho.
Everything is computed once per process and handed out as copies-by-convention: callers must not modify what they get."""
import functools

import numpy as np

from oracle import pyoracle as po

RAGGED = (5, 63, 64, 65, 257, 300)   # partial waves, exactly one wave, one over, more than one pass of 256
SHAPES = {"ragged": (len(RAGGED), list(RAGGED)), "8x40": (8, 40), "5x30": (5, 30)}
K3_FROZEN = 1 << 8
# iterations of the CPU oracle with a = 1.0 and default options (all terminate on FUNCTION): (free, k3 frozen)
ORACLE_ITERATIONS = {"ragged": (10, 10), "8x40": (5, 5), "5x30": (11, 10)}


@functools.lru_cache(maxsize=None)
def dirty_case(shape):
    """dict(off, uv, xyz, intr0, q0, t0, outlier): the shape's problem with planted outliers and its Zhang start."""
    frames, pts = SHAPES[shape]
    off, uv, xyz = po.make_intrinsics_problem(frames, pts)
    rng = np.random.default_rng(3)
    n = len(uv)
    idx = rng.choice(n, n // 10, replace=False)
    shift = rng.uniform(5.0, 30.0, size=(len(idx), 2)) * rng.choice([-1.0, 1.0], size=(len(idx), 2))
    uv = uv.astype(np.float64)
    uv[idx] += shift
    uv = uv.astype(np.float32)
    outlier = np.zeros(n, dtype=bool)
    outlier[idx] = True
    K, q, t = po.zhang_init(off, uv, xyz)
    intr0 = np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2], 0, 0, 0, 0, 0], dtype=np.float64)
    return dict(off=off, uv=uv, xyz=xyz, intr0=intr0, q0=q.astype(np.float64), t0=t.astype(np.float64), outlier=outlier)


def oracle_solve(c, a, const_mask=0, options=None, intr0=None, q0=None, t0=None):
    """The one-frozen-camera rig oracle on case c with HuberLoss(a) (a = 0: no loss). Returns (intr, q, t, obs_cost, summary)."""
    n = int(c["off"][-1])
    opt = options if options is not None else po.default_options()
    intr, _, _, q, t, cost, s = po.rigk_solve(
        1, c["off"], np.zeros(n, dtype=np.uint32), np.arange(n, dtype=np.uint64), c["uv"], c["xyz"],
        c["intr0"] if intr0 is None else intr0, [[1.0, 0.0, 0.0, 0.0]], [[0.0, 0.0, 0.0]], [1],
        c["q0"] if q0 is None else q0, c["t0"] if t0 is None else t0, const_mask, a, opt)
    return intr, q.reshape(-1, 4), t.reshape(-1, 3), cost, s


@functools.lru_cache(maxsize=None)
def oracle_solution(shape, a, const_mask=0):
    """oracle_solve with default options from the case's own start, once per process."""
    return oracle_solve(dirty_case(shape), a, const_mask)


def residuals(c, intr, q, t):
    """(r [N][2], J [N][2][15]) of po.intrinsics_residual at the given point."""
    off = c["off"]
    n = int(off[-1])
    r, J = np.zeros((n, 2)), np.zeros((n, 2, 15))
    for f in range(len(off) - 1):
        for i in range(int(off[f]), int(off[f + 1])):
            r[i], J[i] = po.intrinsics_residual(intr, q[f], t[f], c["xyz"][i].astype(np.float64), c["uv"][i].astype(np.float64))
    return r, J


def huber_blocks(c, intr, q, t, a, const_mask=0):
    """(cost, blocks [F][16][16]) with HuberLoss(a) in extended precision (a <= 0 or inf: no observation in the tail).
    Rows and columns of held coordinates are zero, as the sweep leaves them."""
    r, J = residuals(c, intr, q, t)
    off = c["off"]
    F = len(off) - 1
    s = (r.astype(np.longdouble) ** 2).sum(axis=1)
    al = np.longdouble(a)
    tail = (s > al * al) if a > 0 else np.zeros(len(s), dtype=bool)
    root = np.sqrt(np.where(tail, s, np.longdouble(1)))
    rho = np.where(tail, 2 * al * root - al * al, s)
    w = np.where(tail, np.sqrt(al / root), np.longdouble(1))
    rows = np.concatenate([J.astype(np.longdouble), r.astype(np.longdouble)[:, :, None]], axis=2) * w[:, None, None]   # [N][2][16]
    blocks = np.zeros((F, 16, 16), dtype=np.longdouble)
    for f in range(F):
        v = rows[int(off[f]):int(off[f + 1])].reshape(-1, 16)
        blocks[f] = v.T @ v
    held = [j for j in range(9) if const_mask & (1 << j)]
    blocks[:, held, :] = 0
    blocks[:, :, held] = 0
    return float(rho.sum() / 2), blocks.astype(np.float64)


def assert_solve_matches(summary, state, ref_summary, ref_state):
    """The tolerances of test_solve_matches_oracle_default_options: iterations, termination and the accepted / valid flags equal,
    logged costs 1e-9 relative, fx fy px py 1e-9 relative, distortion 1e-9 absolute, poses 1e-9."""
    s, so = summary, ref_summary
    assert s["iterations"] == so["iterations"] and s["termination"] == so["termination"], (s["iterations"], s["termination"], so["iterations"], so["termination"])
    assert [l["accepted"] for l in s["log"]] == [l["accepted"] for l in so["log"]]
    assert [l["valid"] for l in s["log"]] == [l["valid"] for l in so["log"]]
    assert np.allclose([l["cost"] for l in s["log"]], [l["cost"] for l in so["log"]], rtol=1e-9, atol=0)
    (ig, qg, tg), (io, qo, to) = state, ref_state
    assert np.allclose(ig[:4], io[:4], rtol=1e-9, atol=0) and np.allclose(ig[4:], io[4:], rtol=0, atol=1e-9), (ig, io)
    assert np.abs(np.reshape(qg, (-1, 4)) - np.reshape(qo, (-1, 4))).max() < 1e-9
    assert np.abs(np.reshape(tg, (-1, 3)) - np.reshape(to, (-1, 3))).max() < 1e-9
