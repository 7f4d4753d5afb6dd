"""Huber loss of the single-camera intrinsics solve on the GPU (cc_intrinsics_set_huber / _obs_cost, cc_intrinsics_batch_set_huber,
the *_huber one-shot forms) against the CPU references of tests/huber_ref.py: dirty fixture data (10 % of the observations
displaced by 5 - 30 px), the one-frozen-camera rig oracle for the solves, extended-precision sums for the blocks.

Tolerances are the project's standing ones: blocks 1e-12 of the block's largest entry, cost 1e-12 relative; solves as
test_solve_matches_oracle_default_options (iterations, termination, accepted / valid flags equal; logged costs 1e-9 relative;
fx fy px py 1e-9 relative; distortion 1e-9 absolute; poses 1e-9) -- the Huber weight is continuous at s = a^2, so they carry over."""
import os
import subprocess
import sys

import numpy as np
import pytest

from camera_calibrator_amd import capi
from oracle import pyoracle as po
from tests import huber_ref as hr
from tests.helpers import block_rel_err

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LOG_KEYS = [f[0] for f in capi.Iteration._fields_]


def _problem(c, mask=0, a=None, intr0=None, q0=None, t0=None):
    prob = capi.IntrinsicsProblem(c["off"], c["uv"], c["xyz"])
    prob.set_state(c["intr0"] if intr0 is None else intr0, c["q0"] if q0 is None else q0, c["t0"] if t0 is None else t0, const_mask=mask)
    if a is not None:
        prob.set_huber(a)
    return prob


def _log_array(s):
    return np.array([[l[k] for k in _LOG_KEYS] for l in s["log"]], dtype=np.float64).reshape(len(s["log"]), len(_LOG_KEYS))


def _assert_same_bits(a, b):
    (ia, qa, ta, sa), (ib, qb, tb, sb) = a, b
    assert np.array_equal(ia, ib) and np.array_equal(qa, qb) and np.array_equal(ta, tb)
    assert np.array_equal(_log_array(sa), _log_array(sb))
    for k in ("iterations", "successful_steps", "termination", "initial_cost", "final_cost", "sweeps"):
        assert sa[k] == sb[k], k


# ---- 1. blocks and cost with the loss on -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", [0, hr.K3_FROZEN])
@pytest.mark.parametrize("a", [1.0, 1e-3])
def test_blocks_and_cost_with_the_loss_on(a, mask):
    """Ragged case at the Zhang start (also what the child of test_blocks_with_the_frames_cut_into_three_tiles runs with
    CC_SWEEP_TILES=3). With a = 1e-3 every observation is in the tail."""
    c = hr.dirty_case("ragged")
    prob = _problem(c, mask, a)
    cost_g, blocks_g = prob.eval()
    prob.close()
    cost_r, blocks_r = hr.huber_blocks(c, c["intr0"], c["q0"], c["t0"], a, mask)
    r, _ = hr.residuals(c, c["intr0"], c["q0"], c["t0"])
    tail = (r ** 2).sum(axis=1) > a * a
    print("a", a, "mask", mask, "tail", tail.mean(), "block err", block_rel_err(blocks_g, blocks_r), "cost rel", abs(cost_g - cost_r) / cost_r)
    assert tail.all() if a == 1e-3 else 0 < tail.sum() < len(tail)   # (a = 1: both sides of a^2 occur -- 97.6 % tail at this start)
    assert block_rel_err(blocks_g, blocks_r) < 1e-12
    assert abs(cost_g - cost_r) <= 1e-12 * cost_r


def test_a_threshold_nothing_exceeds_leaves_the_blocks_bit_for_bit():
    """a = 1e6: no observation in the tail -- blocks equal the loss-off eval bit for bit, cost within 1e-14 relative (another
    order of the same sum); +inf is allowed and gives the same."""
    c = hr.dirty_case("ragged")
    prob = _problem(c)
    cost0, blocks0 = prob.eval()
    for a in (1e6, float("inf")):
        prob.set_huber(a)
        cost1, blocks1 = prob.eval()
        print("a", a, "cost rel", abs(cost1 - cost0) / cost0, "max block diff / largest entry", block_rel_err(blocks1, blocks0),
              "entries that differ", int((blocks1 != blocks0).sum()), "of", blocks0.size)
        assert np.array_equal(blocks1, blocks0)
        assert abs(cost1 - cost0) <= 1e-14 * cost0
    prob.set_huber(0.0)
    cost2, blocks2 = prob.eval()
    prob.close()
    assert cost2 == cost0 and np.array_equal(blocks2, blocks0)


def test_blocks_with_the_frames_cut_into_three_tiles():
    """The block tests again in a child process with CC_SWEEP_TILES=3 (read when a handle is created), the way
    tests/test_gpu_tiles.py starts its child: every tile adds its own share of the cost."""
    env = dict(os.environ, CC_SWEEP_TILES="3")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-x", "-p", "no:cacheprovider", "tests/test_gpu_intr_huber.py",
                        "-k", "test_blocks_and_cost_with_the_loss_on or test_a_threshold_nothing_exceeds"], cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0 and "5 passed" in r.stdout, r.stdout[-4000:]


# ---- 2. solve parity, 5. obs_cost -------------------------------------------------------------------------------------------------
def _solve(shape, a, mask=0, graph=0):
    c = hr.dirty_case(shape)
    prob = _problem(c, mask, a)
    s = prob.solve(capi.default_options(use_graph=graph))
    state = prob.get_state()
    cost = prob.obs_cost()
    form, reruns, _ = prob.solver_status()
    prob.close()
    return s, state, cost, (form, reruns)


@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("shape,mask", [("ragged", 0), ("8x40", 0), ("5x30", 0), ("ragged", hr.K3_FROZEN)])
def test_solve_matches_the_oracle(shape, mask, graph):
    a = 1.0
    io, qo, to, cost_o, so = hr.oracle_solution(shape, a, mask)
    assert so["iterations"] == hr.ORACLE_ITERATIONS[shape][1 if mask else 0] and so["termination"] == "FUNCTION"
    s, (ig, qg, tg), cost_g, (form, reruns) = _solve(shape, a, mask, graph)
    cg, co = np.array([l["cost"] for l in s["log"]]), np.array([l["cost"] for l in so["log"]])
    print(shape, mask, graph, "iterations", s["iterations"], so["iterations"], s["termination"],
          "max rel cost diff", float(np.max(np.abs(cg - co) / co)) if len(cg) == len(co) else None, "intr diff", np.abs(ig - io),
          "pose diff", float(np.abs(qg - qo).max()), float(np.abs(tg - to).max()))
    hr.assert_solve_matches(s, (ig, qg, tg), so, (io, qo, to))
    assert form == 0 and reruns == 0
    # not vacuous: between 5 % and 20 % of the observations end in the tail (measured 9.9 %, 10.0 %, 10.7 %) ...
    tail = (cost_o > a * a / 2).mean()
    assert 0.05 <= tail <= 0.20, tail
    # ... and it helps: the oracle's Huber fx is at least twice as close to the fixture's 1000 as its L2 fx (a = 1e6; measured
    # factors 37, 7, 14), and the GPU result inherits that through the parity above
    fx_l2 = hr.oracle_solution(shape, 1e6, mask)[0][0]
    assert 2.0 * abs(io[0] - 1000.0) <= abs(fx_l2 - 1000.0) and 2.0 * abs(ig[0] - 1000.0) <= abs(fx_l2 - 1000.0), (ig[0], io[0], fx_l2)
    # 5. the per-observation costs at the solution: the oracle's, 1e-9 relative + 1e-12 absolute
    print("obs_cost max diff", float(np.abs(cost_g - cost_o).max()))
    assert np.all(np.abs(cost_g - cost_o) <= 1e-9 * np.abs(cost_o) + 1e-12)


def test_obs_cost_with_the_loss_off_is_half_the_squared_residual():
    c = hr.dirty_case("ragged")
    prob = _problem(c)
    cost_g = prob.obs_cost()
    prob.close()
    r, _ = hr.residuals(c, c["intr0"], c["q0"], c["t0"])
    want = 0.5 * (r ** 2).sum(axis=1)
    print("max rel diff", float(np.max(np.abs(cost_g - want) / want)))
    assert np.all(np.abs(cost_g - want) <= 1e-12 * want)


def test_bad_arguments_on_a_live_handle_are_refused():
    """What tests/test_huber_cpu.py cannot reach without a device: a valid handle with a NULL output array or a NaN threshold."""
    import ctypes as C
    c = hr.dirty_case("5x30")
    prob = _problem(c)
    lib = capi.lib()
    assert lib.cc_intrinsics_obs_cost(prob._h, None) == -1 and "NULL" in lib.cc_last_error().decode()
    assert lib.cc_intrinsics_set_huber(prob._h, C.c_double(float("nan"))) == -1 and "NaN" in lib.cc_last_error().decode()
    assert prob.obs_cost().shape == (len(c["uv"]),)      # (the handle is none the worse for it)
    prob.close()
    b = capi.IntrinsicsBatch([(c["off"], c["uv"], c["xyz"])])
    nan = np.array([float("nan")])
    assert lib.cc_intrinsics_batch_set_huber(b._h, nan.ctypes.data_as(C.POINTER(C.c_double))) == -1 and "NaN" in lib.cc_last_error().decode()
    b.close()


# ---- 3. trust-region branches -----------------------------------------------------------------------------------------------------
def _perturbed_start(c, seed, scale):
    rng = np.random.default_rng(seed)
    intr = c["intr0"].copy()
    intr[:2] *= 1.0 + 0.35 * scale
    intr[4:] = np.array([0.3, -0.2, 0.02, -0.02, 0.1]) * scale
    q = c["q0"] + 0.15 * scale * rng.normal(size=c["q0"].shape)
    t = c["t0"] * (1.0 + 0.25 * scale * rng.normal(size=c["t0"].shape))
    return intr, q, t


@pytest.mark.parametrize("shape,seed,scale", [("5x30", 0, 0.3), ("8x40", 2, 1.0)])
def test_rejected_steps_and_radius_shrinking(shape, seed, scale):
    """With the Corrector's Gauss-Newton model (rho'' dropped) a Huber step's relative decrease sits ABOVE 1 on these problems, so
    perturbed starts, small or huge initial radii and monotonic steps were all searched on the oracle without one rejected step
    at the default min_relative_decrease; a threshold of 1.5 with monotonic steps rejects 8 steps of these two starts between
    accepted ones (14 and 13 iterations, PARAMETER). The same trajectory on the GPU, tolerances of the parity test."""
    c = hr.dirty_case(shape)
    start = _perturbed_start(c, seed, scale)
    kw = dict(min_relative_decrease=1.5, use_nonmonotonic_steps=0)
    io, qo, to, _, so = hr.oracle_solve(c, 1.0, 0, po.default_options(**kw), *start)
    acc = [l["accepted"] for l in so["log"]]
    assert acc[:-1].count(0) >= 5 and acc.count(1) >= 2, "the scenario is meant to mix accepted and rejected steps"
    prob = _problem(c, 0, 1.0, *start)
    s = prob.solve(capi.default_options(**kw))
    state = prob.get_state()
    prob.close()
    print(shape, "iterations", s["iterations"], so["iterations"], s["termination"], so["termination"], "accepted", acc)
    hr.assert_solve_matches(s, state, so, (io, qo, to))
    assert np.allclose([l["radius"] for l in s["log"]], [l["radius"] for l in so["log"]], rtol=1e-6)


# ---- 4. form and state ------------------------------------------------------------------------------------------------------------
def test_the_loss_selects_the_two_kernel_form_and_the_handle_gets_its_form_back():
    c = hr.dirty_case("8x40")
    fresh = _problem(c)
    form_created = fresh.solver_form()
    s_fresh = fresh.solve()
    ref = (*fresh.get_state(), s_fresh)
    fresh.close()

    prob = _problem(c)
    prob.set_huber(1.0)
    assert prob.solver_form() == 0
    s1 = prob.solve()
    st1 = prob.get_state()
    form, reruns, note = prob.solver_status()
    assert form == 0 and reruns == 0 and note == ""
    assert s1["final_cost"] < 0.5 * s_fresh["final_cost"]          # (another objective altogether)
    with pytest.raises(capi.CcError, match="cc error -5.*Huber"):
        prob.exchange_export()
    with pytest.raises(capi.CcError, match="cc error -5.*Huber"):
        prob.profile_solve(n=1)
    # reset + solve twice with the loss on: bit-identical
    prob.reset()
    s2 = prob.solve()
    _assert_same_bits((*st1, s1), (*prob.get_state(), s2))
    # off again: the creation form, and a solve from the start equals a fresh handle's bit for bit
    prob.set_huber(0.0)
    assert prob.solver_form() == form_created
    prob.reset()
    s3 = prob.solve()
    _assert_same_bits((*prob.get_state(), s3), ref)
    # an attached handle refuses the loss; a handle with the loss refuses the attachment
    prob.exchange_attach(0, [prob.exchange_export()])
    with pytest.raises(capi.CcError, match="cc error -5"):
        prob.set_huber(1.0)
    prob.close()
    other = _problem(c, 0, 1.0)
    with pytest.raises(capi.CcError, match="cc error -5.*Huber"):
        other.exchange_attach(0, [b"\0" * 64])
    other.close()


def test_a_nan_observation_ends_the_solve_as_it_does_with_the_loss_off():
    c = hr.dirty_case("5x30")
    uv = c["uv"].copy()
    uv[17, 0] = np.nan
    bad = dict(c, uv=uv)

    def run(a):
        prob = _problem(bad, 0, a)
        try:
            s = prob.solve(capi.default_options(max_iterations=20))
            out = ("ok", s["termination"], s["iterations"], np.isfinite(s["final_cost"]))
        except capi.CcError as e:
            out = ("error", str(e).split(":")[0])
        prob.close()
        return out

    off, on = run(None), run(1.0)
    print(off, on)
    assert on == off


# ---- 6. batch ---------------------------------------------------------------------------------------------------------------------
_BATCH = [("5x30", 1.0), ("ragged", 0.0), ("8x40", 2.0)]


def _run_batch(items, set_huber=True):
    cases = [hr.dirty_case(sh) for sh, _ in items]
    b = capi.IntrinsicsBatch([(c["off"], c["uv"], c["xyz"]) for c in cases])
    b.set_state([c["intr0"] for c in cases], [c["q0"] for c in cases], [c["t0"] for c in cases])
    if set_huber:
        b.set_huber([a for _, a in items])
    ss = b.solve()
    intr, qs, ts = b.get_state()
    b.close()
    return [(intr[p], qs[p], ts[p], ss[p]) for p in range(len(items))]


def test_batch_with_a_loss_per_problem():
    got = _run_batch(_BATCH)
    for (shape, a), g in zip(_BATCH, got):
        if a > 0:
            io, qo, to, _, so = hr.oracle_solution(shape, a)
        else:
            c = hr.dirty_case(shape)
            io, qo, to, so = po.intrinsics_solve(c["off"], c["uv"], c["xyz"], c["intr0"], c["q0"], c["t0"])
        print(shape, a, "iterations", g[3]["iterations"], so["iterations"], g[3]["termination"], "intr diff", np.abs(g[0] - io))
        hr.assert_solve_matches(g[3], g[:3], so, (io, qo, to))
    # a problem's bits do not depend on the batch it sits in: alone in a batch of one with the same a
    for item, g in zip(_BATCH, got):
        _assert_same_bits(g, _run_batch([item])[0])
    # the plain problem keeps what a batch that never heard of the loss returns for it
    _assert_same_bits(got[1], _run_batch(_BATCH, set_huber=False)[1])
    # switching everything off again: the plain batch, bit for bit
    cases = [hr.dirty_case(sh) for sh, _ in _BATCH]
    b = capi.IntrinsicsBatch([(c["off"], c["uv"], c["xyz"]) for c in cases])
    b.set_state([c["intr0"] for c in cases], [c["q0"] for c in cases], [c["t0"] for c in cases])
    b.set_huber([a for _, a in _BATCH])
    b.set_huber(None)
    ss = b.solve()
    intr, qs, ts = b.get_state()
    b.close()
    plain = _run_batch(_BATCH, set_huber=False)
    for p in range(len(_BATCH)):
        _assert_same_bits((intr[p], qs[p], ts[p], ss[p]), plain[p])


def test_batch_estimate_with_losses_is_zhang_plus_the_batched_solve():
    cases = [hr.dirty_case(sh) for sh, _ in _BATCH]
    a = [x for _, x in _BATCH]
    K, intr, qs, ts, ss = capi.intrinsics_batch_estimate([(c["off"], c["uv"], c["xyz"]) for c in cases], huber_a=a)
    b = capi.IntrinsicsBatch([(c["off"], c["uv"], c["xyz"]) for c in cases])
    intr0, q0, t0 = [], [], []
    for p, c in enumerate(cases):
        Kp, q, t = capi.zhang_init(c["off"], c["uv"], c["xyz"])
        assert np.array_equal(Kp, K[p])
        intr0.append(np.array([Kp[0, 0], Kp[1, 1], Kp[0, 2], Kp[1, 2], 0, 0, 0, 0, 0], dtype=np.float64))
        q0.append(q.astype(np.float64))
        t0.append(t.astype(np.float64))
    b.set_state(intr0, q0, t0)
    b.set_huber(a)
    s2 = b.solve()
    i2, q2, t2 = b.get_state()
    b.close()
    for p in range(len(cases)):
        _assert_same_bits((intr[p], qs[p], ts[p], ss[p]), (i2[p], q2[p], t2[p], s2[p]))
    # the single-problem one-shot forms take the same loss (two-kernel form, views handed over as their own arrays)
    c = cases[0]
    K1, i1, q1, t1, s1 = capi.intrinsics_estimate(c["off"], c["uv"], c["xyz"], huber_a=a[0])
    hr.assert_solve_matches(s1, (i1, q1, t1), ss[0], (intr[0], qs[0], ts[0]))
    io, qo, to, so = capi.intrinsics_optimize(c["off"], c["uv"], c["xyz"], intr0[0], q0[0], t0[0], huber_a=a[0])
    _assert_same_bits((io, qo, to, so), (i1, q1, t1, s1))
