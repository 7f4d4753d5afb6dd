"""The batched intrinsics solve (cc_intrinsics_batch_*, an extension: many independent single-camera problems in one pair of
launches per LM iteration) against the CPU oracle and against itself.

Tolerances are the standing ones of the single-problem path (tests/test_gpu_intrinsics.py): same
termination, iterations, successful steps and accept sequence; per-iteration costs 1e-9 relative; fx fy px py 1e-9 relative,
distortion 1e-9 absolute, float32 write-back identical or +-1 ulp where float32 is the coarser; poses 1e-9. Independence of a
problem from the rest of its batch is bit for bit.

The batch, in this order: 5 x 100; 5 x 100 with k3 held; 7 ragged frames whose point counts 64 / 65 / 257 / 300 sit on both
sides of the 64-observation wave pass and of the 256-observation workgroup pass; 20 x 88; the 5 x 100 problem started from
the oracle's converged state. With the default options the oracle takes 4, 3, 4, 4 and 1 iterations for them, so the
problems finish in different rounds."""
import numpy as np
import pytest

from camera_calibrator_amd import capi
from oracle import pyoracle as po
from tests.helpers import intrinsics_case
from tests.test_gpu_intrinsics import _assert_intrinsics_close

pytestmark = pytest.mark.gpu

_LOG_KEYS = [f[0] for f in capi.Iteration._fields_]
_cache = {}


def _batch():
    """[(case, const_mask)] in the order above, plus the oracle's result per problem: computed once, never modified."""
    if "batch" not in _cache:
        a, ragged, c3 = intrinsics_case(5, 100), intrinsics_case(7, [8, 64, 65, 300, 5, 257, 128]), intrinsics_case(20, 88)
        io, qo, to, _ = po.intrinsics_solve(a["off"], a["uv"], a["xyz"], a["intr0"], a["q0"], a["t0"])
        conv = dict(a, intr0=io, q0=qo, t0=to)
        probs = [(a, 0), (a, 1 << 8), (ragged, 0), (c3, 0), (conv, 0)]
        _cache["batch"] = probs
        _cache["oracle"] = [_oracle(c, m) for c, m in probs]
    return _cache["batch"], _cache["oracle"]


def _oracle(case, mask, **opt_kw):
    return po.intrinsics_solve(case["off"], case["uv"], case["xyz"], case["intr0"], case["q0"], case["t0"], const_mask=mask,
                               options=po.default_options(**opt_kw))


def _run(probs, **opt_kw):
    """Solves `probs` as one batch; per problem (intr, q, t, summary)."""
    b = capi.IntrinsicsBatch([(c["off"], c["uv"], c["xyz"]) for c, _ in probs])
    b.set_state([c["intr0"] for c, _ in probs], [c["q0"] for c, _ in probs], [c["t0"] for c, _ in probs],
                const_mask=[m for _, m in probs])
    ss = b.solve(capi.default_options(**opt_kw))
    intr, qs, ts = b.get_state()
    b.close()
    return [(intr[p], qs[p], ts[p], ss[p]) for p in range(len(probs))]


def _log_array(s):
    return np.array([[l[k] for k in _LOG_KEYS] for l in s["log"]], dtype=np.float64).reshape(len(s["log"]), len(_LOG_KEYS))


def _assert_same_bits(a, b):
    (ia, qa, ta, sa), (ib, qb, tb, sb) = a, b
    assert np.array_equal(ia, ib) and np.array_equal(qa, qb) and np.array_equal(ta, tb)
    assert np.array_equal(_log_array(sa), _log_array(sb))
    for k in ("iterations", "successful_steps", "termination", "initial_cost", "final_cost", "sweeps"):
        assert sa[k] == sb[k], k


def _assert_parity(got, want, label):
    (ig, qg, tg, sg), (io, qo, to, so) = got, want
    cg = np.array([l["cost"] for l in sg["log"]]); co = np.array([l["cost"] for l in so["log"]])
    print(label, "iterations", sg["iterations"], so["iterations"], "termination", sg["termination"], so["termination"],
          "max rel cost diff", float(np.max(np.abs(cg - co) / co)) if len(cg) == len(co) and len(co) else None,
          "intr diff", np.abs(ig - io), "pose diff", float(np.abs(qg - qo).max()), float(np.abs(tg - to).max()))
    assert sg["termination"] == so["termination"] and sg["iterations"] == so["iterations"]
    assert sg["successful_steps"] == so["successful_steps"]
    assert [l["accepted"] for l in sg["log"]] == [l["accepted"] for l in so["log"]]
    assert np.allclose(cg, co, rtol=1e-9, atol=0)
    _assert_intrinsics_close(ig, io)
    assert np.abs(qg - qo).max() < 1e-9 and np.abs(tg - to).max() < 1e-9


def _results():
    if "results" not in _cache:
        _cache["results"] = _run(_batch()[0])
    return _cache["results"]


def test_every_problem_of_the_batch_matches_the_oracle():
    probs, oracle = _batch()
    assert [o[3]["iterations"] for o in oracle] == [4, 3, 4, 4, 1]       # the problems finish in different rounds
    got = _results()
    for p in range(len(probs)):
        _assert_parity(got[p], oracle[p], "problem %d" % p)
    assert got[1][0][8] == probs[1][0]["intr0"][8]                       # k3 held


def test_a_problem_does_not_depend_on_its_batch_bit_for_bit():
    probs, oracle = _batch()
    got = _results()
    for p in range(len(probs)):                                          # ... alone
        _assert_same_bits(got[p], _run([probs[p]])[0])
    rev = _run(probs[::-1])[::-1]                                        # ... and with the order of the batch reversed
    for p in range(len(probs)):
        _assert_same_bits(got[p], rev[p])
    # the problem that stops in iteration 1 holds its bits while the others run on for three more rounds
    assert got[4][3]["iterations"] == 1 and min(got[p][3]["iterations"] for p in range(4)) >= 3


@pytest.mark.parametrize("max_iterations", [0, 1])
def test_iteration_limits(max_iterations):
    probs, _ = _batch()
    got = _run(probs, max_iterations=max_iterations)
    for p, (case, mask) in enumerate(probs):
        want = _oracle(case, mask, max_iterations=max_iterations)
        _assert_parity(got[p], want, "max_iterations %d, problem %d" % (max_iterations, p))
        assert got[p][3]["iterations"] == max_iterations
        if max_iterations == 0:
            assert got[p][3]["termination"] == "NO_CONVERGENCE" and got[p][3]["final_cost"] == got[p][3]["initial_cost"]
            assert np.array_equal(got[p][0], case["intr0"]) and np.array_equal(got[p][1], case["q0"]) and np.array_equal(got[p][2], case["t0"])


def test_batch_of_one_and_the_state_round_trip():
    probs, oracle = _batch()
    case, mask = probs[2]
    b = capi.IntrinsicsBatch([(case["off"], case["uv"], case["xyz"])])
    b.set_state([case["intr0"]], [case["q0"]], [case["t0"]], const_mask=[mask])
    i0, q0, t0 = b.get_state()                                           # before any solve: what set_state put in
    assert np.array_equal(i0[0], case["intr0"]) and np.array_equal(q0[0], case["q0"]) and np.array_equal(t0[0], case["t0"])
    s1 = b.solve()[0]
    i1, q1, t1 = b.get_state()
    _assert_parity((i1[0], q1[0], t1[0], s1), oracle[2], "batch of one")
    b.set_state([case["intr0"]], [case["q0"]], [case["t0"]], const_mask=[mask])   # a second solve reproduces the first
    s2 = b.solve()[0]
    i2, q2, t2 = b.get_state()
    _assert_same_bits((i1[0], q1[0], t1[0], s1), (i2[0], q2[0], t2[0], s2))
    # continuing from the converged point stops at once without moving
    s3 = b.solve()[0]
    i3, _, _ = b.get_state()
    assert s3["iterations"] <= 1 and np.allclose(i3[0], i1[0], rtol=1e-9)
    with pytest.raises(capi.CcError):
        b.solve(capi.default_options(profile_kernels=1))
    b.close()


def test_batch_estimate_matches_the_single_problem_estimate():
    probs, _ = _batch()
    pick = [probs[0], probs[2], probs[3]]
    masks = [0, 1 << 8, 0]
    d5 = np.array([[0.0] * 5, [0, 0, 0, 0, 1e-3], [1e-2, 0, 0, 0, 0]])
    K, intr, qs, ts, ss = capi.intrinsics_batch_estimate([(c["off"], c["uv"], c["xyz"]) for c, _ in pick], distortion5=d5, const_mask=masks)
    for p, (c, _) in enumerate(pick):
        K1, i1, q1, t1, s1 = capi.intrinsics_estimate(c["off"], c["uv"], c["xyz"], distortion5=d5[p], const_mask=masks[p])
        assert np.array_equal(K[p], K1)                                   # the same initialisation kernels
        _assert_parity((intr[p], qs[p], ts[p], ss[p]), (i1, q1, t1, s1), "estimate, problem %d" % p)
    assert intr[1][8] == 1e-3
