"""Where does the control of k_intr_persist predict that the next decision ends the solve (csrc/cc_intrinsics_persist.hpp:
persist_predicts_end), and was it right? Replayed on the CPU oracle's iteration logs, no GPU: the benchmark's problem
(1000 frames x 500 points from the Zhang start, default options) and the fixtures of tests/test_gpu_intr_final_sweep.py.
    python scripts/final_sweep_predictor.py [--no-bench]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import pyoracle as po  # noqa: E402
import test_gpu_intr_final_sweep as fx  # noqa: E402


def replay(name, s, max_iterations, function_tolerance):
    log = s["log"]
    print("%s: %d iterations, %s" % (name, s["iterations"], s["termination"]))
    cc_prev = 0.0
    for i, rec in enumerate(log):
        last = i == len(log) - 1
        fires = ""
        if rec["accepted"] and not last:
            limit = i + 2 >= max_iterations
            p = rec["cost_change"] * min(1.0, rec["cost_change"] / cc_prev) if cc_prev > 0.0 and rec["cost_change"] > 0.0 else float("nan")
            ftol = fx.predicts_end(rec["cost_change"], cc_prev, function_tolerance, rec["cost"])
            if limit or ftol:
                nxt_ends = i + 1 == len(log) - 1 and s["termination"] in ("NO_CONVERGENCE", "FUNCTION", "PARAMETER")
                fires = "  PREDICTS (%s): next decision %s" % ("limit" if limit else "p = %.3e <= %.3e" % (p, function_tolerance * rec["cost"]),
                                                                 "ends the solve" if nxt_ends else "DOES NOT end the solve")
            elif p == p:
                fires = "  p = %.3e > %.3e" % (p, function_tolerance * rec["cost"])
        if rec["accepted"]:
            cc_prev = rec["cost_change"]
        print("  %2d cost_change %.6e model %.6e accepted %d cost %.10g%s" % (i + 1, rec["cost_change"], rec["model_cost_change"], rec["accepted"], rec["cost"], fires))


def main():
    o = po.default_options()
    max_it, ftol = o.max_iterations, o.function_tolerance
    if "--no-bench" not in sys.argv:
        off, uv, xyz = po.make_intrinsics_problem(1000, 500)
        K, q, t = po.zhang_init(off, uv, xyz)
        intr0 = np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2], 0, 0, 0, 0, 0], dtype=np.float64)
        replay("bench 1000 x 500", po.intrinsics_solve(off, uv, xyz, intr0, q.astype(np.float64), t.astype(np.float64))[3], max_it, ftol)
    inp = fx._inputs()
    for name, mask in fx.MASKS.items():
        replay("fixture default_" + name, po.intrinsics_solve(inp["off"], inp["uv"], inp["xyz"], inp["intr0"], inp["q0"], inp["t0"], const_mask=mask)[3], max_it, ftol)
    for n in (1, 2, 3):
        replay("fixture limit_%d" % n, po.intrinsics_solve(inp["off"], inp["uv"], inp["xyz"], inp["intr0"], inp["q0"], inp["t0"], options=po.default_options(max_iterations=n))[3], n, ftol)
    replay("fixture miss", po.intrinsics_solve(inp["off"], inp["uv"], inp["xyz"], inp["intr_b"], inp["q_b"], inp["t_b"], options=po.default_options(**fx.MISS_OPTIONS))[3],
           fx.MISS_OPTIONS["max_iterations"], ftol)
    for name, kw in fx.OTHER_ENDINGS.items():
        replay("fixture other_" + name, po.intrinsics_solve(inp["off"], inp["uv"], inp["xyz"], inp["intr0"], inp["q0"], inp["t0"], options=po.default_options(**kw))[3],
               kw.get("max_iterations", max_it), kw["function_tolerance"])


if __name__ == "__main__":
    main()
