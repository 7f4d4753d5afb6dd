"""The rig start (cc_rig_estimate_start) next to one LM iteration of the solve at the same shape, and the iterations the solve
takes from the computed start against the scenario's start. One JSON line per shape:

    python scripts/time_rig_start.py [--out profiles/rNN/rig_start.jsonl] [--reps 7] [CxFxM ...]     (default: 4x400x300 8x2000x500)

Times are host clocks around calls that end in a device synchronise (estimate_start reads its report back; solve waits for its
end), medians over --reps repetitions after one untimed warm-up call of each kind on a handle of the same shape. "start_ms" is
the whole call (view kernel, tree on the host, pose kernels, three small copies); "lm_iteration_ms" is the wall time of a solve
from the scenario's start divided by its iterations. Nothing exists to compare the start with: no figure is required of it."""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch  # noqa: F401
from camera_calibrator_amd import capi


def measure(C, F, M, reps):
    sc = capi.rig_scenario(C, F, M)
    cq, ct = capi.affine_to_qt(sc["cam_T"]); fq, ft = capi.affine_to_qt(sc["frame_T"])
    o = capi.default_options(max_iterations=1000)
    make = lambda: capi.RigProblem(C, sc["frame_offsets"], sc["obs_cam"], sc["obs_world"], sc["obs_uv"], sc["world_xyz"], sc["cam_frozen"])
    start_ms, start0_ms, solve_ms, its_given, its_start, cost_given, cost_start, cost0 = [], [], [], [], [], [], [], []
    rep = None
    for r in range(reps + 1):
        p = make()
        p.set_state(cq, ct, fq, ft)
        t0 = time.perf_counter(); s = p.solve(o, log_capacity=0); t1 = time.perf_counter()
        t2 = time.perf_counter(); p.estimate_start(cq, ct, refine_iterations=0); t3 = time.perf_counter()
        t4 = time.perf_counter(); rep = p.estimate_start(cq, ct); t5 = time.perf_counter()
        c0 = p.eval()
        s2 = p.solve(o, log_capacity=0)
        p.close()
        if r == 0:
            continue   # warm-up: code objects, pools
        solve_ms.append((t1 - t0) * 1e3 / max(1, s["iterations"])); start0_ms.append((t3 - t2) * 1e3); start_ms.append((t5 - t4) * 1e3)
        its_given.append(s["iterations"]); its_start.append(s2["iterations"])
        cost_given.append(s["final_cost"]); cost_start.append(s2["final_cost"]); cost0.append(c0)
    med = statistics.median
    return dict(shape=f"{C}x{F}x{M}", observations=int(sc["frame_offsets"][-1]), views=int(rep["views_valid"]), reps=reps,
                start_ms=round(med(start_ms), 3), start_ms_min_max=[round(min(start_ms), 3), round(max(start_ms), 3)],
                start_closed_form_only_ms=round(med(start0_ms), 3), lm_iteration_ms=round(med(solve_ms), 4),
                iterations_from_scenario_start=int(med(its_given)), iterations_from_computed_start=int(med(its_start)),
                initial_cost_scenario_start=float(s["initial_cost"]), initial_cost_computed_start=float(med(cost0)),
                final_cost_scenario_start=float(med(cost_given)), final_cost_computed_start=float(med(cost_start)),
                cameras_unplaced=int(rep["cameras_unplaced"]), frames_unplaced=int(rep["frames_unplaced"]), views_invalid=int(rep["views_invalid"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("shapes", nargs="*", default=["4x400x300", "8x2000x500"])
    a = ap.parse_args()
    if capi.device_count() < 1:
        raise SystemExit("needs a GPU: a time taken anywhere else says nothing")
    lines = [json.dumps(measure(*map(int, s.split("x")), a.reps)) for s in a.shapes]
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
