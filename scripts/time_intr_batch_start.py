"""The batched fisheye focal-length start (cc_intrinsics_batch_estimate_start_fisheye) next to the same problems through the single
handle one after another, and next to the batch's Zhang start. Boards round a fisheye lens, one JSON line per shape:

    python scripts/time_intr_batch_start.py [--out profiles/rNN/intr_batch_start.jsonl] [--reps 7] [BxFxM ...]   (default: 8x12x49 64x12x49 8x200x200)

The method of scripts/time_intr_start.py and scripts/time_intr_batch.py: host clocks round calls that end in a device synchronise,
medians over --reps runs on FRESH handles after one untimed warm-up (a handle's first start allocates its scratch, which is what a
caller pays), the forms alternating within a run. Per run, in this order:
  (a) batch_start      IntrinsicsBatch.estimate_start_fisheye on a fresh batch handle (its creation timed next to it);
  (b) single_starts    IntrinsicsProblem.estimate_start_fisheye on B fresh single handles one after another -- the baseline, the
                       path a caller had before the batch had the start (the B creations timed next to it);
  (c) the batch's Zhang start has no entry point of its own: it runs inside cc_intrinsics_batch_estimate_model. It is measured as
      the one-shot estimate cut off after ONE iteration (upload, start, initial evaluation, one round, read-back) from Zhang,
      next to the same cut-off one-shot from the search: est1_zhang / est1_focal. Their difference is the difference of the starts.
  and the full one-shot estimate at the default options from either start, with every problem's iterations and final costs.
`a_beats_b_disjoint`: every run of (a) is faster than every run of (b). The scene is scripts/time_intr_start.py's, problem b with
seed 2 + b: F boards of M points about 0.4 m from the lens, their centres up to 85 degrees off the axis, 0.3 px noise."""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from camera_calibrator_amd import capi
from tests import fisheye_ref as fr
from tests import intr_start_ref as ref

FISH = capi.MODEL_FISHEYE


def measure(shape, reps):
    B, F, M = (int(v) for v in shape.split("x"))
    scenes = [ref._scene([fr._board(M, 0.3)] * F, 0.40, 85.0, 2 + b, 0.3) for b in range(B)]
    problems = [(c["off"], c["uv"], c["xyz"]) for c in scenes]
    one_round = capi.default_options(max_iterations=1)
    rows = dict(batch_create=[], batch_start=[], single_create=[], single_starts=[], est1_zhang=[], est1_focal=[], est_zhang=[], est_focal=[])
    got = singles = ez = ef = None
    for r in range(reps + 1):
        t0 = time.perf_counter()
        h = capi.IntrinsicsBatch(problems)
        h.set_model(FISH)
        t1 = time.perf_counter()
        got = h.estimate_start_fisheye()
        t2 = time.perf_counter()
        h.close()
        t3 = time.perf_counter()
        ps = [capi.IntrinsicsProblem(*p) for p in problems]
        for p in ps:
            p.set_model(FISH)
        t4 = time.perf_counter()
        singles = [p.estimate_start_fisheye() for p in ps]
        t5 = time.perf_counter()
        for p in ps:
            p.close()
        t6 = time.perf_counter()
        zhang_error = None   # (Zhang's pinhole K may not exist on boards round a wide lens: the call then refuses, which is reported)
        try:
            capi.intrinsics_batch_estimate(problems, model=FISH, options=one_round, log_capacity=1)
        except capi.CcError as e:
            zhang_error = str(e)
        t7 = time.perf_counter()
        capi.intrinsics_batch_estimate(problems, model=FISH, start="fisheye", options=one_round, log_capacity=1)
        t8 = time.perf_counter()
        try:
            ez = capi.intrinsics_batch_estimate(problems, model=FISH, log_capacity=1)
        except capi.CcError as e:
            zhang_error = str(e)
        t9 = time.perf_counter()
        ef = capi.intrinsics_batch_estimate(problems, model=FISH, start="fisheye", log_capacity=1)
        t10 = time.perf_counter()
        if r == 0:
            continue   # warm-up: code objects, pools
        for k, v in (("batch_create", t1 - t0), ("batch_start", t2 - t1), ("single_create", t4 - t3), ("single_starts", t5 - t4), ("est1_zhang", t7 - t6),
                     ("est1_focal", t8 - t7), ("est_zhang", t9 - t8), ("est_focal", t10 - t9)):
            rows[k].append(v * 1e3)
    m = {k: round(statistics.median(v), 3) for k, v in rows.items()}
    span = lambda k: [round(min(rows[k]), 3), round(max(rows[k]), 3)]
    same = all(np.array_equal(got[0][b], singles[b][0]) and got[3][b] == singles[b][3] for b in range(B))
    off = np.cumsum([0] + [F] * B)
    same_poses = all(np.array_equal(got[1][off[b]:off[b + 1]], singles[b][1]) and np.array_equal(got[2][off[b]:off[b + 1]], singles[b][2]) for b in range(B))
    return dict(shape=shape, model="fisheye", problems=B, views=B * F, observations=B * F * M, reps=reps, candidates=24,
                views_searched=[int(x["views_searched"]) for x in got[3]], focal=[round(x["focal"], 2) for x in got[3]],
                views_invalid=sum(int(x["views_invalid"]) for x in got[3]), reports_and_intr_equal_single=bool(same), poses_bit_equal_single=bool(same_poses),
                batch_start_ms=m["batch_start"], batch_start_ms_min_max=span("batch_start"), batch_create_ms=m["batch_create"],
                single_starts_ms=m["single_starts"], single_starts_ms_min_max=span("single_starts"), single_create_ms=m["single_create"],
                a_beats_b_disjoint=bool(max(rows["batch_start"]) < min(rows["single_starts"])),
                est1_zhang_ms=m["est1_zhang"], est1_zhang_ms_min_max=span("est1_zhang"), est1_focal_ms=m["est1_focal"], est1_focal_ms_min_max=span("est1_focal"),
                estimate_zhang_ms=m["est_zhang"], estimate_zhang_ms_min_max=span("est_zhang"), estimate_zhang_error=zhang_error,
                estimate_zhang_iterations=[s["iterations"] for s in ez[4]] if ez else None,
                estimate_zhang_final_cost=[float(s["final_cost"]) for s in ez[4]] if ez else None,
                estimate_zhang_fx=[round(float(k[0]), 2) for k in ez[1]] if ez else None,
                estimate_focal_ms=m["est_focal"], estimate_focal_ms_min_max=span("est_focal"), estimate_focal_iterations=[s["iterations"] for s in ef[4]],
                estimate_focal_final_cost=[float(s["final_cost"]) for s in ef[4]], estimate_focal_fx=[round(float(k[0]), 2) for k in ef[1]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("shapes", nargs="*", default=["8x12x49", "64x12x49", "8x200x200"])
    a = ap.parse_args()
    if capi.device_count() < 1:
        raise SystemExit("needs a GPU: a time taken anywhere else says nothing")
    for s in a.shapes:
        line = json.dumps(measure(s, a.reps))
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
