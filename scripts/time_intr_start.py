"""The fisheye focal-length start (cc_intrinsics_estimate_start_fisheye) at its defaults next to Zhang's start (cc_zhang_init) on the
same pixels, and the one-shot estimate from either start. Boards round a fisheye lens, one JSON line per shape:

    python scripts/time_intr_start.py [--out profiles/rNN/intr_start_fisheye.jsonl] [--reps 7] [FxM ...]      (default: 12x49 200x200 1000x500)

The method of scripts/time_rigk_start.py: host clocks around calls that end in a device synchronise, medians over --reps FRESH
handles after one untimed warm-up -- a handle's first start allocates its scratch, which is what a caller pays. The start's split
into extent, search (with the pick) and pose pass is the device time between hipEvents on the handle's stream, taken in a second
start of the same handle that asks for them (cc_intrinsics_debug_start_marks, then cc_last_call_timing): the timed call records
none. cc_zhang_init is a call of its own that uploads the observations itself; the focal-length start runs on a handle that holds
them, so the handle's creation is timed next to it. The one-shot calls (capi.intrinsics_estimate,
model fisheye, default options) include everything for both starts: upload, start, solve, read-back.
The scene is tests/intr_start_ref's: F boards of M points (the first M of the smallest square grid that has them, half-size 0.3 m)
about 0.4 m from a lens with fx 620, fy 615, k = -0.035 0.004 -0.0009 0.0001, their centres up to 85 degrees off the axis, 0.3 px
noise."""
import argparse, ctypes as C, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from camera_calibrator_amd import capi
from tests import fisheye_ref as fr
from tests import intr_start_ref as ref


def last_timing():
    tm = (C.c_double * 5)()
    capi.lib().cc_last_call_timing(tm)
    return list(tm)


def measure(shape, reps):
    F, M = (int(v) for v in shape.split("x"))
    c = ref._scene([fr._board(M, 0.3)] * F, 0.40, 85.0, 2, 0.3)
    off, uv, xyz = c["off"], c["uv"], c["xyz"]
    med = statistics.median
    rows = dict(create=[], start=[], extent=[], search=[], pose=[], zhang=[], est_zhang=[], est_focal=[])
    rep = ez = ef = None
    for r in range(reps + 1):
        t0 = time.perf_counter()
        p = capi.IntrinsicsProblem(off, uv, xyz)
        p.set_model(capi.MODEL_FISHEYE)
        t1 = time.perf_counter()
        intr, q, t, rep = p.estimate_start_fisheye()
        t2 = time.perf_counter()
        capi._check(capi.lib().cc_intrinsics_debug_start_marks(p._h, C.c_int32(1)))   # a second start of the same handle, with events: the split
        p.estimate_start_fisheye()
        tm = last_timing()
        p.close()
        t3 = time.perf_counter()
        K, qz, tz = capi.zhang_init(off, uv, xyz)
        t4 = time.perf_counter()
        ez = capi.intrinsics_estimate(off, uv, xyz, model=capi.MODEL_FISHEYE, log_capacity=1)
        t5 = time.perf_counter()
        ef = capi.intrinsics_estimate(off, uv, xyz, model=capi.MODEL_FISHEYE, start="fisheye", log_capacity=1)
        t6 = time.perf_counter()
        if r == 0:
            continue   # warm-up: code objects, pools
        for k, v in (("create", t1 - t0), ("start", t2 - t1), ("zhang", t4 - t3), ("est_zhang", t5 - t4), ("est_focal", t6 - t5)):
            rows[k].append(v * 1e3)
        for k, v in (("extent", tm[0]), ("search", tm[1]), ("pose", tm[2])):
            rows[k].append(v)
    m = {k: round(med(v), 3) for k, v in rows.items()}
    return dict(shape=shape, model="fisheye", views=F, observations=int(off[-1]), reps=reps, largest_angle_deg=round(c["max_angle_deg"], 1),
                beyond_90=round(c["beyond_90"], 3), candidates=24, views_searched=int(rep["views_searched"]), focal=round(rep["focal"], 2),
                best_candidate=int(rep["best_candidate"]), candidates_qualified=int(rep["candidates_qualified"]), views_invalid=int(rep["views_invalid"]),
                focal_start_ms=m["start"], focal_start_ms_min_max=[round(min(rows["start"]), 3), round(max(rows["start"]), 3)],
                device_extent_ms=m["extent"], device_search_and_pick_ms=m["search"], device_pose_pass_ms=m["pose"], handle_create_ms=m["create"],
                zhang_init_ms=m["zhang"], zhang_init_ms_min_max=[round(min(rows["zhang"]), 3), round(max(rows["zhang"]), 3)], zhang_fx=round(float(K[0, 0]), 1),
                estimate_zhang_ms=m["est_zhang"], estimate_zhang_iterations=ez[4]["iterations"], estimate_zhang_final_cost=float(ez[4]["final_cost"]),
                estimate_zhang_termination=ez[4]["termination"], estimate_zhang_fx=round(float(ez[1][0]), 2),
                estimate_focal_ms=m["est_focal"], estimate_focal_iterations=ef[4]["iterations"], estimate_focal_final_cost=float(ef[4]["final_cost"]),
                estimate_focal_termination=ef[4]["termination"], estimate_focal_fx=round(float(ef[1][0]), 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("shapes", nargs="*", default=["12x49", "200x200", "1000x500"])
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
