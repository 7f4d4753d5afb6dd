"""The pixel start of a rig handle with intrinsics (cc_rigk_estimate_start) next to the poses-only start (cc_rig_estimate_start) on
the very points it computed -- the difference is the unproject pass, k_rigk_start_unproject -- and the solve's iterations and
final cost from the computed start against the scenario's start. Fisheye handles, one JSON line per shape:

    python scripts/time_rigk_start.py [--out profiles/rNN/rigk_start.jsonl] [--reps 7] [CxFxM[pc] ...]
                                      (default: 4x400x300 4x400x300pc 8x2000x500 8x2000x500pc; pc: one set of intrinsics per camera)

The method of scripts/time_rig_start.py: host clocks around calls that end in a device synchronise (both starts read their report
back), medians over --reps FRESH handles after one untimed warm-up handle of each kind -- a handle's first start allocates its
buffers, which is what a caller pays. The scene is scripts/time_rigk_fisheye.py's: camera_calibrator_amd.harness.rigk_case's rig
seen through a fisheye lens (fx = fy = 1000, k = -0.035 0.004 -0.0009 0.0001, 0.3 px noise); start intrinsics: rigk_case's intr0
(focal lengths 2 % off, principal point 5 px off, no distortion). The twin is a cc_rig_create handle whose observations are
cc_rigk_start_points of the pixel handle. The two solves (default options) run once per shape: they are deterministic."""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import numpy as np
from camera_calibrator_amd import capi
from camera_calibrator_amd.harness import rigk_case
from time_rigk_fisheye import FISH_INTR, fisheye_pixels, parse_shape


def measure(shape, reps):
    C, F, M, pc = parse_shape(shape)
    k = rigk_case(C, F, M, per_camera=pc)
    K = np.tile(FISH_INTR, (C, 1))
    if pc:
        K[:, :2] *= np.atleast_2d(k["intr_true"])[:, :2] / 1000.0
    uv = fisheye_pixels(k, K)
    intr0 = np.atleast_2d(k["intr0"])

    def pixel_handle():
        p = capi.RigProblem(C, k["frame_offsets"], k["obs_cam"], k["obs_world"], uv, k["world_xyz"], k["cam_frozen"], huber_a=0.0,
                            with_intrinsics="per_camera" if pc else True)
        p.set_model(capi.MODEL_FISHEYE)
        if pc:
            for c in range(C):
                p.set_camera_intrinsics(c, intr0[c], 0)
        else:
            p.set_intrinsics(intr0[0], 0)
        return p

    o = capi.default_options(max_iterations=1000)
    pixel_ms, twin_ms, solves, rep, bad = [], [], None, None, 0
    for r in range(reps + 1):
        p = pixel_handle()
        t0 = time.perf_counter(); rep = p.estimate_start_pixels(k["cam_q0"], k["cam_t0"]); t1 = time.perf_counter()
        pts, bad = p.start_points()
        if r == 1:
            c0 = p.eval()
            a = p.solve(o, log_capacity=0)
            p.set_state(k["cam_q0"], k["cam_t0"], k["frame_q0"], k["frame_t0"])
            b = p.solve(o, log_capacity=0)
            solves = dict(iterations_from_computed_start=a["iterations"], iterations_from_scenario_start=b["iterations"],
                          initial_cost_computed_start=float(c0), initial_cost_scenario_start=float(b["initial_cost"]),
                          final_cost_computed_start=float(a["final_cost"]), final_cost_scenario_start=float(b["final_cost"]),
                          termination_computed_start=a["termination"], termination_scenario_start=b["termination"])
        p.close()
        twin = capi.RigProblem(C, k["frame_offsets"], k["obs_cam"], k["obs_world"], pts, k["world_xyz"], k["cam_frozen"])
        t2 = time.perf_counter(); trep = twin.estimate_start(k["cam_q0"], k["cam_t0"]); t3 = time.perf_counter()
        twin.close()
        assert trep["views_valid"] == rep["views_valid"]
        if r == 0:
            continue   # warm-up: code objects, pools
        pixel_ms.append((t1 - t0) * 1e3); twin_ms.append((t3 - t2) * 1e3)
    med = statistics.median
    return dict(shape=shape, model="fisheye", per_camera=pc, observations=int(k["frame_offsets"][-1]), views=int(rep["views_valid"]), reps=reps,
                pixel_start_ms=round(med(pixel_ms), 3), pixel_start_ms_min_max=[round(min(pixel_ms), 3), round(max(pixel_ms), 3)],
                poses_only_twin_start_ms=round(med(twin_ms), 3), poses_only_twin_start_ms_min_max=[round(min(twin_ms), 3), round(max(twin_ms), 3)],
                unproject_pass_ms=round(med(pixel_ms) - med(twin_ms), 3), unproject_share=round(1 - med(twin_ms) / med(pixel_ms), 3),
                points_without_root=int(bad), views_invalid=int(rep["views_invalid"]), cameras_unplaced=int(rep["cameras_unplaced"]),
                frames_unplaced=int(rep["frames_unplaced"]), **solves)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("shapes", nargs="*", default=["4x400x300", "4x400x300pc", "8x2000x500", "8x2000x500pc"])
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
