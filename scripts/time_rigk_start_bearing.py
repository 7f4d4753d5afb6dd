"""The bearing form of the pixel start (cc_rigk_estimate_start_bearing) next to the x / z pixel start (cc_rigk_estimate_start, whose
kernels keep their text) on the same fisheye scenes, each with and without the refinement, so that the difference splits into
closed form and refinement; and the bearing start alone on a scene the x / z form cannot take. One JSON line per shape:

    python scripts/time_rigk_start_bearing.py [--out profiles/rNN/rigk_start_bearing.jsonl] [--reps 7] [CxFxM[pc][w] ...]
                (default: 4x400x300 4x400x300pc 8x2000x500 8x2000x500pc 4x400x300w; pc: one set of intrinsics per camera;
                 w: the world's x, y stretched to +-3 m and z to +-1 m, points beyond 90 degrees -- bearing start only)

The method of scripts/time_rigk_start.py: host clocks around calls that end in a device synchronise (a start reads its report back),
medians over --reps FRESH handles after one untimed warm-up handle of each kind -- a handle's first start allocates its buffers,
which is what a caller pays. The scene and the start intrinsics are that script's."""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import numpy as np
from camera_calibrator_amd import capi
from camera_calibrator_amd.harness import rigk_case
from time_rigk_fisheye import FISH_INTR, fisheye_pixels, parse_shape


def measure(shape, reps):
    wide = shape.endswith("w")
    C, F, M, pc = parse_shape(shape[:-1] if wide else shape)
    k = dict(rigk_case(C, F, M, per_camera=pc))
    if wide:
        world = k["world_xyz"].astype(np.float64)
        world[:, :2] *= 3.0 / 0.2
        world[:, 2] *= 1.0 / 0.2
        k["world_xyz"] = world.astype(np.float32)
    K = np.tile(FISH_INTR, (C, 1))
    if pc:
        K[:, :2] *= np.atleast_2d(k["intr_true"])[:, :2] / 1000.0
    uv = fisheye_pixels(k, K)
    intr0 = np.atleast_2d(k["intr0"])

    def handle():
        p = capi.RigProblem(C, k["frame_offsets"], k["obs_cam"], k["obs_world"], uv, k["world_xyz"], k["cam_frozen"], huber_a=0.0,
                            with_intrinsics="per_camera" if pc else True)
        p.set_model(capi.MODEL_FISHEYE)
        if pc:
            for c in range(C):
                p.set_camera_intrinsics(c, intr0[c], 0)
        else:
            p.set_intrinsics(intr0[0], 0)
        return p

    kinds = [("bearing", 10), ("bearing", 0)] + ([] if wide else [("pinhole", 10), ("pinhole", 0)])
    ms, reports, bad = {kd: [] for kd in kinds}, {}, {}
    for r in range(reps + 1):
        for kd in kinds:
            p = handle()
            call = p.estimate_start_bearings if kd[0] == "bearing" else p.estimate_start_pixels
            t0 = time.perf_counter(); rep = call(k["cam_q0"], k["cam_t0"], refine_iterations=kd[1]); t1 = time.perf_counter()
            if r == reps:
                reports[kd] = rep
                bad[kd] = (p.start_bearings() if kd[0] == "bearing" else p.start_points())[1]
                if kd == ("bearing", 10):
                    beyond = float((p.start_bearings()[0][:, 2] < 0).mean())
                    cost0 = float(p.eval())
                    s = p.solve(capi.default_options(max_iterations=1000), log_capacity=0)
            p.close()
            if r > 0:   # (r = 0: warm-up -- code objects, pools)
                ms[kd].append((t1 - t0) * 1e3)
    med = {kd: statistics.median(v) for kd, v in ms.items()}
    out = dict(shape=shape, model="fisheye", per_camera=pc, observations=int(k["frame_offsets"][-1]), views=int(C * F), reps=reps,
               bearing_start_ms=round(med[("bearing", 10)], 3), bearing_start_ms_min_max=[round(min(ms[("bearing", 10)]), 3), round(max(ms[("bearing", 10)]), 3)],
               bearing_start_no_refinement_ms=round(med[("bearing", 0)], 3),
               bearing_refinement_ms=round(med[("bearing", 10)] - med[("bearing", 0)], 3),
               bearings_beyond_90_share=round(beyond, 4), bearings_without_root=int(bad[("bearing", 10)]),
               bearing_views_invalid=int(reports[("bearing", 10)]["views_invalid"]), initial_cost_bearing_start=cost0,
               iterations_from_bearing_start=s["iterations"], final_cost_bearing_start=float(s["final_cost"]), termination_bearing_start=s["termination"])
    if not wide:
        out.update(pinhole_start_ms=round(med[("pinhole", 10)], 3), pinhole_start_ms_min_max=[round(min(ms[("pinhole", 10)]), 3), round(max(ms[("pinhole", 10)]), 3)],
                   pinhole_start_no_refinement_ms=round(med[("pinhole", 0)], 3), pinhole_refinement_ms=round(med[("pinhole", 10)] - med[("pinhole", 0)], 3),
                   bearing_over_pinhole=round(med[("bearing", 10)] / med[("pinhole", 10)], 3), pinhole_views_invalid=int(reports[("pinhole", 10)]["views_invalid"]),
                   points_without_root=int(bad[("pinhole", 10)]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("shapes", nargs="*", default=["4x400x300", "4x400x300pc", "8x2000x500", "8x2000x500pc", "4x400x300w"])
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
