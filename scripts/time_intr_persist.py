"""Where a round of the persistent intrinsics kernel goes: wall-clock marks (100 MHz, one counter for the chip) left in
round CC_PERSIST_TIMING_ROUND by a worker workgroup (the middle one, or the middle one of the column owners) and by the control workgroup of a timing-only build
(scripts/build_variant.sh ptime cc_intrinsics_persist.hip --patch timing -DCC_PERSIST_TIMING; CC_LIB_PATH=scripts/ablate_build/libcc_ptime.so).
Env F, M. Microseconds, median over solves; `t` = time since the worker's round start.
The END of the solve (third line): the control's marks from the decision that ends the solve to the sequence word, the marked worker's and
every worker's leaving time, all since that decision; and the host's own clock from its stamp in front of the launch (taken by the timing
build's persist_launch) to the return of the solve call, i.e. of the wait for the publication."""
import ctypes as C, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch  # noqa: F401
from camera_calibrator_amd import capi

F, M = int(os.environ.get("F", 1000)), int(os.environ.get("M", 500))
off, uv, xyz = capi.make_intrinsics_problem(F, M)
K0, q0, t0 = capi.zhang_init(off, uv, xyz)
intr0 = np.array([K0[0, 0], K0[1, 1], K0[0, 2], K0[1, 2], 0, 0, 0, 0, 0], dtype=np.float64)
prob = capi.IntrinsicsProblem(off, uv, xyz)
prob.set_state(intr0, q0.astype(np.float64), t0.astype(np.float64))
rows, skews, ends, leaves, host_us = [], [], [], [], []
G = None
opts = capi.default_options(max_iterations=6, function_tolerance=0.0, parameter_tolerance=0.0, gradient_tolerance=0.0)
launch_ns = getattr(capi.lib(), "cc_persist_timing_launch_ns", None)   # (timing builds only)
if launch_ns is not None:
    launch_ns.restype = C.c_longlong
for _ in range(15):
    prob.reset()
    prob.solve_lean(opts)
    t_ret = time.clock_gettime_ns(time.CLOCK_MONOTONIC)
    if launch_ns is not None:
        host_us.append((t_ret - launch_ns()) / 1000.0)
    buf = np.zeros(48)
    capi._check(capi.lib().cc_intrinsics_debug_fetch(prob._h, b"vec_solve", buf.ctypes.data_as(C.POINTER(C.c_double)), C.c_int64(48)))
    rows.append((buf[:32] - buf[0]) / 100.0)
    ends.append((buf[32:48] - buf[32]) / 100.0)
    teams = int(os.environ.get("CC_INTR_PERSIST_TEAMS", 0)) or (1 if F + 1 <= 256 else 2 if (F + 1) // 2 + 1 <= 256 else 4)
    G = (F + teams - 1) // teams
    st = np.zeros(G * 4)
    capi._check(capi.lib().cc_intrinsics_debug_fetch(prob._h, b"stats", st.ctypes.data_as(C.POINTER(C.c_double)), C.c_int64(G * 4)))
    skews.append((st.reshape(G, 4) - buf[0]) / 100.0)
    if teams >= 2:   # every worker workgroup's leaving time, behind the four marks per workgroup
        lv = np.zeros(G * 5)
        capi._check(capi.lib().cc_intrinsics_debug_fetch(prob._h, b"stats", lv.ctypes.data_as(C.POINTER(C.c_double)), C.c_int64(G * 5)))
        leaves.append((lv[G * 4:] - buf[32]) / 100.0)
prob.close()
t = np.median(np.array(rows), axis=0)
wn = ["round start", "pose step + Plus done", "main loop starts", "main loop done (this wave)", "all waves done", "block reduced, statistics",
      "statistics row stored", "assumed elimination + row (+ owner's sum) done", "elimination done", "elimination row stored",
      "broadcast received (step if the assumption held)", "owner: has its column", "after a miss: step received",
      "elimination: 6x6 factor done", "elimination: substitutions done", "broadcast: the poll set that matched was issued"]
cn = ["waits for statistics rows", "rows gathered", "decision taken", "decision stored / skipped", "control has the totals", "solve done", "step stored",
      "solve: gradient maximum", "solve: rows built", "solve: factorisation + substitutions", "solve: tests, log record, flags"]
sk = np.median(np.array(skews), axis=0)     # [G][4]: round start, statistics stored, elimination row stored, broadcast received
names = ["round start", "statistics stored", "elimination row stored", "broadcast received"]
print(json.dumps({"frames": F, "pts": M, "workgroups": G, "per_workgroup_marks_us": {n: {"min": round(float(sk[:, i].min()), 2), "median": round(float(np.median(sk[:, i])), 2),
      "max": round(float(sk[:, i].max()), 2)} for i, n in enumerate(names)}}))
print(json.dumps({"frames": F, "pts": M, "round_us": round(float(max(t[10], t[12])), 2),
                  "worker": {**{n: round(float(t[i]), 2) for i, n in enumerate(wn) if t[i] > -1e6}, "owner: total stored": round(float(t[27]), 2)},
                  "control": {n: round(float(t[16 + i]), 2) for i, n in enumerate(cn)}}))
e = np.median(np.array(ends), axis=0)
en = {0: "ending decision taken", 1: "broadcast stored", 2: "the end's code begins", 3: "failure word read", 4: "publication: first word stored",
      5: "sequence word stored", 6: "(one-thread form) counter read, payload acknowledged", 8: "marked worker: saw done", 9: "marked worker: pose stored / leaving"}
end = {"frames": F, "pts": M, "end_us_since_decision": {n: round(float(e[i]), 2) for i, n in en.items() if e[i] > -1e6}}
if leaves:
    lv = np.median(np.array(leaves), axis=0)
    end["workers_leave_us_since_decision"] = {"min": round(float(lv.min()), 2), "median": round(float(np.median(lv)), 2), "max": round(float(lv.max()), 2)}
    end["sequence_word_to_last_worker_us"] = round(float(lv.max() - e[5]), 2)
if host_us:
    end["host_launch_to_wait_returns_us"] = {"min": round(min(host_us), 2), "median": round(float(np.median(host_us)), 2)}
print(json.dumps(end))
