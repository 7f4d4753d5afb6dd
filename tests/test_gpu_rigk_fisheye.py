"""EXTENSION: the fisheye (Kannala-Brandt) camera model of the rig solve with intrinsics (cc_rigk_set_model; the kernels:
cc_rig_lens.hip). The checker is tests/rigk_fisheye_ref.py: the rig-with-intrinsics LM restated in numpy with a pluggable pixel
model, itself pinned on the CPU (tests/test_rigk_fisheye_cpu.py) against the oracle, the 50-digit model and scipy.

Bounds (the project's standing ones for this path): identical termination, iteration count, accept / valid sequence; logged
costs 1e-9 relative; fx fy px py 1e-9 relative, k1..k4 and poses 1e-9; per-observation costs 1e-8 relative with atol 1e-12; the
total cost of one evaluation 1e-12 relative; a group's 16 x 16 Gram 1e-12 of its largest entry. Every test prints what it
measured (DESIGN.md 4.14 has the table)."""
import ctypes as C
import os

import numpy as np
import pytest

from camera_calibrator_amd import capi
from camera_calibrator_amd.harness import rigk_case
from tests import rigk_fisheye_ref as rr

pytestmark = pytest.mark.gpu


def _problem(k, per_camera=False, const_masks=None, huber_a=0.0, model=capi.MODEL_FISHEYE):
    prob = capi.RigProblem(k["cams"], k["frame_offsets"], k["obs_cam"], k["obs_world"], k["obs_uv_pix"], k["world_xyz"], k["cam_frozen"],
                           huber_a=huber_a, with_intrinsics="per_camera" if per_camera else True)
    if model is not None:
        prob.set_model(model)
    _set_intrinsics(prob, k, per_camera, const_masks)
    prob.set_state(k["cam_q0"], k["cam_t0"], k["frame_q0"], k["frame_t0"])
    return prob


def _set_intrinsics(prob, k, per_camera, const_masks, intr=None):
    intr = k["intr0"] if intr is None else intr
    if per_camera:
        for c in range(k["cams"]):
            prob.set_camera_intrinsics(c, intr[c], 0 if const_masks is None else int(const_masks[c]))
    else:
        prob.set_intrinsics(intr, 0 if const_masks is None else int(const_masks))


def _state(prob, per_camera, summary):
    return ((prob.get_camera_intrinsics() if per_camera else prob.get_intrinsics()),) + tuple(prob.get_state()) + (summary,)


def _gpu(name):
    k, pk, ok = rr.gpu_case(name)
    prob = _problem(k, **pk)
    s = prob.solve(capi.default_options(**ok))
    g = _state(prob, pk.get("per_camera", False), s)
    prob.close()
    return k, g


def _assert_same(g, o, what):
    sg, so = g[6], o[6]
    assert sg["termination"] == so["termination"] and sg["iterations"] == so["iterations"], (sg["termination"], sg["iterations"], so["termination"], so["iterations"])
    assert [l["accepted"] for l in sg["log"]] == [l["accepted"] for l in so["log"]]
    assert [l["valid"] for l in sg["log"]] == [l["valid"] for l in so["log"]]
    gi, oi = np.atleast_2d(g[0]), np.atleast_2d(o[0])
    dev = dict(costs=max(abs(a["cost"] / b["cost"] - 1) for a, b in zip(sg["log"], so["log"])),
               focal=np.abs(gi[:, :4] / oi[:, :4] - 1).max(), dist=np.abs(gi[:, 4:] - oi[:, 4:]).max(),
               poses=max(np.abs(g[a] - o[a]).max() for a in range(1, 5)),
               obs=(np.abs(g[5] - o[5]) / np.maximum(np.abs(o[5]), 1e-4)).max())
    print("%s measured: " % what + ", ".join("%s %.2g" % kv for kv in dev.items()))
    assert dev["costs"] <= 1e-9 and dev["focal"] <= 1e-9 and dev["dist"] <= 1e-9 and dev["poses"] <= 1e-9
    assert np.allclose(g[5], o[5], rtol=1e-8, atol=1e-12)
    return dev


def _fetch(prob, name, n):
    buf = np.zeros(n)
    capi._check(capi.lib().cc_rig_debug_fetch(prob._h, name.encode(), buf.ctypes.data_as(C.POINTER(C.c_double)), C.c_int64(n)))
    return buf


def _groups(k):
    """(frame, camera, caller's observation indices) of every group, in the handle's order (frame-major, camera-minor)."""
    off, cam = np.asarray(k["frame_offsets"]), np.asarray(k["obs_cam"])
    out = []
    for f in range(len(off) - 1):
        for c in np.unique(cam[off[f]:off[f + 1]]):
            out.append((f, int(c), np.nonzero(cam[off[f]:off[f + 1]] == c)[0] + off[f]))
    return out


GRAM = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rigk_fisheye_gram.npz"))


def _assert_gram(prob, k, picks, key, what):
    """The 16 x 16 Gram of X = [J_cam(6) r J_k(9)] the sweep left for the starting point (the compact record's first 256 doubles)
    against the np.longdouble Gram of the 50-digit rows (tests/golden/make_rigk_fisheye_gram.py), 1e-12 of its largest entry."""
    groups = _groups(k)
    rec = _fetch(prob, "gcomp", len(groups) * 320).reshape(len(groups), 320)
    for gi in picks:
        sfx = "_%d" % gi if len(groups) > 1 else ""
        want, uv = GRAM[key + "_gram" + sfx], GRAM[key + "_uv" + sfx]
        assert np.array_equal(uv, k["obs_uv_pix"][groups[gi][2]])          # the fixture belongs to this scenario
        got = rec[gi, :256].reshape(16, 16)
        dev = np.abs(got - want).max() / np.abs(want).max()
        print("%s group %d (%d observations): Gram deviation / largest entry %.2g" % (what, gi, len(uv), dev))
        assert np.all(np.isfinite(got)) and dev <= 1e-12, (gi, dev)
        assert np.array_equal(got[15], np.zeros(16)) and np.array_equal(got[:, 15], np.zeros(16))   # slot 8 has no column


def test_shared_set_one_pass_one_wave_and_its_properties():
    """2 x 12 x 20: one pass of the one-wave form (20 observations per group). Then the properties: the frozen camera untouched,
    the per-observation costs add up to the final cost, a second solve from the solution is a fixed point, reset + solve
    reproduces the first solve bit for bit."""
    k, pk, ok = rr.gpu_case("shared")
    prob = _problem(k)
    assert prob.get_model() == capi.MODEL_FISHEYE
    s1 = prob.solve(capi.default_options(**ok))
    g = _state(prob, False, s1)
    _assert_same(g, rr.gpu_reference("shared"), "shared")
    assert np.array_equal(g[1][0], k["cam_q0"][0]) and np.array_equal(g[2][0], k["cam_t0"][0])
    assert np.isclose(g[5].sum(), s1["final_cost"], rtol=1e-9) and g[0][8] == 0.0
    form, _, _ = prob.solver_status()
    assert form == 0
    prob.reset()
    s1b = prob.solve(capi.default_options(**ok))
    gb = _state(prob, False, s1b)
    for a in range(6):
        assert np.array_equal(g[a], gb[a])
    assert [(l["cost"], l["accepted"]) for l in s1["log"]] == [(l["cost"], l["accepted"]) for l in s1b["log"]]
    prob.set_intrinsics(g[0], 0)
    prob.set_state(g[1], g[2], g[3], g[4])
    s2 = prob.solve(capi.default_options(**ok))
    prob.close()
    assert s2["iterations"] <= 2 and s2["final_cost"] <= s1["final_cost"] * (1 + 1e-9)


def test_ragged_groups_in_both_workgroup_forms(monkeypatch):
    """Two cameras x four frames with (frame, camera) groups of 1, 63, 64, 65, 257, 530, none and 130 observations (eight pairs:
    the six sizes, the empty pair and one more). Four waves by default: a pass is 256 observations, 530 gives the unrolled pair and
    the tail; one wave forced: 530 is nine passes of 64. Both match the reference; the Gram of the groups of 1, 65 and 530
    observations against the 50-digit rows."""
    k, pk, ok = rr.gpu_case("ragged")
    sizes = [len(i) for _, _, i in _groups(k)]
    assert sizes == [1, 63, 64, 65, 257, 530, 130]
    ref = rr.gpu_reference("ragged")
    out = {}
    for waves in (4, 1):
        monkeypatch.setenv("CC_RIG_SWEEP_WG_WAVES", str(waves))
        prob = _problem(k)
        s = prob.solve(capi.default_options(**ok))
        out[waves] = _state(prob, False, s)
        prob.close()
        _assert_same(out[waves], ref, "ragged, %d wave(s)" % waves)
        prob = _problem(k)
        prob.solve(capi.default_options(max_iterations=1))
        _assert_gram(prob, k, [0, 3, 5], "ragged", "ragged, %d wave(s)" % waves)
        prob.close()
    a, b = out[4], out[1]
    print("four waves against one: intrinsics %.2g, poses %.2g, final cost %.2g relative" % (
        np.abs(a[0] - b[0]).max(), max(np.abs(a[i] - b[i]).max() for i in range(1, 5)), abs(a[6]["final_cost"] / b[6]["final_cost"] - 1)))


def test_one_wave_form_by_group_count():
    """4 x 256 frames x 5 points: 1024 groups, so one wave per group; the last frame carries 140 points per camera: three passes."""
    k, g = _gpu("ng1024")
    assert len(_groups(k)) == 1024
    _assert_same(g, rr.gpu_reference("ng1024"), "ng1024")


def test_per_camera_sets_with_masks_and_the_loss():
    """3 x 20 x 25, a set per camera, masks [(k3, k4 held), none, (k4 held)], Huber 1.5 px with a tenth of the pixels displaced by
    5 - 30 px: observations in the linear tail at the minimiser. Held slots come back bit for bit, slot 8 is 0 everywhere."""
    k, g = _gpu("percam")
    o = rr.gpu_reference("percam")
    _assert_same(g, o, "percam")
    assert (np.sqrt(2 * o[5]) > 1.5).sum() > 50     # the tail is populated at the minimiser
    assert np.array_equal(g[0][0, 6:8], k["intr0"][0, 6:8]) and g[0][2, 7] == k["intr0"][2, 7]
    assert np.array_equal(g[0][:, 8], np.zeros(3))


def test_large_rig_kernels():
    """Ten cameras with sets of their own: 9 x 6 + 10 x 9 = 144 > 127 shared coordinates (k_rig_elim_big / k_rig_solve_big read
    the tiles)."""
    k, g = _gpu("big")
    _assert_same(g, rr.gpu_reference("big"), "big")


def test_the_axis():
    """Identity poses, camera 0, world points (0, 0, 1), (1e-9, 0, 1), (0, 1e-6, 1), (1e-3, 1e-3, 1), (0.1, 0, -0.5): cc_rig_eval
    and the per-observation costs are finite and the 50-digit values, the group's Gram is the 50-digit rows', and one LM
    iteration from there leaves every state entry finite."""
    k = rr.axis_case()
    prob = _problem(k)
    want = np.array([0.5 * (r @ r) for r in (rr.mp_rig_residual(k["intr0"], k["cam_q0"][0], k["cam_t0"][0], k["frame_q0"][0], k["frame_t0"][0],
                                                                k["world_xyz"][i].astype(np.float64), k["obs_uv_pix"][i].astype(np.float64), jacobian=False)[0]
                                             for i in range(5))])
    cost = prob.eval()
    oc = prob.get_state()[4]
    print("axis: total cost %.2g relative, per-observation costs %.2g relative" % (abs(cost / want.sum() - 1), np.abs(oc / want - 1).max()))
    assert np.all(np.isfinite(oc)) and np.isfinite(cost)
    assert abs(cost - want.sum()) <= 1e-12 * want.sum()
    assert np.allclose(oc, want, rtol=1e-8, atol=1e-12)
    s = prob.solve(capi.default_options(max_iterations=1))
    assert s["iterations"] == 1 and np.isfinite(s["final_cost"])
    _assert_gram(prob, k, [0], "axis", "axis")
    for a in (prob.get_intrinsics(),) + tuple(prob.get_state()):
        assert np.all(np.isfinite(a))
    prob.close()


def test_nothing_moved_for_the_old_model():
    """rigk_case(3, 20, 30): a handle that never calls set_model, one that calls it with MODEL_RADTAN, and one that went radtan ->
    fisheye -> radtan (set_intrinsics again) give the same bits in state, log and per-observation costs."""
    k = rigk_case(3, 20, 30)
    out = []
    for route in ("never", "radtan", "round trip"):
        prob = _problem(k, model=None)
        if route == "radtan":
            prob.set_model(capi.MODEL_RADTAN)
        if route == "round trip":
            prob.set_model(capi.MODEL_FISHEYE)
            assert prob.get_model() == capi.MODEL_FISHEYE
            prob.set_model(capi.MODEL_RADTAN)
            prob.set_intrinsics(k["intr0"], 0)
        assert prob.get_model() == capi.MODEL_RADTAN
        s = prob.solve(capi.default_options(max_iterations=200))
        out.append(_state(prob, False, s))
        prob.close()
    assert out[0][6]["iterations"] >= 3 and out[0][0][8] != 0.0
    for o in out[1:]:
        for a in range(6):
            assert np.array_equal(out[0][a], o[a])
        assert out[0][6]["termination"] == o[6]["termination"] and out[0][6]["iterations"] == o[6]["iterations"]
        assert [tuple(sorted(l.items())) for l in out[0][6]["log"]] == [tuple(sorted(l.items())) for l in o[6]["log"]]


def test_refusals_and_errors():
    k = rigk_case(2, 10, 6)
    args = (2, k["frame_offsets"], k["obs_cam"], k["obs_world"], k["obs_uv_pix"], k["world_xyz"], k["cam_frozen"])
    plain = capi.RigProblem(*args)
    with pytest.raises(capi.CcError, match="without intrinsics"):
        plain.set_model(capi.MODEL_FISHEYE)
    with pytest.raises(capi.CcError, match="without intrinsics"):
        plain.get_model()
    plain.close()
    prob = capi.RigProblem(*args, with_intrinsics=True)
    with pytest.raises(capi.CcError, match="unknown model"):
        prob.set_model(7)
    prob.set_intrinsics(k["intr0"], 0)
    prob.set_state(k["cam_q0"], k["cam_t0"], k["frame_q0"], k["frame_t0"])
    prob.set_model(capi.MODEL_FISHEYE)
    with pytest.raises(capi.CcError, match="set_intrinsics"):     # the model changed: the slots mean something else
        prob.solve()
    with pytest.raises(capi.CcError, match="set_intrinsics"):
        prob.eval()
    with pytest.raises(capi.CcError, match="fisheye model"):
        prob.comm_init(bytes(128), 0, 1)
    with pytest.raises(capi.CcError, match="fisheye model"):
        prob.exchange_export()
    with pytest.raises(capi.CcError, match="fisheye model"):
        prob.exchange_attach(0, [bytes(64)])
    with pytest.raises(capi.CcError, match="cc_rigk"):
        capi._check(capi.lib().cc_rig_set_inner_iterations(prob._h, C.c_int32(1), C.c_double(1e-3)))
    # slot 8: forced constant, stored as 0
    prob.set_intrinsics(np.array([600.0, 600.0, 800.0, 500.0, 0.01, 0.0, 0.0, 0.0, 0.123]), 0)
    assert prob.get_intrinsics()[8] == 0.0
    prob.set_model(capi.MODEL_FISHEYE)                            # the model it has: a no-op, the intrinsics stay
    assert np.isfinite(prob.eval())
    prob.close()
    # a handle with an exchange refuses the fisheye model
    ex = capi.RigProblem(*args, with_intrinsics=True)
    ex.exchange_export()
    with pytest.raises(capi.CcError, match="exchange or a communicator"):
        ex.set_model(capi.MODEL_FISHEYE)
    ex.set_model(capi.MODEL_RADTAN)
    ex.close()


def test_profiled_rounds_time_the_fisheye_sweep():
    """A profiled solve (Probe .. CC_K_SWEEP) works as on any cc_rigk_* handle."""
    k, pk, ok = rr.gpu_case("shared")
    prob = _problem(k)
    s = prob.solve(capi.default_options(profile_kernels=1, **ok))
    prob.close()
    assert s["iterations"] == rr.gpu_reference("shared")[6]["iterations"]
    assert s["kernel_ms"]["sweep"] > 0.0 and s["kernel_launches"]["sweep"] >= s["iterations"]
