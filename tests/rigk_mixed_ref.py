"""CPU reference of the rig solve with intrinsics with a pixel model PER CAMERA (cc_rigk_set_camera_model; the kernels:
cc_rig_lens.hip): tests/rigk_fisheye_ref.py's problem with the rows of camera c taken from models[c], its LM (rigk_solve) run on it
unchanged, and the scenarios of tests/test_rigk_mixed_cpu.py / tests/test_gpu_rigk_mixed.py. Shares no code with the kernels.
A helper module, not a test. Callers must not modify what they get."""
import functools

import mpmath as mp
import numpy as np

from camera_calibrator_amd.harness import rigk_case
from oracle import pyoracle as po
from tests import fisheye_ref as fr
from tests import rigk_fisheye_ref as rr

MODELS = {"R": fr.pinhole_model, "F": fr.fisheye_model}
MODEL_ID = {"R": 0, "F": 1}   # CC_MODEL_RADTAN, CC_MODEL_FISHEYE


class MixedRigKData(rr.RigKData):
    """RigKData with a set of intrinsics per camera and the pixel model of camera c = models[c]; slot 8 of a fisheye camera's set
    is held (cc_rigk_set_camera_intrinsics forces the bit on such a set only)."""

    def __init__(self, models, n_cams, frame_offsets, obs_cam, obs_world, obs_uv_pix, world_xyz, cam_frozen, huber_a=0.0, const_masks=0):
        models = tuple(models)
        assert len(models) == int(n_cams)
        masks = np.broadcast_to(np.asarray(const_masks, dtype=np.int64), (int(n_cams),)).copy()
        for c, m in enumerate(models):
            if m is fr.fisheye_model:
                masks[c] |= fr.K8_HELD
        super().__init__(None, n_cams, frame_offsets, obs_cam, obs_world, obs_uv_pix, world_xyz, cam_frozen, huber_a=huber_a,
                         per_camera=True, const_masks=masks)
        self.models = models

    def rows(self, st, dtype=np.float64):
        K, cq, ct, fq, ft = st
        N = len(self.cam)
        r, J = np.zeros((N, 2), dtype=dtype), np.zeros((N, 2, 21), dtype=dtype)
        Rf = np.array([rr._rot(q) for q in fq], dtype=dtype).reshape(-1, 3, 3)
        ident, zero = np.array([1, 0, 0, 0], dtype=dtype), np.zeros(3, dtype=dtype)
        for c in range(self.C):
            idx = self.by_cam[c]
            if len(idx) == 0:
                continue
            Rc = rr._rot(cq[c])
            b = np.einsum("nij,nj->ni", Rf[self.frame[idx]], self.X[idx].astype(dtype))
            a = (b + ft[self.frame[idx]]) @ Rc.T
            rc, Jm = self.models[c](K[self.kset(c)], ident, zero, a + ct[c], self.uv[idx])
            B = Jm[:, :, 12:15]
            m = B @ Rc
            r[idx] = rc
            J[idx, :, 0:3] = 2 * np.cross(a[:, None, :], B)
            J[idx, :, 3:6] = B
            J[idx, :, 6:9] = 2 * np.cross(b[:, None, :], m)
            J[idx, :, 9:12] = m
            J[idx, :, 12:21] = Jm[:, :, 0:9]
        return r, J


def problem(k, kinds=None, huber_a=0.0, const_masks=None):
    kinds = k["kinds"] if kinds is None else kinds
    return MixedRigKData([MODELS[x] for x in kinds], k["cams"], k["frame_offsets"], k["obs_cam"], k["obs_world"], k["obs_uv_pix"],
                         k["world_xyz"], k["cam_frozen"], huber_a=huber_a, const_masks=0 if const_masks is None else const_masks)


def model_ids(kinds):
    return [MODEL_ID[x] for x in kinds]


@functools.lru_cache(maxsize=None)
def mixed_rig_case(cams, frames, pts, kinds, half=0.5, sigma=0.3, seed=0):
    """rigk_case(cams, frames, pts, seed, per_camera=True)'s rig, poses, starting offsets and world points, x and y of the points
    stretched from +-0.2 m to +-half as fisheye_rig_case does. kinds[c] = "F": camera c is a fisheye lens with fisheye_rig_case's
    per-camera true set and INTR0 as its start; "R": it keeps rigk_case's intr_true[c] / intr0[c]. Pixels: each camera's own
    model at the true state (fisheye: the 50-digit projection; radial-tangential: the numpy model in float64) from the float32
    world points as stored, + N(0, sigma) px, rounded to float32. Adds kinds and max_angle_deg."""
    assert len(kinds) == cams and set(kinds) <= {"R", "F"}
    k = dict(rigk_case(cams, frames, pts, seed=seed, per_camera=True))
    world = k["world_xyz"].astype(np.float64).copy()
    world[:, :2] *= half / 0.2
    world = world.astype(np.float32)
    Kf = np.tile(rr.TRUE_INTR, (cams, 1))          # (fisheye_rig_case's per-camera sets: the same stream)
    krng = np.random.default_rng(seed + 12345)
    Kf[:, :2] *= 1 + krng.uniform(-0.03, 0.03, size=(cams, 2))
    Kf[:, 2:4] += krng.uniform(-15, 15, size=(cams, 2))
    Kf[:, 4:8] *= krng.uniform(0.7, 1.3, size=(cams, 1))
    K = np.array([Kf[c] if kinds[c] == "F" else k["intr_true"][c] for c in range(cams)])
    K0 = np.array([rr.INTR0 if kinds[c] == "F" else k["intr0"][c] for c in range(cams)])
    rng = np.random.default_rng(seed + 777)
    N = len(k["obs_cam"])
    frame = np.repeat(np.arange(frames), np.diff(k["frame_offsets"]))
    uv = np.zeros((N, 2))
    Xw = world[k["obs_world"].astype(np.int64)].astype(np.float64)
    ident, zero = np.array([1.0, 0, 0, 0]), np.zeros(3)
    ang = 0.0
    for c in range(cams):
        idx = np.nonzero(k["obs_cam"] == c)[0]
        Rf = np.array([rr._rot(q) for q in k["frame_q_true"]])[frame[idx]]
        p = (np.einsum("nij,nj->ni", Rf, Xw[idx]) + k["frame_t_true"][frame[idx]]) @ rr._rot(k["cam_q_true"][c]).T + k["cam_t_true"][c]
        ang = max(ang, float(np.degrees(np.arctan2(np.hypot(p[:, 0], p[:, 1]), p[:, 2])).max()))
        if kinds[c] == "F":
            with mp.workdps(50):
                f = lambda v: [mp.mpf(float(x)) for x in v]
                for i in idx:
                    fi = int(frame[i])
                    u, v = rr._mp_pixel(f(K[c][:8]), f(k["cam_q_true"][c]), f(k["cam_t_true"][c]), f(k["frame_q_true"][fi]),
                                        f(k["frame_t_true"][fi]), f(world[int(k["obs_world"][i])]))
                    uv[i] = float(u), float(v)
        else:
            uv[idx] = fr.pinhole_model(K[c], ident, zero, p, np.zeros((len(idx), 2)))[0]
    uv = uv + rng.normal(0.0, sigma, size=(N, 2)) if sigma > 0 else uv
    k.update(obs_uv_pix=np.ascontiguousarray(uv.astype(np.float32)), world_xyz=world, intr0=K0, intr_true=K, kinds=kinds, max_angle_deg=ang)
    return k


def solve_case(k, P, options=None, dtype=np.float64):
    return rr.rigk_solve(P, k["intr0"], k["cam_q0"], k["cam_t0"], k["frame_q0"], k["frame_t0"], options=options, dtype=dtype)


# ---------------------------------------------------------------------------------------------------------------------------
# the shapes of tests/test_gpu_rigk_mixed.py (tests/test_rigk_mixed_cpu.py checks every one for a stable trajectory)
# ---------------------------------------------------------------------------------------------------------------------------
# masks of `percam` (kinds FRF): k3 and k4 of the fisheye camera 0 held, slot 8 (k3) of the radial-tangential camera 1 held,
# k4 of the fisheye camera 2 held (bit 8 of the fisheye sets comes on its own)
PC_MASKS = np.array([(1 << 6) | (1 << 7), 1 << 8, 1 << 7], dtype=np.uint32)
# ragged_rf / ragged_fr: with two cameras and four frames each camera (each model) gets the groups of 1, 64, 257, 0 observations in
# one of the shapes and of 63, 65, 530, 130 in the other (rr.RAGGED_PAIRS: one pass, the unrolled pair, the tail, nine passes
# with one wave, an empty pair)


def _without_camera(k, c):
    """Every observation of camera c removed: the camera keeps its model and its set and has no group."""
    keep = np.asarray(k["obs_cam"]) != c
    off = k["frame_offsets"]
    offs = np.concatenate([[0], np.cumsum([keep[off[f]:off[f + 1]].sum() for f in range(len(off) - 1)])]).astype(np.int64)
    return dict(k, frame_offsets=offs, obs_cam=np.ascontiguousarray(k["obs_cam"][keep]), obs_world=np.ascontiguousarray(k["obs_world"][keep]),
                obs_uv_pix=np.ascontiguousarray(k["obs_uv_pix"][keep]))


@functools.lru_cache(maxsize=None)
def gpu_case(name):
    """(scenario with its kinds, keyword arguments of problem(), keyword arguments of the options) of a named shape."""
    if name in ("rf", "fr"):        # one pass, one wave per group
        return mixed_rig_case(2, 12, 20, name.upper()), {}, dict(max_iterations=200)
    if name in ("ragged_rf", "ragged_fr"):
        return rr._cut(mixed_rig_case(2, 4, 530, name[-2:].upper()), rr.RAGGED_PAIRS), {}, dict(max_iterations=200)
    if name == "ng1024":            # one wave per group by the group count; one frame of three passes
        k = mixed_rig_case(4, 255, 5, "RFFR")
        return rr._append_frames(k, mixed_rig_case(4, 1, 140, "RFFR")), {}, dict(max_iterations=6)
    if name == "percam":            # masks, the loss with observations in its tail
        return rr._displace(mixed_rig_case(3, 20, 25, "FRF")), dict(const_masks=PC_MASKS, huber_a=1.5), dict(max_iterations=300)
    if name == "percam_start":      # percam's rig and loss without displaced pixels and without the masks: the pixel start's scenario.
        # The bounds of that test compare two solves that stop by the same rule. With PC_MASKS the reference's OWN two solves (from
        # the scenario's start and from its pixel start, tight tolerances) end 7.1e-10 rad apart in a camera rotation -- the one
        # from the scenario's start stops on the function tolerance after 6 iterations -- which is 1.23 of the bound; without the
        # masks they end 2.4e-15 apart.
        return mixed_rig_case(3, 20, 25, "FRF"), dict(huber_a=1.5), dict(max_iterations=300)
    if name == "big":               # 9 x 6 + 10 x 9 = 144 shared coordinates: the large-rig kernels
        return mixed_rig_case(10, 12, 10, "RFRFRFRFRF"), {}, dict(max_iterations=300)
    if name == "rrf_unseen":        # the only fisheye camera has no observation: the fisheye list is empty
        return _without_camera(mixed_rig_case(3, 12, 20, "RRF"), 2), {}, dict(max_iterations=200)
    if name == "ffr_unseen":        # ... and the radial-tangential list
        return _without_camera(mixed_rig_case(3, 12, 20, "FFR"), 2), {}, dict(max_iterations=200)
    raise KeyError(name)


GPU_CASES = ("rf", "fr", "ragged_rf", "ragged_fr", "ng1024", "percam", "big", "rrf_unseen", "ffr_unseen")


@functools.lru_cache(maxsize=None)
def gpu_reference(name, dtype=np.float64):
    k, pk, ok = gpu_case(name)
    return solve_case(k, problem(k, **pk), options=po.default_options(**ok), dtype=dtype)


def groups(k):
    """(frame, camera, caller's observation indices) of every group, in the handle's order (frame-major, camera-minor)."""
    off, cam = np.asarray(k["frame_offsets"]), np.asarray(k["obs_cam"])
    out = []
    for f in range(len(off) - 1):
        for c in np.unique(cam[off[f]:off[f + 1]]):
            out.append((f, int(c), np.nonzero(cam[off[f]:off[f + 1]] == c)[0] + off[f]))
    return out


def group_gram(P, st, idx):
    """The 16 x 16 Gram of X = [J_cam(6) r J_k(9)] over the observations idx (one group) at state st, in np.longdouble, held
    columns zero as the sweep leaves them (no loss)."""
    ld = np.longdouble
    r, J = P.rows(tuple(np.asarray(a, dtype=ld) for a in st), ld)
    c = int(P.cam[idx[0]])
    X = np.concatenate([J[idx][:, :, 0:6], r[idx][:, :, None], J[idx][:, :, 12:21]], axis=2).reshape(-1, 16)
    held = np.array([bool(P.masks[P.kset(c)] & (1 << j)) for j in range(9)])
    X[:, 7:16][:, held] = 0
    return X.T @ X
