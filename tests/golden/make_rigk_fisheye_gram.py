"""Writes tests/golden/rigk_fisheye_gram.npz: the 16 x 16 Gram of X = [J_cam(6) r J_k(9)] of single (frame, camera) groups at the
starting point, summed in np.longdouble from the rows of the 50-digit fisheye model (tests/rigk_fisheye_ref.py mp_gram_rows;
a quarter of a second per observation, which is why tests/test_gpu_rigk_fisheye.py loads them instead of recomputing):
  ragged   the groups of 1, 65 and 530 observations of gpu_case("ragged") (group indices 0, 3, 5)
  axis     the one group of axis_case()
with the pixels of each group as a guard against a fixture that no longer belongs to the scenario.
    python tests/golden/make_rigk_fisheye_gram.py      (from the repository root, ~3 minutes)"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests import rigk_fisheye_ref as rr  # noqa: E402

RAGGED_PICKS = (0, 3, 5)


def groups(k):
    off, cam = np.asarray(k["frame_offsets"]), np.asarray(k["obs_cam"])
    out = []
    for f in range(len(off) - 1):
        for c in np.unique(cam[off[f]:off[f + 1]]):
            out.append((f, int(c), np.nonzero(cam[off[f]:off[f + 1]] == c)[0] + off[f]))
    return out


def gram(k, g):
    f, c, idx = g
    Xw = np.asarray(k["world_xyz"], dtype=np.float32)[np.asarray(k["obs_world"], dtype=np.int64)].astype(np.float64)
    rows = np.concatenate([rr.mp_gram_rows(np.atleast_2d(k["intr0"])[0], k["cam_q0"][c], k["cam_t0"][c], k["frame_q0"][f], k["frame_t0"][f],
                                           Xw[i], k["obs_uv_pix"][i].astype(np.float64)) for i in idx])
    return (rows.T @ rows).astype(np.float64), k["obs_uv_pix"][idx]


if __name__ == "__main__":
    k = rr.gpu_case("ragged")[0]
    gs = groups(k)
    out = {}
    for j, gi in enumerate(RAGGED_PICKS):
        out["ragged_gram_%d" % gi], out["ragged_uv_%d" % gi] = gram(k, gs[gi])
    ka = rr.axis_case()
    out["axis_gram"], out["axis_uv"] = gram(ka, groups(ka)[0])
    np.savez(os.path.join(os.path.dirname(os.path.abspath(__file__)), "rigk_fisheye_gram.npz"), **out)
