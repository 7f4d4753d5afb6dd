"""Clearing the retired glued kernel's leftovers out of the rig path moves no arithmetic, but it may change the
code of the lean persistent kernels (k_rig_persist_w<1|2|4>, k_rig_persist_ctl), so the rig solver has to give, BIT FOR BIT, what
it gave before: tests/golden/rig_lean_parent.npz was recorded on the GPU from the parent commit
(tests/golden/make_rig_lean_parent.py) in the lean form with one, two and four frames per workgroup -- plain, ragged with blocks
in the Huber tail, with steps that are rejected (miss rounds: the workers eliminate a second time) -- and in the three-kernel
form. Compared: camera and frame poses, iteration count, termination, accept / reject sequence, logged costs, per-observation
costs."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _generator():
    spec = importlib.util.spec_from_file_location("make_rig_lean_parent", os.path.join(HERE, "golden", "make_rig_lean_parent.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


GEN = _generator()


@pytest.fixture(scope="module")
def recorded():
    with np.load(os.path.join(HERE, "golden", "rig_lean_parent.npz")) as z:
        return {k: z[k] for k in z.files}


def test_the_fixture_covers_what_it_is_for(recorded):
    """Every case is a solve of at least three iterations, and a lean case contains a rejected step the solve went on from."""
    assert str(recorded["parent_commit"]) == GEN.PARENT_COMMIT
    for name in GEN.CASES:
        assert int(recorded[name + "_iterations"]) >= 3, name
    assert any(np.any(recorded[name + "_accepted"][:-1] == 0) for name in GEN.LEAN)
    assert set(recorded["lean_cases_with_a_rejected_step"]) <= set(GEN.LEAN) and len(recorded["lean_cases_with_a_rejected_step"]) >= 1


@pytest.mark.parametrize("name", list(GEN.CASES))
def test_solve_is_bit_equal_to_the_parent_commit(recorded, name):
    inp = {k: recorded[name + "_in_" + k] for k in GEN.IN_FIELDS}
    cams, frames = GEN.CASES[name][0], GEN.CASES[name][1]
    assert len(inp["frame_offsets"]) == frames + 1 and inp["cam_q0"].shape == (cams, 4)
    got = GEN.solve_case(name, inp)      # (asserts the form the case means -- lean or three kernels -- and zero reruns)
    assert int(got["iterations"]) == int(recorded[name + "_iterations"])
    assert str(got["termination"]) == str(recorded[name + "_termination"])
    for field in ("accepted", "costs", "cam_q", "cam_t", "frame_q", "frame_t", "obs_cost"):
        g, want = np.ascontiguousarray(got[field]), np.ascontiguousarray(recorded[name + "_" + field])
        assert g.shape == want.shape and g.dtype == want.dtype, (field, g.shape, want.shape, g.dtype, want.dtype)
        diff = np.flatnonzero(g.view(np.uint8).reshape(-1) != want.view(np.uint8).reshape(-1))
        assert diff.size == 0, (field, "first differing element", int(diff[0]) // g.itemsize,
                                g.reshape(-1)[diff[0] // g.itemsize], want.reshape(-1)[diff[0] // g.itemsize])
