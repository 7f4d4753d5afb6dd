"""Restructurings of k_intr_persist that move LDS traffic, barriers and stores but no arithmetic (wave 0 of
the control stores the broadcast itself, the Jacobi scales of the reduced system are applied in its row build instead of a
pass of their own; 4.8: the main loop with both Gram row sets staged before one burst of products, which this test caught
changing the last bits of the one-team form) have to give, BIT FOR BIT, what the kernel gave before them:
tests/golden/intr_loop_order_parent.npz was recorded on the GPU from the parent commit
(tests/golden/make_intr_loop_order.py) on a ragged problem whose frames give a team's waves zero, one and two passes and
partly valid last passes, in the persistent form with one, two and four frames per workgroup, with every intrinsic free and
with three distortion coefficients held."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _generator():
    spec = importlib.util.spec_from_file_location("make_intr_loop_order", os.path.join(HERE, "golden", "make_intr_loop_order.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def recorded():
    with np.load(os.path.join(HERE, "golden", "intr_loop_order_parent.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def solved(recorded):
    gen = _generator()
    assert list(recorded["points"]) == gen.POINTS and list(np.diff(recorded["in_off"])) == gen.POINTS
    return gen.solve_all({k[3:]: v for k, v in recorded.items() if k.startswith("in_")})


@pytest.mark.parametrize("mask", ["free", "distortion_held"])
@pytest.mark.parametrize("teams", [1, 2, 4])
def test_solve_is_bit_equal_to_the_parent_commit(recorded, solved, teams, mask):
    k = "t%d_%s_" % (teams, mask)
    assert int(solved[k + "iterations"]) == int(recorded[k + "iterations"])
    assert int(recorded[k + "iterations"]) >= 3          # (the fixture is a solve, not a start that ends at once)
    for field in ("accepted", "costs", "intr", "q", "t"):
        got, want = np.ascontiguousarray(solved[k + field]), np.ascontiguousarray(recorded[k + field])
        assert got.shape == want.shape and got.dtype == want.dtype, (field, got.shape, want.shape)
        diff = np.flatnonzero(got.view(np.uint8).reshape(-1) != want.view(np.uint8).reshape(-1))
        assert diff.size == 0, (field, "first differing element", int(diff[0]) // got.itemsize,
                                got.reshape(-1)[diff[0] // got.itemsize], want.reshape(-1)[diff[0] // got.itemsize])
