"""k_intr_persist forms a frame's Gram block on the ten upper 4 x 4 blocks of the 16 x 16 block (csrc/cc_gram_blocks.hpp: 4 x 4 x 4
matrix products with broadcast A operands, the lower triangle mirrored where the block is assembled) instead of whole 16 x 16 x 4
products. Every entry is still the same chain of products of the same factors in the same order and the reduction adds the same
terms in the same order, so the solve has to give, BIT FOR BIT, what the kernel gave before:
tests/golden/intr_gram_blocks_parent.npz was recorded on the GPU from the parent commit (tests/golden/make_intr_gram_blocks.py) on
26 ragged frames -- waves with less than one row set of four rows and with an odd number of them, second and third passes with
ragged tails, one frame too long for the residual-only tiles -- in the forms of one, two and four frames per workgroup: default
options, iteration limits 1 and 2, a held-coordinate mask (the mirroring crosses gram_entry_held), the miss route, and the three
final-sweep modes. There is no tolerance."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _generator():
    spec = importlib.util.spec_from_file_location("make_intr_gram_blocks", os.path.join(HERE, "golden", "make_intr_gram_blocks.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


GEN = _generator()


@pytest.fixture(scope="module")
def recorded():
    with np.load(os.path.join(HERE, "golden", "intr_gram_blocks_parent.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def solved(recorded):
    assert list(recorded["points"]) == GEN.POINTS and list(np.diff(recorded["in_off"])) == GEN.POINTS
    return GEN.solve_all({k[3:]: v for k, v in recorded.items() if k.startswith("in_")})


def test_the_recorded_cases_end_as_intended(recorded):
    GEN.check_ends_as_intended(recorded)


@pytest.mark.parametrize("case", list(GEN.CASES))
@pytest.mark.parametrize("teams", GEN.TEAMS)
def test_solve_is_bit_equal_to_the_parent_commit(recorded, solved, teams, case):
    k = "t%d_%s_" % (teams, case)
    print(k, "iterations", int(solved[k + "iterations"]), str(solved[k + "termination"]), "accepted", solved[k + "log_accepted"].tolist(), "counts", solved[k + "counts"].tolist())
    assert int(solved[k + "iterations"]) == int(recorded[k + "iterations"]) and str(solved[k + "termination"]) == str(recorded[k + "termination"])
    assert int(solved[k + "sweeps"]) == int(recorded[k + "sweeps"]) and solved[k + "counts"].tolist() == recorded[k + "counts"].tolist()
    for field in ["log_" + f for f in GEN.LOG_FIELDS] + ["costs2", "intr", "q", "t"]:
        got, want = np.ascontiguousarray(solved[k + field]), np.ascontiguousarray(recorded[k + field])
        assert got.shape == want.shape and got.dtype == want.dtype, (field, got.shape, want.shape)
        diff = np.flatnonzero(got.view(np.uint8).reshape(-1) != want.view(np.uint8).reshape(-1))
        assert diff.size == 0, (field, "first differing element", int(diff[0]) // got.itemsize,
                                got.reshape(-1)[diff[0] // got.itemsize], want.reshape(-1)[diff[0] // got.itemsize])
