"""Results of the persistent intrinsics solve on a ragged problem of 203 frames, recorded on the GPU from PARENT_COMMIT: the state
before the elimination rows of a round were added up by column owners instead of leaders. The change moves who
pulls which words and in which wave the additions run; every sum and every maximum keeps its operands and its order
(csrc/cc_persist_sum.hpp), so the solver must reproduce these numbers BIT FOR BIT (tests/test_gpu_intr_column_owners.py). The
problem of tests/golden/intr_seam_polls_parent.npz never has more than 37 workers; here one frame per workgroup gives 203 workers
(every column has an owner of its own; thirteen groups of sixteen rows, the last of eleven), two give 102 (seven groups, the last of
six), four give 51 (fewer workers than columns: workers 0..28 own two). The solves are those of make_intr_seam_polls.py
(solve_all, bad_start: loaded by path) on these inputs. Run once, on a GPU, on a build of PARENT_COMMIT:
    python tests/golden/make_intr_column_owners.py      -> tests/golden/intr_column_owners_parent.npz
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PARENT_COMMIT = "d5bcbf6"   # "Fisheye (Kannala-Brandt) camera model for the intrinsics solve"
FRAMES = 203
CYCLE = [4, 20, 33, 63, 64, 65]   # 8,401 observations: an .npz the size of intr_seam_polls_parent.npz
POINTS = [CYCLE[i % len(CYCLE)] for i in range(FRAMES)]


def seam_polls():
    spec = importlib.util.spec_from_file_location("make_intr_seam_polls", os.path.join(HERE, "make_intr_seam_polls.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def make_inputs():
    sys.path.insert(0, ROOT)
    from tests.helpers import intrinsics_case
    c = intrinsics_case(FRAMES, POINTS)
    inputs = {k: c[k] for k in ("off", "uv", "xyz", "intr0", "q0", "t0")}
    inputs["intr_b"], inputs["q_b"], inputs["t_b"] = seam_polls().bad_start(inputs)
    return inputs


if __name__ == "__main__":
    inputs = make_inputs()
    res = seam_polls().solve_all(inputs)
    for k, v in res.items():
        assert np.all(np.isfinite(v)), k
        if k.endswith("iterations"):
            print(k, int(v), "accepted", res[k[:-10] + "accepted"].tolist(), "costs", repr(float(res[k[:-10] + "costs"][0])), "->",
                  repr(float(res[k[:-10] + "costs"][-1])))
    dst = os.environ.get("INTR_COLUMN_OWNERS_OUT", os.path.join(HERE, "intr_column_owners_parent.npz"))
    np.savez_compressed(dst, parent_commit=PARENT_COMMIT, points=np.array(POINTS), **{"in_" + k: v for k, v in inputs.items()}, **res)
    print("wrote", dst, os.path.getsize(dst), "bytes")
