"""The one-shot intrinsics calls answer a refused call as the library did before they got one pipeline (cc::intr_one_shot,
cc::batch_one_shot): tests/golden/oneshot_refusals.json holds, for every public one-shot of the ladder, the return code and the
full cc_last_error() text of each refusal that is decided before any device call -- single faults and pairs of them, so that the
order of the checks is pinned too -- as scripts/record_oneshot_refusals.py recorded them from the parent commit's library on a
machine without a GPU. Needs no GPU."""
import json
import os

import pytest

from camera_calibrator_amd import capi
from tests import oneshot_refusal_cases as cases

BAD_ARGUMENT = -1
GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "oneshot_refusals.json")))
CASES = cases.cases()


def test_the_fixture_holds_every_case_and_every_symbol():
    assert sorted(GOLDEN) == sorted(c[0] for c in CASES)
    for sym in cases.SINGLE + cases.BATCH:
        mine = [GOLDEN[c[0]] for c in CASES if c[2] == sym]
        assert any(not g["device"] for g in mine) and any(g["device"] for g in mine), sym
    # a few of the recorded facts, by name: the pairs that pin an order
    assert "NaN" in GOLDEN["cc_intrinsics_batch_estimate_start:nan_huber+unknown_model"]["message"]
    assert "unknown model" in GOLDEN["cc_intrinsics_batch_estimate_model:nan_huber+unknown_model"]["message"]
    assert "NaN" in GOLDEN["cc_intrinsics_estimate_views_model:nan_huber+unknown_model"]["message"]
    for sym in ("cc_intrinsics_estimate_views_start", "cc_intrinsics_batch_estimate_start"):   # (the start's own option checks are reached)
        for fault in ("candidates_0", "nan_huber+candidates_0") + (("theta_hi_pi", "candidates_0+short_view") if "views" in sym else
                                                                   ("candidates_0+too_few_frames", "candidates_0+problem_offsets_decrease")):
            want = "NaN" if fault.startswith("nan_huber") else "theta_hi" if fault == "theta_hi_pi" else "candidates"
            assert want in GOLDEN["%s:%s" % (sym, fault)]["message"], (sym, fault)
        assert "fisheye model" in GOLDEN[sym + ":start_on_radtan+candidates_0"]["message"]
    assert not GOLDEN["cc_intrinsics_estimate_views_huber:short_view"]["device"] and GOLDEN["cc_intrinsics_estimate_views_model:fisheye+short_view"]["device"]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_a_refusal_is_the_parents(case):
    want = GOLDEN[case[0]]
    rc, msg = cases.run(capi.lib(), case)
    if not want["device"]:
        assert (rc, msg) == (want["rc"], want["message"])
    elif capi.device_count() == 0:
        assert rc == want["rc"], msg   # (the message is the machine's)
    else:   # with a GPU, what the parent's answer stood for: every check passed, and device -1 is none of the machine's
        assert rc == BAD_ARGUMENT and "device -1 out of range" in msg, (rc, msg)
