"""Register budget and kernel set of the fisheye focal-length start's unit (cc_intr_start.hip), checked on the CPU as
tests/test_rigk_lens_budgets.py does for the lens unit (hipcc cross-compiles gfx950 without a GPU; scripts/kernel_regs.py reads
the code object metadata).
k_intr_start_view is k_rig_start_view_bearing with the bearing formed from the pixel: it sits at ONE wave per SIMD like that
kernel (264 + 16 registers there; 282 + 26 here, the 9 x 9 / 12 x 12 eigenproblem in registers sets it and the iteration that runs
until the vector settles keeps the previous vector, 12 doubles), which is accepted -- the grid is views x candidates waves and
nothing waits on another wave. No kernel spills or uses scratch; the extent and the pick are
small (DESIGN.md 4.19 has the table)."""
import os

import pytest

from tests.test_kernel_budgets import _table

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")

KERNELS = ("cc::k_intr_start_extent", "cc::k_intr_start_view", "cc::k_intr_start_pick")


def test_the_start_unit_is_these_kernels():
    assert set(_table("cc_intr_start.hip")) == set(KERNELS)


def test_no_kernel_of_the_start_unit_spills_or_uses_scratch():
    t = _table("cc_intr_start.hip")
    for k in KERNELS:
        assert t[k]["vspill"] == 0 and t[k]["sspill"] == 0 and t[k]["scratch"] == 0, (k, t[k])


def test_register_budgets():
    t = _table("cc_intr_start.hip")
    view = t["cc::k_intr_start_view"]
    assert 256 < view["vgpr"] + view["agpr"] <= 320, view      # one wave per SIMD: its parent's 280 + the settled iteration's 24, a granule of room; a wave may have 512
    assert view["lds"] == 8192, view                            # the staged rows of one wave
    for k in ("cc::k_intr_start_extent", "cc::k_intr_start_pick"):
        assert t[k]["vgpr"] + t[k]["agpr"] <= 64 and t[k]["lds"] <= 128, (k, t[k])   # eight waves per SIMD; the extent's sixteen words
