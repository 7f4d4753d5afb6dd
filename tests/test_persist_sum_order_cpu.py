"""The order in which k_intr_persist adds the workers' elimination rows is written once, in csrc/cc_persist_sum.hpp, as the pieces
the kernel's column owners call. tests/cpp/persist_sum_order.cpp composes them on the host as the kernel does and compares the
totals, as raw bits, with a literal transcription of the two gather_rows levels (leaders, then the control) the order comes from:
G in {1, 5, 10, 16, 17, 19, 37, 79, 80, 81, 203, 250, 256} x NG in {3, 6, 12}, sum columns and the maximum column, values of mixed
sign over thirty decades, exact cancellations, -0.0, NaN in the maximum column. Built with the host compiler, no GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "camera_calibrator_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs a host compiler")
def test_column_owner_sums_have_the_two_level_gathers_order(tmp_path):
    exe = str(tmp_path / "persist_sum_order")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-I", CSRC,
                        os.path.join(ROOT, "tests", "cpp", "persist_sum_order.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    m = re.search(r"(\d+) cases of 80 columns, 0 mismatches", r.stdout)
    assert m and int(m.group(1)) == 13 * 3 * 10, r.stdout[-500:]


def test_the_maximum_column_of_the_program_is_the_kernels():
    text = open(os.path.join(CSRC, "cc_intrinsics_dev.hpp")).read() + open(os.path.join(CSRC, "cc_common.hpp")).read()
    m = re.search(r"\bPC_GMAXP\s*=\s*(\d+)", text)
    assert m and int(m.group(1)) == 73, m and m.group(0)
    assert "maxcol = 73" in open(os.path.join(ROOT, "tests", "cpp", "persist_sum_order.cpp")).read()
