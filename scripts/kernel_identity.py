#!/usr/bin/env python3
"""Compares the gfx950 text of every kernel of some translation units between two trees (no GPU needed).

    python scripts/kernel_identity.py BEFORE_DIR AFTER_DIR [unit.hip ...] > profiles/rNN/<name>_identity.txt

BEFORE_DIR and AFTER_DIR are two checkouts of the repository (for instance `git worktree add /tmp/parent HEAD~1` and `.`).
Each unit's device side is compiled to assembly in both with the compile line of scripts/kernel_regs.py
(hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S, plus -ffp-contract=off for cc_points.hip as in the Makefile),
and for every kernel (.amdhsa_kernel entry) the instruction text from its label to its end marker and its kernel descriptor are
compared line by line. Exit status 1 when a kernel that exists on both sides differs or one disappeared."""
import os
import re
import subprocess
import sys
import tempfile

UNITS = ["cc_rig.hip", "cc_rig_inner.hip", "cc_rig_fisheye.hip", "cc_rig_mixed.hip", "cc_rig_start.hip", "cc_rig_start_bearing.hip", "cc_rigk_start.hip", "cc_zhang.hip", "cc_intrinsics.hip", "cc_intrinsics_batch_fisheye.hip", "cc_intrinsics_batch.hip", "cc_intrinsics_batch_huber.hip",
         "cc_intrinsics_persist.hip", "cc_points.hip"]
FLAGS = {"cc_points.hip": ["-ffp-contract=off"]}


def assembly(tree, unit, out):
    src = os.path.join(tree, "camera_calibrator_amd", "csrc", unit)
    if not os.path.exists(src):   # a unit one of the trees does not have yet: no kernels on that side
        return ""
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", "-o", out, src]
                          + FLAGS.get(unit, []), stderr=subprocess.DEVNULL)
    return open(out).read()


def kernels(text):
    """{demangled-free symbol: (instruction lines, descriptor lines)} of every kernel in the assembly text."""
    lines = text.split("\n")
    names = [m.group(1) for m in (re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l) for l in lines) if m]
    out = {}
    for name in names:
        start = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
        end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
        d0 = next(i for i, l in enumerate(lines) if re.match(r"\s*\.amdhsa_kernel\s+" + re.escape(name) + r"\s*$", l))
        d1 = next(i for i in range(d0, len(lines)) if ".end_amdhsa_kernel" in lines[i])
        out[name] = (lines[start:end], lines[d0:d1])
    return out


def main():
    before, after = sys.argv[1], sys.argv[2]
    units = sys.argv[3:] or UNITS
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        for unit in units:
            a = kernels(assembly(before, unit, os.path.join(tmp, "a.s")))
            b = kernels(assembly(after, unit, os.path.join(tmp, "b.s")))
            print("%s: %d kernels before, %d after" % (unit, len(a), len(b)))
            for name in sorted(set(a) | set(b)):
                if name not in b:
                    verdict, bad = "MISSING after", bad + 1
                elif name not in a:
                    verdict = "new"
                elif a[name] == b[name]:
                    verdict = "identical (%d lines of text, descriptor identical)" % len(a[name][0])
                else:
                    n = sum(1 for x, y in zip(a[name][0], b[name][0]) if x != y) + abs(len(a[name][0]) - len(b[name][0]))
                    verdict, bad = "DIFFERENT (%d lines of text differ, descriptor %s)" % (n, "identical" if a[name][1] == b[name][1] else "differs"), bad + 1
                print("  %-90s %s" % (name, verdict))
    print("every pre-existing kernel's text is unchanged" if not bad else "%d kernels changed" % bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
