#!/usr/bin/env python3
"""Compares the gfx950 text of every kernel of some translation units between two trees (no GPU needed).

    python scripts/kernel_identity.py BEFORE_DIR AFTER_DIR [--map OLD_UNIT:OLD=NEW_UNIT:NEW ...] [unit.hip ...] > profiles/rNN/<name>_identity.txt

BEFORE_DIR and AFTER_DIR are two checkouts of the repository (for instance `git worktree add /tmp/parent HEAD~1` and `.`).
Each unit's device side is compiled to assembly in both with the compile line of scripts/kernel_regs.py
(hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S, plus -ffp-contract=off for cc_points.hip as in the Makefile),
and for every kernel (.amdhsa_kernel entry) the instruction text from its label to its end marker and its kernel descriptor are
compared line by line. Before the comparison, on both sides, the ordinal of the function in local labels and their comments is
dropped (.LBB<n>_ -> .LBB_, BB<n>_ -> BB_: a kernel that merely moves within its unit keeps its text) and the kernel's own
mangled name becomes a placeholder.

--map (repeatable) follows a kernel that was renamed or moved to another unit: the one kernel of BEFORE_DIR's OLD_UNIT whose
mangled name contains OLD is compared with the one kernel of AFTER_DIR's NEW_UNIT whose mangled name contains NEW; neither
counts as missing or new. The units a --map names are compiled in addition to the listed ones.

Descriptor lines that differ are printed. Exit status 1 when a kernel's text or descriptor differs or a kernel disappeared."""
import os
import re
import subprocess
import sys
import tempfile

UNITS = ["cc_rig.hip", "cc_rig_inner.hip", "cc_rig_lens.hip", "cc_rig_start.hip", "cc_rig_start_bearing.hip", "cc_rigk_start.hip", "cc_zhang.hip", "cc_intrinsics.hip", "cc_intr_start.hip", "cc_intr_start_batch.hip", "cc_intrinsics_batch_fisheye.hip", "cc_intrinsics_batch.hip", "cc_intrinsics_batch_huber.hip",
         "cc_intrinsics_persist.hip", "cc_points.hip"]
FLAGS = {"cc_points.hip": ["-ffp-contract=off"]}


def assembly(tree, unit, out):
    src = os.path.join(tree, "camera_calibrator_amd", "csrc", unit)
    if not os.path.exists(src):   # a unit one of the trees does not have: no kernels on that side
        return ""
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", "-o", out, src]
                          + FLAGS.get(unit, []), stderr=subprocess.DEVNULL)
    return open(out).read()


def kernels(text):
    """{mangled symbol: (instruction lines, descriptor lines)} of every kernel in the assembly text, normalised (see above)."""
    lines = text.split("\n")
    names = [m.group(1) for m in (re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l) for l in lines) if m]
    out = {}
    for name in names:
        start = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
        end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
        d0 = next(i for i, l in enumerate(lines) if re.match(r"\s*\.amdhsa_kernel\s+" + re.escape(name) + r"\s*$", l))
        d1 = next(i for i in range(d0, len(lines)) if ".end_amdhsa_kernel" in lines[i])
        norm = lambda ls: [re.sub(r"\bBB\d+_", "BB_", re.sub(r"\.LBB\d+_", ".LBB_", l)).replace(name, "<kernel>") for l in ls]
        text = lines[start:d0] + lines[d1:end] if start <= d0 < end else lines[start:end]   # (the descriptor counts once, as descriptor)
        out[name] = (norm(text), norm(lines[d0:d1]))
    return out


def the_one(table, unit, part, side):
    hits = [n for n in table.get(unit, {}) if part in n]
    if len(hits) != 1:
        sys.exit("--map: %r names %d kernels of %s (%s): %s" % (part, len(hits), unit, side, hits))
    return hits[0]


def main():
    argv, maps = sys.argv[1:], []
    while "--map" in argv:
        i = argv.index("--map")
        old, new = argv[i + 1].split("=", 1)
        maps.append(tuple(old.split(":", 1)) + tuple(new.split(":", 1)))
        del argv[i:i + 2]
    before, after = argv[0], argv[1]
    units = argv[2:] or UNITS
    compiled = units + [u for m in maps for u in (m[0], m[2]) if u not in units]
    compiled = sorted(set(compiled), key=compiled.index)
    with tempfile.TemporaryDirectory() as tmp:
        a = {u: kernels(assembly(before, u, os.path.join(tmp, "a.s"))) for u in compiled}
        b = {u: kernels(assembly(after, u, os.path.join(tmp, "b.s"))) for u in compiled}
    successor, mapped_new = {}, set()
    for ou, op, nu, np_ in maps:
        target = (nu, the_one(b, nu, np_, "after"))
        successor[(ou, the_one(a, ou, op, "before"))] = target
        mapped_new.add(target)
    changed = descriptor_only = missing = 0
    for unit in compiled:
        print("%s: %d kernels before, %d after" % (unit, len(a[unit]), len(b[unit])))
        for name in sorted(a[unit]):
            nu, nn = successor.get((unit, name), (unit, name))
            label = name if (nu, nn) == (unit, name) else "%s -> %s:%s" % (name, nu, nn)
            if nn not in b[nu]:
                print("  %-90s MISSING after" % label)
                missing += 1
                continue
            (ta, da), (tb, db) = a[unit][name], b[nu][nn]
            n = sum(1 for x, y in zip(ta, tb) if x != y) + abs(len(ta) - len(tb))
            text = "identical (%d lines of text" % len(ta) if n == 0 else "DIFFERENT (%d lines of text differ" % n
            print("  %-90s %s, descriptor %s)" % (label, text, "identical" if da == db else "differs"))
            for x, y in zip(da, db):
                if x != y:
                    print("      descriptor: %s -> %s" % (x.strip(), y.strip()))
            if len(da) != len(db):
                print("      descriptor: %d lines -> %d lines" % (len(da), len(db)))
            changed += n != 0
            descriptor_only += n == 0 and da != db
        for name in sorted(set(b[unit]) - set(a[unit])):
            if (unit, name) not in mapped_new:
                print("  %-90s new" % name)
    print("%d kernels before, %d after" % (sum(len(v) for v in a.values()), sum(len(v) for v in b.values())))
    if changed or descriptor_only or missing:
        print("%d kernels changed their text, %d differ in their descriptor only, %d are missing" % (changed, descriptor_only, missing))
        return 1
    print("every pre-existing kernel's text and descriptor are unchanged")
    return 0


if __name__ == "__main__":
    sys.exit(main())
