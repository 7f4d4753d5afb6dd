#!/usr/bin/env python3
"""Records tests/golden/oneshot_refusals.json: what a library answers to every case of tests/oneshot_refusal_cases.py.

    python scripts/record_oneshot_refusals.py PATH/TO/libcc_hip.so > tests/golden/oneshot_refusals.json

The library is the one whose behaviour is to be pinned -- the build of the commit BEFORE a change to the one-shot calls (for
instance `git worktree add /tmp/parent HEAD~1`, built there) -- and tests/test_oneshot_contract_cpu.py then holds the tree's own
library to it. Run on a machine without a GPU: every case calls on device -1 and most are refused by the argument checks; one that
passes them all is answered by the device ("device": true in the file), with a message that differs between machines, so only
its return code is compared."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import oneshot_refusal_cases as cases   # noqa: E402

CC_ERR_NO_DEVICE, CC_ERR_HIP = -2, -3


def main():
    lib = C.CDLL(os.path.abspath(sys.argv[1]))
    out = {}
    for case in cases.cases():
        rc, msg = cases.run(lib, case)
        if rc == 0:
            sys.exit("%s was not refused: record on a machine without a GPU" % case[0])
        out[case[0]] = {"rc": rc, "message": msg, "device": rc in (CC_ERR_HIP, CC_ERR_NO_DEVICE)}
    json.dump(out, sys.stdout, indent=1, sort_keys=True)
    sys.stdout.write("\n")


if __name__ == "__main__":
    main()
