#!/usr/bin/env python3
"""Record tests/golden/request_policy.json: what every public solver symbol answers to every combination of armed
requests (the cells of tests/request_policy_cells.py), as given by the library of commit 05a66a3 ("McICA clouds and
aerosols on the daylit-column shortwave chain"), the last one whose csrc/api.cpp held the request ladders that
csrc/requests.cpp replaced.  The fixture pins the policy table to that commit's behaviour, so it is only ever produced
from that commit's library, never from the tree under test:

    git worktree add /tmp/parent 05a66a3 && make -C /tmp/parent/rte-rrtmgp-nn_amd librrtmgpnn.so
    python tests/golden/make_request_policy_golden.py /tmp/parent/rte-rrtmgp-nn_amd/librrtmgpnn.so

on an MI355X (the arming calls need a context).  The library is loaded by path; unless the csrc/api.cpp beside it is
that commit's (git blob a913fb777397) it is refused.  Each distinct (status, message) is stored once, and one index array
per symbol over the cells."""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for d in ("rte-rrtmgp-nn_amd", "tests"):
    sys.path.insert(0, os.path.join(ROOT, d))

COMMIT = "05a66a3"
API_CPP_BLOB = "a913fb777397122e2d992db6e4f2ac0fe1c51b68"  # git hash-object of that commit's csrc/api.cpp


def main():
    if len(sys.argv) not in (2, 3):
        raise SystemExit(__doc__)
    lib = os.path.abspath(sys.argv[1])
    src_path = os.path.join(os.path.dirname(lib), "csrc", "api.cpp")
    with open(src_path, "rb") as f:
        src = f.read()
    blob = hashlib.sha1(b"blob %d\0" % len(src) + src).hexdigest()
    if blob != API_CPP_BLOB:
        raise SystemExit("%s is not commit %s's csrc/api.cpp (git blob %s, expected %s)"
                         % (src_path, COMMIT, blob, API_CPP_BLOB))
    import request_policy_cells as C
    w = C.Walker(C.load(lib))
    answers, symbols = [], {}
    for s in C.SYMBOLS:
        got = w.walk(s)
        for a in got:
            if list(a) not in answers:
                answers.append(list(a))
        symbols[s] = [answers.index(list(a)) for a in got]
        print("%-40s %d cells, %d refused" % (s, len(got), sum(a != C.accepted(s) for a in got)), flush=True)
    w.close()
    dst = sys.argv[2] if len(sys.argv) == 3 else os.path.join(HERE, "request_policy.json")
    head = {"commit": COMMIT, "api_cpp_blob": API_CPP_BLOB, "kinds": C.KINDS, "states": C.STATES, "cells": C.CELLS,
            "answers": answers}
    def lines(d):
        return ",\n".join("%s:%s" % (json.dumps(k), json.dumps(v, separators=(",", ":"))) for k, v in d.items())

    with open(dst, "w") as f:
        f.write("{\n%s,\n\"symbols\":{\n%s\n}\n}\n" % (lines(head), lines(symbols)))
    print("wrote %s (%d symbols x %d cells, %d answers, %d bytes)"
          % (dst, len(symbols), len(C.CELLS), len(answers), os.path.getsize(dst)))


if __name__ == "__main__":
    main()
