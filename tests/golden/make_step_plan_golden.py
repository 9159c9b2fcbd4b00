#!/usr/bin/env python3
"""Record tests/golden/step_plan.json: ClearSkyStep's call plan for every case of tests/step_plan.py, as built by the
pipeline.py of commit 67cf983 ("By-band fluxes under McICA masks"), the last one before the constructor was split into
steps.  The fixture pins the refactored constructor to that commit's behaviour, so it is only ever produced from that
file, never from the tree under test:

    git show 67cf983:rte-rrtmgp-nn_amd/rrtmgpnn/pipeline.py > /tmp/parent/pipeline.py
    python tests/golden/make_step_plan_golden.py /tmp/parent/pipeline.py

on an MI355X, with this tree's built library (the default CU caps in the plan depend on the device's CU count).  The
file given is loaded in place of rrtmgpnn.pipeline; any file but that commit's (git blob 4da20124e034) is refused.
One case per key, compact separators.
"""
import hashlib
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for d in ("oracle", "rte-rrtmgp-nn_amd", "tests"):
    sys.path.insert(0, os.path.join(ROOT, d))

COMMIT = "67cf983"
PIPELINE_BLOB = "4da20124e03400860e96f033608b4f6f2d29c621"  # git hash-object of that commit's pipeline.py


def load_pinned_pipeline(path):
    with open(path, "rb") as f:
        src = f.read()
    blob = hashlib.sha1(b"blob %d\0" % len(src) + src).hexdigest()
    if blob != PIPELINE_BLOB:
        raise SystemExit("%s is not commit %s's rrtmgpnn/pipeline.py (git blob %s, expected %s)"
                         % (path, COMMIT, blob, PIPELINE_BLOB))
    import rrtmgpnn
    spec = importlib.util.spec_from_file_location("rrtmgpnn.pipeline", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules["rrtmgpnn.pipeline"] = rrtmgpnn.pipeline = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    pipeline = load_pinned_pipeline(sys.argv[1])
    import torch
    import step_plan as P
    from rrtmgpnn import data
    torch.cuda.set_device(0)
    env = P.environment(data.rfmip_problem())
    plan = {}
    for cid, build in P.CASES:
        plan[cid] = P.run_case(build, env, pipeline.ClearSkyStep)
        print(cid, plan[cid].get("message") or "%d calls" % len(plan[cid]["calls"]), flush=True)
    dst = os.path.join(HERE, "step_plan.json")
    with open(dst, "w") as f:
        f.write("{\n" + ",\n".join("%s:%s" % (json.dumps(k), json.dumps(v, separators=(",", ":")))
                                   for k, v in plan.items()) + "\n}\n")
    print("wrote %s (%d cases, %d bytes)" % (dst, len(plan), os.path.getsize(dst)))


if __name__ == "__main__":
    main()
