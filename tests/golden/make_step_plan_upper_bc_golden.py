#!/usr/bin/env python3
"""Record tests/golden/step_plan_upper_bc.json: ClearSkyStep's call plan for every case of tests/step_plan_upper_bc.py
(the upper_bc=True option sets), as this tree builds it, on an MI355X with this tree's built library (the default CU caps
in the plan depend on the device's CU count):

    python tests/golden/make_step_plan_upper_bc_golden.py [output.json]

The fixture pins the plans the upper-boundary step tests verified against the oracle
(tests/test_gpu_compute_bc_step.py), so it is re-recorded only together with a change that is meant to move them.  One
case per key, compact separators.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for d in ("oracle", "rte-rrtmgp-nn_amd", "tests"):
    sys.path.insert(0, os.path.join(ROOT, d))


def main():
    import torch
    import step_plan_upper_bc as PU
    from rrtmgpnn import data
    torch.cuda.set_device(0)
    env = PU.environment(data.rfmip_problem())
    plan = {}
    for cid, build in PU.CASES:
        plan[cid] = PU.run_case(build, env)
        print(cid, plan[cid].get("message") or "%d calls" % len(plan[cid]["calls"]), flush=True)
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "step_plan_upper_bc.json")
    os.makedirs(os.path.dirname(os.path.abspath(dst)), exist_ok=True)
    with open(dst, "w") as f:
        f.write("{\n" + ",\n".join("%s:%s" % (json.dumps(k), json.dumps(v, separators=(",", ":")))
                                   for k, v in plan.items()) + "\n}\n")
    print("wrote %s (%d cases, %d bytes)" % (dst, len(plan), os.path.getsize(dst)))


if __name__ == "__main__":
    main()
