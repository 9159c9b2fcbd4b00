#!/usr/bin/env python3
"""Generate tests/golden/mlp_shapes.npz from the REFERENCE itself (oracle/_ref/librrtmgp_ref.so: the reference's
network_type%output_sgemm_flat, neural/mod_network.F90:273, on MKL sgemm).  Run in the build container:

    make -C oracle && python tests/golden/make_mlp_golden.py

The fixture is DATA: for every case of tests/mlp_cases.py the reference can run (all hidden widths equal, at least two
layers, activations linear..hard_sigmoid) the reference library's outputs on mlp_cases.inputs(dims, 17, seed), with the
case's name and seed.  No weights and no inputs: both are regenerated from the seed.  Only the reference library runs
here; the oracle is compared with the file by tests/test_mlp_shapes_host.py.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle as O  # noqa: E402
import mlp_cases as M  # noqa: E402


def main():
    ref = O.Reference()
    out = {"names": np.array([c.name for c in M.REF_CASES]), "seeds": np.array([c.seed for c in M.REF_CASES], np.int64),
           "nbatch": np.int32(M.NBATCH)}
    for c in M.REF_CASES:
        out["y:" + c.name] = ref.mlp(M.model_of(c), M.inputs(c.dims, M.NBATCH, c.seed))
    path = os.path.join(HERE, "mlp_shapes.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d cases, %d bytes)" % (path, len(M.REF_CASES), os.path.getsize(path)))


if __name__ == "__main__":
    main()
