#!/usr/bin/env python3
"""Surrogate k-distribution tables for the reduced-resolution (2021) networks as files: kdist_lw_g128.rbin (16 bands x 8
g-points) and kdist_sw_g112.rbin (14 bands x 8 g-points), derived from the committed g256 / g224 surrogates alone by
rrtmgpnn.data.reduce_kdist -- the tables data.load_kdist(which, ngpt) forms in memory.  Hosts that read files (the
Fortran host program's k-distribution arguments) write them where they need them; the copies under tests/golden/ pin
the derivation byte for byte (tests/test_reduced_spectral_host.py).

    python tools/make_reduced_kdist.py [outdir]     (default: tests/golden)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rte-rrtmgp-nn_amd"))
from rrtmgpnn import data, rbin  # noqa: E402

FILES = {"lw": "kdist_lw_g128.rbin", "sw": "kdist_sw_g112.rbin"}


def main(outdir):
    """Write the two files into outdir; returns their paths (LW, SW)."""
    os.makedirs(outdir, exist_ok=True)
    paths = []
    for which, name in FILES.items():
        full = rbin.read(os.path.join(data.DATA_DIR, data.KDIST_FILES[which]))
        paths.append(os.path.join(outdir, name))
        rbin.write(paths[-1], data.reduce_kdist(full))
    return paths


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden"))
