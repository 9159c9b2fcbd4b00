"""compute_bc through the Fortran drop-in (rte-rrtmgp-nn_amd/fortran/mo_compute_bc.F90): the host program
tests/fortran/compute_bc.F90, built the way tests/test_fortran_byband.py builds byband.F90, against the comparator of
tests/compute_bc_ref.py, bit for bit, in both orientations; its refusals are checked by the program itself."""
import os
import subprocess

import numpy as np
import pytest

import compute_bc_ref as B
from conftest import ROOT
from test_fortran import FBUILD, FC, _make, needs_fc, write_problem


def _build(tmp_path):
    _make()
    lib = os.path.join(ROOT, "rte-rrtmgp-nn_amd")
    exe = str(tmp_path / "compute_bc")
    r = subprocess.run([FC, "-O1", "-fopenmp", "-I", FBUILD, os.path.join(ROOT, "tests", "fortran", "compute_bc.F90"),
                        "-o", exe, os.path.join(FBUILD, "librrtmgpnn_fortran.a"), "-L" + lib, "-lrrtmgpnn",
                        "-Wl,-rpath," + lib], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return exe


@needs_fc
def test_fortran_compute_bc_program_builds(tmp_path):
    """CPU: mo_compute_bc and its bindings exist and the host program compiles and links."""
    assert os.path.exists(_build(tmp_path))


@pytest.mark.gpu
@needs_fc
@pytest.mark.parametrize("top_at_1", [True, False])
def test_fortran_compute_bc_matches_comparator(tmp_path, orc, rfmip, top_at_1):
    from rrtmgpnn import data, rbin
    exe = _build(tmp_path)
    prob = B.truncated(rfmip, B.COLS["c7"], 3, 5, top_at_1, mixed_gases=False)
    fin, fout = str(tmp_path / "in.rbin"), str(tmp_path / "out.rbin")
    write_problem(prob, fin)
    r = subprocess.run(["timeout", "-k", "10", "120", exe, fin, fout, data.DATA_DIR], capture_output=True, text=True)
    # exit status 6 / 7 / 8: a refusal's string differs or the refused call wrote to flux_bc
    assert r.returncode == 0, r.stdout + r.stderr
    got = rbin.read(fout)
    radn = B.lw(orc, prob)
    np.testing.assert_array_equal(got["bc_lw"], radn)
    np.testing.assert_array_equal(got["bc_lw_flux"], B.in_flux_units(radn))
    np.testing.assert_array_equal(got["bc_sw"], B.sw(orc, prob))
