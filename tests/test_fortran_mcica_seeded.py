"""mo_cloud_sampling's seeded functions through the Fortran drop-in: the archive binds the new C entries and the module
exports mcica_randoms, sampled_mask_max_ran_seeded and sampled_mask_exp_ran_seeded; the host program
tests/fortran/mcica_seeded.F90 (built the way tests/test_fortran_byband.py builds its program) against
tests/philox_ref.py and tests/mcica_ref.py, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import mcica_ref as M
import mcica_seeded_cases as C
import philox_ref as P
from conftest import ROOT
from test_fortran import FBUILD, FC, _make, needs_fc

C_ENTRIES = ("rrtmgpnn_mcica_rng_set", "rrtmgpnn_mcica_randoms", "rrtmgpnn_sampled_mask_max_ran_seeded",
             "rrtmgpnn_sampled_mask_exp_ran_seeded")
FUNCTIONS = ("mcica_randoms", "sampled_mask_max_ran_seeded", "sampled_mask_exp_ran_seeded")


def _build(tmp_path, make=True):
    if make:
        _make()
    lib = os.path.join(ROOT, "rte-rrtmgp-nn_amd")
    exe = str(tmp_path / "mcica_seeded")
    r = subprocess.run([FC, "-O1", "-fopenmp", "-I", FBUILD, os.path.join(ROOT, "tests", "fortran", "mcica_seeded.F90"),
                        "-o", exe, os.path.join(FBUILD, "librrtmgpnn_fortran.a"), "-L" + lib, "-lrrtmgpnn",
                        "-Wl,-rpath," + lib], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return exe


@needs_fc
def test_fortran_mcica_seeded_binds_and_exports(tmp_path):
    """CPU: the archive binds the new C entries (nm -u), the module defines the new functions, and a program that uses
    them compiles and links."""
    assert os.path.exists(_build(tmp_path))
    arc = os.path.join(FBUILD, "librrtmgpnn_fortran.a")
    nm = subprocess.run(["nm", "-u", arc], capture_output=True, text=True, check=True).stdout
    for name in C_ENTRIES:
        assert name in nm, name
    defined = [ln.split()[-1].lower() for ln in
               subprocess.run(["nm", "--defined-only", arc], capture_output=True, text=True, check=True).stdout.splitlines()
               if " T " in ln or " t " in ln]
    for name in FUNCTIONS:
        assert any("mo_cloud_sampling" in s and s.endswith(name) for s in defined), name


@pytest.mark.gpu
@needs_fc
def test_fortran_mcica_seeded_program(tmp_path):
    """ngpt 40 (a partial last word), 5 layers (a partial last group), 3 columns; a seed with a non-zero high word and a
    col0 whose global columns wrap."""
    from rrtmgpnn import rbin
    ngpt, nlay, ncol = 40, 5, 3
    seed, stream, col0 = C.SEEDS[1] & 0x7FFFFFFFFFFFFFFF, 2 ** 31 + 5, 2 ** 32 - 2
    cf, ov = C.inputs(ngpt, nlay, ncol)
    fin, fout = str(tmp_path / "in.rbin"), str(tmp_path / "out.rbin")
    rbin.write(fin, {"cloud_frac": cf, "overlap_param": ov})
    exe = _build(tmp_path, make=not os.path.exists(os.path.join(FBUILD, "librrtmgpnn_fortran.a")))
    r = subprocess.run(["timeout", "-k", "10", "120", exe, fin, fout, str(ngpt), str(seed), str(stream), str(col0)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    got = rbin.read(fout)
    want_r = P.randoms(seed, stream, col0, ngpt, nlay, ncol)
    np.testing.assert_array_equal(got["randoms"].view(np.uint32), want_r.view(np.uint32))
    for name, o in (("mask_max_ran", None), ("mask_exp_ran", ov)):
        want = M.sampled_mask(want_r, cf, o)
        assert want[cf > 0].any() and not want[cf > 0].all()
        np.testing.assert_array_equal(got[name], want.astype(np.float32), err_msg=name)
    assert (got["mask_max_ran"] != got["mask_exp_ran"]).any()
