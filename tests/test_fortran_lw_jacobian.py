"""flux_up_Jac through the Fortran drop-in (rte_rrtmgp_config_jacobian + rte_lw, rte-rrtmgp-nn_amd/fortran/mo_rte_lw.F90):
the host program tests/fortran/lw_jacobian.F90, built the way tests/test_fortran_byband.py builds byband.F90, against the
oracle's flux_up on zero sources with sfc_source_Jac as the surface source, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import lw_jacobian_ref as J
from conftest import ROOT, subset
from test_fortran import FBUILD, FC, _make, needs_fc, write_problem


def _build(tmp_path):
    _make()
    lib = os.path.join(ROOT, "rte-rrtmgp-nn_amd")
    exe = str(tmp_path / "lw_jacobian")
    r = subprocess.run([FC, "-O1", "-fopenmp", "-I", FBUILD, os.path.join(ROOT, "tests", "fortran", "lw_jacobian.F90"),
                        "-o", exe, os.path.join(FBUILD, "librrtmgpnn_fortran.a"), "-L" + lib, "-lrrtmgpnn",
                        "-Wl,-rpath," + lib], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return exe


@needs_fc
def test_fortran_lw_jacobian_program_builds(tmp_path):
    """CPU: the drop-in's compute_Jac switch and binding exist and the host program compiles and links."""
    assert os.path.exists(_build(tmp_path))


@pytest.mark.gpu
@needs_fc
def test_fortran_lw_jacobian_matches_oracle(tmp_path, orc, rfmip):
    from rrtmgpnn import data, rbin
    exe = _build(tmp_path)
    prob = subset(rfmip, np.arange(5, 1800, 300))
    fin, fout = str(tmp_path / "in.rbin"), str(tmp_path / "out.rbin")
    write_problem(prob, fin)
    r = subprocess.run(["timeout", "-k", "10", "120", exe, fin, fout, data.DATA_DIR], capture_output=True, text=True)
    # exit status 5: written to with the switch off; 6 / 7: an error string differs; 8: flux_dn_Jac written to
    assert r.returncode == 0, r.stdout + r.stderr
    got = rbin.read(fout)
    kd = data.load_kdist("lw")
    go = orc.lw_gas_optics(prob, [data.load_model("lw_abs"), data.load_model("lw_pfrac")], kd)
    np.testing.assert_array_equal(got["tau"], go["tau"])
    ncol, nlay, ngpt = go["tau"].shape
    emis = np.repeat(np.asarray(prob["sfc_emis"], np.float32)[:, None], ngpt, axis=1)
    t1 = prob["top_at_1"]
    src = (go["tau"], go["lay_source"], go["lev_source"], emis, go["sfc_source"], t1)
    jin = (go["tau"], emis, go["sfc_source_Jac"], t1)
    sc = dict(ssa=np.full_like(go["tau"], 0.5), g=np.full_like(go["tau"], 0.3))
    for tag, nmus, kw in (("a", 1, {}), ("b", 3, {}), ("c", 1, sc), ("d", 1, {})):
        up, dn = orc.lw_solver(*src, nmus, **kw)
        np.testing.assert_array_equal(got["flux_up_" + tag], up, err_msg=tag)
        np.testing.assert_array_equal(got["flux_dn_" + tag], dn, err_msg=tag)
        want = J.zero_source_flux_up(orc, *jin, nmus, **kw)
        assert (want > 0).all()
        np.testing.assert_array_equal(got["jac_" + tag], want, err_msg=tag)
    np.testing.assert_array_equal(got["flux_up_off"], got["flux_up_a"])
    np.testing.assert_array_equal(got["flux_dn_off"], got["flux_dn_a"])
