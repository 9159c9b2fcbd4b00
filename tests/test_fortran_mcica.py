"""mo_cloud_sampling through the Fortran drop-in: the module is part of librrtmgpnn_fortran.a and binds the new C
entries; the host program rrtmgpnn_mcica (rrtmgpnn_allsky's command line and cloud recipe plus an RBIN with the cloud
fraction and the random numbers; per block cloud_optics -> mask -> draw_samples -> increment -> rte_*) against the
composed oracle, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import mcica_ref as M
from conftest import subset
from test_fortran import FBUILD, _make, needs_fc, write_problem

EXE = os.path.join(FBUILD, "rrtmgpnn_mcica")


@needs_fc
def test_fortran_mcica_builds_and_binds():
    """CPU: the module and the program build, and the archive binds the new C entries (nm -u)."""
    _make()
    assert os.path.exists(EXE) and os.path.exists(os.path.join(FBUILD, "mo_cloud_sampling.mod"))
    nm = subprocess.run(["nm", "-u", os.path.join(FBUILD, "librrtmgpnn_fortran.a")], capture_output=True, text=True,
                        check=True).stdout
    for name in ("rrtmgpnn_sampled_mask_max_ran", "rrtmgpnn_sampled_mask_exp_ran", "rrtmgpnn_draw_samples"):
        assert name in nm, name
    syms = subprocess.run(["nm", os.path.join(FBUILD, "librrtmgpnn_fortran.a")], capture_output=True, text=True,
                          check=True).stdout.lower()
    for name in ("sampled_mask_max_ran", "sampled_mask_exp_ran", "draw_samples"):
        assert "mo_cloud_sampling" in syms and name in syms


@pytest.mark.gpu
@needs_fc
@pytest.mark.parametrize("overlap", ["max_ran", "exp_ran"])
def test_fortran_mcica_driver_matches_oracle(tmp_path, orc, rfmip, overlap):
    """36 RFMIP columns in blocks of 16 (a ragged last block of 4)."""
    from rrtmgpnn import data, rbin
    if not os.path.exists(EXE):
        _make()
    prob = subset(rfmip, np.arange(0, 1800, 50))
    ncol, nlay = prob["ncol"], prob["nlay"]
    assert ncol == 36
    clouds = data.allsky_clouds(prob, data.load_cloud_optics("lw"))
    cloudy = (clouds[0] > 0) | (clouds[1] > 0)
    rng = np.random.default_rng(41)
    cf = np.where(cloudy, rng.uniform(0.2, 0.9, cloudy.shape), 0).astype(np.float32)
    r_lw = rng.random((ncol, nlay, data.load_kdist("lw")["ngpt"]), dtype=np.float32)
    r_sw = rng.random((ncol, nlay, data.load_kdist("sw")["ngpt"]), dtype=np.float32)
    arrays = {"cloud_frac": cf, "randoms_lw": r_lw, "randoms_sw": r_sw}
    ov = None
    if overlap == "exp_ran":
        ov = arrays["overlap_param"] = rng.uniform(-1, 1, (ncol, nlay - 1)).astype(np.float32)
    fin, fmc, fout = str(tmp_path / "prob.rbin"), str(tmp_path / "mcica.rbin"), str(tmp_path / "flux.rbin")
    write_problem(prob, fin)
    rbin.write(fmc, arrays)
    r = subprocess.run(["timeout", "-k", "10", "300", EXE, fin, fout, data.DATA_DIR, fmc, "16"], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    got = rbin.read(fout)
    want = M.step_oracle(orc, prob, clouds, cf, ov, r_lw, r_sw)
    use = prob["usecol"]
    np.testing.assert_array_equal(got["lw_flux_up"], want["lw_up"])
    np.testing.assert_array_equal(got["lw_flux_dn"], want["lw_dn"])
    for k in ("up", "dn", "dir"):
        np.testing.assert_array_equal(got["sw_flux_" + k][use], want["sw_" + k][use], err_msg=k)
    assert not got["sw_flux_up"][~use].any()
