"""mo_rrtmgp_clr_all_sky through the Fortran drop-in: the host program rrtmgpnn_clr_all_sky (rrtmgpnn_allsky's command
line and cloud recipe, one rte_lw and one rte_sw call per block) writes the clear-sky and the all-sky fluxes; both sets
against the oracle, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from conftest import subset
from test_fortran import FBUILD, _make, needs_fc, write_problem

EXE = os.path.join(FBUILD, "rrtmgpnn_clr_all_sky")


@needs_fc
def test_fortran_clr_all_sky_builds():
    """CPU: the module is part of librrtmgpnn_fortran.a and the host program links; the LW path binds the dual entry."""
    _make()
    assert os.path.exists(EXE) and os.path.exists(os.path.join(FBUILD, "mo_rrtmgp_clr_all_sky.mod"))
    nm = subprocess.run(["nm", "-u", os.path.join(FBUILD, "librrtmgpnn_fortran.a")], capture_output=True, text=True,
                        check=True).stdout
    assert "rrtmgpnn_lw_solver_noscat_planck_clr_all" in nm


@pytest.mark.gpu
@needs_fc
def test_fortran_clr_all_sky_driver_matches_oracle(tmp_path, orc, rfmip):
    """100 RFMIP columns in blocks of 32 (a ragged last block of 4): all-sky fluxes == the oracle's all-sky pipeline,
    clear-sky fluxes == its clear-sky pipeline, and the two differ in the cloudy columns."""
    from rrtmgpnn import data, rbin
    if not os.path.exists(EXE):
        _make()
    prob = subset(rfmip, np.arange(0, 1800, 18))
    assert prob["ncol"] % 32 != 0
    fin, fout = str(tmp_path / "prob.rbin"), str(tmp_path / "flux.rbin")
    write_problem(prob, fin)
    r = subprocess.run(["timeout", "-k", "10", "300", EXE, fin, fout, data.DATA_DIR, "32"], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    got = rbin.read(fout)
    co_lw, co_sw = data.load_cloud_optics("lw"), data.load_cloud_optics("sw")
    clouds = data.allsky_clouds(prob, co_lw)
    lw = [data.load_model("lw_abs"), data.load_model("lw_pfrac")]
    sw = [data.load_model("sw_abs"), data.load_model("sw_ray")]
    kl, ks = data.load_kdist("lw"), data.load_kdist("sw")
    want = {"": orc.all_sky_lw(prob, lw, kl, co_lw, clouds)[:2] + orc.all_sky_sw(prob, sw, ks, co_sw, clouds)[:3],
            "_clr": orc.clear_sky_lw(prob, lw, kl)[:2] + orc.clear_sky_sw(prob, sw, ks)[:3]}
    use = prob["usecol"]
    for sfx, (lu, ld, su, sd, sr) in want.items():
        for k, ref, g in (("lw_flux_up", lu, got["lw_flux_up" + sfx]), ("lw_flux_dn", ld, got["lw_flux_dn" + sfx]),
                          ("sw_flux_up", su, got["sw_flux_up" + sfx]), ("sw_flux_dn", sd, got["sw_flux_dn" + sfx]),
                          ("sw_flux_dir", sr[use], got["sw_flux_dir" + sfx][use])):
            np.testing.assert_array_equal(g, ref, err_msg=k + sfx + ": not bit-identical")
    cloudy = (clouds[0] > 0).any(axis=1) | (clouds[1] > 0).any(axis=1)
    assert cloudy.sum() * 3 >= prob["ncol"]
    assert (got["lw_flux_dn"][cloudy] != got["lw_flux_dn_clr"][cloudy]).any(axis=1).all()
    np.testing.assert_array_equal(got["lw_flux_dn"][~cloudy], got["lw_flux_dn_clr"][~cloudy])
