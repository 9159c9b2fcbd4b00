"""ty_fluxes_byband through the Fortran drop-in (rte-rrtmgp-nn_amd/fortran/mo_fluxes_byband.F90; rte_lw / rte_sw detect
it with select type): the host program tests/fortran/byband.F90, built the way tests/test_fortran.py builds
devstate.F90, against the oracle's g-point outputs reduced by tests/byband_ref.py, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import byband_ref as R
from conftest import ROOT, subset
from test_fortran import FBUILD, FC, _make, needs_fc, write_problem


def _build(tmp_path):
    _make()
    lib = os.path.join(ROOT, "rte-rrtmgp-nn_amd")
    exe = str(tmp_path / "byband")
    r = subprocess.run([FC, "-O1", "-fopenmp", "-I", FBUILD, os.path.join(ROOT, "tests", "fortran", "byband.F90"),
                        "-o", exe, os.path.join(FBUILD, "librrtmgpnn_fortran.a"), "-L" + lib, "-lrrtmgpnn",
                        "-Wl,-rpath," + lib], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return exe


@needs_fc
def test_fortran_byband_program_builds(tmp_path):
    """CPU: mo_fluxes_byband is part of the drop-in and the host program compiles and links against it."""
    assert os.path.exists(_build(tmp_path))
    assert os.path.exists(os.path.join(FBUILD, "mo_fluxes_byband.mod"))


@pytest.mark.gpu
@needs_fc
def test_fortran_byband_matches_oracle(tmp_path, orc, rfmip):
    from oracle import gauss
    from rrtmgpnn import data, rbin
    exe = _build(tmp_path)
    prob = subset(rfmip, np.arange(5, 1800, 300))
    fin, fout = str(tmp_path / "in.rbin"), str(tmp_path / "out.rbin")
    write_problem(prob, fin)
    r = subprocess.run(["timeout", "-k", "10", "120", exe, fin, fout, data.DATA_DIR], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr  # exit status 6 / 7 / 8: an error string of (e) differs
    got = rbin.read(fout)
    kd = data.load_kdist("lw")
    lims = np.asarray(kd["band_lims_gpt"], np.int32).reshape(-1, 2)
    go = orc.lw_gas_optics(prob, [data.load_model("lw_abs"), data.load_model("lw_pfrac")], kd)
    np.testing.assert_array_equal(got["tau"], go["tau"])
    ncol, nlay, ngpt = go["tau"].shape
    emis = np.repeat(np.asarray(prob["sfc_emis"], np.float32)[:, None], ngpt, axis=1)
    args = (go["tau"], go["lay_source"], go["lev_source"], emis, go["sfc_source"], prob["top_at_1"])
    # (a), (c): one angle -- the band sums add fac * radiance; (c)'s g-point arrays are the radiances
    up, dn, gu, gd = orc.lw_solver(*args, 1, gpt=True)
    w = gauss(1)[1][0]
    bu, bd = R.sum_byband(R.lw_one_angle_terms(gu, w, ngpt), lims), R.sum_byband(R.lw_one_angle_terms(gd, w, ngpt), lims)
    for tag in ("a", "c"):
        np.testing.assert_array_equal(got["flux_up_" + tag], up, err_msg=tag)
        np.testing.assert_array_equal(got["flux_dn_" + tag], dn, err_msg=tag)
        np.testing.assert_array_equal(got["bnd_up_" + tag], bu, err_msg=tag)
        np.testing.assert_array_equal(got["bnd_dn_" + tag], bd, err_msg=tag)
    np.testing.assert_array_equal(got["bnd_net_a"], bd - bu)
    np.testing.assert_array_equal(got["gpt_up_c"], gu)
    np.testing.assert_array_equal(got["gpt_dn_c"], gd)
    # (b): three angles
    up, dn, gu, gd = orc.lw_solver(*args, 3, gpt=True)
    for k, want in (("flux_up_b", up), ("flux_dn_b", dn), ("gpt_up_b", gu), ("gpt_dn_b", gd),
                    ("bnd_up_b", R.sum_byband(gu, lims)), ("bnd_dn_b", R.sum_byband(gd, lims))):
        np.testing.assert_array_equal(got[k], want, err_msg=k)
    # (d): rte_sw; the broadband fluxes are the plain solver's (no g-point outputs were asked for)
    t2 = (np.float32(0.1) * go["tau"]).astype(np.float32)
    sw = (t2, np.full_like(t2, 0.5), np.full_like(t2, 0.3), np.full(ncol, 0.6, np.float32),
          np.ones((ncol, ngpt), np.float32), np.full((ncol, ngpt), 0.2, np.float32),
          np.full((ncol, ngpt), 0.2, np.float32), prob["top_at_1"])
    want = orc.sw_solver(*sw, gpt=True)
    b3 = [R.sum_byband(y, lims) for y in want[3:]]
    for k, y in zip(("bnd_up_d", "bnd_dn_d", "bnd_dir_d"), b3):
        np.testing.assert_array_equal(got[k], y, err_msg=k)
    np.testing.assert_array_equal(got["bnd_net_d"], b3[1] - b3[0])
    for k, y in zip(("flux_up_d", "flux_dn_d", "flux_dir_d"), orc.sw_solver(*sw)):
        np.testing.assert_array_equal(got[k], y, err_msg=k)
