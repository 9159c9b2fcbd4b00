"""LW scattering clouds through the Fortran drop-in: mo_rrtmgp_clr_all_sky's rte_lw with by-band 2str clouds (the host
program tests/fortran/lw_scat_allsky.F90, built the way tests/test_fortran_aerosol.py builds its program) takes the
fused scattering route (rrtmgpnn_lw_solver_noscat_planck, then rrtmgpnn_lw_solver_1rescl_planck_inc).  Its four flux
arrays equal the Python class layer's (rrtmgpnn.clr_all_sky.rte_lw on the same arrays) and the composed oracle's bit for
bit."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, subset
from test_fortran import FBUILD, FC, _make, needs_fc, write_problem

KEYS = ("up", "dn", "up_clr", "dn_clr")


def _build(tmp_path):
    _make()
    lib = os.path.join(ROOT, "rte-rrtmgp-nn_amd")
    exe = str(tmp_path / "lw_scat_allsky")
    r = subprocess.run([FC, "-O1", "-fopenmp", "-I", FBUILD, os.path.join(ROOT, "tests", "fortran", "lw_scat_allsky.F90"),
                        "-o", exe, os.path.join(FBUILD, "librrtmgpnn_fortran.a"), "-L" + lib, "-lrrtmgpnn",
                        "-Wl,-rpath," + lib], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return exe


def band_arrays(ncol, nlay, nbnd):
    """The program's synthetic band clouds (its header comment), (ncol, nlay, nbnd) float32: tau, ssa, g."""
    f = np.float32
    ic, il, ib = np.meshgrid(np.arange(1, ncol + 1), np.arange(1, nlay + 1), np.arange(1, nbnd + 1), indexing="ij")
    tau = f(0.05) * (1 + (3 * ib + 5 * il + 7 * ic) % 13).astype(f)
    ssa = f(0.2) + f(0.05) * ((ib + 2 * il + 3 * ic) % 14).astype(f)
    g = f(0.5) + f(0.03) * ((2 * ib + il + 5 * ic) % 15).astype(f)
    return tau.astype(f), ssa.astype(f), g.astype(f)


@needs_fc
def test_fortran_lw_scat_program_builds_and_binds_the_entry(tmp_path):
    """CPU: the host program compiles and links, and the Fortran layer calls the new entry."""
    assert os.path.exists(_build(tmp_path))
    nm = subprocess.run(["nm", "-u", os.path.join(FBUILD, "librrtmgpnn_fortran.a")], capture_output=True, text=True,
                        check=True).stdout
    assert "rrtmgpnn_lw_solver_1rescl_planck_inc" in nm


@pytest.mark.gpu
@needs_fc
def test_fortran_rte_lw_with_scattering_clouds_matches_the_class_layer(tmp_path, orc, rfmip):
    torch = pytest.importorskip("torch")
    from rrtmgpnn import api, clr_all_sky, data, rbin
    exe = _build(tmp_path)
    prob = subset(rfmip, np.arange(7, 1800, 150))  # 12 columns
    ncol, nlay = prob["ncol"], prob["nlay"]
    fin, fout = str(tmp_path / "in.rbin"), str(tmp_path / "out.rbin")
    write_problem(prob, fin)
    r = subprocess.run(["timeout", "-k", "10", "120", exe, fin, fout, data.DATA_DIR], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    got = rbin.read(fout)
    # the Python class layer on the same arrays
    dev = torch.device("cuda", 0)
    T = lambda a: torch.as_tensor(np.array(a, dtype=np.float32), device=dev)  # noqa: E731
    kd = api.GasOpticsRRTMGP()
    api.stop_on_err(kd.load("lw"))
    nets = [api.RrtmgpNetwork(0).load_netcdf(data.path(n)) for n in ("lw_abs", "lw_pfrac")]
    gc = api.GasConcs()
    api.stop_on_err(gc.init(list(prob["gases"])))
    for k, v in prob["gases"].items():
        api.stop_on_err(gc.set_vmr(k, T(v)))
    nb, ng = kd.get_nband(), kd.get_ngpt()
    cloud = band_arrays(ncol, nlay, nb)
    cld = api.OpticalProps2str()
    assert cld.init(kd.get_band_lims_wavenumber()) == "" and cld.alloc_2str(ncol, nlay, device=dev) == ""
    for name, a in zip(("tau", "ssa", "g"), cloud):
        getattr(cld, name).copy_(T(a))
    emis = T(np.repeat(np.asarray(prob["sfc_emis"], np.float32)[:, None], nb, axis=1))
    outs = [torch.full((ncol, nlay + 1), float("nan"), device=dev) for _ in range(4)]
    e = clr_all_sky.rte_lw(kd, gc, T(prob["play"]), T(prob["tlay"]), T(prob["plev"]), T(prob["tsfc"]), emis, cld,
                           api.FluxesBroadband(flux_up=outs[0], flux_dn=outs[1]),
                           api.FluxesBroadband(flux_up=outs[2], flux_dn=outs[3]), t_lev=T(prob["tlev"]),
                           neural_nets=nets)
    assert e == "", e
    torch.cuda.synchronize()
    py = {k: o.cpu().numpy() for k, o in zip(KEYS, outs)}
    # the composed oracle
    kl = data.load_kdist("lw")
    go = orc.lw_gas_optics(prob, [data.load_model("lw_abs"), data.load_model("lw_pfrac")], kl)
    z = np.zeros_like(go["tau"])
    io = orc.increment_bybnd(kl["band_lims_gpt"], (go["tau"], z, z), cloud)
    emis_g = np.repeat(np.asarray(prob["sfc_emis"], np.float32)[:, None], ng, axis=1)
    src = (go["lay_source"], go["lev_source"], emis_g, go["sfc_source"], prob["top_at_1"], 1)
    want = dict(zip(KEYS, orc.lw_solver(io[0], *src, ssa=io[1], g=io[2]) + orc.lw_solver(go["tau"], *src)))
    for k in KEYS:
        assert np.isfinite(got[k + "_bnd"]).all()
        np.testing.assert_array_equal(got[k + "_bnd"], py[k], err_msg=k + ": Fortran against the Python class layer")
        np.testing.assert_array_equal(got[k + "_bnd"], want[k], err_msg=k + ": Fortran against the oracle")
    # the clouds show
    assert (got["dn_bnd"] != got["dn_clr_bnd"]).any(axis=1).all()
