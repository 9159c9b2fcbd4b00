"""Scattering clouds with aerosols through the Fortran drop-in: mo_rrtmgp_clr_all_sky's rte_lw with by-band two-stream
clouds and by-band 1scl aerosols (the host program tests/fortran/lw_scat_dual.F90, built the way
tests/test_fortran_aerosol.py builds its program) arms rrtmgpnn_solver_request_aerosol and calls
rrtmgpnn_lw_solver_1rescl_planck_clr_all.  Its four flux arrays equal the Python class layer's
(rrtmgpnn.clr_all_sky.rte_lw on the same arrays) and the composed oracle's bit for bit; without aerosols the route is
the one of before."""
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
    exe = str(tmp_path / "lw_scat_dual")
    r = subprocess.run([FC, "-O1", "-fopenmp", "-I", FBUILD, os.path.join(ROOT, "tests", "fortran", "lw_scat_dual.F90"),
                        "-o", exe, os.path.join(FBUILD, "librrtmgpnn_fortran.a"), "-L" + lib, "-lrrtmgpnn",
                        "-Wl,-rpath," + lib], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return exe


def band_arrays(ncol, nlay, nbnd):
    """The program's synthetic band properties (its header comment), (ncol, nlay, nbnd) float32: cloud tau, ssa, g and
    the aerosol's tau."""
    f = np.float32
    ic, il, ib = np.meshgrid(np.arange(1, ncol + 1), np.arange(1, nlay + 1), np.arange(1, nbnd + 1), indexing="ij")
    tau = f(0.05) * (1 + (3 * ib + 5 * il + 7 * ic) % 13).astype(f)
    ssa = f(0.2) + f(0.05) * ((ib + 2 * il + 3 * ic) % 14).astype(f)
    g = f(0.5) + f(0.03) * ((2 * ib + il + 5 * ic) % 15).astype(f)
    aer = f(0.01) * (1 + (ib + 3 * il + 11 * ic) % 17).astype(f)
    return tau.astype(f), ssa.astype(f), g.astype(f), aer.astype(f)


@needs_fc
def test_fortran_lw_scat_dual_program_builds_and_binds_the_entry(tmp_path):
    """CPU: the host program compiles and links, and the Fortran layer calls the new entry and the request."""
    assert os.path.exists(_build(tmp_path))
    nm = subprocess.run(["nm", "-u", os.path.join(FBUILD, "librrtmgpnn_fortran.a")], capture_output=True, text=True,
                        check=True).stdout
    assert "rrtmgpnn_lw_solver_1rescl_planck_clr_all" in nm and "rrtmgpnn_solver_request_aerosol" in nm


@pytest.mark.gpu
@needs_fc
def test_fortran_rte_lw_scattering_clouds_with_aerosols_matches_the_class_layer(tmp_path, orc, rfmip):
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
    T = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=dev)  # noqa: E731
    kd = api.GasOpticsRRTMGP()
    api.stop_on_err(kd.load("lw"))
    nets = [api.RrtmgpNetwork(0).load_netcdf(data.path(n)) for n in ("lw_abs", "lw_pfrac")]
    gc = api.GasConcs()
    api.stop_on_err(gc.init(list(prob["gases"])))
    for k, v in prob["gases"].items():
        api.stop_on_err(gc.set_vmr(k, T(v)))
    nb, ng = kd.get_nband(), kd.get_ngpt()
    ct, cw, cg, aer = band_arrays(ncol, nlay, nb)
    cld = api.OpticalProps2str()
    assert cld.init(kd.get_band_lims_wavenumber()) == "" and cld.alloc_2str(ncol, nlay, device=dev) == ""
    cld.tau.copy_(T(ct))
    cld.ssa.copy_(T(cw))
    cld.g.copy_(T(cg))
    ap = api.OpticalProps1scl()
    assert ap.init(kd.get_band_lims_wavenumber()) == "" and ap.alloc_1scl(ncol, nlay, device=dev) == ""
    ap.tau.copy_(T(aer))
    emis = T(np.repeat(np.asarray(prob["sfc_emis"], np.float32)[:, None], nb, axis=1))
    py = {}
    for tag, a in (("bnd", ap), ("none", None)):
        outs = [torch.full((ncol, nlay + 1), float("nan"), device=dev) for _ in range(4)]
        e = clr_all_sky.rte_lw(kd, gc, T(prob["play"]), T(prob["tlay"]), T(prob["plev"]), T(prob["tsfc"]), emis, cld,
                               api.FluxesBroadband(flux_up=outs[0], flux_dn=outs[1]),
                               api.FluxesBroadband(flux_up=outs[2], flux_dn=outs[3]), aer_props=a,
                               t_lev=T(prob["tlev"]), neural_nets=nets)
        assert e == "", e
        torch.cuda.synchronize()
        py[tag] = {k: o.cpu().numpy() for k, o in zip(KEYS, outs)}
    # the composed oracle: the aerosol (1scl into the 2str gas set), then the cloud, the rescaled solver
    kl = data.load_kdist("lw")
    go = orc.lw_gas_optics(prob, [data.load_model("lw_abs"), data.load_model("lw_pfrac")], kl)
    z = np.zeros_like(go["tau"])
    io = orc.increment_bybnd(kl["band_lims_gpt"], (go["tau"], z, z), (aer,))
    (ta,) = orc.increment_bybnd(kl["band_lims_gpt"], (go["tau"],), (aer,))
    io = orc.increment_bybnd(kl["band_lims_gpt"], io, (ct, cw, cg))
    emis_g = np.repeat(np.asarray(prob["sfc_emis"], np.float32)[:, None], ng, axis=1)
    src = (go["lay_source"], go["lev_source"], emis_g, go["sfc_source"], prob["top_at_1"], 1)
    want = dict(zip(KEYS, orc.lw_solver(io[0], *src, ssa=io[1], g=io[2]) + orc.lw_solver(ta, *src)))
    for k in KEYS:
        for tag in ("bnd", "none"):
            f = got["%s_%s" % (k, tag)]
            assert np.isfinite(f).all()
            np.testing.assert_array_equal(np.ascontiguousarray(f, np.float32).view(np.uint32),
                                          np.ascontiguousarray(py[tag][k], np.float32).view(np.uint32),
                                          err_msg="%s (%s): Fortran against the Python class layer" % (k, tag))
        np.testing.assert_array_equal(np.ascontiguousarray(got[k + "_bnd"], np.float32).view(np.uint32),
                                      want[k].view(np.uint32), err_msg=k + ": Fortran against the oracle")
    # the aerosols show in both sets, the cloud beside the clear set
    assert (got["dn_clr_none"] != got["dn_clr_bnd"]).any(axis=1).all()
    assert (got["dn_none"] != got["dn_bnd"]).any(axis=1).all()
    assert (got["dn_bnd"] != got["dn_clr_bnd"]).any()
