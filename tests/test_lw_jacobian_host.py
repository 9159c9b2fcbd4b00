"""CPU: the definition of flux_up_Jac (rrtmgpnn_solver_request_jacobian; include/rrtmgpnn.h) against the oracle.

(a) the direct recurrence -- J = emis * sfc_source_Jac, J = T * J, flux_up's sums -- equals the oracle's flux_up on zero
    sources with sfc_source_Jac as the surface source, bit for bit, also through the rescaled solver;
(b) where the reference's own rte_lw is built (oracle/_ref), it gives the oracle's bits on those zero-source inputs;
(c) it is a derivative: flux_up(sfc_source + sfc_source_Jac) - flux_up(sfc_source) against it;
(d) the entry is declared, bound and exported;
(e) the Fortran host program builds: tests/test_fortran_lw_jacobian.py.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import lw_jacobian_ref as J
from conftest import ROOT, subset


@pytest.mark.parametrize("top_at_1", [True, False])
@pytest.mark.parametrize("nmus", [1, 3])
@pytest.mark.parametrize("nlay", [1, 2, 5, 9])
@pytest.mark.parametrize("ngpt", [256, 254, 60])
def test_direct_recurrence_is_zero_source_flux_up(orc, ngpt, nlay, nmus, top_at_1):
    c = J.random_case(ngpt, nlay, seed=31)
    want = J.zero_source_flux_up(orc, c["tau"], c["emis"], c["sjac"], top_at_1, nmus)
    got = J.direct_jacobian(orc, c["tau"], c["emis"], c["sjac"], top_at_1, nmus)
    assert np.isfinite(want).all() and (want > 0).all()
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("top_at_1", [True, False])
@pytest.mark.parametrize("nmus", [1, 3])
@pytest.mark.parametrize("ngpt,nlay", [(256, 9), (254, 5), (60, 2), (60, 1)])
def test_direct_recurrence_rescaled(orc, ngpt, nlay, nmus, top_at_1):
    """The rescaled solver (lw_transport_1rescl): its adjustment term vanishes on zero sources, so U = trans * U with the
    rescaled transmittance."""
    c = J.random_case(ngpt, nlay, seed=32, scat=True)
    want = J.zero_source_flux_up(orc, c["tau"], c["emis"], c["sjac"], top_at_1, nmus, ssa=c["ssa"], g=c["g"])
    got = J.direct_jacobian(orc, c["tau"], c["emis"], c["sjac"], top_at_1, nmus, ssa=c["ssa"], g=c["g"])
    plain = J.zero_source_flux_up(orc, c["tau"], c["emis"], c["sjac"], top_at_1, nmus)
    assert (want != plain).any(), "the scattering does not show in the rescaled Jacobian"
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("flipped", [False, True])
@pytest.mark.parametrize("nmus", [1, 3])
def test_reference_rte_lw_on_zero_sources(orc, rfmip, nmus, flipped):
    """(b) the reference's compiled rte_lw, zero sources and sfc_source_Jac as the surface source, in the RFMIP columns'
    own orientation and flipped."""
    import oracle as O
    from rrtmgpnn import data
    try:
        ref = O.Reference()
    except FileNotFoundError as e:
        pytest.skip(str(e))
    prob = subset(rfmip, np.arange(3, 1800, 230))
    kd = data.load_kdist("lw")
    go = orc.lw_gas_optics(prob, [data.load_model("lw_abs"), data.load_model("lw_pfrac")], kd)
    tau, sjac, top_at_1 = go["tau"], go["sfc_source_Jac"], bool(prob["top_at_1"])
    if flipped:
        tau, top_at_1 = np.ascontiguousarray(tau[:, ::-1]), not top_at_1
    emis_band = np.repeat(np.asarray(prob["sfc_emis"], np.float32)[:, None], kd["nband"], axis=1)
    emis = np.repeat(np.asarray(prob["sfc_emis"], np.float32)[:, None], kd["ngpt"], axis=1)
    want = J.zero_source_flux_up(orc, tau, emis, sjac, top_at_1, nmus)
    got = ref.rte_lw(kd, tau, np.zeros_like(tau), np.zeros_like(go["lev_source"]), sjac, sjac, emis_band, top_at_1, nmus)[0]
    assert (want > 0).all()
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("nmus", [1, 3])
def test_it_is_a_derivative(orc, nmus):
    """(c) flux_up is affine in the surface source, so flux_up(sfc_source + sfc_source_Jac) - flux_up(sfc_source) is the
    Jacobian up to the rounding of the two fluxes.  Measured on these inputs with the oracle alone: the largest
    difference is 1.87 (one angle) and 5.43 (three angles) float32 epsilons of max |flux_up| (DIFF_EPS); the bound is
    four times that (both fluxes carry their own rounding, and the margin covers another seed)."""
    c = J.random_case(256, 9, seed=33)
    args = (c["tau"], c["lay"], c["lev"], c["emis"])
    up0 = orc.lw_solver(*args, c["sfc"], True, nmus)[0]
    up1 = orc.lw_solver(*args, (c["sfc"] + c["sjac"]).astype(np.float32), True, nmus)[0]
    jac = J.zero_source_flux_up(orc, c["tau"], c["emis"], c["sjac"], True, nmus)
    diff = np.abs((up1.astype(np.float64) - up0) - jac).max() / (J.EPS * np.abs(up1).max())
    print("derivative check, nmus %d: %.2f eps of max |flux_up|" % (nmus, diff))
    assert jac.min() > 100 * J.EPS * np.abs(up1).max(), "the Jacobian is lost in the fluxes' rounding"
    assert diff <= 4 * DIFF_EPS[nmus]


# measured with the oracle on test_it_is_a_derivative's inputs (float32 epsilons of max |flux_up|)
DIFF_EPS = {1: 1.87, 3: 5.43}


def test_entry_is_declared_bound_and_exported():
    """(d)"""
    from rrtmgpnn import _lib
    name = "rrtmgpnn_solver_request_jacobian"
    header = open(os.path.join(ROOT, "include", "rrtmgpnn.h")).read()
    fortran = open(os.path.join(ROOT, "rte-rrtmgp-nn_amd", "fortran", "mo_rrtmgpnn_c.F90")).read()
    m = re.search(r"int %s\(([^;]*)\);" % name, header)
    assert m, name
    args = [a.strip().split()[-1].lstrip("*") for a in m.group(1).replace("\n", " ").split(",")]
    assert args == ["ctx", "ngpt", "nlay", "ncol", "sfc_source_Jac", "flux_up_Jac"]
    assert len(_lib.SIGNATURES[name][1]) == 6
    assert 'name="%s"' % name in fortran and "c_" + name in fortran
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name), name + " is not exported by librrtmgpnn.so"
