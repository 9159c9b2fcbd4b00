"""CPU: the clear + all-sky interface is declared consistently in every layer, and the Python class functions' extent
checks return the reference's messages (extensions/mo_rrtmgp_clr_all_sky.F90) before anything touches a device."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("rrtmgpnn_lw_solver_noscat_planck_clr_all", "rrtmgpnn_context_set_lw_clr_all")


def test_entries_are_declared_in_every_layer():
    from rrtmgpnn import _lib
    header = open(os.path.join(ROOT, "include", "rrtmgpnn.h")).read()
    fortran = open(os.path.join(ROOT, "rte-rrtmgp-nn_amd", "fortran", "mo_rrtmgpnn_c.F90")).read()
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES, name
        assert re.search(r'bind\(C,\s*name="%s"\)' % name, fortran), name
    assert "extensions/mo_rrtmgp_clr_all_sky.F90:146-172" in header
    # the dual entry: _planck_inc's arguments plus the two clear-sky outputs
    inc = _lib.SIGNATURES["rrtmgpnn_lw_solver_noscat_planck_inc"]
    both = _lib.SIGNATURES["rrtmgpnn_lw_solver_noscat_planck_clr_all"]
    assert both[0] is inc[0] and both[1][:len(inc[1])] == inc[1] and len(both[1]) == len(inc[1]) + 2
    L = _lib.lib()
    assert L.rrtmgpnn_context_set_lw_clr_all(None, 3) != 0 and b"clr_all mode" in L.rrtmgpnn_last_error()
    for mode in (1, 2, 0):
        assert L.rrtmgpnn_context_set_lw_clr_all(None, mode) == 0


class _Spec:
    """A k-distribution's sizes, as much as the extent checks read."""

    def __init__(self, ngpt, nband):
        self.ngpt, self.nband = ngpt, nband

    def get_ngpt(self):
        return self.ngpt

    def get_nband(self):
        return self.nband


class _Aer:
    def __init__(self, ncol, nlay, ngpt):
        self.s = (ncol, nlay, ngpt)

    def get_ncol(self):
        return self.s[0]

    def get_nlay(self):
        return self.s[1]

    def get_ngpt(self):
        return self.s[2]


def test_extent_checks_return_the_reference_strings_without_a_device():
    from rrtmgpnn import clr_all_sky
    ncol, nlay, k = 3, 5, _Spec(256, 16)
    z = lambda *s: np.zeros(s, np.float32)  # noqa: E731
    lw = lambda **kw: clr_all_sky.rte_lw(k, None, z(ncol, nlay), z(ncol, nlay), z(ncol, nlay + 1), z(ncol),  # noqa: E731
                                         z(ncol, 16), None, None, None, **kw)
    assert lw(t_lev=z(ncol, nlay)) == "rrtmpg_lw: t_lev inconsistently sized"
    assert lw(inc_flux=z(ncol, 255)) == "rrtmpg_lw: incident flux inconsistently sized"
    assert lw(aer_props=_Aer(ncol, nlay + 1, 256)) == "rrtmpg_lw: aerosol properties inconsistently sized"
    # the last failing check wins, as in the reference
    assert lw(aer_props=_Aer(ncol + 1, nlay, 16), t_lev=z(ncol + 1, nlay + 1)) == "rrtmpg_lw: t_lev inconsistently sized"
    sw = lambda **kw: clr_all_sky.rte_sw(k, None, z(ncol, nlay), z(ncol, nlay), z(ncol, nlay + 1), z(ncol),  # noqa: E731
                                         z(ncol, 16), z(ncol, 16), None, None, None, **kw)
    assert sw(inc_flux=z(ncol, 256), tsi_scaling=1.0) == "rrtmpg_sw: only one of inc_flux, tsi_scaling may be supplied."
    assert sw(tsi_scaling=0.0) == "rrtmpg_sw: tsi_scaling is < 0"
    assert sw(inc_flux=z(ncol, 2)) == "rrtmpg_sw: incident flux inconsistently sized"
    assert sw(aer_props=_Aer(ncol, nlay - 1, 16)) == "rrtmpg_sw: aerosol properties inconsistently sized"
    # the reference's second aerosol check only fires when ngpt == nband
    assert clr_all_sky.rte_lw(_Spec(16, 16), None, z(ncol, nlay), z(ncol, nlay), z(ncol, nlay + 1), z(ncol), z(ncol, 16),
                              None, None, None, aer_props=_Aer(ncol, nlay, 16)) == \
        "rrtmpg_lw: aerosol properties inconsistently sized"


def test_step_refuses_clrsky_with_byband_before_any_device_work():
    import pytest
    from rrtmgpnn.pipeline import ClearSkyStep
    with pytest.raises(ValueError, match="by-band clear-sky fluxes"):
        ClearSkyStep({}, clouds=(), clrsky=True, byband=True)
    with pytest.raises(ValueError, match="need clouds"):
        ClearSkyStep({}, clrsky=True)
