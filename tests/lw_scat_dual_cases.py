"""Clear-sky beside all-sky LW fluxes for scattering clouds, with aerosols (rrtmgpnn_lw_solver_1rescl_planck_clr_all):
the inputs and the composed-oracle expectation shared by tests/test_lw_scat_dual_host.py and
tests/test_gpu_lw_scat_dual.py.

The inputs are tests/lw_scat_cases.py's (its CASES, 3 columns, its designed cloud column) with a 1scl aerosol tau_aer
(NCOL, nlay, nb), lognormal(-1, 1) from default_rng(77 + ng + nlay).  For nlay >= 7 column 1 has a zero-aerosol row at
layer nlay // 2: a zero aerosol is still an increment (at nlay == 1 a zero row would hide the aerosol from that column).

The composed oracle, bit for bit what the entry must give:
  clear set: the no-scattering solve of tau [+ tau_aer by band] (Oracle.increment_bybnd of (tau,) by (tau_aer,));
  all-sky set, no aerosol: lw_scat_cases.expect;
  all-sky set, aerosol: Oracle.increment_bybnd(lims, [tau, 0, 0], [tau_aer]) (inc_2stream_by_1scalar_bybnd), that
  incremented by the cloud -- masked: each band array through mcica_ref.draw at identity limits, as lw_scat_cases.props
  does --, then Oracle.lw_solver(..., ssa=, g=).  The two adds are rounded separately: (tau + tau_aer) + tau_cld."""
import numpy as np

import lw_scat_cases as S
import mcica_ref as M
from lw_scat_cases import CASES, MASKS, NCOL  # noqa: F401

_aer = {}


def aerosol(ng, nlay):
    """tau_aer (NCOL, nlay, nb) of the case, built once and read-only."""
    if (ng, nlay) not in _aer:
        c = S.case(ng, nlay)
        a = np.random.default_rng(77 + ng + nlay).lognormal(-1, 1, (NCOL, nlay, c["nb"])).astype(np.float32)
        if nlay >= 7:
            a[1, nlay // 2] = 0
        a.setflags(write=False)
        _aer[(ng, nlay)] = a
    return _aer[(ng, nlay)]


def cloud(c, mask):
    """(limits, band-or-g-point cloud arrays) that increment_bybnd takes: by band, or sampled at identity limits."""
    arrs = [c["tb"], c["wb"], c["gb"]]
    if mask is None:
        return c["lims"], arrs
    return S._ident(c["ng"]), [M.draw(mask, a, c["lims"]) for a in arrs]


def props(orc, c, mask, aer, order="aer_first"):
    """(tau, ssa, g) of the all-sky set.  order: "aer_first" (the entry's), "cloud_first", or "presummed" (one
    increment by tau_aer + tau_cld, unmasked only) -- the two orders the entry must NOT compute."""
    z = np.zeros_like(c["tau"])
    io = [c["tau"], z, z]
    lims, cl = cloud(c, mask)
    if aer is None:
        return orc.increment_bybnd(lims, io, cl)
    if order == "aer_first":
        return orc.increment_bybnd(lims, orc.increment_bybnd(c["lims"], io, [aer]), cl)
    if order == "cloud_first":
        return orc.increment_bybnd(c["lims"], orc.increment_bybnd(lims, io, cl), [aer])
    assert order == "presummed" and mask is None
    # the aerosol and the cloud as one two-stream set: tau summed, the cloud's scattering over it, the cloud's g
    t = c["tb"] + aer
    w = (c["tb"] * c["wb"]) / np.maximum(t, S.EPS)
    return orc.increment_bybnd(c["lims"], io, [t, w.astype(np.float32), c["gb"]])


def clear_tau(orc, c, aer):
    return c["tau"] if aer is None else orc.increment_bybnd(c["lims"], [c["tau"]], [aer])[0]


def _emis(c, emis_by_band):
    return S.expand(c["emis_bnd"], c["lims"], c["ng"]) if emis_by_band else c["emis_gpt"]


_expect = {}


def expect(orc, c, kind, aer_on, top_at_1, nmus, emis_by_band=True, inc=False):
    """The composed oracle's (flux_up, flux_dn, flux_up_clr, flux_dn_clr) under the mask `kind`; cached."""
    key = (c["ng"], c["nlay"], kind, bool(aer_on), bool(top_at_1), nmus, bool(emis_by_band), bool(inc))
    if key in _expect:
        return _expect[key]
    aer = aerosol(c["ng"], c["nlay"]) if aer_on else None
    lay, lev, sfc, _ = S.sources(orc, c, top_at_1)
    emis = _emis(c, emis_by_band)
    kw = dict(top_at_1=top_at_1, nmus=nmus, inc_flux=c["inc"] if inc else None)
    if aer_on:
        io = props(orc, c, S.mask_for(c, kind), aer)
        all_sky = orc.lw_solver(io[0], lay, lev, emis, sfc, ssa=io[1], g=io[2], **kw)
    else:
        all_sky = S.expect(orc, c, kind, top_at_1, nmus, emis_by_band=emis_by_band, inc=inc)
    ckey = key[:2] + key[3:]
    if ckey not in _expect:
        _expect[ckey] = orc.lw_solver(clear_tau(orc, c, aer), lay, lev, emis, sfc, **kw)
    _expect[key] = tuple(all_sky) + tuple(_expect[ckey])
    return _expect[key]
