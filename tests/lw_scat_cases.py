"""Fused all-sky LW solve with scattering clouds (rrtmgpnn_lw_solver_1rescl_planck_inc): the inputs and the
composed-oracle expectation shared by tests/test_lw_scat_allsky_host.py (which establishes on the CPU that the masks,
ssa_bnd and g_bnd all show in the expected fluxes) and tests/test_gpu_lw_scat_allsky.py.

The composed oracle, bit for bit what the fused entry must give:
  Oracle.planck_source; Oracle.increment_bybnd of (tau, 0, 0) by (tau_bnd, ssa_bnd, g_bnd) on the band limits -- masked:
  by mcica_ref.draw of each band array, at identity limits --; Oracle.lw_solver(..., ssa=, g=), the rescaled solver.

Shapes, the smallest that reach every code path of the kernel: 3 columns;
  (256, 7)  the shipped g-points, one partial ring chunk of 8;
  (256, 11) a full chunk and a partial one;
  (72, 7)   two bands, the second wave partial, the last mask word partial;
  (72, 8)   nlay equal to one flush ring (kScatRing = 8): the chunk walk ends on a full ring with no partial chunk behind
            it, and the prefetch clamps on the ring boundary;
  (30, 7)   ngpt % 4 != 0: the sequential broadband sum of bare radiances (quirk B-5);
  (30, 16)  nlay equal to two flush rings, with the sequential sum;
  (30, 1)   one layer: lev(l+1)'s Planck fraction is the layer's own (min(l+1, nlay-1)).
Column 2 is designed (DESIGNED): a layer with tau_bnd = 0 (and a negative g_bnd in band 0: the sign of the zero g
depends on the gas operands staying in the expression), a layer with tau_bnd * ssa_bnd < eps = 3 FLT_MIN, where
max(eps, .) bites, and a layer with a negative g_bnd -- interior layers, since a cloudless layer at the top of the walk
leaves the level below it without any trace of the cloud.  The one-layer case has two bands: band 0 of column 2 holds
tau_bnd = 0 with a negative g_bnd, band 1 a negative g_bnd; a band with tau_bnd * ssa_bnd < eps as well would leave that
column without scattering, and the host test wants ssa_bnd to show in every column."""
import numpy as np

import mcica_ref as M

NCOL = 3
CASES = ((256, 7), (256, 11), (72, 7), (72, 8), (30, 7), (30, 16), (30, 1))
MASK_SEED = 5
MASKS = (None, "sampled", "ones", "zeros")
EPS = np.float32(3.0) * np.finfo(np.float32).tiny


def _ident(ng):
    return np.stack([np.arange(1, ng + 1)] * 2, axis=1).astype(np.int32)


def expand(bnd, lims, ngpt):
    out = np.zeros(bnd.shape[:-1] + (ngpt,), np.float32)
    for ib, (lo, hi) in enumerate(np.asarray(lims).reshape(-1, 2)):
        out[..., lo - 1:hi] = bnd[..., ib:ib + 1]
    return out


def designed(nlay):
    """(layer of tau_bnd = 0, layer of tau_bnd * ssa_bnd < eps, layer of negative g_bnd) of column 2; one layer: no
    layer of the second kind."""
    return (1, nlay // 2, nlay - 2) if nlay >= 7 else (0, None, 0)


_cases = {}


def case(ng, nlay):
    """The inputs at (ng, nlay), built once and never modified: tau lognormal(-2, 2), pfrac U(0, 0.2), tau_bnd
    lognormal(0, 1), ssa_bnd U(0.2, 0.9), g_bnd U(0.5, 0.95), temperatures as mcica_byband_cases.lw_inputs, from
    default_rng(1000 ng + nlay); bands mcica_ref.bands(ng) on the first rows of the shipped Planck table."""
    if (ng, nlay) in _cases:
        return _cases[(ng, nlay)]
    from rrtmgpnn import data
    kl = data.load_kdist("lw")
    lims = M.bands(ng)
    nb = len(lims)
    kd = {"nband": nb, "ngpt": ng, "band_lims_gpt": lims, "nPlanckTemp": kl["nPlanckTemp"],
          "temp_ref_min": kl["temp_ref_min"], "totplnk_delta": kl["totplnk_delta"],
          "totplnk": np.ascontiguousarray(kl["totplnk"][:nb])}
    if ng == kl["ngpt"]:
        assert (np.asarray(kl["band_lims_gpt"]).reshape(-1, 2) == lims).all()
        kd["band_lims_wvn"] = kl["band_lims_wvn"]
    rng = np.random.default_rng(1000 * ng + nlay)
    f = np.float32
    c = {"kd": kd, "ng": ng, "nb": nb, "nlay": nlay, "lims": lims}
    c["tau"] = rng.lognormal(-2, 2, (NCOL, nlay, ng)).astype(f)
    c["pfrac"] = rng.uniform(0, 0.2, (NCOL, nlay, ng)).astype(f)
    c["tb"] = rng.lognormal(0, 1, (NCOL, nlay, nb)).astype(f)
    c["wb"] = rng.uniform(0.2, 0.9, (NCOL, nlay, nb)).astype(f)
    c["gb"] = rng.uniform(0.5, 0.95, (NCOL, nlay, nb)).astype(f)
    c["tlay"] = rng.uniform(200, 300, (NCOL, nlay)).astype(f)
    c["tlev"] = rng.uniform(200, 300, (NCOL, nlay + 1)).astype(f)
    c["tsfc"] = rng.uniform(250, 310, NCOL).astype(f)
    c["emis_bnd"] = rng.uniform(0.9, 1, (NCOL, nb)).astype(f)
    c["emis_gpt"] = rng.uniform(0.9, 1, (NCOL, ng)).astype(f)
    c["inc"] = rng.uniform(0, 2, (NCOL, ng)).astype(f)
    l0, le, lg = designed(nlay)
    if nlay >= 7:
        c["tb"][2, l0] = 0
        c["gb"][2, l0, 0] = f(-0.3)
        c["tb"][2, le] = f(1e-30)
        c["wb"][2, le] = f(1e-10)
        c["gb"][2, lg] = f(-0.4)
    else:
        c["tb"][2, 0, 0] = 0
        c["gb"][2, 0, 0] = f(-0.3)
        c["gb"][2, 0, -1] = f(-0.4)
    assert c["wb"].max() <= 0.95 and c["gb"].max() <= 0.95
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    _cases[(ng, nlay)] = c
    return c


def mask_for(c, kind):
    """None (unmasked), or the (ncol, nlay, ngpt) bool mask of `kind`; "sampled": mcica_ref.build(..., 5)."""
    if kind is None:
        return None
    shape = (NCOL, c["nlay"], c["ng"])
    if kind == "ones":
        return np.ones(shape, bool)
    if kind == "zeros":
        return np.zeros(shape, bool)
    r, cf, ov = M.build(c["ng"], c["nlay"], NCOL, MASK_SEED)
    return M.sampled_mask(r, cf, ov)


def props(orc, c, mask, wb=None, gb=None):
    """(tau, ssa, g) of the composed oracle; wb / gb: other ssa_bnd / g_bnd than the case's."""
    z = np.zeros_like(c["tau"])
    cloud = [c["tb"], c["wb"] if wb is None else wb, c["gb"] if gb is None else gb]
    if mask is None:
        return orc.increment_bybnd(c["lims"], [c["tau"], z, z], cloud)
    return orc.increment_bybnd(_ident(c["ng"]), [c["tau"], z, z], [M.draw(mask, a, c["lims"]) for a in cloud])


def sources(orc, c, top_at_1):
    nlay = c["nlay"]
    return orc.planck_source(c["kd"], c["tlay"], c["tlev"], c["tsfc"], c["pfrac"], nlay if top_at_1 else 1)


_expect = {}


def expect(orc, c, kind, top_at_1, nmus, emis_by_band=True, inc=False, wb=None, gb=None):
    """The composed oracle's (flux_up, flux_dn) under the mask `kind`; cached for the case's own ssa_bnd / g_bnd."""
    key = (c["ng"], c["nlay"], kind, bool(top_at_1), nmus, bool(emis_by_band), bool(inc))
    if wb is None and gb is None and key in _expect:
        return _expect[key]
    io = props(orc, c, mask_for(c, kind), wb, gb)
    lay, lev, sfc, _ = sources(orc, c, top_at_1)
    emis = expand(c["emis_bnd"], c["lims"], c["ng"]) if emis_by_band else c["emis_gpt"]
    res = orc.lw_solver(io[0], lay, lev, emis, sfc, top_at_1=top_at_1, nmus=nmus, inc_flux=c["inc"] if inc else None,
                        ssa=io[1], g=io[2])
    if wb is None and gb is None:
        _expect[key] = res
    return res


def clear_expect(orc, c, top_at_1, nmus):
    """The oracle's no-scattering clear sky of the same columns (emissivity by band, no incident flux)."""
    lay, lev, sfc, _ = sources(orc, c, top_at_1)
    return orc.lw_solver(c["tau"], lay, lev, expand(c["emis_bnd"], c["lims"], c["ng"]), sfc, top_at_1=top_at_1, nmus=nmus)
