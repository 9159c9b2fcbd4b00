"""Aerosols as a second band increment fused into the all-sky solvers (rrtmgpnn_solver_request_aerosol): the inputs and
the composed-oracle expectations shared by tests/test_aerosol_host.py (which establishes on the CPU that the order of
the two increments, their sum and the aerosol itself all show in the expected fluxes) and tests/test_gpu_aerosol.py.

The gas, cloud and mask inputs are those of tests/mcica_byband_cases.py: 3 columns (odd: the SW block of two columns
has a ragged last block) x 7 layers (no multiple of the LW ring, the prefetch depths or the SW checkpoint stride),
256 / 224 g-points, every layer cloudy.  Added here: the aerosols, by band, and LW cases of 72 and 30 g-points in two
bands (mcica_ref.bands: the per-lane mask word of the dual entries, and the ngpt % 4 != 0 flush).

The composed oracle, bit for bit what the fused solvers must give:
  increment_bybnd(band limits, gas, aerosol); then increment_bybnd(identity limits, ., draw(mask, cloud, band limits))
  -- without a mask increment_bybnd(band limits, ., cloud) --; then the plain solver.
`order` states the variants the host test proves different: "swapped" (cloud first), "presummed" (LW: one increment by
the float32 sum of the two band arrays), "noaer" (the aerosol ignored)."""
import numpy as np

import mcica_byband_cases as C
import mcica_ref as M
from mcica_byband_cases import NCOL, NLAY

LW_AER_SEED, SW_AER_SEED = 91, 92
# The LW mask seed is 6, not mcica_byband_cases' 5: with seed 5 the case (256 g-points, bottom first, three angles,
# sampled mask) has the same broadband bits in either order of the two increments, which tests/test_aerosol_host.py
# does not accept; with 6 every case tells the orders apart.  The SW mask seed is mcica_byband_cases' 9.
LW_MASK_SEED = 6
# aerosol seeds of the small LW cases (two bands of 36 / 15 g-points: few g-points for a reordered pair of adds to show
# in a broadband sum): the first of 91 + ng + 1000 k under which every case of tests/test_aerosol_host.py tells the
# orders apart with mask seed 6 -- k = 22 for 72 g-points, k = 4 for 30
LW_AER_SEEDS = {72: LW_AER_SEED + 72 + 22000, 30: LW_AER_SEED + 30 + 4000}
LW_NGPTS = (256, 72, 30)
ORDERS = ("right", "swapped", "presummed", "noaer")


def _ident(ng):
    return np.stack([np.arange(1, ng + 1)] * 2, axis=1).astype(np.int32)


def expand(bnd, lims, ngpt):
    out = np.zeros(bnd.shape[:-1] + (ngpt,), np.float32)
    for ib, (lo, hi) in enumerate(np.asarray(lims).reshape(-1, 2)):
        out[..., lo - 1:hi] = bnd[..., ib:ib + 1]
    return out


def lw_case(ng=256):
    """LW inputs at ng g-points.  256: mcica_byband_cases.lw_inputs() with the aerosol lognormal(-1, 1) from
    default_rng(91), (3, 7, 16).  72 / 30: two bands (mcica_ref.bands) on the first rows of the shipped Planck table,
    inputs drawn as lw_inputs draws them from default_rng(77 + ng), the aerosol from default_rng(LW_AER_SEEDS[ng])."""
    if ng == 256:
        c = C.lw_inputs()
        c["lims"] = np.asarray(c["kd"]["band_lims_gpt"], np.int32).reshape(-1, 2)
        c["aer"] = np.random.default_rng(LW_AER_SEED).lognormal(-1, 1, (NCOL, NLAY, c["nb"])).astype(np.float32)
        return c
    from rrtmgpnn import data
    kl = data.load_kdist("lw")
    lims = M.bands(ng)
    nb = len(lims)
    kd = {"nband": nb, "ngpt": ng, "band_lims_gpt": lims, "nPlanckTemp": kl["nPlanckTemp"],
          "temp_ref_min": kl["temp_ref_min"], "totplnk_delta": kl["totplnk_delta"],
          "totplnk": np.ascontiguousarray(kl["totplnk"][:nb])}
    rng = np.random.default_rng(77 + ng)
    c = {"kd": kd, "ng": ng, "nb": nb, "lims": lims}
    c["tau"] = rng.lognormal(-2, 2, (NCOL, NLAY, ng)).astype(np.float32)
    c["pfrac"] = rng.uniform(0, 0.2, (NCOL, NLAY, ng)).astype(np.float32)
    c["tb"] = rng.lognormal(0, 1, (NCOL, NLAY, nb)).astype(np.float32)
    c["tlay"] = rng.uniform(200, 300, (NCOL, NLAY)).astype(np.float32)
    c["tlev"] = rng.uniform(200, 300, (NCOL, NLAY + 1)).astype(np.float32)
    c["tsfc"] = rng.uniform(250, 310, NCOL).astype(np.float32)
    c["emis_bnd"] = rng.uniform(0.9, 1, (NCOL, nb)).astype(np.float32)
    c["aer"] = np.random.default_rng(LW_AER_SEEDS[ng]).lognormal(-1, 1, (NCOL, NLAY, nb)).astype(np.float32)
    return c


def sw_case():
    """mcica_byband_cases.sw_inputs() with the aerosol from default_rng(92): tau lognormal(-1, 1), then ssa U(0.6, 1),
    then g U(0.3, 0.8), (3, 7, 14) each."""
    c = C.sw_inputs()
    rng = np.random.default_rng(SW_AER_SEED)
    shape = (NCOL, NLAY, c["nb"])
    c["at"] = rng.lognormal(-1, 1, shape).astype(np.float32)
    c["aw"] = rng.uniform(0.6, 1, shape).astype(np.float32)
    c["ag"] = rng.uniform(0.3, 0.8, shape).astype(np.float32)
    return c


def lw_mask(c, kind):
    """None (unmasked), or the mask of `kind` ("sampled": LW_MASK_SEED) at the case's g-points."""
    return None if kind is None else C.mask_for(c["ng"], LW_MASK_SEED, kind)


def sw_mask(c, kind):
    return None if kind is None else C.mask_for(c["ng"], C.SW_MASK_SEED, kind)


def _cloud_inc(orc, io, cloud, lims, mask):
    """The second increment: by band, or (masked) the sampled g-point arrays at identity limits."""
    if mask is None:
        return orc.increment_bybnd(lims, io, cloud)
    return orc.increment_bybnd(_ident(mask.shape[-1]), io, [M.draw(mask, a, lims) for a in cloud])


def lw_taus(orc, c, mask, order="right"):
    """(clear, all-sky) optical depths of the composed oracle: tau + aerosol, and that + the (sampled) cloud."""
    lims = c["lims"]
    (clear,) = orc.increment_bybnd(lims, [c["tau"]], [c["aer"]])
    if order == "right":
        (allsky,) = _cloud_inc(orc, [clear], [c["tb"]], lims, mask)
    elif order == "swapped":
        (t,) = _cloud_inc(orc, [c["tau"]], [c["tb"]], lims, mask)
        (allsky,) = orc.increment_bybnd(lims, [t], [c["aer"]])
    elif order == "presummed":
        cloud = expand(c["tb"], lims, c["ng"]) if mask is None else M.draw(mask, c["tb"], lims)
        both = (expand(c["aer"], lims, c["ng"]) + cloud).astype(np.float32)
        (allsky,) = orc.increment_bybnd(_ident(c["ng"]), [c["tau"]], [both])
    else:
        (allsky,) = _cloud_inc(orc, [c["tau"]], [c["tb"]], lims, mask)
    return clear, allsky


def lw_expect(orc, c, mask, top_at_1, nmus, order="right"):
    """The composed oracle of the LW entries -> (up, dn, up_clr, dn_clr): the all-sky set and the clear set (gases plus
    aerosols), emissivity by band."""
    kd, ng = c["kd"], c["ng"]
    clear, allsky = lw_taus(orc, c, mask, order)
    lay, lev, sfc, _ = orc.planck_source(kd, c["tlay"], c["tlev"], c["tsfc"], c["pfrac"], NLAY if top_at_1 else 1)
    emis = expand(c["emis_bnd"], c["lims"], ng)
    up, dn = orc.lw_solver(allsky, lay, lev, emis, sfc, top_at_1=top_at_1, nmus=nmus)
    upc, dnc = orc.lw_solver(clear, lay, lev, emis, sfc, top_at_1=top_at_1, nmus=nmus)
    return up, dn, upc, dnc


def sw_props(orc, c, mask, with_g, order="right", lims=None, aer=None):
    """(tau, ssa, g) of the composed SW oracle.  aer: the aerosol triple (default the case's; zeros: an increment by
    zeros, which still rounds tau * ssa / max(eps, tau))."""
    lims = c["lims"]["pair"] if lims is None else lims
    gas = [c["tau"], c["ssa"], c["g"] if with_g else np.zeros_like(c["g"])]
    aer = [c["at"], c["aw"], c["ag"]] if aer is None else aer
    cloud = [c["bt"], c["bw"], c["bg"]]
    if order == "right":
        return _cloud_inc(orc, orc.increment_bybnd(lims, gas, aer), cloud, lims, mask)
    if order == "swapped":
        return orc.increment_bybnd(lims, _cloud_inc(orc, gas, cloud, lims, mask), aer)
    assert order == "noaer"
    return _cloud_inc(orc, gas, cloud, lims, mask)


def sw_expect(orc, c, mask, with_g, top_at_1, order="right", bc=None, lims=None, aer=None):
    """The composed oracle of the SW entries -> (up, dn, dir).  bc: (mu0, toa, alb) of the _rfmip form."""
    io = sw_props(orc, c, mask, with_g, order, lims, aer)
    mu0, inc, alb = bc if bc is not None else (c["mu0"], c["inc"], c["alb"])
    return tuple(orc.sw_solver(*io, mu0, inc, alb, alb, top_at_1=top_at_1))


def sw_clear_expect(orc, c, with_g, top_at_1, bc=None):
    """Clear sky with aerosols: the gas properties incremented by the aerosol alone."""
    gas = [c["tau"], c["ssa"], c["g"] if with_g else np.zeros_like(c["g"])]
    io = orc.increment_bybnd(c["lims"]["pair"], gas, [c["at"], c["aw"], c["ag"]])
    mu0, inc, alb = bc if bc is not None else (c["mu0"], c["inc"], c["alb"])
    return tuple(orc.sw_solver(*io, mu0, inc, alb, alb, top_at_1=top_at_1))


def bound_sza():
    """Zenith angles around the driver's usecol bound 90 - 2 spacing(90): the last float below it, the bound itself
    and 120 degrees (mu0 = 1 from the bound on)."""
    b = np.float32(90) - 2 * np.spacing(np.float32(90))
    return np.array([np.nextafter(b, np.float32(0)), b, 120.0], np.float32)


def rfmip_bc(c, sza=None):
    """(mu0, toa, alb): the boundary conditions the _rfmip entry forms from the case's solar source, TSI, albedo and
    zenith angles (rrtmgp_rfmip_sw.F90:403-434), as rrtmgpnn.data forms them on the CPU (ref_cosf, the sequential sum,
    toa * tsi / def_tsi left to right).  tests/test_gpu_aerosol.py asserts that the entry stores these very bits."""
    from rrtmgpnn import data
    sza = np.asarray(c["sza"] if sza is None else sza, np.float32)
    use = sza < np.float32(90.0) - np.float32(2.0) * data.spacing(90.0)
    deg_to_rad = np.float32(np.arccos(np.float32(-1.0)) / np.float32(180.0))
    mu0 = np.where(use, data.ref_cosf(sza * deg_to_rad), np.float32(1.0)).astype(np.float32)
    sol = np.asarray(c["solar"], np.float32)
    toa = np.broadcast_to(sol, (NCOL, sol.size)).astype(np.float32)
    def_tsi = data.seqsum(toa, axis=1)
    toa = ((toa * np.asarray(c["tsi"], np.float32)[:, None]) / def_tsi[:, None]).astype(np.float32)
    alb = np.repeat(np.asarray(c["sfc_alb"], np.float32)[:, None], c["ng"], axis=1)
    return mu0, toa, alb
