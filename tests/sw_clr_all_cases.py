"""Clear-sky beside all-sky SW fluxes from one call (rrtmgpnn_sw_solver_2stream_clr_all / _rfmip_clr_all): the inputs
and the oracle's expectations shared by tests/test_sw_clr_all_host.py and tests/test_gpu_sw_clr_all.py.  Everything is
built once per case on the CPU and never modified.

* `nn_case(nlay, ncol)`: synthetic columns (rrtmgpnn.data.synthetic_problem), the NN SW gas optics through the oracle
  (224 g-points on the shipped band limits, g = 0), delta-scaled 2str band clouds as tests/test_gpu_clouds.py forms them
  (about every third column cloud-free, two thirds of the remaining layers cloudy), a seeded 2str band aerosol, boundary
  conditions per g-point, and two packed masks from tests/mcica_ref.py.
* `seeded_case(ngpt, lims)`: gas properties drawn in the oracle's valid ranges for band layouts the two-per-lane kernel
  treats specially.

`expect(orc, c, ...)` is oracle.sw_solver on increment_bybnd of the gas properties, in the reference's order
(extensions/mo_rrtmgp_clr_all_sky.F90:288-299): the aerosol first (both skies), then the (sampled) cloud (all sky
only) -> (up, dn, dir, up_clr, dn_clr, dir_clr)."""
import numpy as np

import mcica_ref as M

NLAYS = (1, 2, 3, 4, 7, 9, 10, 19, 28)
NCOL = 11
MASK_SEEDS = (9, 10)
_cache = {}


def _ident(ng):
    return np.stack([np.arange(1, ng + 1)] * 2, axis=1).astype(np.int32)


def _clouds_and_aerosol(c, rng, orc):
    ncol, nlay, nb = c["ncol"], c["nlay"], c["nb"]
    shape = (ncol, nlay, nb)
    # clouds: column i is cloud-free when i % 3 == 2 (ncol 1: cloudy); elsewhere two layers in three carry cloud
    cloudy = (rng.uniform(size=(ncol, nlay)) < 0.67) & ((np.arange(ncol) % 3 != 2)[:, None])
    cloudy[0, 0] = True
    bt = np.where(cloudy[..., None], rng.lognormal(0, 1, shape), 0.0).astype(np.float32)
    bw = rng.uniform(0.5, 1, shape).astype(np.float32)
    bg = rng.uniform(0, 0.9, shape).astype(np.float32)
    c["bt"], c["bw"], c["bg"] = orc.delta_scale(bt, bw, bg)
    c["cloudy_cols"] = cloudy.any(axis=1)
    c["at"] = rng.lognormal(-2, 1, shape).astype(np.float32)
    c["aw"] = rng.uniform(0.6, 1, shape).astype(np.float32)
    c["ag"] = rng.uniform(0.3, 0.8, shape).astype(np.float32)
    c["masks"] = [_mask(c, s) for s in MASK_SEEDS]


def _mask(c, seed):
    """A McICA mask (ncol, nlay, ngpt) of 0 / 1 bytes from mcica_ref's maximum-random sampler on seeded cloud fractions
    (cloud-free layers get fraction 0, so their bits are clear)."""
    rng = np.random.default_rng(1000 + seed)
    ncol, nlay, ng = c["ncol"], c["nlay"], c["ng"]
    frac = np.where(c["bt"][..., 0] > 0, rng.uniform(0.2, 0.9, (ncol, nlay)), 0.0).astype(np.float32)
    rand = rng.uniform(0, 1, (ncol, nlay, ng)).astype(np.float32)
    return M.sampled_mask(rand, frac)


def nn_case(orc, nlay, ncol=NCOL):
    key = ("nn", nlay, ncol)
    if key in _cache:
        return _cache[key]
    from rrtmgpnn import data
    ks = data.load_kdist("sw")
    prob = data.synthetic_problem(ncol, nlay=nlay)
    go = orc.sw_gas_optics(prob, [data.load_model("sw_abs"), data.load_model("sw_ray")])
    ng, nb = ks["ngpt"], ks["nband"]
    rng = np.random.default_rng(4000 + 100 * nlay + ncol)
    c = {"ng": ng, "nb": nb, "nlay": nlay, "ncol": ncol, "tau": go["tau"], "ssa": go["ssa"],
         "lims": np.array(ks["band_lims_gpt"], dtype=np.int32).reshape(-1, 2)}
    _boundary(c, rng)
    _clouds_and_aerosol(c, rng, orc)
    _cache[key] = c
    return c


def _boundary(c, rng):
    ncol, ng = c["ncol"], c["ng"]
    c["g"] = rng.uniform(0.05, 0.6, c["tau"].shape).astype(np.float32)  # used by the "with a gas g array" tests only
    c["mu0"] = rng.uniform(0.1, 1, ncol).astype(np.float32)
    c["inc"] = rng.uniform(0, 5, (ncol, ng)).astype(np.float32)
    c["inc_dif"] = rng.uniform(0, 1, (ncol, ng)).astype(np.float32)
    c["alb"] = rng.uniform(0, 1, (ncol, ng)).astype(np.float32)
    # the RFMIP form: one column at and one past the usecol bound (mu0 = 1 there)
    c["solar"] = rng.uniform(0.1, 5, ng).astype(np.float32)
    c["tsi"] = rng.uniform(1300, 1400, ncol).astype(np.float32)
    c["sfc_alb"] = rng.uniform(0, 1, ncol).astype(np.float32)
    sza = rng.uniform(0, 89, ncol).astype(np.float32)
    sza[ncol // 2] = 95.0
    sza[-1] = 90.0
    c["sza"] = sza


def seeded_case(orc, ngpt, lims, nlay=7, ncol=5):
    key = ("seeded", ngpt, nlay, ncol)
    if key in _cache:
        return _cache[key]
    lims = np.asarray(lims, np.int32).reshape(-1, 2)
    rng = np.random.default_rng(7000 + ngpt)
    c = {"ng": ngpt, "nb": len(lims), "nlay": nlay, "ncol": ncol, "lims": lims}
    c["tau"] = rng.lognormal(-2, 2, (ncol, nlay, ngpt)).astype(np.float32)
    c["ssa"] = rng.uniform(0, 1, (ncol, nlay, ngpt)).astype(np.float32)
    _boundary(c, rng)
    _clouds_and_aerosol(c, rng, orc)
    _cache[key] = c
    return c


LAYOUTS = {
    18: [(1, 5), (6, 11), (12, 18)],      # odd starts; ngpt & 3 != 0: the per-level flush (ring_flush_sw)
    20: [(1, 6), (7, 13), (14, 20)],      # one wave; with nlay <= 2 the lanes flush in short rows
    256: [(16 * i + 1, 16 * i + 16) for i in range(16)],  # the thread-count edge
}


def gas(c, with_g):
    return [c["tau"], c["ssa"], c["g"] if with_g else np.zeros_like(c["tau"])]


def props(orc, c, with_g=False, aer=False, mask=None):
    """((tau, ssa, g) clear, (tau, ssa, g) all sky)."""
    clear = gas(c, with_g)
    if aer:
        clear = orc.increment_bybnd(c["lims"], clear, [c["at"], c["aw"], c["ag"]])
    cloud = [c["bt"], c["bw"], c["bg"]]
    if mask is None:
        allsky = orc.increment_bybnd(c["lims"], clear, cloud)
    else:
        allsky = orc.increment_bybnd(_ident(c["ng"]), clear, [M.draw(mask, a, c["lims"]) for a in cloud])
    return clear, allsky


def expect(orc, c, top_at_1, with_g=False, aer=False, mask=None, dif=False, bc=None):
    """-> (up, dn, dir, up_clr, dn_clr, dir_clr) of the oracle; bc: (mu0, inc, alb) instead of the case's."""
    key = ("expect", id(c), top_at_1, with_g, aer, None if mask is None else id(mask), dif, bc is None)
    if bc is None and key in _cache:
        return _cache[key]
    clear, allsky = props(orc, c, with_g, aer, mask)
    mu0, inc, alb = (c["mu0"], c["inc"], c["alb"]) if bc is None else bc
    kw = dict(top_at_1=top_at_1, inc_flux_dif=c["inc_dif"] if dif else None)
    out = tuple(orc.sw_solver(*allsky, mu0, inc, alb, alb, **kw)) + tuple(orc.sw_solver(*clear, mu0, inc, alb, alb, **kw))
    if bc is None:
        _cache[key] = out
    return out
