"""Shared inputs and oracle results of the clear + all-sky tests (tests/test_gpu_clr_all_sky.py and its CPU
companion): built once per (nlay, orientation) on the CPU and never modified afterwards."""
import numpy as np

# below the prefetch depth, at and around the dual kernel's ring of 4 and the single kernels' ring of 8, several chunks
NLAYS = (1, 2, 3, 4, 5, 7, 8, 9, 17, 65)
NCOL = 23
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def flip(prob):
    out = dict(prob)
    for k in ("play", "plev", "tlay", "tlev"):
        out[k] = np.ascontiguousarray(prob[k][:, ::-1])
    out["gases"] = {k: np.ascontiguousarray(v[:, ::-1]) for k, v in prob["gases"].items()}
    out["top_at_1"] = False
    return out


def cloud_tau(orc, prob, nband, seed):
    """Band cloud optical depth (ncol, nlay, nband) of the all-sky example's recipe (every third column cloud-free);
    where the recipe puts no cloud at all in these pressures, a seeded random tau in [0, 5] on the same two thirds of
    the columns."""
    from rrtmgpnn import data
    co = data.load_cloud_optics("lw")
    (cld,) = orc.cloud_optics(co, *data.allsky_clouds(prob, co), nstr=1, icergh=2)
    if not (cld > 0).any():
        ncol, nlay = prob["play"].shape
        rng = np.random.default_rng(seed)
        cloudy = (np.arange(ncol) + 1) % 3 != 0
        cld = (rng.uniform(0, 5, (ncol, nlay, nband)) * cloudy[:, None, None]).astype(np.float32)
    return cld


def solver_case(orc, nlay, top_at_1, ngpt=None):
    """The setup of test_fused_lw_any_nlay -- synthetic_problem(23, nlay, seed=11), NN gas optics -- with the cloud tau
    of cloud_tau, and the oracle's clear (tau) and all-sky (increment_bybnd(tau, cloud tau)) fluxes.  ngpt: the
    k-distribution cut to its first ngpt g-points, the last band ending there (254: quirk B-5's plain sums)."""
    def make():
        from rrtmgpnn import data
        prob = data.synthetic_problem(NCOL, nlay, seed=11)
        if not top_at_1:
            prob = flip(prob)
        kd = dict(data.load_kdist("lw"))
        go = orc.lw_gas_optics(prob, [data.load_model("lw_abs"), data.load_model("lw_pfrac")], kd)
        tau, pfrac = go["tau"], go["pfrac"]
        lay, lev, sfc = go["lay_source"], go["lev_source"], go["sfc_source"]
        sfc_lay = 1 if prob["play"][0, 0] > prob["play"][0, nlay - 1] else nlay
        lims = np.array(kd["band_lims_gpt"], np.int32).reshape(-1, 2).copy()
        if ngpt is not None:
            assert lims[-1, 0] <= ngpt < lims[-1, 1]
            lims[-1, 1] = ngpt
            tau, pfrac = (np.ascontiguousarray(a[..., :ngpt]) for a in (tau, pfrac))
            kd["band_lims_gpt"] = lims
            lay, lev, sfc, _ = orc.planck_source(kd, prob["tlay"], go["tlev"], prob["tsfc"], pfrac, sfc_lay)
        ng = tau.shape[-1]
        cld = cloud_tau(orc, prob, kd["nband"], seed=100 + nlay)
        emis_band = np.random.default_rng(7).uniform(0.8, 1.0, (NCOL, kd["nband"])).astype(np.float32)
        band_of = np.zeros(ng, np.int64)
        for b, (lo, hi) in enumerate(lims):
            band_of[lo - 1:hi] = b
        emis = np.ascontiguousarray(emis_band[:, band_of])
        inc_flux = np.random.default_rng(8).uniform(0, 2, (NCOL, ng)).astype(np.float32)
        (tau_all,) = orc.increment_bybnd(lims, (tau,), (cld,))
        want = {}
        for name, inc in (("plain", None), ("inc", inc_flux)):
            for nmus in ((1, 2, 3, 4) if (nlay == 17 and name == "plain" and ngpt is None) else (1,)):
                want[name, nmus] = (orc.lw_solver(tau_all, lay, lev, emis, sfc, top_at_1, nmus, inc_flux=inc),
                                    orc.lw_solver(tau, lay, lev, emis, sfc, top_at_1, nmus, inc_flux=inc))
        return dict(prob=prob, kd=kd, lims=lims, tau=tau, pfrac=pfrac, cld=cld, emis=emis, emis_band=emis_band,
                    inc_flux=inc_flux, sfc_lay=sfc_lay, tlev=go["tlev"], want=want,
                    cloudy=(cld > 0).any(axis=(1, 2)))
    return cached(("solver", nlay, top_at_1, ngpt), make)


def sets_differ(case, key=("plain", 1)):
    """Per column: do the oracle's clear and all-sky flux sets differ anywhere?"""
    (up_a, dn_a), (up_c, dn_c) = case["want"][key]
    return (up_a != up_c).any(axis=1) | (dn_a != dn_c).any(axis=1)
