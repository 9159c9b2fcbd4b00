"""By-band fluxes under a McICA mask: the inputs, masks and composed-oracle expectations shared by
tests/test_mcica_byband_host.py (which establishes on the CPU that the chosen masks matter) and
tests/test_gpu_mcica_byband.py.

Shapes as tests/test_gpu_mcica.py: 3 columns (odd: the SW block of two columns has a ragged last block) x 7 layers (no
multiple of the LW ring, the prefetch depths or the SW checkpoint stride of 3), the shipped k-distributions' 256 / 224
g-points, every layer cloudy, so the mask decides."""
import numpy as np

import byband_ref as R
import mcica_ref as M

NCOL, NLAY = 3, 7
LW_MASK_SEED, SW_MASK_SEED, RFMIP_MASK_SEED = 5, 9, 11


def mask_for(ngpt, seed, kind="sampled"):
    if kind == "ones":
        return np.ones((NCOL, NLAY, ngpt), bool)
    if kind == "zeros":
        return np.zeros((NCOL, NLAY, ngpt), bool)
    r, cf, ov = M.build(ngpt, NLAY, NCOL, seed)
    return M.sampled_mask(r, cf, ov)


def byband_layouts(kd):
    """The by-band layouts of the outputs: the shipped limits, irregular widths and starts, and g-points outside
    every band."""
    ng = kd["ngpt"]
    return {"shipped": np.asarray(kd["band_lims_gpt"], np.int32).reshape(-1, 2), "irregular": R.irregular_limits(ng),
            "uncovered": R.uncovered_limits(ng)}


def lw_inputs():
    from rrtmgpnn import data
    kl = data.load_kdist("lw")
    rng = np.random.default_rng(77)
    ng, nb = kl["ngpt"], kl["nband"]
    c = {"kd": kl, "ng": ng, "nb": nb}
    c["tau"] = rng.lognormal(-2, 2, (NCOL, NLAY, ng)).astype(np.float32)
    c["pfrac"] = rng.uniform(0, 0.2, (NCOL, NLAY, ng)).astype(np.float32)
    c["tb"] = rng.lognormal(0, 1, (NCOL, NLAY, nb)).astype(np.float32)  # every layer cloudy: the mask decides
    c["tlay"] = rng.uniform(200, 300, (NCOL, NLAY)).astype(np.float32)
    c["tlev"] = rng.uniform(200, 300, (NCOL, NLAY + 1)).astype(np.float32)
    c["tsfc"] = rng.uniform(250, 310, NCOL).astype(np.float32)
    c["emis_bnd"] = rng.uniform(0.9, 1, (NCOL, nb)).astype(np.float32)
    return c


def sw_inputs():
    from rrtmgpnn import data
    ks = data.load_kdist("sw")
    rng = np.random.default_rng(78)
    ng, nb = ks["ngpt"], ks["nband"]
    c = {"kd": ks, "ng": ng, "nb": nb}
    c["tau"] = rng.lognormal(-2, 2, (NCOL, NLAY, ng)).astype(np.float32)
    c["ssa"] = rng.uniform(0, 1, (NCOL, NLAY, ng)).astype(np.float32)
    c["g"] = rng.uniform(0, 0.8, (NCOL, NLAY, ng)).astype(np.float32)
    c["bt"] = rng.lognormal(0, 1, (NCOL, NLAY, nb)).astype(np.float32)
    c["bw"] = rng.uniform(0.5, 1, (NCOL, NLAY, nb)).astype(np.float32)
    c["bg"] = rng.uniform(0, 0.9, (NCOL, NLAY, nb)).astype(np.float32)
    c["mu0"] = rng.uniform(0.1, 1, NCOL).astype(np.float32)
    c["inc"] = rng.uniform(0, 5, (NCOL, ng)).astype(np.float32)
    c["alb"] = rng.uniform(0, 1, (NCOL, ng)).astype(np.float32)
    # the RFMIP form's inputs: sza below and above the usecol bound, spectrally constant albedo
    c["solar"] = rng.uniform(0.1, 5, ng).astype(np.float32)
    c["tsi"] = rng.uniform(1300, 1400, NCOL).astype(np.float32)
    c["sfc_alb"] = rng.uniform(0, 1, NCOL).astype(np.float32)
    c["sza"] = np.array([10.0, 60.0, 85.0], np.float32)
    # the cloud bands of the increment: the shipped ones (every band starts at an even g-point) and a layout with an odd
    # start; the by-band layouts of the outputs are others (byband_layouts)
    bl = np.array(ks["band_lims_gpt"], dtype=np.int64).reshape(-1, 2)
    odd = bl.copy()
    odd[0, 1] -= 1
    odd[1, 0] -= 1
    c["lims"] = {"pair": bl, "general": odd}
    return c


def _ident(ng):
    return np.stack([np.arange(1, ng + 1)] * 2, axis=1).astype(np.int32)


def _expand(bnd, lims, ngpt):
    out = np.zeros(bnd.shape[:-1] + (ngpt,), np.float32)
    for ib, (lo, hi) in enumerate(np.asarray(lims).reshape(-1, 2)):
        out[..., lo - 1:hi] = bnd[..., ib:ib + 1]
    return out


def lw_expect(orc, c, mask, top_at_1, nmus):
    """The composed oracle: restated mask -> merge -> same-resolution increment -> Planck sources -> solver with
    g-point outputs.  Returns the broadband (up, dn) and the g-point values the by-band sums add (up, dn): the one-angle
    terms, or the g-point fluxes with several angles."""
    from oracle import gauss
    kl, ng = c["kd"], c["ng"]
    (tau_all,) = orc.increment_bybnd(_ident(ng), [c["tau"]], [M.draw(mask, c["tb"], kl["band_lims_gpt"])])
    lay, lev, sfc, _ = orc.planck_source(kl, c["tlay"], c["tlev"], c["tsfc"], c["pfrac"], NLAY if top_at_1 else 1)
    emis = _expand(c["emis_bnd"], kl["band_lims_gpt"], ng)
    up, dn, gu, gd = orc.lw_solver(tau_all, lay, lev, emis, sfc, top_at_1=top_at_1, nmus=nmus, gpt=True)
    if nmus == 1:
        w = gauss(1)[1][0]
        gu, gd = R.lw_one_angle_terms(gu, w, ng), R.lw_one_angle_terms(gd, w, ng)
    return up, dn, gu, gd


def sw_expect(orc, c, mask, cloud_lims, with_g, top_at_1, bc=None):
    """The composed oracle of the SW entries -> (up, dn, dir) broadband as the plain solver sums them, and the g-point
    (up, total down, direct).  bc: (mu0, toa, alb) of the _rfmip form, else the case's own."""
    ng = c["ng"]
    g_in = c["g"] if with_g else np.zeros_like(c["g"])
    io = orc.increment_bybnd(_ident(ng), [c["tau"], c["ssa"], g_in],
                             [M.draw(mask, c[k], cloud_lims) for k in ("bt", "bw", "bg")])
    mu0, inc, alb = bc if bc is not None else (c["mu0"], c["inc"], c["alb"])
    bb = orc.sw_solver(*io, mu0, inc, alb, alb, top_at_1=top_at_1)
    gp = orc.sw_solver(*io, mu0, inc, alb, alb, top_at_1=top_at_1, gpt=True)
    return tuple(bb), tuple(gp[3:])
