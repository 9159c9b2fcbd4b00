"""McICA cloud sampling, restated in numpy float32 (extensions/cloud_optics/mo_cloud_sampling.F90), with the input
builders the tests share.  tests/golden/mcica_masks.npz pins the restatement to the reference module itself
(tests/golden/make_mcica_golden.py).

Arrays are C-ordered with the Fortran shape of this project's layout reversed, as everywhere in the tests:
randoms and masks (ncol, nlay, ngpt), cloud_frac (ncol, nlay), overlap_param (ncol, nlay-1), packed masks
(ncol, nlay, nw) uint32 with nw = ceil(ngpt / 32), bit g % 32 of word g / 32 for 0-based g-point g."""
import numpy as np

F = np.float32
ONE, HALF = F(1.0), F(0.5)


def sampled_mask(randoms, cloud_frac, overlap_param=None):
    """sampled_mask_max_ran (:125-192; overlap_param None) / sampled_mask_exp_ran (:200-285), statement by statement in
    float32.  The mask starts all false, which is what the reference's max_ran assigns everywhere it does not compare
    and what its exp_ran leaves unassigned in a clear layer between cloudy ones (quirk)."""
    r = np.asarray(randoms, F)
    cf = np.asarray(cloud_frac, F)
    ncol, nlay, ngpt = r.shape
    mask = np.zeros((ncol, nlay, ngpt), bool)
    for ic in range(ncol):
        cloudy = cf[ic] > 0
        if not cloudy.any():
            continue
        fst = int(np.argmax(cloudy))
        lst = nlay - 1 - int(np.argmax(cloudy[::-1]))
        local = r[ic, fst].copy()
        mask[ic, fst] = local > (ONE - cf[ic, fst])
        for il in range(fst + 1, lst + 1):
            if not cloudy[il]:
                continue
            if cloudy[il - 1]:
                if overlap_param is not None:
                    rho = F(overlap_param[ic, il - 1])
                    sq = np.sqrt(ONE - rho * rho, dtype=F)
                    local = (rho * (local - HALF) + sq * (r[ic, il] - HALF)) + HALF
            else:
                local = r[ic, il].copy()
            assert local.dtype == F
            mask[ic, il] = local > (ONE - cf[ic, il])
    return mask


def pack_bits(mask):
    """(ncol, nlay, ngpt) bool -> (ncol, nlay, nw) uint32; unused high bits zero."""
    m = np.asarray(mask, bool)
    ngpt = m.shape[-1]
    nw = (ngpt + 31) // 32
    pad = np.zeros(m.shape[:-1] + (nw * 32,), np.uint64)
    pad[..., :ngpt] = m
    w = (pad.reshape(m.shape[:-1] + (nw, 32)) << np.arange(32, dtype=np.uint64)).sum(axis=-1)
    return w.astype(np.uint32)


def unpack_bits(bits, ngpt):
    b = np.asarray(bits, np.uint32)
    u = (b[..., :, None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)
    return u.reshape(b.shape[:-1] + (-1,))[..., :ngpt].astype(bool)


def draw(mask, bnd, lims):
    """apply_cloud_mask (:291-307): (ncol, nlay, nbnd) band values -> (ncol, nlay, ngpt), 0 where the mask is false."""
    out = np.zeros(mask.shape, F)
    for ib, (lo, hi) in enumerate(np.asarray(lims).reshape(-1, 2)):
        out[..., lo - 1:hi] = np.where(mask[..., lo - 1:hi], np.asarray(bnd, F)[..., ib:ib + 1], F(0))
    return out


def bands(ngpt):
    """Band limits (nbnd, 2), 1-based inclusive: RRTMGP's 16 g-points per band for 256 and 224; uneven widths with odd
    starts (a general, not band-pair, layout) for 40; two bands for anything else."""
    if ngpt in (256, 224):
        lo = np.arange(1, ngpt + 1, 16)
        return np.stack([lo, lo + 15], axis=1).astype(np.int32)
    widths = [3, 5, 8, 7, 9, 8] if ngpt == 40 else [ngpt // 2, ngpt - ngpt // 2]
    hi = np.cumsum(widths)
    return np.stack([hi - np.asarray(widths) + 1, hi], axis=1).astype(np.int32)


def build(ngpt, nlay, ncol, seed):
    """Inputs of one case: (randoms, cloud_frac, overlap_param).  Column 0 is generic; columns 1.. are designed where
    the extents allow (the denser designs first, so that small cases keep clouds): 1 every layer cloudy with rho
    1, -1, 0 on its first pairs, cloud_frac 1 against a random of exactly 0, and a random exactly equal to
    1 - cloud_frac; 2 a clear gap between cloudy layers; 4 no cloud; 5 cloud in the first array layer only; 6 in the
    last only; 7 cloud fractions so small that 1 - cloud_frac == 1, next to a thick layer.  All others are generic:
    about 30 % of the layers clear, fractions in (0.3, 1], overlap parameters in (-1, 1)."""
    rng = np.random.default_rng(seed)
    r = rng.random((ncol, nlay, ngpt), dtype=F)
    cf = (F(0.3) + F(0.7) * rng.random((ncol, nlay), dtype=F)).astype(F)
    cf[rng.random((ncol, nlay)) < 0.3] = 0
    ov = (F(2) * rng.random((ncol, max(nlay - 1, 0)), dtype=F) - ONE).astype(F)
    if ncol > 1:
        cf[1] = (F(0.4) + F(0.5) * rng.random(nlay, dtype=F)).astype(F)
        cf[1, 0] = 1
        r[1, 0, 0] = 0  # cloud_frac 1, random exactly 0: 0 > 0 is false
        if nlay > 1:
            cf[1, -1] = F(0.25)
        for k, rho in enumerate((1, -1, 0)):
            if k < nlay - 1:
                ov[1, k] = rho
    if ncol > 2 and nlay >= 3:
        cf[2] = 0
        cf[2, 0], cf[2, 2] = F(0.6), F(0.7)
        if nlay > 4:
            cf[2, 3], cf[2, nlay - 1] = F(0.5), F(0.8)
    if ncol > 4:
        cf[4] = 0
    if ncol > 5:
        cf[5] = 0
        cf[5, 0] = F(0.9)
    if ncol > 6:
        cf[6] = 0
        cf[6, -1] = F(0.9)
    if ncol > 7:
        cf[7] = F(1e-9)
        cf[7, nlay // 2] = F(0.75)
    # a random exactly equal to 1 - cloud_frac in the first cloudy layer of every column that has one (strict: false)
    for ic in range(ncol):
        cl = np.nonzero(cf[ic] > 0)[0]
        if len(cl) and ngpt > 1:
            r[ic, cl[0], 1] = ONE - cf[ic, cl[0]]
    return r, cf, ov


def coverage(r, cf, ov):
    """Which of the required situations the inputs hold (tests/test_mcica_host.py asserts them on the CPU)."""
    cl = cf > 0
    nlay = cf.shape[1]
    one = cl.sum(axis=1) == 1
    gap = adj = False
    rho = set()
    for ic in range(cf.shape[0]):
        idx = np.nonzero(cl[ic])[0]
        if len(idx) >= 2:
            gap = gap or bool((np.diff(idx) > 1).any())
            for il in idx[1:]:
                if cl[ic, il - 1]:
                    adj = True
                    rho.add(float(ov[ic, il - 1]))
    thresh = (ONE - cf)[:, :, None]
    return {
        "no_cloud": bool((~cl.any(axis=1)).any()),
        "first_only": bool((one & cl[:, 0]).any()),
        "last_only": bool((one & cl[:, nlay - 1]).any()),
        "adjacent": adj,
        "gap": gap,
        "frac1_rand0": bool(((cf == 1)[:, :, None] & (r == 0)).any()),
        "rand_eq_thresh": bool((cl[:, :, None] & (r == thresh)).any()),
        "tiny_frac": bool((cl & ((ONE - cf) == 1)).any()),
        "rho_pm1_0": {-1.0, 0.0, 1.0} <= rho,
        "rho_generic": any(abs(x) not in (0.0, 1.0) for x in rho),
    }


def non_vacuity(mask, lims):
    """(share of set bits, share of columns with a layer whose bits differ inside one band, mixed 32-bit words)."""
    bits = pack_bits(mask)
    ngpt = mask.shape[-1]
    full = pack_bits(np.ones_like(mask))
    mixed_words = int(((bits != 0) & (bits != full)).sum())
    cols = np.zeros(mask.shape[0], bool)
    for lo, hi in np.asarray(lims).reshape(-1, 2):
        s = mask[..., lo - 1:hi]
        cols |= (s.any(axis=-1) & ~s.all(axis=-1)).any(axis=1)
    return float(mask.mean()), float(cols.mean()), mixed_words


def step_oracle(orc, prob, clouds, cf, ov, r_lw, r_sw):
    """The composed oracle: gas optics, cloud optics (and delta scaling), restated mask -> merge -> same-resolution
    increment -> solver, as the all-sky oracle does with overcast clouds."""
    from rrtmgpnn import data
    m = {k: data.load_model(k) for k in ("lw_abs", "lw_pfrac", "sw_abs", "sw_ray")}
    kl, ks = data.load_kdist("lw"), data.load_kdist("sw")
    out = {}
    go = orc.lw_gas_optics(prob, [m["lw_abs"], m["lw_pfrac"]], kl)
    (ct,) = orc.cloud_optics(data.load_cloud_optics("lw"), *clouds, nstr=1, lut=True, icergh=2)
    ng = go["tau"].shape[-1]
    ident = np.stack([np.arange(1, ng + 1)] * 2, axis=1).astype(np.int32)
    (tau,) = orc.increment_bybnd(ident, (go["tau"],), (draw(sampled_mask(r_lw, cf, ov), ct, kl["band_lims_gpt"]),))
    emis = np.repeat(np.asarray(prob["sfc_emis"], np.float32)[:, None], ng, axis=1)
    out["lw_up"], out["lw_dn"] = orc.lw_solver(tau, go["lay_source"], go["lev_source"], emis, go["sfc_source"],
                                               prob["top_at_1"], 1)
    go = orc.sw_gas_optics(prob, [m["sw_abs"], m["sw_ray"]])
    cld = orc.delta_scale(*orc.cloud_optics(data.load_cloud_optics("sw"), *clouds, nstr=2, lut=True, icergh=2))
    ng = go["tau"].shape[-1]
    ident = np.stack([np.arange(1, ng + 1)] * 2, axis=1).astype(np.int32)
    mask = sampled_mask(r_sw, cf, ov)
    io = orc.increment_bybnd(ident, (go["tau"], go["ssa"], go["g"]),
                             [draw(mask, a, ks["band_lims_gpt"]) for a in cld])
    alb = np.repeat(np.asarray(prob["sfc_alb"], np.float32)[:, None], ng, axis=1)
    out["sw_up"], out["sw_dn"], out["sw_dir"] = orc.sw_solver(*io, prob["mu0"], data.toa_flux(prob, ks), alb, alb,
                                                              prob["top_at_1"])
    return out


# the GPU mask cases: every ngpt with every nlay and ncol of the issue's sets
CASES = [(ngpt, nlay, ncol) for ngpt in (256, 224, 40, 33) for nlay in (1, 7, 12) for ncol in (1, 3, 5)]
FIXTURE_SHAPE = (40, 12, 36)  # ngpt, nlay, ncol of tests/golden/mcica_masks.npz
FIXTURE_SEED = 20


def case_seed(ngpt, nlay, ncol):
    return 1000 * ngpt + 10 * nlay + ncol
