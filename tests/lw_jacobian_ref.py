"""Shared inputs and expectations of the flux-Jacobian tests (tests/test_lw_jacobian_host.py,
tests/test_gpu_lw_jacobian.py): flux_up_Jac, d flux_up / d T_sfc at every level (rte/kernels/mo_rte_solver_kernels.F90:270,
290, 319, 390-411, 967, 975, 1761, 1782; compiled out in the reference by compute_Jac = .false.).

The expectation is the oracle's flux_up on the same optical properties with zero layer and level sources, no incident flux
and sfc_source_Jac as the surface source (zero_source_flux_up); direct_jacobian restates the definition itself -- J = emis *
sfc_source_Jac, J = T * J, flux_up's sums -- with T taken from one-layer oracle solves.  Everything is built once on the
CPU and never modified."""
import numpy as np

import clr_all_sky_ref as R

NLAYS = R.NLAYS
NCOL = R.NCOL
EPS = float(np.finfo(np.float32).eps)


def zero_source_flux_up(orc, tau, emis, sjac, top_at_1, nmus, ssa=None, g=None, lw_Ds=None):
    """The oracle's flux_up with lay_source = lev_source = 0, no incident flux and sfc_source_Jac as sfc_source."""
    ncol, nlay, ngpt = tau.shape
    z_lay = np.zeros((ncol, nlay, ngpt), np.float32)
    z_lev = np.zeros((ncol, nlay + 1, ngpt), np.float32)
    return orc.lw_solver(tau, z_lay, z_lev, emis, sjac, top_at_1, nmus, ssa=ssa, g=g, lw_Ds=lw_Ds)[0]


def layer_trans(orc, tau, D, ssa=None, g=None):
    """The float the solver's up pass multiplies by in each layer, (ncol, nlay, ngpt), for the secant D: every layer is
    solved by the oracle as a one-layer column with emissivity 1, surface source 1 and no other source, whose upward
    radiance at the top is T * 1 + 0 (the rescaled solver's adjustment term is 0 on zero sources)."""
    ncol, nlay, ngpt = tau.shape
    n = ncol * nlay
    one = np.ones((n, ngpt), np.float32)
    sub = lambda a: None if a is None else np.ascontiguousarray(a.reshape(n, 1, ngpt))  # noqa: E731
    out = orc.lw_solver(sub(tau), np.zeros((n, 1, ngpt), np.float32), np.zeros((n, 2, ngpt), np.float32), one, one, True,
                        1, ssa=sub(ssa), g=sub(g), lw_Ds=np.full((n, ngpt), D, np.float32), gpt=True)
    return out[2][:, 0, :].reshape(ncol, nlay, ngpt)  # the radiance at the top level (level 0 with top_at_1)


def direct_jacobian(orc, tau, emis, sjac, top_at_1, nmus, ssa=None, g=None):
    """The definition, one float32 operation per line: per angle J = emis * sfc_source_Jac at the surface and J = T * J
    through each layer going up; one angle: the sum of fac * J in four partials combined ((s0 + s1) + s2) + s3 when
    ngpt % 4 == 0, the plain sequential sum of the bare J otherwise (quirk B-5); several angles: fac * J accumulated per
    g-point in angle order, then the sequential sum."""
    import oracle as O
    ncol, nlay, ngpt = tau.shape
    Ds, W = O.gauss(nmus)
    f = np.float32
    acc = None
    for D, w in zip(Ds, W):
        T = layer_trans(orc, tau, f(D), ssa, g)
        fac = f(2.0) * f(np.pi) * f(w) if (nmus > 1 or ngpt % 4 == 0) else f(1.0)
        Jl = np.zeros((ncol, nlay + 1, ngpt), np.float32)
        J = emis * sjac
        Jl[:, nlay if top_at_1 else 0] = J
        for j in range(nlay):
            l = nlay - 1 - j if top_at_1 else j
            J = T[:, l] * J
            Jl[:, l if top_at_1 else l + 1] = J
        term = fac * Jl
        acc = term if acc is None else acc + term
    if nmus == 1 and ngpt % 4 == 0:
        s = np.zeros((ncol, nlay + 1, 4), np.float32)
        for i in range(0, ngpt, 4):
            s = s + acc[..., i:i + 4]
        return ((s[..., 0] + s[..., 1]) + s[..., 2]) + s[..., 3]
    s = np.zeros((ncol, nlay + 1), np.float32)
    for i in range(ngpt):
        s = s + acc[..., i]
    return s


def random_case(ngpt, nlay, seed, scat=False):
    """Random optical properties: tau over five decades (thin layers take the solver's series branch), emissivity in
    [0.8, 1], a surface source and its Jacobian of Planck magnitudes; scat: ssa and g too."""
    def make():
        rng = np.random.default_rng(seed)
        u = lambda lo, hi, *s: rng.uniform(lo, hi, s).astype(np.float32)  # noqa: E731
        c = dict(tau=(10.0 ** u(-5, 1, NCOL, nlay, ngpt)).astype(np.float32), emis=u(0.8, 1.0, NCOL, ngpt),
                 sfc=u(0.5, 2.0, NCOL, ngpt), sjac=u(0.005, 0.03, NCOL, ngpt), lay=u(0.2, 2.0, NCOL, nlay, ngpt),
                 lev=u(0.2, 2.0, NCOL, nlay + 1, ngpt), lw_Ds=u(1.2, 2.2, NCOL, ngpt))
        if scat:
            c["ssa"] = u(0.0, 0.9, NCOL, nlay, ngpt)
            c["g"] = u(0.0, 0.9, NCOL, nlay, ngpt)
        return c
    return R.cached(("jac-random", ngpt, nlay, seed, scat), make)


def mask_bits(ngpt, nlay, seed):
    """A packed McICA mask (NCOL, nlay, ceil(ngpt / 32)) uint32, about half the bits set, unused high bits zero, and the
    same mask as booleans (NCOL, nlay, ngpt)."""
    rng = np.random.default_rng(seed)
    m = rng.random((NCOL, nlay, ngpt)) < 0.5
    nw = (ngpt + 31) // 32
    pad = np.zeros((NCOL, nlay, nw * 32), bool)
    pad[..., :ngpt] = m
    bits = (pad.reshape(NCOL, nlay, nw, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(axis=-1)
    return bits.astype(np.uint32), m


def solver_case(orc, nlay, top_at_1, ngpt=None):
    """clr_all_sky_ref.solver_case (23 synthetic columns, NN gas optics, band cloud tau) with the Planck sources and
    sfc_source_Jac, a McICA mask and the optical depths of the three fused routes: clear, overcast (tau + cloud tau of
    the band) and masked (the cloud tau added where the mask bit is set)."""
    def make():
        c = dict(R.solver_case(orc, nlay, top_at_1, ngpt))
        lay, lev, sfc, sjac = orc.planck_source(c["kd"], c["prob"]["tlay"], c["tlev"], c["prob"]["tsfc"], c["pfrac"],
                                                c["sfc_lay"])
        ng = c["tau"].shape[-1]
        band_of = np.zeros(ng, np.int64)
        for b, (lo, hi) in enumerate(c["lims"]):
            band_of[lo - 1:hi] = b
        cld_g = c["cld"][..., band_of]
        bits, m = mask_bits(ng, nlay, 500 + nlay)
        c.update(lay=lay, lev=lev, sfc=sfc, sjac=sjac, bits=bits,
                 taus={"clear": c["tau"], "overcast": (c["tau"] + cld_g).astype(np.float32),
                       "masked": (c["tau"] + np.where(m, cld_g, np.float32(0))).astype(np.float32)})
        c["jac"] = {}
        return c
    return R.cached(("jac-solver", nlay, top_at_1, ngpt), make)


def expect(orc, case, route, top_at_1, nmus):
    """(flux_up, flux_dn, flux_up_Jac) of the oracle for one route of solver_case, computed once."""
    key = (route, nmus)
    if key not in case["jac"]:
        tau = case["taus"][route]
        up, dn = orc.lw_solver(tau, case["lay"], case["lev"], case["emis"], case["sfc"], top_at_1, nmus)
        case["jac"][key] = (up, dn, zero_source_flux_up(orc, tau, case["emis"], case["sjac"], top_at_1, nmus))
    return case["jac"][key]
