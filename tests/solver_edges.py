"""Operand-edge inputs for the RTE solvers, shared by tests/test_solver_edges_host.py (the conditions, on the CPU oracle)
and tests/test_gpu_solver_edges.py (the kernels, bit for bit against the oracle).

One case per column: a column has ONE lit g-point and ONE edge layer.  Every other layer of the lit g-point and every
unlit g-point hold benign properties (tau 0.05, ssa 0.5, g 0), and the unlit g-points get no incident flux, no albedo
and no source, so they carry exactly +-0 at every level: a broadband flux is then the lit g-point's flux bit for bit,
and a last-bit error at that one g-point cannot hide in a sum over the spectrum.  The lit g-point walks over every
residue mod 4 (the four interleaved partial sums) and both halves of a g-point pair (the two-per-lane kernels); the
edge layer sits at position column % nlay.

build_sw() / build_lw() return a dict of numpy arrays in the oracle's layout ((ncol, nlay, ngpt) ...) plus `cases`, one
named tuple of operand values per column, and `describe`, which names the cases of a list of columns for a failure
message.  Nothing here is random.

build_lw_scat() is the LW problem of the scattering and fused solvers (an edge (ssa, g) pair beside the edge tau, the
same edge through band arrays, an aerosol and a packed mask); ref_* are the oracle references both test files share,
computed once; classes() names the operand-domain classes of one run.

build_sw_fused() is the SW problem of the fused entries (the band increment with a cloud mask and a 2str aerosol, clear
beside all sky, by band, active columns): build_sw()'s cases with the edge as the cloud's band operand; ref_sw_fused() is
its shared reference, classes_sw() its classes and tile() repeats a problem's columns for the large-grid instances.
"""
import collections
import functools

import numpy as np

NLAY = 5
SW_NGPT = 224
LW_NGPT = 256
F = np.float32
FLT_MIN = F(1.17549435e-38)
FLT_EPS = F(np.finfo(np.float32).eps)
K_MIN = F(1.0e-4)
TAU_THRESH = np.sqrt(FLT_EPS)  # float32
EXP_UNDERFLOW = F(float.fromhex("-0x1.9fe368p6"))  # glibc expf returns 0 below this

BG_TAU, BG_SSA, BG_G = F(0.05), F(0.5), F(0.0)

TAUS = np.array([0, 1e-45, 1e-38, FLT_MIN, 1e-30, 1e-10, 1e-2, 1, 20, 53, 63, 88, 104, 1e4, 1e30, 2e38], F)
SSAS = np.array([0, 1e-45, 1e-38, 2.0 ** -101, 2.0 ** -99, 1e-20, 1e-3, 0.5, 0.9999, 0.99997, 1 - 2.0 ** -24, 1], F)
GS = np.array([0, 0.3, 0.85, 1], F)
MU0S = np.array([1, 0.5, 1e-3, 1e-30, FLT_MIN], F)
RESONANT = [(F(0.5), F(0.0)), (F(0.3), F(0.85))]  # (w0, g) whose 1/k is a mu0 of its own
ALBS = np.array([0, 0.3, 1], F)
INC_DIRS = np.array([1, 1e-38, 1000], F)
INC_DIFS = np.array([0.5, 0, 1e-38], F)

# the band increment of rrtmgpnn_sw_solver_2stream_inc (per column, every layer and band)
INC_NBND = 14
INC_TAUS = np.array([0, 1e-30, 0.1, 5], F)
INC_SSAS = np.array([0, 1e-10, 0.9, 1], F)
INC_GS = np.array([0, 0.5, 0.85], F)

LW_SRCS = np.array([0, 1e-38, 1, 300], F)
LW_EMIS = np.array([0, 0.5, 1], F)
LW_INCS = np.array([0, 0.05], F)
LW_DS = np.array([1.0, 1.66, 2.5], F)  # the lit values of the lw_Ds array
LW_LEVS = np.array([0.8, 0], F)  # the level sources on both sides of the edge layer: with 0 the layer source's term
#                                  2 * fact * lay_source is the whole source, so fact's last bit reaches the flux
LW_PFRACS = np.array([0, 1e-38, 0.1, 1], F)  # the edge layer's Planck fraction (fused-Planck entry)
LW_BG_LAY, LW_BG_LEV, LW_BG_SFC, LW_BG_PFRAC = F(1.0), F(0.8), F(1.2), F(0.05)

SwCase = collections.namedtuple("SwCase", "col mu0 tau ssa g alb_dir alb_dif inc_dir inc_dif lit layer")
LwCase = collections.namedtuple("LwCase", "col tau src lev emis inc lw_d pfrac lit layer")


def gauss_ds(nmus):
    """The Gauss secants of rte_lw (oracle.gauss), as float32."""
    return {1: [1.66], 3: [1.09719858, 1.69338507, 4.70941630]}[nmus]


def sw_k(w0, g):
    """k of sw_two_stream in float32, operation by operation."""
    w0, g = np.asarray(w0, F), np.asarray(g, F)
    gamma1 = (F(8) - w0 * (F(5) + F(3) * g)) * F(.25)
    gamma2 = F(3) * (w0 * (F(1) - g)) * F(.25)
    return np.sqrt(np.maximum((gamma1 - gamma2) * (gamma1 + gamma2), K_MIN)), (gamma1 - gamma2) * (gamma1 + gamma2)


def in_eps_branch(w0, g, mu0):
    """|1 - (k mu0)^2| < eps in float32: sw_two_stream replaces the denominator by eps."""
    k_mu = sw_k(w0, g)[0] * np.asarray(mu0, F)
    return np.abs(F(1) - k_mu * k_mu) < FLT_EPS


def resonant_mu0(w0, g):
    """The float nearest 1/k(w0, g) that puts sw_two_stream into its eps branch, found by stepping a few ulps."""
    k = sw_k(w0, g)[0]
    m = F(1) / k
    cands = [m]
    lo = hi = m
    for _ in range(8):
        lo, hi = np.nextafter(lo, F(0)), np.nextafter(hi, F(2))
        cands += [lo, hi]
    hits = [c for c in cands if in_eps_branch(w0, g, c)]
    assert hits, "no float32 mu0 near 1/k(%r, %r) reaches the eps branch" % (w0, g)
    return F(hits[0])  # cands are ordered by distance from 1/k


def tau_at_thresh(D, scale=1):
    """The largest float32 tau with (tau*D)*scale <= sqrt(FLT_EPSILON) in float32 (the solvers' operation order; scale:
    the rescaled solver's scaleTau), and the next float above it."""
    D, scale = F(D), F(scale)
    prod = lambda t: F(F(t * D) * scale)  # noqa: E731
    t = F(TAU_THRESH / F(D * scale))
    while prod(t) <= TAU_THRESH:
        t = np.nextafter(t, F(1))
    while prod(t) > TAU_THRESH:
        t = np.nextafter(t, F(0))
    return t, np.nextafter(t, F(1))


def _describe(cases):
    def describe(cols, limit=6):
        cols = list(cols)
        s = "; ".join(str(cases[c]) for c in cols[:limit])
        return "%d column(s) differ: %s%s" % (len(cols), s, " ..." if len(cols) > limit else "")
    return describe


def mismatch_columns(got, want):
    """Columns (axis 0) in which any value differs (assert_array_equal's notion: NaN equals NaN, -0 equals 0)."""
    got, want = np.asarray(got), np.asarray(want)
    bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    return np.unique(np.nonzero(bad.reshape(bad.shape[0], -1))[0])


def assert_bitwise(got, want, prob, what, cols=None):
    """assert_array_equal on the columns `cols` (default all), naming the operand cases of the columns that differ."""
    got, want = np.asarray(got), np.asarray(want)
    if cols is not None:
        got, want = got[cols], want[cols]
    bad = mismatch_columns(got, want)
    if bad.size:
        ids = bad if cols is None else np.asarray(cols)[bad]
        np.testing.assert_array_equal(got, want, err_msg="%s: %s" % (what, prob["describe"](ids)))


def _freeze(d):
    """The problems are built once and shared: their arrays are read-only."""
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    for v in d.get("edge", {}).values():
        v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def build_sw():
    """The SW problem: every (mu0, tau, ssa) of the lists above is one column; g, the albedos, the incident fluxes and
    the band increment cycle with the three indices so that each pairing occurs."""
    mu0s = np.concatenate([MU0S, np.array([resonant_mu0(w, g) for w, g in RESONANT], F)])
    n_s, n_t, n_m = len(SSAS), len(TAUS), len(mu0s)
    ncol, nlay, ngpt = n_s * n_t * n_m, NLAY, SW_NGPT
    tau = np.full((ncol, nlay, ngpt), BG_TAU, F)
    ssa = np.full((ncol, nlay, ngpt), BG_SSA, F)
    g = np.full((ncol, nlay, ngpt), BG_G, F)
    mu0 = np.empty(ncol, F)
    inc, inc_dif, alb_dir, alb_dif = (np.zeros((ncol, ngpt), F) for _ in range(4))
    tau_bnd, ssa_bnd, g_bnd = (np.empty((ncol, nlay, INC_NBND), F) for _ in range(3))
    cases = []
    for c in range(ncol):
        i_s, i_t, i_m = c % n_s, (c // n_s) % n_t, c // (n_s * n_t)
        lit, layer = (37 * c) % ngpt, c % nlay
        w_e, g_e = SSAS[i_s], GS[(i_s + i_t + i_m) % len(GS)]
        if i_m >= len(MU0S):  # a resonant mu0: the edge layer holds the (w0, g) it belongs to
            w_e, g_e = RESONANT[i_m - len(MU0S)]
        case = SwCase(col=c, mu0=mu0s[i_m], tau=TAUS[i_t], ssa=w_e, g=g_e,
                      alb_dir=ALBS[(i_s + i_t + 2 * i_m) % 3], alb_dif=ALBS[(i_s // 3 + i_t + i_m) % 3],
                      inc_dir=INC_DIRS[(i_s + i_m + i_t // 2) % 3], inc_dif=INC_DIFS[(i_s // 2 + i_t + i_m) % 3],
                      lit=lit, layer=layer)
        cases.append(case)
        mu0[c] = case.mu0
        tau[c, layer, lit], ssa[c, layer, lit], g[c, layer, lit] = case.tau, case.ssa, case.g
        inc[c, lit], inc_dif[c, lit] = case.inc_dir, case.inc_dif
        alb_dir[c, lit], alb_dif[c, lit] = case.alb_dir, case.alb_dif
        tau_bnd[c] = INC_TAUS[(i_s + i_m) % 4]
        ssa_bnd[c] = INC_SSAS[(i_s // 4 + i_t + i_m) % 4]
        g_bnd[c] = INC_GS[(i_s + i_t // 4) % 3]
    edge = {k: np.array([getattr(x, k) for x in cases], F) for k in ("tau", "ssa", "g", "mu0")}
    lims = np.array([[16 * b + 1, 16 * b + 16] for b in range(INC_NBND)], np.int32)
    return _freeze({"ncol": ncol, "nlay": nlay, "ngpt": ngpt, "tau": tau, "ssa": ssa, "g": g, "mu0": mu0, "inc": inc,
            "inc_dif": inc_dif, "alb_dir": alb_dir, "alb_dif": alb_dif, "cases": cases, "edge": edge,
            "lit": np.array([x.lit for x in cases]), "layer": np.array([x.layer for x in cases]),
            "band_lims_gpt": lims, "tau_bnd": tau_bnd, "ssa_bnd": ssa_bnd, "g_bnd": g_bnd,
            # the operand domain the shortened divisions state (tests that must pass outright)
            "in_domain": (edge["tau"] <= F(1e4)) & ((edge["ssa"] == 0) | (edge["ssa"] >= F(2.0 ** -99))),
            "g0": np.nonzero(edge["g"] == 0)[0], "describe": _describe(cases)})


def lw_secants():
    """Every secant the LW tests use: the Gauss secants of one and three angles and the lit lw_Ds values."""
    return sorted(set(F(d) for d in gauss_ds(1) + gauss_ds(3)) | set(LW_DS))


def lw_taus():
    thr = [t for D in lw_secants() for t in tau_at_thresh(D)]
    return np.concatenate([TAUS, np.array(thr, F)])


@functools.lru_cache(maxsize=None)
def build_lw():
    """The LW problem: every (tau, source, emissivity, incident flux) is one column; tau runs over the SW list plus, for
    each secant in use, the two floats around tau*D == sqrt(FLT_EPSILON).  The edge layer's source runs over LW_SRCS and
    the sources of the two levels around it over LW_LEVS."""
    taus = lw_taus()
    ncol, nlay, ngpt = len(taus) * len(LW_SRCS) * len(LW_EMIS) * len(LW_INCS), NLAY, LW_NGPT
    tau = np.full((ncol, nlay, ngpt), BG_TAU, F)
    lay, pfrac = (np.zeros((ncol, nlay, ngpt), F) for _ in range(2))
    lev = np.zeros((ncol, nlay + 1, ngpt), F)
    sfc, emis, inc = (np.zeros((ncol, ngpt), F) for _ in range(3))
    lw_ds = np.full((ncol, ngpt), F(1.66), F)
    cases = []
    for c in range(ncol):
        i_src, i_em, i_inc, i_tau = c % 4, (c // 4) % 3, (c // 12) % 2, c // 24
        lit, layer = (37 * c) % ngpt, c % nlay
        case = LwCase(col=c, tau=taus[i_tau], src=LW_SRCS[i_src], lev=LW_LEVS[(i_src // 2 + i_em + i_inc + i_tau) % 2],
                      emis=LW_EMIS[i_em], inc=LW_INCS[i_inc],
                      lw_d=LW_DS[(i_src + i_em) % 3], pfrac=LW_PFRACS[i_src], lit=lit, layer=layer)
        cases.append(case)
        lay[c, :, lit], lev[c, :, lit], sfc[c, lit] = LW_BG_LAY, LW_BG_LEV, LW_BG_SFC
        pfrac[c, :, lit] = LW_BG_PFRAC
        tau[c, layer, lit], lay[c, layer, lit], pfrac[c, layer, lit] = case.tau, case.src, case.pfrac
        lev[c, layer:layer + 2, lit] = case.lev
        emis[c, lit], inc[c, lit], lw_ds[c, lit] = case.emis, case.inc, case.lw_d
    # temperatures of the fused-Planck entry: inside the Planck table, layers and levels different
    tlay = (F(220) + F(15) * np.arange(nlay, dtype=F)[None, :] + (np.arange(ncol) % 7).astype(F)[:, None]).astype(F)
    tlev = np.concatenate([tlay - F(7), tlay[:, -1:] + F(8)], axis=1).astype(F)
    edge = {k: np.array([getattr(x, k) for x in cases], F) for k in ("tau", "lw_d")}
    return _freeze({"ncol": ncol, "nlay": nlay, "ngpt": ngpt, "tau": tau, "lay": lay, "lev": lev, "sfc": sfc, "emis": emis,
            "inc": inc, "lw_ds": lw_ds, "pfrac": pfrac, "tlay": tlay, "tlev": tlev, "cases": cases, "edge": edge,
            "lit": np.array([x.lit for x in cases]), "layer": np.array([x.layer for x in cases]),
            "in_domain": edge["tau"] <= F(1e4),
            # tau * D beyond 2^126 for every secant in use (all are >= 1): past the bound that solver_div states
            "beyond_2p126": edge["tau"] > F(2.0 ** 126), "describe": _describe(cases)})


def lw_tsfc(prob, top_at_1):
    """Surface temperature of the fused-Planck entry: a little above the surface level's."""
    return (prob["tlev"][:, -1 if top_at_1 else 0] + F(2)).astype(F)


# ---- the scattering and fused LW solvers ----------------------------------------------------------------------------
SCAT_SSAS = np.array([0, 1e-45, 1e-38, 2.0 ** -99, 1e-20, 1e-3, 0.5, 0.9999, 1 - 2.0 ** -24, 1], F)
SCAT_GS = np.array([0, 0.3, 0.85, -0.4, 1 - 2.0 ** -24, 1], F)
# (1, 1) is left out: scaleTau = 0 and gamma1 = gamma2 = 0 there, the entries exclude it (ssa (1 + g) / 2 < 1) and the
# oracle itself is nan
SCAT_PAIRS = [(w, g) for w in SCAT_SSAS for g in SCAT_GS if not (w == 1 and g == 1)]
THRESH_PAIRS = [(F(0.5), F(0.3)), (F(0.9999), F(0.85))]  # scaleTau != 1: the series / quotient switch moves with it
TAUS_1E8 = np.array([np.nextafter(F(1e-8), F(0)), F(1e-8), np.nextafter(F(1e-8), F(1))], F)  # l2_layer's branch
# more huge optical depths: the fused entries see the edge tau as the gas tau in a third of the columns only, and every
# compared class wants 20 columns (tau * D below 2^126 for the first two, beyond it or inf for the others)
SCAT_BIG_TAUS = np.array([1e32, 1e34, 1e38, 3e38], F)
AER_TAUS = np.array([0, 1e-30, 0.1], F)
LW_SJAC = F(0.02)  # sfc_source_Jac at the lit g-point
EPS_INC = F(3) * FLT_MIN  # the band increment's max(eps, .)

ScatCase = collections.namedtuple("ScatCase", "col tau ssa g src lev emis inc pfrac gas_tau aer bit lit layer")


def scale_tau(ssa, g):
    """(wb, scaleTau, Cn) of the rescaled layer in float32, operation by operation (rs_layer)."""
    ssa, g = np.asarray(ssa, F), np.asarray(g, F)
    wb = ssa * (F(1) - g) * F(0.5)
    scale = (F(1) - ssa) + wb
    with np.errstate(divide="ignore", invalid="ignore"):
        return wb, scale, F(0.4) * wb / scale


def l2_terms(tau, w0, g):
    """(k^2 before the clamp, emk, em2k) of lw_two_stream in float32, operation by operation (expf taken by numpy: only
    its zeros are used, and those lie far from any rounding question)."""
    tau, w0, g = np.asarray(tau, F), np.asarray(w0, F), np.asarray(g, F)
    d = F(1.66)
    gamma1 = d * (F(1) - F(0.5) * w0 * (F(1) + g))
    gamma2 = d * F(0.5) * w0 * (F(1) - g)
    k2 = (gamma1 - gamma2) * (gamma1 + gamma2)
    k = np.sqrt(np.maximum(k2, K_MIN))
    with np.errstate(over="ignore", under="ignore"):
        emk = np.exp(-tau * k, dtype=F)
        return k2, emk, emk * emk


def rescl_secants():
    """The secants the rescaled solver is run with (Gauss, one and three angles)."""
    return sorted(set(F(d) for d in gauss_ds(1) + gauss_ds(3)))


def lw_scat_taus():
    """[(tau, forced (ssa, g) pair or None)]: lw_taus(), the three floats around 1e-8, SCAT_BIG_TAUS and, for each pair of
    THRESH_PAIRS and every Gauss secant, the two floats around tau * D * scaleTau == sqrt(FLT_EPSILON)."""
    out = [(t, None) for t in lw_taus()] + [(t, None) for t in TAUS_1E8] + [(t, None) for t in SCAT_BIG_TAUS]
    for w, g in THRESH_PAIRS:
        sc = scale_tau(w, g)[1]
        assert sc != 1
        out += [(t, (w, g)) for D in rescl_secants() for t in tau_at_thresh(D, sc)]
    return out


def inc_2str_gas(t1, t2, w2, g2):
    """inc_2stream_by_2stream of (t1, 0, 0) by (t2, w2, g2) in float32, operation by operation -> (tau, ssa, g, tauscat12)."""
    t1, t2, w2, g2 = (np.asarray(a, F) for a in (t1, t2, w2, g2))
    z = F(0)
    with np.errstate(over="ignore", under="ignore"):
        tau12 = t1 + t2
        scat = t1 * z + t2 * w2
        gq = (t1 * z * z + t2 * w2 * g2) / np.maximum(EPS_INC, scat)
        return tau12, scat / np.maximum(EPS_INC, tau12), gq, scat


@functools.lru_cache(maxsize=None)
def build_lw_scat():
    """The LW problem of the scattering and fused solvers, on build_lw()'s design: one lit g-point at (37 c) % ngpt, the
    edge layer at c % nlay, background tau 0.05 / ssa 0.5 / g 0, no source, emissivity or incident flux at the unlit
    g-points.  Every tau of lw_scat_taus() is 24 columns (source x emissivity x incident flux, as build_lw()); the edge
    (ssa, g) pair cycles through SCAT_PAIRS with the column number (59 pairs against 24 columns a tau: every tau meets 24
    pairs and every pair about 20 of the 51 taus), except at the taus built for a pair of THRESH_PAIRS, which hold it.

    The fused-Planck entries get the same edge through the band arrays: tau_bnd / ssa_bnd / g_bnd hold the edge values
    at the edge layer in the lit g-point's band (the shipped LW bands) and cycle over INC_TAUS / INC_SSAS / INC_GS
    elsewhere; the gas tau there (tau_gas) cycles over {0, BG_TAU, the edge tau} (0 where the edge tau is 0); tau_aer cycles over AER_TAUS by column,
    layer and band; mask: the lit bit at the edge layer set in even columns, clear in odd ones, every other bit
    alternating by layer and g-point; emis_bnd: the edge emissivity in the lit band, 0 elsewhere."""
    from rrtmgpnn import data
    kd = data.load_kdist("lw")
    lims = np.asarray(kd["band_lims_gpt"], np.int32).reshape(-1, 2)
    taus = lw_scat_taus()
    per = len(LW_SRCS) * len(LW_EMIS) * len(LW_INCS)
    ncol, nlay, ngpt, nb = len(taus) * per, NLAY, LW_NGPT, len(lims)
    assert kd["ngpt"] == ngpt
    band_of = np.zeros(ngpt, np.int64)
    for b, (lo, hi) in enumerate(lims):
        band_of[lo - 1:hi] = b
    tau = np.full((ncol, nlay, ngpt), BG_TAU, F)
    ssa = np.full((ncol, nlay, ngpt), BG_SSA, F)
    g = np.full((ncol, nlay, ngpt), BG_G, F)
    tau_gas = np.full((ncol, nlay, ngpt), BG_TAU, F)
    lay, pfrac = (np.zeros((ncol, nlay, ngpt), F) for _ in range(2))
    lev = np.zeros((ncol, nlay + 1, ngpt), F)
    sfc, sjac, emis, inc = (np.zeros((ncol, ngpt), F) for _ in range(4))
    emis_bnd = np.zeros((ncol, nb), F)
    ci, li, bi = np.meshgrid(np.arange(ncol), np.arange(nlay), np.arange(nb), indexing="ij")
    tau_bnd = INC_TAUS[(ci + li + bi) % 4]
    ssa_bnd = INC_SSAS[(ci // 4 + li + 2 * bi) % 4]
    g_bnd = INC_GS[(ci + li // 2 + bi) % 3]
    tau_aer = AER_TAUS[(ci + 2 * li + bi) % 3]
    gi = np.arange(ngpt)
    mask = ((np.arange(nlay)[None, :, None] + gi[None, None, :]) % 2 == 0) & np.ones((ncol, 1, 1), bool)
    cases = []
    for c in range(ncol):
        i_src, i_em, i_inc, i_tau = c % 4, (c // 4) % 3, (c // 12) % 2, c // per
        lit, layer = (37 * c) % ngpt, c % nlay
        t_e, forced = taus[i_tau]
        w_e, g_e = forced if forced is not None else SCAT_PAIRS[(7 * c) % len(SCAT_PAIRS)]
        r = c % per
        gas = (F(0), BG_TAU, t_e)[(r + r // 4 + i_tau) % 3] if t_e != 0 else F(0)  # tau_bnd = 0: always t1 = t2 = 0
        b = band_of[lit]
        aer = AER_TAUS[(r // 2 + i_tau) % 3]
        case = ScatCase(col=c, tau=t_e, ssa=w_e, g=g_e, src=LW_SRCS[i_src],
                        lev=LW_LEVS[(i_src // 2 + i_em + i_inc + i_tau) % 2], emis=LW_EMIS[i_em], inc=LW_INCS[i_inc],
                        pfrac=LW_PFRACS[i_src], gas_tau=gas, aer=aer, bit=c % 2 == 0, lit=lit, layer=layer)
        cases.append(case)
        lay[c, :, lit], lev[c, :, lit], sfc[c, lit], sjac[c, lit] = LW_BG_LAY, LW_BG_LEV, LW_BG_SFC, LW_SJAC
        pfrac[c, :, lit] = LW_BG_PFRAC
        tau[c, layer, lit], ssa[c, layer, lit], g[c, layer, lit] = t_e, w_e, g_e
        lay[c, layer, lit], pfrac[c, layer, lit] = case.src, case.pfrac
        lev[c, layer:layer + 2, lit] = case.lev
        emis[c, lit], inc[c, lit], emis_bnd[c, b] = case.emis, case.inc, case.emis
        tau_gas[c, layer, lit] = gas
        tau_bnd[c, layer, b], ssa_bnd[c, layer, b], g_bnd[c, layer, b], tau_aer[c, layer, b] = t_e, w_e, g_e, aer
        mask[c, layer, lit] = case.bit
    tlay = (F(220) + F(15) * np.arange(nlay, dtype=F)[None, :] + (np.arange(ncol) % 7).astype(F)[:, None]).astype(F)
    tlev = np.concatenate([tlay - F(7), tlay[:, -1:] + F(8)], axis=1).astype(F)
    edge = {k: np.array([getattr(x, k) for x in cases], F) for k in ("tau", "ssa", "g", "gas_tau", "aer")}
    edge["bit"] = np.array([x.bit for x in cases])
    return _freeze({"ncol": ncol, "nlay": nlay, "ngpt": ngpt, "nb": nb, "kd": kd, "lims": lims, "band_of": band_of,
                    "tau": tau, "ssa": ssa, "g": g, "lay": lay, "lev": lev, "sfc": sfc, "sjac": sjac, "emis": emis,
                    "inc": inc, "pfrac": pfrac, "tlay": tlay, "tlev": tlev, "tau_gas": tau_gas,
                    "tau_bnd": np.ascontiguousarray(tau_bnd, F), "ssa_bnd": np.ascontiguousarray(ssa_bnd, F),
                    "g_bnd": np.ascontiguousarray(g_bnd, F), "tau_aer": np.ascontiguousarray(tau_aer, F),
                    "mask": mask, "emis_bnd": emis_bnd, "cases": cases, "edge": edge,
                    "lit": np.array([x.lit for x in cases]), "layer": np.array([x.layer for x in cases]),
                    "describe": _describe(cases)})


def edge_values(p, a):
    """a (ncol, nlay, ngpt) at every column's (edge layer, lit g-point)."""
    return np.asarray(a)[np.arange(p["ncol"]), p["layer"], p["lit"]]


def classes(p, tau_op, scale=None, secants=None):
    """p with the domain classes of one run: in_domain (the operand tau_op <= 1e4), beyond_2p126 (the operand the
    layer's division sees, (tau_op * D) * scale, beyond 2^126 for any secant of the run; never, without secants); what
    is in neither is large_tau."""
    tau_op = np.asarray(tau_op, F)
    beyond = np.zeros(p["ncol"], bool)
    with np.errstate(over="ignore", invalid="ignore"):
        for D in secants or ():
            t = tau_op * F(D)
            beyond |= (t if scale is None else t * np.asarray(scale, F)) > F(2.0 ** 126)
    return dict(p, in_domain=tau_op <= F(1e4), beyond_2p126=beyond)


def with_background_pair(p, key_ssa="ssa", key_g="g"):
    """Copies of the (ssa, g) arrays with the background pair at every edge layer (condition 4)."""
    c = np.arange(p["ncol"])
    w, q = p[key_ssa].copy(), p[key_g].copy()
    if w.shape[-1] == p["ngpt"]:
        w[c, p["layer"], p["lit"]], q[c, p["layer"], p["lit"]] = BG_SSA, BG_G
    else:
        b = p["band_of"][p["lit"]]
        w[c, p["layer"], b], q[c, p["layer"], b] = BG_SSA, BG_G
    return w, q


def flipped_lit_mask(p):
    m = p["mask"].copy()
    c = np.arange(p["ncol"])
    m[c, p["layer"], p["lit"]] = ~m[c, p["layer"], p["lit"]]
    return m


def _expand(bnd, lims, ngpt):
    out = np.zeros(bnd.shape[:-1] + (ngpt,), F)
    for ib, (lo, hi) in enumerate(np.asarray(lims).reshape(-1, 2)):
        out[..., lo - 1:hi] = bnd[..., ib:ib + 1]
    return out


def _ident(ng):
    return np.stack([np.arange(1, ng + 1)] * 2, axis=1).astype(np.int32)


def fused_props(orc, p, masked=False, aer=False, cloud=None, mask=None):
    """(tau, ssa, g) of the composed oracle of the fused rescaled entries: increment_bybnd of (tau_gas, 0, 0) by the
    1scl aerosol first (aer), then by the cloud (tau_bnd, ssa_bnd, g_bnd) -- masked: each band array through
    mcica_ref.draw, at identity limits.  cloud / mask: others than the problem's."""
    import mcica_ref as M
    z = np.zeros_like(p["tau_gas"])
    io = [p["tau_gas"], z, z]
    if aer:
        io = orc.increment_bybnd(p["lims"], io, [p["tau_aer"]])
    cloud = [p["tau_bnd"], p["ssa_bnd"], p["g_bnd"]] if cloud is None else cloud
    if not masked:
        return orc.increment_bybnd(p["lims"], io, cloud)
    mask = p["mask"] if mask is None else mask
    return orc.increment_bybnd(_ident(p["ngpt"]), io, [M.draw(mask, a, p["lims"]) for a in cloud])


def planck_sources(orc, p, top_at_1):
    lay, lev, sfc, _ = orc.planck_source(p["kd"] if "kd" in p else _kd(), p["tlay"], p["tlev"], lw_tsfc(p, top_at_1),
                                         p["pfrac"], p["nlay"] if top_at_1 else 1)
    return lay, lev, sfc


def _kd():
    from rrtmgpnn import data
    return data.load_kdist("lw")


_refs = {}


def _cached(key, make):
    if key not in _refs:
        _refs[key] = make()
    return _refs[key]


def ref_rescl(orc, top_at_1, nmus, gpt=False):
    """Entries 1 and 2: the oracle's rescaled solver on the edge problem, with incident flux."""
    p = build_lw_scat()
    return _cached(("rescl", top_at_1, nmus, gpt), lambda: orc.lw_solver(
        p["tau"], p["lay"], p["lev"], p["emis"], p["sfc"], top_at_1, nmus, inc_flux=p["inc"], ssa=p["ssa"], g=p["g"],
        gpt=gpt))


def ref_rescl_jac(orc, top_at_1, nmus):
    """Entry 3: flux_up_Jac, the oracle's flux_up on zero sources with sfc_source_Jac as the surface source."""
    import lw_jacobian_ref as J
    p = build_lw_scat()
    return _cached(("jac", top_at_1, nmus), lambda: J.zero_source_flux_up(
        orc, p["tau"], p["emis"], p["sjac"], top_at_1, nmus, ssa=p["ssa"], g=p["g"]))


def ref_2stream(orc, top_at_1, with_inc, gpt=False):
    """Entry 4: the oracle's lw_solver_2stream."""
    p = build_lw_scat()
    return _cached(("2str", top_at_1, with_inc, gpt), lambda: orc.lw_solver_2stream(
        p["tau"], p["ssa"], p["g"], p["lev"], p["emis"], p["sfc"], top_at_1, p["inc"] if with_inc else None, gpt=gpt))


def ref_fused(orc, top_at_1, nmus, masked, aer=False, emis_by_band=False):
    """Entries 5 and 6: (flux_up, flux_dn, flux_up_clr, flux_dn_clr, (tau, ssa, g) of the all-sky set, tau of the clear
    set) of the composed oracle."""
    p = build_lw_scat()

    def make():
        io = fused_props(orc, p, masked, aer)
        lay, lev, sfc = planck_sources(orc, p, top_at_1)
        emis = _expand(p["emis_bnd"], p["lims"], p["ngpt"]) if emis_by_band else p["emis"]
        up, dn = orc.lw_solver(io[0], lay, lev, emis, sfc, top_at_1, nmus, inc_flux=p["inc"], ssa=io[1], g=io[2])
        tc = orc.increment_bybnd(p["lims"], [p["tau_gas"]], [p["tau_aer"]])[0] if aer else p["tau_gas"]
        cu, cd = orc.lw_solver(tc, lay, lev, emis, sfc, top_at_1, nmus, inc_flux=p["inc"])
        return up, dn, cu, cd, io, tc
    return _cached(("fused", top_at_1, nmus, masked, aer, emis_by_band), make)


# ---- the no-scattering fused entries on build_lw()'s problem ---------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lw_band_inc():
    """The band increment of the no-scattering fused entries on build_lw(): tau_bnd (ncol, nlay, nbnd) cycling INC_TAUS
    by column, layer and band on the shipped LW bands, and a mask whose lit bit at the edge layer is set in the even
    columns."""
    p = build_lw()
    kd = _kd()
    lims = np.asarray(kd["band_lims_gpt"], np.int32).reshape(-1, 2)
    ci, li, bi = np.meshgrid(np.arange(p["ncol"]), np.arange(p["nlay"]), np.arange(len(lims)), indexing="ij")
    tau_bnd = np.ascontiguousarray(INC_TAUS[(ci + li + bi) % 4], F)
    mask = ((np.arange(p["nlay"])[None, :, None] + np.arange(p["ngpt"])[None, None, :]) % 2 == 0) & \
        np.ones((p["ncol"], 1, 1), bool)
    c = np.arange(p["ncol"])
    mask[c, p["layer"], p["lit"]] = c % 2 == 0
    return _freeze({"kd": kd, "lims": lims, "nb": len(lims), "tau_bnd": tau_bnd, "mask": mask})


def ref_noscat_fused(orc, top_at_1, nmus, kind):
    """Entry 7.  kind "inc" / "masked": (up, dn, tau) of tau + tau_bnd(band) [where the mask bit is set]; "clear": of tau;
    "gpt": (up, dn, gpt_up, gpt_dn) with the lw_Ds secants."""
    import mcica_ref as M
    p, b = build_lw(), lw_band_inc()

    def make():
        lay, lev, sfc = planck_sources(orc, dict(p, kd=b["kd"]), top_at_1)
        if kind == "gpt":
            return orc.lw_solver(p["tau"], lay, lev, p["emis"], sfc, top_at_1, 1, inc_flux=p["inc"], lw_Ds=p["lw_ds"],
                                 gpt=True)
        if kind == "inc":
            tau = orc.increment_bybnd(b["lims"], [p["tau"]], [b["tau_bnd"]])[0]
        elif kind == "masked":
            tau = orc.increment_bybnd(_ident(p["ngpt"]), [p["tau"]], [M.draw(b["mask"], b["tau_bnd"], b["lims"])])[0]
        else:
            tau = p["tau"]
        return orc.lw_solver(tau, lay, lev, p["emis"], sfc, top_at_1, nmus, inc_flux=p["inc"]) + (tau,)
    return _cached(("noscat_fused", top_at_1, nmus, kind), make)


# ---- the fused SW solvers: band increment, cloud mask, aerosol, clear beside all sky, by band -------------------------
SW_AER_TAUS = np.array([0, 1e-30, 0.1], F)
SW_AER_SSAS = np.array([0, 0.9, 1], F)
SW_AER_GS = np.array([0, 0.6], F)

FusedSwCase = collections.namedtuple("FusedSwCase", SwCase._fields + ("gas_tau", "gas_ssa", "gas_g", "bit"))


@functools.lru_cache(maxsize=None)
def build_sw_fused():
    """The SW problem of the fused entries, on build_sw()'s design and with its 1344 cases (edge (tau, ssa, g), mu0,
    albedos, incident fluxes, lit g-point and edge layer), on the shipped SW bands (14 x 16, the band-pair layout).

    The case's edge (tau, ssa, g) is the CLOUD's: tau_bnd / ssa_bnd / g_bnd hold it at (edge layer, lit g-point's band)
    and cycle over INC_TAUS / INC_SSAS / INC_GS by column, layer and band elsewhere.  The gas tau and ssa at (edge layer,
    lit g-point) cycle over {0, background, the case's edge value}, each on its own (all nine pairings occur); the gas
    tau falls back to the background where tau_gas + tau_edge overflows to inf in float32 (2e38 + 2e38: the oracle's
    own properties are inf there).  The gas g holds the case's g where the gas ssa is the edge ssa and 0 elsewhere.
    The 2str aerosol cycles over SW_AER_TAUS / SW_AER_SSAS / SW_AER_GS by column, layer and band.  mask: alternating by
    layer + g-point, except the lit bit at the edge layer, which is set in half the columns by a mix of the three case
    indices (the column's parity alone would follow the ssa index: there are 12 of them)."""
    from rrtmgpnn import data
    b = build_sw()
    lims = np.asarray(data.load_kdist("sw")["band_lims_gpt"], np.int32).reshape(-1, 2)
    ncol, nlay, ngpt, nb = b["ncol"], b["nlay"], b["ngpt"], len(lims)
    assert nb == INC_NBND and np.array_equal(lims, b["band_lims_gpt"])
    band_of = np.zeros(ngpt, np.int64)
    for ib, (lo, hi) in enumerate(lims):
        band_of[lo - 1:hi] = ib
    n_s, n_t = len(SSAS), len(TAUS)
    tau = np.full((ncol, nlay, ngpt), BG_TAU, F)
    ssa = np.full((ncol, nlay, ngpt), BG_SSA, F)
    g = np.full((ncol, nlay, ngpt), BG_G, F)
    ci, li, bi = np.meshgrid(np.arange(ncol), np.arange(nlay), np.arange(nb), indexing="ij")
    tau_bnd = INC_TAUS[(ci + li + bi) % 4]
    ssa_bnd = INC_SSAS[(ci // 4 + li + 2 * bi) % 4]
    g_bnd = INC_GS[(ci + li // 2 + bi) % 3]
    tau_aer = SW_AER_TAUS[(ci + 2 * li + bi) % 3]
    ssa_aer = SW_AER_SSAS[(ci // 3 + li + bi) % 3]
    g_aer = SW_AER_GS[(ci // 2 + li + bi) % 2]
    mask = ((np.arange(nlay)[None, :, None] + np.arange(ngpt)[None, None, :]) % 2 == 0) & np.ones((ncol, 1, 1), bool)
    cases = []
    for c, x in enumerate(b["cases"]):
        i_s, i_t, i_m = c % n_s, (c // n_s) % n_t, c // (n_s * n_t)
        k_t, k_w = (i_s + i_m) % 3, (i_s // 3 + i_t + 2 * i_m) % 3
        gas_tau = (F(0), BG_TAU, x.tau)[k_t]
        with np.errstate(over="ignore"):
            if np.isinf(gas_tau + x.tau):
                gas_tau = BG_TAU
        gas_ssa = (F(0), BG_SSA, x.ssa)[k_w]
        gas_g = x.g if k_w == 2 else F(0)
        case = FusedSwCase(*x, gas_tau=gas_tau, gas_ssa=gas_ssa, gas_g=gas_g, bit=(i_s // 2 + i_t // 2 + i_m) % 2 == 1)
        cases.append(case)
        ib = band_of[x.lit]
        tau[c, x.layer, x.lit], ssa[c, x.layer, x.lit], g[c, x.layer, x.lit] = gas_tau, gas_ssa, gas_g
        tau_bnd[c, x.layer, ib], ssa_bnd[c, x.layer, ib], g_bnd[c, x.layer, ib] = x.tau, x.ssa, x.g
        mask[c, x.layer, x.lit] = case.bit
    edge = {k: np.array([getattr(x, k) for x in cases], F) for k in ("tau", "ssa", "g", "mu0", "gas_tau", "gas_ssa", "gas_g")}
    edge["bit"] = np.array([x.bit for x in cases])
    p = {k: b[k] for k in ("ncol", "nlay", "ngpt", "mu0", "inc", "inc_dif", "alb_dir", "alb_dif", "lit", "layer")}
    p.update({"nb": nb, "lims": lims, "band_of": band_of, "tau": tau, "ssa": ssa, "g": g, "mask": mask, "cases": cases,
              "edge": edge, "describe": _describe(cases)})
    for k, a in (("tau_bnd", tau_bnd), ("ssa_bnd", ssa_bnd), ("g_bnd", g_bnd), ("tau_aer", tau_aer), ("ssa_aer", ssa_aer),
                 ("g_aer", g_aer)):
        p[k] = np.ascontiguousarray(a, F)
    return _freeze(p)


def sw_fused_props(orc, p, masked=False, aer=False, with_g=True, cloud=None, mask=None):
    """((tau, ssa, g) all sky, (tau, ssa, g) clear) of the composed oracle of the fused SW entries: increment_bybnd of
    the gases by the 2str aerosol first (aer: both sets), then by the cloud (the all-sky set) -- masked: each band array
    through mcica_ref.draw, at identity limits, as fused_props.  with_g False: the gas g is zero (the entries' g = NULL).
    cloud / mask: others than the problem's."""
    import mcica_ref as M
    clear = (p["tau"], p["ssa"], p["g"] if with_g else np.zeros_like(p["g"]))
    if aer:
        clear = orc.increment_bybnd(p["lims"], clear, [p["tau_aer"], p["ssa_aer"], p["g_aer"]])
    cloud = [p["tau_bnd"], p["ssa_bnd"], p["g_bnd"]] if cloud is None else cloud
    if not masked:
        return orc.increment_bybnd(p["lims"], clear, cloud), clear
    mask = p["mask"] if mask is None else mask
    return orc.increment_bybnd(_ident(p["ngpt"]), clear, [M.draw(mask, a, p["lims"]) for a in cloud]), clear


def sw_fused_solve(orc, p, io, top_at_1, gpt=False):
    return orc.sw_solver(*io, p["mu0"], p["inc"], p["alb_dir"], p["alb_dif"], top_at_1, inc_flux_dif=p["inc_dif"], gpt=gpt)


def ref_sw_fused(orc, top_at_1, masked, aer, with_g, gpt=False):
    """(all-sky fluxes, clear fluxes, all-sky (tau, ssa, g), clear (tau, ssa, g)) of the composed oracle on
    build_sw_fused(); the flux tuples are (up, dn, dir), with gpt followed by the three g-point arrays."""
    p = build_sw_fused()
    io, clr = _cached(("sw_props", masked, aer, with_g), lambda: sw_fused_props(orc, p, masked, aer, with_g))
    allsky = _cached(("sw_all", top_at_1, masked, aer, with_g, gpt), lambda: sw_fused_solve(orc, p, io, top_at_1, gpt))
    clear = _cached(("sw_clr", top_at_1, aer, with_g, gpt), lambda: sw_fused_solve(orc, p, clr, top_at_1, gpt))
    return allsky, clear, io, clr


def classes_sw(p, tau_op, ssa_op):
    """p with the operand-domain classes of one SW run, from the INCREMENTED operands at (edge layer, lit g-point):
    in_domain is tau <= 1e4 and (ssa == 0 or ssa >= 2^-99), the domain the shortened divisions state; out_of_domain is
    the rest."""
    tau_op, ssa_op = np.asarray(tau_op, F), np.asarray(ssa_op, F)
    return dict(p, in_domain=(tau_op <= F(1e4)) & ((ssa_op == 0) | (ssa_op >= F(2.0 ** -99))))


def classes_sw_of(p, io):
    return classes_sw(p, edge_values(p, io[0]), edge_values(p, io[1]))


def with_background_cloud(p):
    """Copies of the cloud band arrays with the background triple at every (edge layer, lit band)."""
    c, ib = np.arange(p["ncol"]), p["band_of"][p["lit"]]
    out = [p[k].copy() for k in ("tau_bnd", "ssa_bnd", "g_bnd")]
    for a, v in zip(out, (BG_TAU, BG_SSA, BG_G)):
        a[c, p["layer"], ib] = v
    return out


def tile(p, n):
    """The problem with its columns repeated n times (column c of tile k is column k * ncol + c)."""
    ncol = p["ncol"]
    q = {k: (np.concatenate([v] * n, axis=0) if isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == ncol
             and k not in ("lims", "band_of") else v) for k, v in p.items()}
    q["ncol"], q["cases"], q["tiles"] = n * ncol, list(p["cases"]) * n, n
    q["edge"] = {k: np.concatenate([v] * n) for k, v in p["edge"].items()}
    q["describe"] = _describe(q["cases"])
    return _freeze(q)
