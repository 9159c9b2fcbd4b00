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


def tau_at_thresh(D):
    """The largest float32 tau with tau*D <= sqrt(FLT_EPSILON) in float32, and the next float above it."""
    D = F(D)
    t = F(TAU_THRESH / D)
    while F(t * D) <= TAU_THRESH:
        t = np.nextafter(t, F(1))
    while F(t * D) > TAU_THRESH:
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
