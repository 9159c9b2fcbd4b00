"""Temperature and table edges of the Planck source (compute_Planck_source_nn and its interpolate1D,
rrtmgp/kernels/mo_gas_optics_kernels.F90:615-683 and :1024-1043), shared by tests/test_planck_edges_host.py (the oracle
pinned to a restatement, the census, a float64 reference) and tests/test_gpu_planck_edges.py (every copy of interp1d in
the kernels, bit for bit against the oracle).

Tables (tables()): kd-like dicts, what Oracle.planck_source takes.  "shipped" is the LW k-distribution (temp_ref_min 160,
totplnk_delta exactly 1, 196 temperatures, 16 x 16 g-points); "d07" (150.3, 0.7, 7 temperatures, 3 bands of 3 / 9 / 8
g-points, values not monotone, with an exact 0, a denormal and falling pairs); "two" (200, 50, the 2 temperatures the
entries require at least, 1 band of 5 g-points); "d3" (187.5, 3, 33 temperatures, 16 x 16, positive and increasing).
A delta other than 1 tells a division from a multiplication by the reciprocal; nothing on the shipped table can.

Temperatures (edge_temps): around every knot from three steps below the table to three above it -- the knot, its two
float32 neighbours, the quarter and the half step -- and 0, 1, 100 steps below and 1000 above.  With
val0 = (T - temp_ref_min) / totplnk_delta in float32, the reference clamps the INDEX to the table and takes the fraction
as val0 - int(val0), int() truncating toward zero: T = temp_ref_max returns the last but one value, the float below it
about the last, T < temp_ref_min - delta returns the first value on a knot and extrapolates with a negative fraction
between knots.  classes() counts these.

Problems: build(name), nlay 5, every temperature of the table's set in every role (tlay, tlev, tsfc) at least once,
Planck fractions cycling over 0, the denormal range, FLT_MIN and its neighbours, 1e-30, a seeded value and 1;
build_loop(name, nlay), 3 columns for the fused kernels' band-table loops (a second round of the loop and its clamp);
build_kernel(nlay, ngpt) for planck_source_kernel's layer blocks and g-point counts (kernel_shapes()).  Everything is seeded,
built once and read-only.
"""
import functools

import numpy as np

import solver_edges as E

F = np.float32
NLAY = 5
FLT_MIN = E.FLT_MIN
FLT_TRUE_MIN = F(1.4e-45)
TABLES = ("shipped", "d07", "two", "d3")
# the Planck fraction's cycle; None: a seeded value in (0, 1)
PFRACS = (F(0), FLT_TRUE_MIN, np.nextafter(FLT_MIN, F(0)), FLT_MIN, np.nextafter(FLT_MIN, F(1)), F(1e-30), None, F(1))
N_TEMPS = {"shipped": 1014, "d07": 69, "two": 44, "d3": 199}


def _table(tmin, delta, lims, totplnk):
    lims = np.asarray(lims, np.int32).reshape(-1, 2)
    totplnk = np.ascontiguousarray(totplnk, F)
    assert totplnk.shape[0] == len(lims)
    tmax = F(F(tmin) + F(totplnk.shape[1] - 1) * F(delta))
    return {"band_lims_gpt": lims, "totplnk": totplnk, "temp_ref_min": np.array([tmin], F),
            "temp_ref_max": np.array([tmax], F), "nband": len(lims), "ngpt": int(lims[-1, 1]),
            "nPlanckTemp": totplnk.shape[1], "totplnk_delta": F(delta)}


@functools.lru_cache(maxsize=None)
def tables():
    from rrtmgpnn import data
    rng = np.random.default_rng(20240611)
    d07 = rng.uniform(0.1, 5.0, (3, 7)).astype(F)
    d07[0, 2] = F(0)                                 # an exact zero
    d07[1, 3], d07[1, 4] = F(1e-40), F(0)            # a denormal above a zero: hi - lo = -1e-40, frac * that underflows
    d07[2, 5], d07[2, 6] = F(3.5), F(0.25)           # a falling last interval: the extrapolation above the table falls
    d07[0, 0], d07[0, 1] = F(2.0), F(0.5)            # and a falling first one
    two = rng.uniform(0.5, 3.0, (1, 2)).astype(F)
    d3 = np.cumsum(rng.uniform(0.01, 0.3, (16, 33)), axis=1).astype(F)
    t = {"shipped": dict(data.load_kdist("lw")),
         "d07": _table(150.3, 0.7, [(1, 3), (4, 12), (13, 20)], d07),
         "two": _table(200.0, 50.0, [(1, 5)], two),
         "d3": _table(187.5, 3.0, [(16 * b + 1, 16 * b + 16) for b in range(16)], d3)}
    for kd in t.values():
        for v in kd.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return t


def tmin_delta(kd):
    return F(kd["temp_ref_min"][0]), F(kd["totplnk_delta"])


def tmax(kd):
    """The last knot, in float32 as the knots of edge_temps are formed."""
    t0, d = tmin_delta(kd)
    return F(t0 + F(kd["nPlanckTemp"] - 1) * d)


def val0(kd, T):
    """(T - offset) / delta in float32: interpolate1D's first line."""
    t0, d = tmin_delta(kd)
    return ((np.asarray(T, F) - t0) / d).astype(F)


@functools.lru_cache(maxsize=None)
def edge_temps(name):
    """The sorted unique float32 temperatures of one table: for k in -3 .. ntemp + 2 the knot x = tmin + k delta, its two
    neighbours, x + delta / 2 and x + delta / 4; and 0, 1, tmin - 100 delta, tmin + 1000 delta.  Finite, |val0| < 2^31."""
    kd = tables()[name]
    t0, d = tmin_delta(kd)
    out = [F(0), F(1), F(t0 - F(100) * d), F(t0 + F(1000) * d)]
    for k in range(-3, kd["nPlanckTemp"] + 3):
        x = F(t0 + F(k) * d)
        out += [x, np.nextafter(x, F(-np.inf)), np.nextafter(x, F(np.inf)), F(x + F(0.5) * d), F(x + F(0.25) * d)]
    t = np.unique(np.array(out, F))
    t = t[np.isfinite(t) & (np.abs(val0(kd, t).astype(np.float64)) < 2.0 ** 31)]
    t.setflags(write=False)
    return t


def tsfc_extras(kd):
    """Surface temperatures whose + 1 K (the Jacobian's delta_Tsurf) crosses an edge of the table."""
    t0, hi = tmin_delta(kd)[0], tmax(kd)
    a = F(hi - F(1))
    return np.array([a, np.nextafter(a, F(-np.inf)), np.nextafter(a, F(np.inf)), F(hi - F(0.5)), F(t0 - F(1)),
                     F(t0 - F(1.5)), F(t0 - F(2))], F)


def classes(kd, T):
    """The census classes of temperatures T on a table: boolean arrays by name."""
    v = val0(kd, T)
    n = kd["nPlanckTemp"]
    integer = v == np.trunc(v)
    return {"below_minus_one": v <= -1, "between_minus_one_and_zero": (v > -1) & (v < 0),
            "on_a_knot_inside": integer & (v >= 0) & (v < n - 1),
            "above_with_fraction": (v >= n - 1) & ~integer, "above_on_an_integer": (v >= n - 1) & integer}


# the counts found when the builder was written (the issue's CPU run gave the same): asserted as lower bounds
CENSUS = {"below_minus_one": {"shipped": 15, "d07": 14, "two": 15, "d3": 15},
          "between_minus_one_and_zero": {"shipped": 4, "d07": 5, "two": 4, "d3": 4},
          "on_a_knot_inside": {"shipped": 195, "d07": 2, "two": 1, "d3": 32},
          "above_with_fraction": {"shipped": 15, "d07": 18, "two": 15, "d3": 15},
          "above_on_an_integer": {"shipped": 5, "d07": 1, "two": 5, "d3": 5}}


def _describe(p):
    def describe(cols, limit=4):
        cols = list(cols)
        s = "; ".join("col %d: tsfc %r tlay %s tlev %s" % (c, float(p["tsfc"][c]), p["tlay"][c].tolist(),
                                                           p["tlev"][c].tolist()) for c in cols[:limit])
        return "%d column(s) differ: %s%s" % (len(cols), s, " ..." if len(cols) > limit else "")
    return describe


def _band_of(lims, ngpt):
    out = np.zeros(ngpt, np.int64)
    for b, (lo, hi) in enumerate(lims):
        out[lo - 1:hi] = b
    return out


def _problem(kd, tlay, tlev, tsfc, seed):
    """The operands around the temperatures: pfrac over PFRACS by column, layer and g-point; tau seeded in [0.05, 2] and
    emissivities in [0.9, 1] (every layer's source reaches both boundary fluxes); an incident flux in [0, 0.05]; the
    cloud and aerosol band operands and the mask of solver_edges.build_lw_scat, on this table's bands."""
    rng = np.random.default_rng(seed)
    ncol, nlay = tlay.shape
    ngpt, nb = kd["ngpt"], kd["nband"]
    lims = np.asarray(kd["band_lims_gpt"], np.int32).reshape(-1, 2)
    u = lambda lo, hi, *s: rng.uniform(lo, hi, s).astype(F)  # noqa: E731
    ci, li, gi = np.meshgrid(np.arange(ncol), np.arange(nlay), np.arange(ngpt), indexing="ij")
    k = (gi + 3 * li + ci) % len(PFRACS)
    pfrac = u(0.001, 0.999, ncol, nlay, ngpt)
    for i, v in enumerate(PFRACS):
        if v is not None:
            pfrac[k == i] = v
    tau = u(0.05, 2.0, ncol, nlay, ngpt)
    ci, li, bi = np.meshgrid(np.arange(ncol), np.arange(nlay), np.arange(nb), indexing="ij")
    mask = ((np.arange(nlay)[None, :, None] + np.arange(ngpt)[None, None, :] + np.arange(ncol)[:, None, None]) % 2 == 0)
    p = {"ncol": ncol, "nlay": nlay, "ngpt": ngpt, "nb": nb, "kd": kd, "lims": lims, "band_of": _band_of(lims, ngpt),
         "tlay": np.ascontiguousarray(tlay, F), "tlev": np.ascontiguousarray(tlev, F),
         "tsfc": np.ascontiguousarray(tsfc, F), "pfrac": pfrac, "tau": tau, "tau_gas": tau,
         "emis": u(0.9, 1.0, ncol, ngpt), "emis_bnd": u(0.9, 1.0, ncol, nb), "inc": u(0.0, 0.05, ncol, ngpt),
         "tau_bnd": np.ascontiguousarray(E.INC_TAUS[(ci + li + bi) % 4], F),
         "ssa_bnd": np.ascontiguousarray(E.INC_SSAS[(ci // 4 + li + 2 * bi) % 4], F),
         "g_bnd": np.ascontiguousarray(E.INC_GS[(ci + li // 2 + bi) % 3], F),
         "tau_aer": np.ascontiguousarray(E.AER_TAUS[(ci + 2 * li + bi) % 3], F), "mask": mask}
    p["describe"] = _describe(p)
    return E._freeze(p)


@functools.lru_cache(maxsize=None)
def build(name):
    """The nlay-5 problem of one table: column c < n holds temperature c of edge_temps(name) as tsfc, temperatures
    5 c .. 5 c + 4 (mod n) as tlay and 6 c + 3 .. 6 c + 8 (mod n) as tlev, so each of the n values stands in each role;
    the columns behind them hold tsfc_extras() and go on dealing tlay and tlev."""
    kd = tables()[name]
    t = edge_temps(name)
    n = len(t)
    tsfc = np.concatenate([t, tsfc_extras(kd)])
    c = np.arange(len(tsfc))
    tlay = t[(5 * c[:, None] + np.arange(NLAY)[None, :]) % n]
    tlev = t[(6 * c[:, None] + 3 + np.arange(NLAY + 1)[None, :]) % n]
    return _problem(kd, tlay, tlev, tsfc, 1000 + n)


def _seeded_temps(kd, rng, *shape):
    """In-range temperatures: uniform over the table."""
    return rng.uniform(float(kd["temp_ref_min"][0]), float(tmax(kd)), shape).astype(F)


def _outside(kd):
    """(tsfc, first tlay, last tlev) of three columns, all outside the table on one side or the other."""
    t0, d = tmin_delta(kd)
    hi = tmax(kd)
    return (np.array([hi + F(0.375) * d, t0 - F(1.625) * d, hi], F),
            np.array([t0 - F(0.5) * d, hi + F(2.25) * d, t0 - F(3) * d], F),
            np.array([hi + F(0.5) * d, t0 - F(1.25) * d, hi + F(7) * d], F))


# (table, nlay) of the fused kernels' band-table loops.  A block of T threads forms 8 T entries per round out of
# ntab = nbnd (2 nlay + 2) (nbnd more with the Jacobian row).  256 g-points: 2048 per round, ntab 64, 96, 2048, 2080,
# 4096 and 4128 -- one round partly filled, exactly one, a second begun, exactly two, a third begun.  20 and 5 g-points
# run 64 threads, 512 entries per round: nlay 100 on three bands is 606 entries and nlay 300 on one band 602, a second
# round either way.
LOOP_SHAPES = [("d3", 1), ("d3", 2), ("d3", 63), ("d3", 64), ("d3", 127), ("d3", 128), ("shipped", 64), ("two", 300),
               ("d07", 100)]


def loop_id(s):
    return "%s-nlay%d" % s


@functools.lru_cache(maxsize=None)
def build_loop(name, nlay):
    kd = tables()[name]
    rng = np.random.default_rng(7 * nlay + len(name))
    tlay, tlev, tsfc = _seeded_temps(kd, rng, 3, nlay), _seeded_temps(kd, rng, 3, nlay + 1), _seeded_temps(kd, rng, 3)
    tsfc[:], tlay[:, 0], tlev[:, -1] = _outside(kd)
    return _problem(kd, tlay, tlev, tsfc, 2000 + nlay)


def ntab(p, jac=False):
    """Entries of the fused kernels' band table for the problem p."""
    return p["nb"] * (2 * p["nlay"] + 2 + (1 if jac else 0))


# planck_source_kernel: 4 layers per block (below, at and above one and two blocks), sfc_lay in the first / last / a
# middle block position, and g-point counts around the wave and at the block's limit
KERNEL_NLAYS = (1, 3, 4, 5, 8, 9)
KERNEL_NGPTS = (1, 63, 64, 65, 256, 1000, 1024)


def kernel_shapes():
    out = []
    for nlay in KERNEL_NLAYS:
        for sfc_lay in sorted({1, nlay, nlay // 2 + 1}):
            out.append((nlay, 65, sfc_lay))
    out += [(5, ngpt, s) for ngpt in KERNEL_NGPTS if ngpt != 65 for s in (1, 5)]
    return out


@functools.lru_cache(maxsize=None)
def build_kernel(nlay, ngpt):
    """3 columns on the d3 table's values with min(16, ngpt) bands of uneven widths over ngpt g-points; seeded in-range
    temperatures with _outside()'s values as tsfc, the first tlay and the last tlev."""
    d3 = tables()["d3"]
    nb = min(16, ngpt)
    cuts = np.linspace(0, ngpt, nb + 1).round().astype(int)
    cuts[1:-1] += (np.arange(1, nb) % 2) * (1 if ngpt >= 3 * nb else 0)  # uneven widths where there is room
    lims = [(cuts[b] + 1, cuts[b + 1]) for b in range(nb)]
    kd = _table(float(d3["temp_ref_min"][0]), float(d3["totplnk_delta"]), lims, d3["totplnk"][:nb])
    assert kd["ngpt"] == ngpt and all(lo <= hi for lo, hi in lims)
    rng = np.random.default_rng(31 * nlay + ngpt)
    tlay, tlev, tsfc = _seeded_temps(kd, rng, 3, nlay), _seeded_temps(kd, rng, 3, nlay + 1), _seeded_temps(kd, rng, 3)
    tsfc[:], tlay[:, 0], tlev[:, -1] = _outside(kd)
    return _problem(kd, tlay, tlev, tsfc, 3000 + 31 * nlay + ngpt)


# ---- references: the oracle's compositions, each computed once and shared ----------------------------------------------
_refs = {}


def _cached(key, make):
    if key not in _refs:
        _refs[key] = make()
    return _refs[key]


def sources(orc, p, sfc_lay):
    """(lay_source, lev_source, sfc_source, sfc_source_Jac) of the oracle."""
    return _cached(("src", id(p), sfc_lay), lambda: orc.planck_source(p["kd"], p["tlay"], p["tlev"], p["tsfc"], p["pfrac"],
                                                                    sfc_lay))


def sfc_lay_of(p, top_at_1):
    return p["nlay"] if top_at_1 else 1


def ref_noscat(orc, p, top_at_1, nmus, kind="clear", emis_by_band=False, gpt=False, jac=False):
    """The no-scattering entries on the oracle's sources.  kind "clear": tau; "inc": tau + tau_bnd(band); "masked": where
    the mask bit is set (mcica_ref.draw at identity limits, as solver_edges.ref_noscat_fused).  -> (up, dn(, gpt_up,
    gpt_dn)(, flux_up_Jac))"""
    import lw_jacobian_ref as J
    import mcica_ref as M

    def make():
        lay, lev, sfc, sjac = sources(orc, p, sfc_lay_of(p, top_at_1))
        if kind == "inc":
            tau = orc.increment_bybnd(p["lims"], [p["tau"]], [p["tau_bnd"]])[0]
        elif kind == "masked":
            tau = orc.increment_bybnd(E._ident(p["ngpt"]), [p["tau"]], [M.draw(p["mask"], p["tau_bnd"], p["lims"])])[0]
        else:
            tau = p["tau"]
        emis = E._expand(p["emis_bnd"], p["lims"], p["ngpt"]) if emis_by_band else p["emis"]
        out = orc.lw_solver(tau, lay, lev, emis, sfc, top_at_1, nmus, inc_flux=p["inc"], gpt=gpt)
        if jac:
            out = out + (J.zero_source_flux_up(orc, tau, emis, sjac, top_at_1, nmus),)
        return out
    return _cached(("noscat", id(p), top_at_1, nmus, kind, emis_by_band, gpt, jac), make)


def ref_rescl(orc, p, top_at_1, nmus, masked=False, aer=False):
    """The rescaled fused entries: (up, dn, up_clr, dn_clr) of solver_edges.fused_props' properties on the oracle's
    sources, as solver_edges.ref_fused."""
    def make():
        io = E.fused_props(orc, p, masked, aer)
        lay, lev, sfc, _ = sources(orc, p, sfc_lay_of(p, top_at_1))
        up, dn = orc.lw_solver(io[0], lay, lev, p["emis"], sfc, top_at_1, nmus, inc_flux=p["inc"], ssa=io[1], g=io[2])
        tc = orc.increment_bybnd(p["lims"], [p["tau_gas"]], [p["tau_aer"]])[0] if aer else p["tau_gas"]
        cu, cd = orc.lw_solver(tc, lay, lev, p["emis"], sfc, top_at_1, nmus, inc_flux=p["inc"])
        return up, dn, cu, cd
    return _cached(("rescl", id(p), top_at_1, nmus, masked, aer), make)


def assert_bits(got, want, p, what):
    """Equal as uint32 views (so -0 differs from +0 and a nan from another nan), naming the columns that differ."""
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    assert got.shape == want.shape, "%s: shape %s against %s" % (what, got.shape, want.shape)
    bad = got.view(np.uint32) != want.view(np.uint32)
    if bad.any():
        cols = np.unique(np.nonzero(bad.reshape(bad.shape[0], -1))[0])
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError("%s: %d value(s) differ, first at %s: got %r, want %r; %s" % (
            what, int(bad.sum()), i, float(got[i]), float(want[i]), p["describe"](cols)))


# ---- the restatement and the float64 reference ---------------------------------------------------------------------------
def interpolate1d_f32(val, offset, delta, table):
    """interpolate1D (mo_gas_optics_kernels.F90:1024-1043) in float32 numpy, one Fortran operation per numpy operation;
    val any shape, table (nbnd, ntemp) -> val.shape + (nbnd,)."""
    val, offset, delta = np.asarray(val, F), F(offset), F(delta)
    table = np.asarray(table, F)
    ntemp = table.shape[1]
    val0 = (val - offset) / delta                                   # :1039
    iv = np.trunc(val0).astype(np.int64)                            # int(val0)
    frac = val0 - iv.astype(F)                                      # :1040
    index = np.minimum(ntemp - 1, np.maximum(1, iv + 1))            # :1041, 1-based
    lo = np.moveaxis(table[:, index - 1], 0, -1)                    # table(index, :)
    hi = np.moveaxis(table[:, index], 0, -1)                        # table(index + 1, :)
    d = hi - lo
    prod = frac[..., None] * d
    return lo + prod                                                # :1042


def planck_source_f32(kd, tlay, tlev, tsfc, pfrac, sfc_lay):
    """compute_Planck_source_nn (mo_gas_optics_kernels.F90:615-683) in float32 numpy, line by line -> (lay_source,
    lev_source, sfc_source, sfc_source_Jac) in the oracle's layout ((ncol, nlay, ngpt) ...)."""
    t0, delta = tmin_delta(kd)
    tab = kd["totplnk"]
    tlay, tlev, tsfc, pfrac = (np.asarray(a, F) for a in (tlay, tlev, tsfc, pfrac))
    ncol, nlay, ngpt = pfrac.shape
    b = _band_of(np.asarray(kd["band_lims_gpt"]).reshape(-1, 2), ngpt)
    pl_sfc = interpolate1d_f32(tsfc, t0, delta, tab)                # :648
    pl_jac = interpolate1d_f32(tsfc + F(1.0), t0, delta, tab)       # :649, delta_Tsurf = 1
    pl_lev = interpolate1d_f32(tlev, t0, delta, tab)                # :650, :667
    pl_lay = interpolate1d_f32(tlay, t0, delta, tab)                # :668
    lev = np.empty((ncol, nlay + 1, ngpt), F)
    lev[:, nlay] = pfrac[:, nlay - 1] * pl_lev[:, nlay][:, b]       # :657
    sfc = pfrac[:, sfc_lay - 1] * pl_sfc[:, b]                      # :660
    jac = pfrac[:, sfc_lay - 1] * (pl_jac[:, b] - pl_sfc[:, b])     # :661-662
    lev[:, :nlay] = pfrac * pl_lev[:, :nlay][:, :, b]               # :675
    lay = pfrac * pl_lay[:, :, b]                                   # :676
    return lay, lev, sfc, jac


U = 2.0 ** -24      # float32 unit roundoff
ETA = 2.0 ** -150   # half the smallest denormal: the absolute error of a product that underflows


def planck_f64(kd, T, pf):
    """pf * interpolate1D(T) per band in float64 on the float32 inputs T, pf (same shape) -> (value, bound, excused),
    each T.shape + (nbnd,) (excused: T.shape).

    value: the piecewise expression in float64 with float64's own val0, truncation and index.
    bound: a forward-error bound of the float32 evaluation against it, from the operations alone.  Write u = 2^-24 and
    eta = 2^-150.  (1) val0: one subtraction and one division, so val0_32 = val0 (1 + e), |e| <= 2 u + u^2 =: g2, i.e.
    |val0_32 - val0| <= dv := g2 |val0|.  (2) val0_32 - int(val0_32) is exact in float32 (the fractional part of a float
    below 2^24 is a float; beyond 2^24 it is 0), so float32 evaluates f(v) = lo(v) + frac(v) (hi(v) - lo(v)) AT v = val0_32
    with three rounded operations: d = (hi - lo)(1 + e3); p = frac d (1 + e4) + eta (the product may underflow; sums and
    differences of floats do not lose bits there); r = (lo + p)(1 + e5).  Against the exact f(val0_32) =: F32 this is at
    most  e_r = |frac| |D| (2 u + u^2) + eta + u (|lo| + |frac| |D| (1 + u)^2 + eta)  with D = hi - lo exact.
    (3) |F32 - f(val0)| <= dv max|D| over the intervals val0_32 and val0 fall in: f is piecewise linear with slopes D and,
    inside the table, continuous, so this holds there even when the two truncations differ; outside the table it holds
    when they agree (same interval, same clamped index) -- where they differ there, f jumps and the case is `excused`.
    (4) the product by pfrac: out = pf r (1 + e6) + eta.  Together
        bound = pf (e_r + dv max|D|) (1 + u) + u pf |f(val0)| + eta.
    """
    T, pf = np.asarray(T, F), np.asarray(pf, F)
    t0, delta = (float(x) for x in tmin_delta(kd))
    tab = np.asarray(kd["totplnk"], np.float64)
    ntemp = tab.shape[1]

    def pieces(v):
        iv = np.trunc(v).astype(np.int64)
        frac = v - iv
        index = np.minimum(ntemp - 1, np.maximum(1, iv + 1))
        return iv, frac, np.moveaxis(tab[:, index - 1], 0, -1), np.moveaxis(tab[:, index], 0, -1)

    v64 = (T.astype(np.float64) - t0) / delta
    v32 = val0(kd, T).astype(np.float64)
    iv64, fr64, lo64, hi64 = pieces(v64)
    iv32, fr32, lo32, hi32 = pieces(v32)
    value = pf.astype(np.float64)[..., None] * (lo64 + fr64[..., None] * (hi64 - lo64))
    inside = (np.minimum(v32, v64) >= 0) & (np.maximum(v32, v64) <= ntemp - 1)
    excused = (iv32 != iv64) & ~inside
    g2 = 2 * U + U * U
    dv = (g2 * np.abs(v64))[..., None]
    D32 = np.abs(hi32 - lo32)
    Dmax = np.maximum(D32, np.abs(hi64 - lo64))
    fD = np.abs(fr32)[..., None] * D32
    e_r = fD * g2 + ETA + U * (np.abs(lo32) + fD * (1 + U) ** 2 + ETA)
    pfa = np.abs(pf.astype(np.float64))[..., None]
    bound = pfa * (e_r + dv * Dmax) * (1 + U) + U * np.abs(value) + ETA
    return value, bound, excused
