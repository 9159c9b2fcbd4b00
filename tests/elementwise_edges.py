"""Operand-edge inputs for the elementwise kernels and the gas-optics glue, shared by tests/test_elementwise_edges_host.py
(the pin to the reference, the conditions and the float64 check of the glue, on the CPU) and
tests/test_gpu_elementwise_edges.py (the kernels, bit for bit against the oracle).

One builder per family; each returns a dict of numpy arrays in the oracle's layout ((ncol, nlay, ngpt) ...), `cases`
(one named tuple of operand values per element, row or column) and `describe`, which names the cases of a list of
indices for a failure message.  The problems are built once and their arrays are read-only.  Nothing here is random.

  build_delta_scale()      delta_scale_2str, f = g**2 and an explicit forward fraction (g**2 and max(g, 0))
  build_increment(layout)  increment by band and at the same resolution, every 1scl/2str pairing, six band layouts
  build_cloud_optics(co)   ty_cloud_optics%cloud_optics on every LUT knot and Pade size-regime bound
  build_heating()          both heating-rate forms, one-layer columns
  build_expand(layout)     expand band -> g-point
  build_glue(model, v)     compute_nn_inputs / get_col_dry and the fused entries, one-layer columns
  build_tlev(nlay)         interpolate_tlev
"""
import collections
import functools

import numpy as np

F = np.float32
FLT_MIN = F(1.17549435e-38)
FLT_EPS = F(np.finfo(np.float32).eps)
EPS3 = F(3) * FLT_MIN            # 3*tiny(1.0_wp): the max(eps, .) of increment and delta_scale
ONE_M = F(1 - 2.0 ** -24)        # the float below 1
U = 2.0 ** -24                   # unit roundoff of float32


def gamma(n):
    """Higham's gamma_n = n u / (1 - n u): the relative error of n float32 roundings."""
    return n * U / (1 - n * U)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def is_denormal(a):
    a = np.abs(np.asarray(a, F))
    return (a > 0) & (a < FLT_MIN)


def next_up(x):
    return np.nextafter(F(x), F(np.inf))


def next_down(x):
    return np.nextafter(F(x), F(-np.inf))


def _describe(cases, what):
    def describe(idx, limit=6):
        idx = [int(i) for i in idx]
        s = "; ".join(str(cases[i]) for i in idx[:limit])
        return "%d %s(s) differ: %s%s" % (len(idx), what, s, " ..." if len(idx) > limit else "")
    return describe


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
        elif isinstance(v, (tuple, list)):
            for a in v:
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
    return d


def mismatch(got, want):
    """Indices along axis 0 at which the bit patterns differ anywhere."""
    bad = bits(got) != bits(want)
    return np.unique(np.nonzero(bad.reshape(bad.shape[0], -1))[0])


def assert_bits(got, want, what, describe=None):
    """Equality of bit patterns (inf and nan compare as their bits; -0 is not +0), naming the cases that differ."""
    got, want = np.asarray(got, F), np.asarray(want, F)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if got.size == 0:
        return
    bad = mismatch(got, want)
    if bad.size:
        msg = "%s: %s" % (what, describe(bad) if describe else "%d index(es) of axis 0 differ, first %d" % (bad.size, bad[0]))
        np.testing.assert_array_equal(bits(got), bits(want), err_msg=msg)


# ---- delta scaling ------------------------------------------------------------------------------------------------------
DS_TAUS = np.array([0, 1e-45, 1e-38, FLT_MIN, 1e-30, 1e-3, 1, 50, 1e30, 3e38], F)
DS_SSAS = np.array([0, 1e-45, 1e-38, 1e-20, 0.5, ONE_M, 1], F)
DS_GS = np.array([0, 1e-23, 1e-19, 0.3, 0.85, ONE_M, 1, -0.5, -1], F)
DS_FORMS = (None, "g2", "gpos")  # f = g**2 in the kernel; fwd = g**2; fwd = max(g, 0)
DS_SHAPE = (5, 9, 14)            # the 630 cases as (ncol, nlay, nband) for the reference's class layer (SW bands)

DsCase = collections.namedtuple("DsCase", "i tau ssa g")


@functools.lru_cache(maxsize=None)
def build_delta_scale():
    cases = [DsCase(i, t, w, g) for i, (t, w, g) in
             enumerate((t, w, g) for t in DS_TAUS for w in DS_SSAS for g in DS_GS)]
    tau, ssa, g = (np.array([getattr(c, k) for c in cases], F) for k in ("tau", "ssa", "g"))
    assert tau.size == 630 == int(np.prod(DS_SHAPE))
    return _freeze({"n": tau.size, "tau": tau, "ssa": ssa, "g": g, "cases": cases, "describe": _describe(cases, "element"),
                    "fwd": {None: None, "g2": (g * g).astype(F), "gpos": np.maximum(g, F(0))}})


# ---- increment -------------------------------------------------------------------------------------------------------------
INC_IO_TAUS = np.array([0, 1e-45, 1e-38, 1e-30, 1e-2, 20, 1e30], F)
INC_IO_SSAS = np.array([0, 1e-45, 1e-20, 0.5, 1], F)
INC_IO_GS = np.array([0, 0.85, 1], F)
INC_IN_TAUS = np.array([0, 1e-45, 2e-38, 1e-30, 0.1, 5, 3e38], F)
INC_IN_SSAS = np.array([0, 1e-10, 0.9, 1], F)
INC_IN_GS = np.array([0, 0.85], F)
INC_IO = [(t, w, g) for t in INC_IO_TAUS for w in INC_IO_SSAS for g in INC_IO_GS]   # 105
INC_IN = [(t, w, g) for t in INC_IN_TAUS for w in INC_IN_SSAS for g in INC_IN_GS]   # 56
INC_LAYOUTS = ("sw", "lw", "one", "same", "odd", "gap")
PAIRINGS = [(1, 1), (1, 2), (2, 1), (2, 2)]  # (nstr of the incremented set, nstr of the increment)

IncCase = collections.namedtuple("IncCase", "row io_of_gpt0 inc_of_band0")


def band_layout(name):
    """(ngpt, lims (nbnd, 2) int32 1-based inclusive) of a layout: the shipped SW (224 / 14) and LW (256 / 16) bands, one
    band over everything, one g-point per band (the same-resolution entry), odd band starts, a gap (band 3 shortened at
    both ends: five g-points in no band)."""
    from rrtmgpnn import data
    if name == "lw":
        kd = data.load_kdist("lw")
        return int(kd["ngpt"]), np.ascontiguousarray(np.asarray(kd["band_lims_gpt"]).reshape(-1, 2), np.int32)
    kd = data.load_kdist("sw")
    ngpt = int(kd["ngpt"])
    lims = np.ascontiguousarray(np.asarray(kd["band_lims_gpt"]).reshape(-1, 2), np.int32).copy()
    if name == "one":
        lims = np.array([[1, ngpt]], np.int32)
    elif name == "same":
        lims = np.stack([np.arange(1, ngpt + 1)] * 2, axis=1).astype(np.int32)
    elif name == "odd":
        lims[0, 1] -= 1
        lims[1, 0] -= 1
        assert (lims[1, 0] - 1) % 2 == 1
    elif name == "gap":
        lims[3, 0] += 2
        lims[3, 1] -= 3
    else:
        assert name == "sw", name
    return ngpt, lims


def in_a_band(ngpt, lims):
    m = np.zeros(ngpt, bool)
    for lo, hi in lims:
        m[lo - 1:hi] = True
    return m


@functools.lru_cache(maxsize=None)
def build_increment(layout):
    """io (tau, ssa, g) (2, 56, ngpt) and inc (tau, ssa, g) (2, 56, nbnd).  The io case walks the g-point index (case
    (g + 37 col) % 105: every layout has more than 105 g-points, so every io case stands in every row) and the
    increment case walks the layer (case (lay + col * band) % 56: column 0 holds increment case `lay` in every band),
    so column 0 alone holds every io triple beside every increment triple."""
    ngpt, lims = band_layout(layout)
    nb, ncol, nlay = len(lims), 2, len(INC_IN)
    assert ngpt >= 2 * len(INC_IO)
    c, l, g = np.meshgrid(np.arange(ncol), np.arange(nlay), np.arange(ngpt), indexing="ij")
    io_case = (g + 37 * c) % len(INC_IO)
    c, l, b = np.meshgrid(np.arange(ncol), np.arange(nlay), np.arange(nb), indexing="ij")
    in_case = (l + c * b) % len(INC_IN)
    io_tab, in_tab = np.array(INC_IO, F), np.array(INC_IN, F)
    io = tuple(np.ascontiguousarray(io_tab[io_case, k]) for k in range(3))
    inc = tuple(np.ascontiguousarray(in_tab[in_case, k]) for k in range(3))
    cases = [IncCase(r, INC_IO[io_case.reshape(-1, ngpt)[r, 0]], INC_IN[in_case.reshape(-1, nb)[r, 0]])
             for r in range(ncol * nlay)]
    return _freeze({"layout": layout, "ncol": ncol, "nlay": nlay, "ngpt": ngpt, "nb": nb, "lims": lims, "io": io,
                    "inc": inc, "io_case": io_case, "in_case": in_case, "covered": in_a_band(ngpt, lims),
                    "cases": cases, "describe": _describe(cases, "row")})


def increment_ref(orc, p, nstr_io, nstr_in):
    """The oracle's increment of the problem's io set (its first nstr_io arrays) by its inc set."""
    return orc.increment_bybnd(p["lims"], p["io"][:1 if nstr_io == 1 else 3], p["inc"][:1 if nstr_in == 1 else 3])


# ---- cloud optics ---------------------------------------------------------------------------------------------------------
CO_PATHS = np.array([1e-45, 1e-38, FLT_MIN, 1e-30, 1e-6, 1, 200, 1e6, 1e30, 3e38], F)
CO_SHAPE = (60, 31)

CoCase = collections.namedtuple("CoCase", "s lwp iwp reliq reice")


def lut_knots(lwr, upr, nsize):
    """The LUT's knots lwr + i * step in float32, step as load_lut forms it."""
    lwr, upr = F(lwr), F(upr)
    step = F(upr - lwr) / F(nsize - 1)
    return np.array([lwr + F(i) * step for i in range(nsize)], F), step


def edge_radii(co, phase):
    """Every LUT knot and every Pade size-regime bound of the phase's three arrays, each with its two float neighbours,
    kept where it lies inside [lwr, upr]: sorted, unique."""
    p = {"liq": ("radliq", "lut_extliq", -1), "ice": ("radice", "lut_extice", -1)}[phase]
    lwr, upr = F(co[p[0] + "_lwr"][0]), F(co[p[0] + "_upr"][0])
    knots, _ = lut_knots(lwr, upr, co[p[1]].shape[p[2]])
    vals = list(knots)
    for k in ("ext", "ssa", "asy"):
        vals += list(np.asarray(co["pade_sizreg_" + k + phase], F).ravel())
    out = []
    for v in vals:
        out += [next_down(v), F(v), next_up(v)]
    out = np.unique(np.array(out, F))
    return out[(out >= lwr) & (out <= upr)]


_CO = {}


def build_cloud_optics(co, which):
    """clwp, ciwp, reliq, reice (60, 31): every (liquid radius, water path) with no ice, every (ice radius, water path)
    with no liquid, then every liquid case beside an ice case (ice case (3 k + 1) % n_ice: all of them occur).  A phase
    that is absent carries a radius inside its table all the same (the reference reads it only under a positive path)."""
    if which in _CO:
        return _CO[which]
    rl, ri = edge_radii(co, "liq"), edge_radii(co, "ice")
    liq = [(r, w) for r in rl for w in CO_PATHS]
    ice = [(r, w) for r in ri for w in CO_PATHS]
    rows = [(w, F(0), r, ri[0]) for r, w in liq] + [(F(0), w, rl[0], r) for r, w in ice]
    rows += [(w, ice[(3 * k + 1) % len(ice)][1], r, ice[(3 * k + 1) % len(ice)][0]) for k, (r, w) in enumerate(liq)]
    n = CO_SHAPE[0] * CO_SHAPE[1]
    assert len(rows) <= n, (len(rows), n)
    rows += [rows[(7 * k) % len(rows)] for k in range(n - len(rows))]
    a = np.array(rows, F)
    cases = [CoCase(s, *rows[s]) for s in range(n)]
    _CO[which] = _freeze({"which": which, "ncol": CO_SHAPE[0], "nlay": CO_SHAPE[1], "rl": rl, "ri": ri,
                          "args": tuple(np.ascontiguousarray(a[:, k].reshape(CO_SHAPE)) for k in range(4)),
                          "cases": cases, "describe": _describe(cases, "(col, lay) sample")})
    return _CO[which]


def co_rows(a):
    """A cloud-optics output (ncol, nlay, nband) as (sample, nband), for assert_bits to name the samples."""
    return np.asarray(a).reshape(-1, a.shape[-1])


def table_index(re, lwr, step, nsteps):
    """(index, fint) of compute_all_from_table in float32, operation by operation."""
    q = (np.asarray(re, F) - F(lwr)) / F(step)
    index = np.minimum(np.floor(q).astype(np.int64) + 1, nsteps - 1)
    return index, (q - (index - 1).astype(F)).astype(F)


def pade_irad(re, bounds):
    re, bounds = np.asarray(re, F), np.asarray(bounds, F)
    return np.minimum(np.floor((re - bounds[1]) / bounds[2]).astype(np.int64) + 2, 3)


def pade_eval(coef, irad, re, m, n):
    """pade_eval_1 in float32, operation by operation; coef (ncoef, nsizereg, nband) -> (len(re), nband)."""
    re = np.asarray(re, F)[:, None]
    c = lambda i: np.asarray(coef, F)[i][irad - 1]  # noqa: E731  (len(re), nband)
    denom = c(n + m)
    for i in range(n - 1 + m, m, -1):
        denom = c(i) + re * denom
    denom = F(1) + re * denom
    numer = c(m)
    for i in range(m - 1, 0, -1):
        numer = c(i) + re * numer
    numer = c(0) + re * numer
    with np.errstate(all="ignore"):
        return (numer / denom).astype(F)


# ---- heating rates --------------------------------------------------------------------------------------------------------
HR_FLUXES = np.array([0, 1e-45, 1e-38, 1, 300, 1361, 1e30], F)
# (level 0, level 1): top first, bottom first (dp < 0), one ulp apart in both orders; never equal (dp = 0 -> inf / inf)
HR_PLEVS = [(F(1e4), F(2e4)), (F(101325), F(9.5e4)), (F(5e4), next_up(5e4)), (next_up(5e4), F(5e4)),
            (F(1), F(1e-3))]

HrCase = collections.namedtuple("HrCase", "col up0 up1 dn0 dn1 p0 p1")


@functools.lru_cache(maxsize=None)
def build_heating():
    """One-layer columns: every (up0, up1, dn0, dn1) of HR_FLUXES (2401: the difference cancels exactly where the two
    levels agree, and is denormal where they differ by a denormal) under every pressure pair."""
    n = len(HR_FLUXES)
    cases = []
    for ip, (p0, p1) in enumerate(HR_PLEVS):
        for k in range(n ** 4):
            a, b, c, d = k % n, (k // n) % n, (k // n ** 2) % n, k // n ** 3
            cases.append(HrCase(len(cases), HR_FLUXES[a], HR_FLUXES[b], HR_FLUXES[c], HR_FLUXES[d], p0, p1))
    col = lambda *ks: np.ascontiguousarray(np.array([[getattr(c, k) for k in ks] for c in cases], F))  # noqa: E731
    return _freeze({"ncol": len(cases), "nlay": 1, "up": col("up0", "up1"), "dn": col("dn0", "dn1"),
                    "plev": col("p0", "p1"), "cases": cases, "describe": _describe(cases, "column")})


# ---- expand ---------------------------------------------------------------------------------------------------------------
EXPAND_VALUES = np.array([0, -0.0, 1e-45, -1e-45, 1e-38, FLT_MIN, 0.5, 1, -1, 3e38, np.inf, -np.inf], F)
SENTINEL = F(-777.0)


@functools.lru_cache(maxsize=None)
def build_expand(layout):
    ngpt, lims = band_layout(layout)
    nb, ncol = len(lims), 37
    c, b = np.meshgrid(np.arange(ncol), np.arange(nb), indexing="ij")
    arr = np.ascontiguousarray(EXPAND_VALUES[(c + 5 * b) % len(EXPAND_VALUES)])
    cases = ["column %d" % i for i in range(ncol)]
    return _freeze({"ncol": ncol, "ngpt": ngpt, "nb": nb, "lims": lims, "arr": arr, "covered": in_a_band(ngpt, lims),
                    "cases": cases, "describe": _describe(cases, "column")})


def expand_ref(orc, p):
    """orc_expand into a sentinel-filled array: a g-point in no band keeps the sentinel."""
    out = np.full((p["ncol"], p["ngpt"]), SENTINEL, F)
    orc.L.orc_expand(p["nb"], p["ngpt"], p["ncol"], np.ascontiguousarray(p["lims"], np.int32), p["arr"], out)
    return out


# ---- the gas-optics glue and the networks' front end ----------------------------------------------------------------------
GL_PLAYS = np.array([1e-45, FLT_MIN, 1e-3, 1, 1005, 101325, 1e7], F)
GL_TLAYS = np.array([0, 160, 250, 340, 1e4], F)
GL_VMRS = np.array([0, 1e-45, 1e-38, FLT_MIN, 1e-12, 4e-6, 0.04, 1], F)
# (level 0, level 1) of the one layer: zero thickness, top first, bottom first, one ulp apart, (1e-45, 0)
GL_PLEVS = [(F(5e4), F(5e4)), (F(1e4), F(2e4)), (F(101325), F(9.5e4)), (F(5e4), next_up(5e4)), (F(1e-45), F(0))]
GL_DENORMAL = F(1e-40)
GL_FORMS = ("scalar", "1d", "2d", "absent")  # gas_ndims 0, 1, 2 and a NULL pointer
GL_VARIANTS = (0, 1, 2, 3)

GlCase = collections.namedtuple("GlCase", "col play tlay h2o o3 p0 p1")

_GL = {}


def build_glue(model, key, variant=0):
    """One-layer columns (nlay = 1: a column's level pair is its own): every (play, tlay, h2o, o3), the level pair
    cycling with (play index + tlay index) so that every h2o meets every pair.  The gases behind o3: gas i has the form
    GL_FORMS[(i + variant) % 4]; a 2-D gas cycles by column over (0, a denormal, a typical value: the middle of the
    network's input range), a scalar or 1-D one holds the value (i // 4 + variant) % 3 of those.  key: the model's name
    (the cache's)."""
    if (key, variant) in _GL:
        return _GL[(key, variant)]
    from rrtmgpnn import rbin
    names = rbin.unchars(model["input_names"])
    mn, mx = np.asarray(model["input_min"], F), np.asarray(model["input_max"], F)
    n_p, n_t, n_v = len(GL_PLAYS), len(GL_TLAYS), len(GL_VMRS)
    ncol = n_p * n_t * n_v * n_v
    c = np.arange(ncol)
    i_p, i_t, i_h, i_o = c % n_p, (c // n_p) % n_t, (c // (n_p * n_t)) % n_v, c // (n_p * n_t * n_v)
    pair = np.array(GL_PLEVS, F)[(i_p + i_t) % len(GL_PLEVS)]
    play, tlay = GL_PLAYS[i_p][:, None], GL_TLAYS[i_t][:, None]
    gases = {names[2]: GL_VMRS[i_h][:, None], names[3]: GL_VMRS[i_o][:, None]}
    forms = {names[2]: "2d", names[3]: "2d"}
    for i, n in enumerate(names[4:]):
        k = 4 + i
        vals = np.array([0, GL_DENORMAL, F(0.5) * (mn[k] + mx[k])], F)
        form = GL_FORMS[(i + variant) % 4]
        forms[n] = form
        if form == "2d":
            gases[n] = vals[(c + i) % 3][:, None]
        elif form == "1d":
            gases[n] = vals[(i // 4 + variant) % 3].reshape(1)
        elif form == "scalar":
            gases[n] = F(vals[(i // 4 + variant) % 3])
    gases = {k: (np.ascontiguousarray(v) if np.ndim(v) else v) for k, v in gases.items()}
    cases = [GlCase(int(k), play[k, 0], tlay[k, 0], gases[names[2]][k, 0], gases[names[3]][k, 0], pair[k, 0], pair[k, 1])
             for k in c]
    _GL[(key, variant)] = _freeze({
        "ncol": ncol, "nlay": 1, "names": names, "forms": forms, "gases": gases, "play": np.ascontiguousarray(play),
        "tlay": np.ascontiguousarray(tlay), "plev": np.ascontiguousarray(pair), "cases": cases,
        "describe": _describe(cases, "column")})
    return _GL[(key, variant)]


def glue_rows(a, p):
    """An output (ncol, 1, n) or (ncol * 1, n) of a glue problem as (column, n)."""
    return np.asarray(a).reshape(p["ncol"], -1)


TL_RATIOS = np.array([1 + 2.0 ** -23, 1 + 2.0 ** -20, 1.001, 1.5, 10, 1e3, 1e6], F)
TlCase = collections.namedtuple("TlCase", "col ratio at top_first tlay")


@functools.lru_cache(maxsize=None)
def build_tlev(nlay):
    """interpolate_tlev (nlay >= 2): one pair of neighbouring layers per column has the pressure ratio TL_RATIOS[.], the
    others 1.3; the level between two layers lies at play * sqrt(ratio) in float32 (on one of the two layers where they
    are neighbouring floats).  Both orientations; the layer temperatures cycle over GL_TLAYS.  Pressures from 100 Pa up:
    no product in the expressions leaves the normal range, and no two layer pressures are equal."""
    cases = []
    play, plev, tlay = [], [], []
    for ir, r in enumerate(TL_RATIOS):
        for at in range(nlay - 1):
            for shift in range(len(GL_TLAYS)):
                for top_first in (True, False):
                    pa, pv = [F(100)], [F(100) / F(1.1)]
                    for l in range(nlay - 1):
                        q = r if l == at else F(1.3)
                        pv.append(F(pa[-1] * np.sqrt(q)))
                        pa.append(F(pa[-1] * q))
                    pv.append(F(pa[-1] * F(1.1)))
                    ta = [GL_TLAYS[(shift + 2 * l + ir) % len(GL_TLAYS)] for l in range(nlay)]
                    if not top_first:
                        pa, pv, ta = pa[::-1], pv[::-1], ta[::-1]
                    assert all(a != b for a, b in zip(pa[:-1], pa[1:]))
                    cases.append(TlCase(len(cases), r, at, top_first, tuple(ta)))
                    play.append(pa), plev.append(pv), tlay.append(ta)
    return _freeze({"ncol": len(cases), "nlay": nlay, "play": np.array(play, F), "plev": np.array(plev, F),
                    "tlay": np.array(tlay, F), "cases": cases, "describe": _describe(cases, "column")})


# ---- the glue in float64, from the reference's text ---------------------------------------------------------------------------
def nn_inputs_f64(p, model):
    """compute_nn_inputs (rrtmgp/mo_gas_optics_rrtmgp.F90:618-798) in float64 -> (value, bound) (ncol, nlay, nx).

    Input k is (v_k - min_k) / (max_k - min_k) with v_1 = tlay, v_2 = log(play), v_3,4 = sqrt(sqrt(vmr)), the others the
    vmr itself (0 for an absent gas).  In float32 that is the roundings of v_k (none for an operand taken as it is; the
    two square roots, each correctly rounded: the first's error is halved by the second, together 1.5 u, counted as 2;
    logf, below one ulp = 2 u: 2), one for each of the two subtractions and one for the division, so with
    v^ = v (1 + theta_k):  |error| <= gamma_(k+3) (|v| + |min|) / |max - min|, the sum of the magnitudes of the two terms
    subtracted over the denominator.  One more rounding is granted for the float64 evaluation itself."""
    names = p["names"]
    nx = len(names)
    mn, mx = np.asarray(model["input_min"], np.float64), np.asarray(model["input_max"], np.float64)
    ncol, nlay = p["play"].shape
    v = np.zeros((ncol, nlay, nx))
    nround = np.zeros(nx, int)
    with np.errstate(divide="ignore"):
        v[..., 0], v[..., 1] = p["tlay"], np.log(p["play"].astype(np.float64))
    nround[1] = 2
    for k in (2, 3):
        v[..., k] = np.sqrt(np.sqrt(p["gases"][names[k]].astype(np.float64)))
        nround[k] = 2
    for k in range(4, nx):
        g = p["gases"].get(names[k])
        if g is not None:
            g = np.asarray(g, np.float64)
            v[..., k] = g if g.ndim == 0 else (g[None, :] if g.ndim == 1 else g)
    val = (v - mn) / (mx - mn)
    bound = np.array([gamma(n + 4) for n in nround]) * (np.abs(v) + np.abs(mn)) / np.abs(mx - mn)
    return val, bound


def col_dry_f64(h2o, plev):
    """get_col_dry (rrtmgp/mo_gas_optics_rrtmgp.F90:1662-1707) in float64 -> (value, bound) (ncol, nlay), with the
    constants of mo_rrtmgp_constants.F90 in the working precision (float32), as the reference's kernels see them.

    col_dry = 10 delta_plev avogad fact / (1000 m_air 100 grav), delta_plev = |p(l) - p(l+1)|, fact = 1 / (1 + h2o),
    m_air = (m_dry + m_h2o h2o) fact.  Every addition has terms of one sign and the one subtraction has exact operands,
    so every rounding is a relative one: delta_plev 1, fact 2 (the sum, the reciprocal), the numerator's three products
    3; m_air 2 + fact's 2 + 1, the denominator's three products 3; the division 1: 15 roundings, and one more for the
    float64 evaluation: |error| <= gamma_16 |col_dry| (the one term there is).  No intermediate is denormal but
    delta_plev, and 10 * delta_plev is exact there (a multiple of 2^-149 below 2^-126)."""
    m_dry, m_h2o, avogad, grav = (float(F(x)) for x in (0.028964, 0.018016, 6.02214076e23, 9.80665))
    v, pl = np.asarray(h2o, np.float64), np.asarray(plev, np.float64)
    delta = np.abs(pl[:, :-1] - pl[:, 1:])
    fact = 1.0 / (1.0 + v)
    m_air = (m_dry + m_h2o * v) * fact
    val = 10.0 * delta * avogad * fact / (1000.0 * m_air * 100.0 * grav)
    return val, gamma(16) * np.abs(val)


def tlev_f64(p):
    """The three level-temperature expressions of gas_optics_int (rrtmgp/mo_gas_optics_rrtmgp.F90:317-337) in float64
    -> (value, bound) (ncol, nlay + 1).

    Ends: t(1) + (plev(1) - play(1)) (t(2) - t(1)) / (play(2) - play(1)).  The three differences have exact operands
    (relative roundings), with the product and the quotient the second term T carries 5, and the sum one more on
    |t(1)| + |T|:  |error| <= gamma_6 (|t(1)| + |T|), plus one for the float64 evaluation: gamma_7.
    Interior: (N1 + N2) / D, N1 = play(l-1) t(l-1) (plev(l) - play(l)), N2 = play(l) t(l) (play(l-1) - plev(l)),
    D = plev(l) (play(l-1) - play(l)).  N1 and N2 carry 3 relative roundings each, their sum 1 on |N1| + |N2|, D 2 and
    the quotient 1:  |error| <= gamma_7 (|N1| + |N2|) / |D|, plus one: gamma_8."""
    pa, pv, ta = (np.asarray(p[k], np.float64) for k in ("play", "plev", "tlay"))
    nlay = pa.shape[1]
    val, bound = np.zeros(pv.shape), np.zeros(pv.shape)
    t0 = (pv[:, 0] - pa[:, 0]) * (ta[:, 1] - ta[:, 0]) / (pa[:, 1] - pa[:, 0])
    val[:, 0], bound[:, 0] = ta[:, 0] + t0, gamma(7) * (np.abs(ta[:, 0]) + np.abs(t0))
    tn = (pv[:, nlay] - pa[:, nlay - 1]) * (ta[:, nlay - 1] - ta[:, nlay - 2]) / (pa[:, nlay - 1] - pa[:, nlay - 2])
    val[:, nlay], bound[:, nlay] = ta[:, nlay - 1] + tn, gamma(7) * (np.abs(ta[:, nlay - 1]) + np.abs(tn))
    for l in range(1, nlay):
        n1 = pa[:, l - 1] * ta[:, l - 1] * (pv[:, l] - pa[:, l])
        n2 = pa[:, l] * ta[:, l] * (pa[:, l - 1] - pv[:, l])
        d = pv[:, l] * (pa[:, l - 1] - pa[:, l])
        val[:, l], bound[:, l] = (n1 + n2) / d, gamma(8) * (np.abs(n1) + np.abs(n2)) / np.abs(d)
    return val, bound


# ---- the networks of the fused entries ---------------------------------------------------------------------------------------
NET_KINDS = {"lw_pair": ("lw_abs", "lw_pfrac"), "sw_pair": ("sw_abs", "sw_ray"), "lw_both": ("lw_g128_both",),
             "lw_g128_pair": ("lw-g128-210809_absorption_BEST.nc", "lw-g128-210809_planck_frac_BEST.nc"),
             "sw_g112_pair": ("sw-g112-210809_absorption_BEST.nc", "sw-g112-210809_rayleigh_BEST.nc")}
NET_NGPT = {"lw_pair": 256, "sw_pair": 224, "lw_both": 128, "lw_g128_pair": 128, "sw_g112_pair": 112}


def model_path(name):
    """The shipped model of that name, or the reduced-resolution netCDF fixture under tests/golden/reference_files."""
    import os
    from rrtmgpnn import data
    if name.endswith(".nc"):
        return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_files", name)
    return data.path(name)


_MODELS = {}


def models(kind):
    from rrtmgpnn import data
    if kind not in _MODELS:
        _MODELS[kind] = [data.load_model(model_path(n)) for n in NET_KINDS[kind]]
    return _MODELS[kind]


_NET_REF = {}


def network_ref(orc, kind, variant=0):
    """(problem, x, col_dry, out0, out1) of the oracle's nn_inputs -> mlp -> tau_post / both_post on the glue problem:
    LW (tau, pfrac), SW (tau, ssa); computed once per (kind, variant)."""
    if (kind, variant) not in _NET_REF:
        ms = models(kind)
        p = build_glue(ms[0], kind, variant)
        x = orc.nn_inputs(p["play"], p["tlay"], p["gases"], ms[0])
        cd = orc.col_dry(p["gases"][p["names"][2]], p["plev"])
        xf = x.reshape(-1, x.shape[-1])
        with np.errstate(all="ignore"):
            if kind == "lw_both":
                o0, o1 = orc.both_post(ms[0], orc.mlp(ms[0], xf), cd)
            elif kind.startswith("lw"):
                y = orc.mlp(ms[1], xf)
                o0, o1 = orc.tau_post(ms[0], orc.mlp(ms[0], xf), cd), (y * y).astype(F)
            else:
                o0 = orc.tau_post(ms[0], orc.mlp(ms[0], xf), cd)
                o1 = orc.tau_post(ms[1], orc.mlp(ms[1], xf), cd, tau_abs_to_tot=o0)
        for a in (x, cd, o0, o1):
            a.setflags(write=False)
        _NET_REF[(kind, variant)] = (p, x, cd, o0, o1)
    return _NET_REF[(kind, variant)]
