"""CPU: the Planck source at temperature and table edges (tests/planck_edges.py) on the oracle.

* The pin.  No build of the reference's mo_gas_optics_kernels exists here (its module chain needs netCDF), so
  orc_planck_source_nn is held to a float32 numpy restatement of interpolate1D and compute_Planck_source_nn
  (rrtmgp/kernels/mo_gas_optics_kernels.F90:1024-1043 and :615-683), one Fortran operation per numpy operation, bit for
  bit as uint32 views on every problem the GPU file runs: the four tables' nlay-5 problems, the band-table-loop shapes
  and planck_source_kernel's shapes.  The same kind of pin test_glue_oracle.py gives tlev.
* The census, on the inputs alone: each table's temperatures reach every class of val0 -- at or below -1, between -1
  and 0, on a knot inside the table, at or beyond the last knot with and without a fraction -- and every temperature
  stands in each role (tlay, tlev, tsfc).
* The reference's behaviour outside the table as literal facts of the oracle: B(temp_ref_max) is the last but one table
  value, B(temp_ref_min - delta) the first, sfc_source_Jac is 0 at tsfc = temp_ref_max - 1 on the shipped table (and
  NEGATIVE there on d3, an increasing table whose step is not 1).
* A float64 evaluation of the same piecewise expression on the float32 inputs, with a forward-error bound derived from
  the operations (planck_edges.planck_f64): the one check here that shares no arithmetic with the oracle.
"""
import numpy as np
import pytest

import planck_edges as P

F = np.float32
SFC = pytest.mark.parametrize("top_at_1", [True, False], ids=["top", "bot"])
TABLE = pytest.mark.parametrize("name", P.TABLES)


def _equal_restatement(orc, p, sfc_lay, what):
    got = orc.planck_source(p["kd"], p["tlay"], p["tlev"], p["tsfc"], p["pfrac"], sfc_lay)
    want = P.planck_source_f32(p["kd"], p["tlay"], p["tlev"], p["tsfc"], p["pfrac"], sfc_lay)
    for x, y, k in zip(got, want, ("lay_source", "lev_source", "sfc_source", "sfc_source_Jac")):
        P.assert_bits(x, y, p, "%s %s" % (what, k))


@SFC
@TABLE
def test_oracle_equals_restatement(orc, name, top_at_1):
    p = P.build(name)
    _equal_restatement(orc, p, P.sfc_lay_of(p, top_at_1), name)


@pytest.mark.parametrize("shape", P.LOOP_SHAPES, ids=P.loop_id)
def test_oracle_equals_restatement_loop_shapes(orc, shape):
    p = P.build_loop(*shape)
    for top_at_1 in (True, False):
        _equal_restatement(orc, p, P.sfc_lay_of(p, top_at_1), P.loop_id(shape))


@pytest.mark.parametrize("shape", P.kernel_shapes(), ids=lambda s: "nlay%d-ngpt%d-sfc%d" % s)
def test_oracle_equals_restatement_kernel_shapes(orc, shape):
    nlay, ngpt, sfc_lay = shape
    _equal_restatement(orc, P.build_kernel(nlay, ngpt), sfc_lay, str(shape))


@TABLE
def test_temperature_set_and_roles(name):
    t, p = P.edge_temps(name), P.build(name)
    assert len(t) == P.N_TEMPS[name]
    assert np.isfinite(t).all() and (np.diff(t) > 0).all()
    assert p["nlay"] == P.NLAY
    for role in ("tlay", "tlev", "tsfc"):
        assert np.isin(t, p[role]).all(), "a temperature of the set is missing as " + role
    assert np.isin(P.tsfc_extras(p["kd"]), p["tsfc"]).all()
    # the Planck fraction's cycle: every value of it at every layer
    for v in P.PFRACS:
        if v is not None:
            assert (p["pfrac"] == v).any(axis=(0, 2)).all()
    assert ((p["tau"] >= F(0.05)) & (p["tau"] <= F(2))).all() and ((p["emis"] >= F(0.9)) & (p["emis"] <= F(1))).all()


@TABLE
def test_census(name):
    kd, t = P.tables()[name], P.edge_temps(name)
    for cls, m in P.classes(kd, t).items():
        assert int(m.sum()) >= P.CENSUS[cls][name] >= 1, (cls, name, int(m.sum()))


def test_loop_shapes_reach_the_later_rounds():
    """Entries of the band table against the 8 x threads a round forms: the shapes end inside the first round, on its
    end, inside the second, on its end and inside the third (256 g-points), and inside the second at 64 threads."""
    n = {s: P.ntab(P.build_loop(*s)) for s in P.LOOP_SHAPES}
    assert [n[("d3", k)] for k in (1, 2, 63, 64, 127, 128)] == [64, 96, 2048, 2080, 4096, 4128]
    assert [P.ntab(P.build_loop("d3", k), jac=True) - n[("d3", k)] for k in (1, 128)] == [16, 16]
    assert 512 < n[("two", 300)] < 1024 and 512 < n[("d07", 100)] < 1024
    for s in P.LOOP_SHAPES:
        p = P.build_loop(*s)
        kd = p["kd"]
        lo, hi = kd["temp_ref_min"][0], P.tmax(kd)
        for a in (p["tsfc"], p["tlay"][:, 0], p["tlev"][:, -1]):
            assert ((a < lo) | (a >= hi)).all()
        assert ((p["tlay"][:, 1:] >= lo) & (p["tlay"][:, 1:] <= hi)).all()


def _B(orc, kd, T):
    """interpolate1D(T) per g-point through the oracle: one column, one layer, pfrac 1."""
    one = np.ones((1, 1, kd["ngpt"]), F)
    t = np.array([[T]], F)
    lay, lev, sfc, jac = orc.planck_source(kd, t, np.array([[T, T]], F), np.array([T], F), one, 1)
    return lay[0, 0], sfc[0], jac[0]


@TABLE
def test_quirks_outside_the_table(orc, name):
    kd = P.tables()[name]
    tab = np.asarray(kd["totplnk"], F)
    b = P._band_of(np.asarray(kd["band_lims_gpt"]).reshape(-1, 2), kd["ngpt"])
    t0, d = P.tmin_delta(kd)
    n = kd["nPlanckTemp"]
    hi = P.tmax(kd)
    eq = lambda x, y: np.testing.assert_array_equal(x.view(np.uint32), np.ascontiguousarray(y, F).view(np.uint32))  # noqa: E731
    # d07's step and offset (0.7, 150.3) are no float32 numbers, so its knots need not land on integers of val0; the
    # other tables' do, and there the facts are literal
    exact = P.val0(kd, hi) == n - 1 and P.val0(kd, F(t0 - d)) == -1
    assert exact or name == "d07"
    if exact:
        eq(_B(orc, kd, hi)[0], tab[b, n - 2])      # T = temp_ref_max: the last but one value
        eq(_B(orc, kd, F(t0 - d))[0], tab[b, 0])   # one step below the table: the first value
    eq(_B(orc, kd, t0)[0], tab[b, 0])
    if name == "shipped":
        assert (t0, d, n, hi) == (F(160), F(1), 196, F(355))
        for T in (159, 100, 0):                    # the index is clamped and the fraction of an integer val0 is 0
            eq(_B(orc, kd, F(T))[0], tab[b, 0])
        eq(_B(orc, kd, F(159.5))[0], tab[b, 0] + F(-0.5) * (tab[b, 1] - tab[b, 0]))  # extrapolates with frac = -0.5
        for T in (354, 354.5):
            assert (_B(orc, kd, F(T))[2] == 0).all()  # sfc_source_Jac == 0
        # the float below temp_ref_max is about B(355), the float above it about B(354) again
        below, above = _B(orc, kd, np.nextafter(hi, F(0)))[0], _B(orc, kd, np.nextafter(hi, F(400)))[0]
        np.testing.assert_allclose(below, tab[b, n - 1], rtol=1e-5)
        np.testing.assert_allclose(above, tab[b, n - 2], rtol=1e-5)
    elif name == "d3":
        # an increasing table with a step other than 1: tsfc + 1 reaches the last knot, whose value is the last but
        # one, so the Jacobian of an increasing Planck function comes out negative
        assert (np.diff(tab, axis=1) > 0).all()
        assert (_B(orc, kd, F(hi - F(1)))[2] < 0).all()


@TABLE
def test_float64_reference(orc, name):
    """The oracle's four outputs against planck_edges.planck_f64 (the derivation of the bound is its docstring: one
    subtraction and one division into val0, the exact fractional part, one subtraction, one product, one sum, the product
    by pfrac).  Outside the table the function jumps at integers of val0, and a case whose float32 and float64
    truncations differ there is excused: none on the shipped table and d3, at most 5 % of a table's temperatures
    elsewhere.  Inside the table nothing is excused.  sfc_source_Jac is a difference of two such values times pfrac: the
    two bounds add, plus the rounding of the difference and of the product."""
    p = P.build(name)
    kd, b = p["kd"], p["band_of"]
    sfc_lay = 2
    lay, lev, sfc, jac = orc.planck_source(kd, p["tlay"], p["tlev"], p["tsfc"], p["pfrac"], sfc_lay)
    nlay = p["nlay"]
    pf_lev = np.concatenate([p["pfrac"], p["pfrac"][:, -1:]], axis=1)  # lev_source(nlay + 1) takes pfrac(nlay)
    pf_sfc = p["pfrac"][:, sfc_lay - 1]
    n_excused = 0

    def check(got, T, pf, what):
        nonlocal n_excused
        Tb = np.broadcast_to(T[..., None], pf.shape)
        value, bound, excused = P.planck_f64(kd, Tb, pf)
        value, bound = (np.take_along_axis(a, np.broadcast_to(b, pf.shape)[..., None], axis=-1)[..., 0]
                        for a in (value, bound))
        err = np.abs(got.astype(np.float64) - value)
        bad = (err > bound) & ~excused
        assert not bad.any(), "%s %s: %d beyond the bound, worst %.3g x" % (name, what, int(bad.sum()),
                                                                           float((err / bound)[bad].max()))
        return excused[..., 0]

    ex_lay = check(lay, p["tlay"], p["pfrac"], "lay_source")
    ex_lev = check(lev, p["tlev"], pf_lev, "lev_source")
    ex_sfc = check(sfc, p["tsfc"], pf_sfc, "sfc_source")
    # excused temperatures, counted once per value of the set
    t = P.edge_temps(name)
    excused_T = np.unique(np.concatenate([p["tlay"][ex_lay], p["tlev"][ex_lev], p["tsfc"][ex_sfc]]))
    n_excused = int(np.isin(t, excused_T).sum())
    allowed = 0 if name in ("shipped", "d3") else int(0.05 * len(t))
    assert n_excused <= allowed, (name, n_excused, excused_T)
    # the Jacobian
    Ts = np.broadcast_to(p["tsfc"][:, None], pf_sfc.shape)
    one = np.ones_like(pf_sfc)
    v0, b0, e0 = P.planck_f64(kd, Ts, one)
    v1, b1, e1 = P.planck_f64(kd, (Ts + F(1)).astype(F), one)
    pick = lambda a: np.take_along_axis(a, np.broadcast_to(b, pf_sfc.shape)[..., None], axis=-1)[..., 0]  # noqa: E731
    v0, b0, v1, b1 = (pick(a) for a in (v0, b0, v1, b1))
    pfd = pf_sfc.astype(np.float64)
    value = pfd * (v1 - v0)
    bound = pfd * ((b0 + b1) * (1 + P.U) + P.U * np.abs(v1 - v0)) * (1 + P.U) + P.U * np.abs(value) + P.ETA
    err = np.abs(jac.astype(np.float64) - value)
    bad = (err > bound) & ~(e0 | e1)
    assert not bad.any(), "%s sfc_source_Jac: %d beyond the bound" % (name, int(bad.sum()))
    assert nlay == P.NLAY


def test_restatement_tells_the_tidied_forms_apart():
    """What the edge set is for: floorf, a clamped fraction, a clamped val0, a reciprocal and a contracted fma each change
    the restatement's bits somewhere on the tables -- the reciprocal and nothing else only on the tables whose step is
    not 1."""
    def variant(kd, T, how):
        t0, d = P.tmin_delta(kd)
        tab = np.asarray(kd["totplnk"], F)
        n = tab.shape[1]
        T = np.asarray(T, F)
        v = (T - t0) * (F(1) / d) if how == "rcp" else (T - t0) / d
        if how == "clamp_val":
            v = np.clip(v, F(0), F(n - 1))
        iv = (np.floor(v) if how == "floor" else np.trunc(v)).astype(np.int64)
        frac = v - iv.astype(F)
        if how == "clamp_frac":
            frac = np.clip(frac, F(0), F(1))
        idx = np.minimum(n - 1, np.maximum(1, iv + 1))
        lo, hi = tab[:, idx - 1], tab[:, idx]
        if how == "fma":
            return (lo.astype(np.float64) + frac.astype(np.float64) * (hi - lo).astype(np.float64)).astype(F)
        return lo + frac * (hi - lo)

    differs = {}
    for name in P.TABLES:
        kd, t = P.tables()[name], P.edge_temps(name)
        base = variant(kd, t, "plain")
        np.testing.assert_array_equal(base.view(np.uint32), np.moveaxis(P.interpolate1d_f32(
            t, *P.tmin_delta(kd), kd["totplnk"]), -1, 0).view(np.uint32))
        differs[name] = {h: bool((variant(kd, t, h).view(np.uint32) != base.view(np.uint32)).any())
                         for h in ("floor", "clamp_frac", "clamp_val", "rcp", "fma")}
    assert not differs["shipped"]["rcp"], "a reciprocal is a division by one on the shipped table"
    assert differs["d07"]["rcp"] and differs["d3"]["rcp"]
    for h in ("floor", "clamp_frac", "clamp_val"):
        assert all(differs[n][h] for n in P.TABLES), (h, differs)
    assert differs["shipped"]["fma"] and differs["d3"]["fma"]
