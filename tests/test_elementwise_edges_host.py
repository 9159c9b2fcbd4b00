"""CPU: the operand-edge cases of tests/elementwise_edges.py on the oracle.

* The pin: the oracle (oracle/rrtmgpnn_oracle.c) equals the reference's own Fortran (oracle/_ref) bit for bit on the
  delta-scale, increment and cloud-optics cases -- as uint32 views, because the Pade ice runs return inf.
* The conditions, without which tests/test_gpu_elementwise_edges.py could pass on an empty edge: no nan in the oracle's
  outputs (but the SW ssa of the fused networks, nan exactly where tau == 0), denormal outputs, both sides of every
  max(eps, .) guard, the clamped negative Pade co-albedo, fint == 0 on a knot, index == nsteps - 1 at the upper end.
* The glue (compute_nn_inputs, get_col_dry, the three tlev expressions) against a plain float64 evaluation of the
  reference's formulas, within a forward-error bound of the float32 expression (derived in elementwise_edges.*_f64):
  the one check of the glue that shares neither code nor arithmetic with the oracle.
* The refusal of overlapping band limits, which needs no device.
"""
import numpy as np
import pytest

import elementwise_edges as E

F = np.float32


def _ref():
    import oracle as O
    try:
        return O.Reference()
    except FileNotFoundError as e:
        pytest.skip(str(e))


def _co(which):
    from rrtmgpnn import data
    return data.load_cloud_optics(which)


# ---- delta scaling ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", E.DS_FORMS, ids=str)
def test_delta_scale_oracle_equals_reference(orc, form):
    from rrtmgpnn import data
    ref, p = _ref(), E.build_delta_scale()
    kd = data.load_kdist("sw")
    shp = E.DS_SHAPE
    assert shp[2] == kd["nband"]
    fwd = p["fwd"][form]
    a = orc.delta_scale(p["tau"], p["ssa"], p["g"], fwd)
    b = ref.delta_scale(kd, p["tau"].reshape(shp), p["ssa"].reshape(shp), p["g"].reshape(shp),
                        None if fwd is None else fwd.reshape(shp))
    for x, y, name in zip(a, b, ("tau", "ssa", "g")):
        E.assert_bits(x, y.reshape(-1), "delta_scale %s (%s)" % (name, form), p["describe"])


@pytest.mark.parametrize("form", E.DS_FORMS, ids=str)
def test_delta_scale_conditions(orc, form):
    p = E.build_delta_scale()
    fwd = p["fwd"][form]
    tau, ssa, g = orc.delta_scale(p["tau"], p["ssa"], p["g"], fwd)
    assert not any(np.isnan(a).any() for a in (tau, ssa, g))
    assert E.is_denormal(tau).sum() >= 120 and E.is_denormal(ssa).sum() >= 120
    f = p["g"] * p["g"] if fwd is None else fwd
    assert ((f >= 0) & (f <= 1)).all()
    for d in (F(1) - p["ssa"] * f, F(1) - f):  # the operands of the two max(eps, .)
        assert (d < E.EPS3).any() and (d > E.EPS3).any()


# ---- increment -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nstr_io,nstr_in", E.PAIRINGS)
def test_increment_oracle_equals_reference(orc, nstr_io, nstr_in):
    from rrtmgpnn import data
    ref, p = _ref(), E.build_increment("sw")
    io, inc = p["io"][:1 if nstr_io == 1 else 3], p["inc"][:1 if nstr_in == 1 else 3]
    a = E.increment_ref(orc, p, nstr_io, nstr_in)
    b = ref.increment_bybnd(data.load_kdist("sw"), io, inc)
    for x, y, name in zip(a, b, ("tau", "ssa", "g")):
        assert np.isfinite(x).all(), name
        E.assert_bits(x.reshape(-1, p["ngpt"]), y.reshape(-1, p["ngpt"]), "increment %d by %d, %s" % (nstr_io, nstr_in, name),
                      p["describe"])


@pytest.mark.parametrize("layout", E.INC_LAYOUTS)
def test_increment_conditions(orc, layout):
    p = E.build_increment(layout)
    # column 0 alone holds every io triple beside every increment triple
    seen = set(zip(p["io_case"][0].ravel().tolist(), np.repeat(p["in_case"][0][:, :1], p["ngpt"], axis=1).ravel().tolist()))
    assert len(seen) == len(E.INC_IO) * len(E.INC_IN)
    assert (~p["covered"]).sum() == (5 if layout == "gap" else 0)
    band_of = np.zeros(p["ngpt"], int)
    for b, (lo, hi) in enumerate(p["lims"]):
        band_of[lo - 1:hi] = b
    t1, w1 = p["io"][0], p["io"][1]
    t2, w2 = (a[..., band_of] for a in p["inc"][:2])
    with np.errstate(all="ignore"):
        for d in (t1 + t2, t1 * w1 + t2 * w2):  # the operands of the two max(eps, .)
            d = d[..., p["covered"]]
            assert (d < E.EPS3).any() and (d > E.EPS3).any()
    for nstr_io, nstr_in in E.PAIRINGS:
        out = E.increment_ref(orc, p, nstr_io, nstr_in)
        assert all(np.isfinite(a).all() for a in out)
        assert any(E.is_denormal(a).any() for a in out)
        for a, b in zip(out, p["io"]):  # a g-point in no band comes back untouched
            E.assert_bits(a[..., ~p["covered"]], b[..., ~p["covered"]], "outside every band")


# ---- cloud optics ---------------------------------------------------------------------------------------------------------
CO_RUNS = [(lut, nstr, icergh) for lut in (True, False) for nstr in (1, 2) for icergh in (1, 2, 3)]


@pytest.mark.parametrize("which", ["lw", "sw"])
def test_cloud_optics_radii(which):
    co = _co(which)
    p = E.build_cloud_optics(co, which)
    assert (len(p["rl"]), len(p["ri"])) == (67, 52)
    lwp, iwp, rl, ri = p["args"]
    assert ((lwp > 0) & (iwp == 0)).any() and ((lwp == 0) & (iwp > 0)).any() and ((lwp > 0) & (iwp > 0)).any()
    for r, phase in ((rl, "liq"), (ri, "ice")):  # never a radius outside the table
        k = "radliq" if phase == "liq" else "radice"
        assert (r >= F(co[k + "_lwr"][0])).all() and (r <= F(co[k + "_upr"][0])).all()
        # every (radius, water path) of the phase occurs
        w = lwp if phase == "liq" else iwp
        pairs = set(zip(r[w > 0].tolist(), w[w > 0].tolist()))
        assert len(pairs) == len(p["rl" if phase == "liq" else "ri"]) * len(E.CO_PATHS)
        # the table walk: fint == 0 on a knot, index == nsteps - 1 (and fint == 1) at the upper end
        nsteps = co["lut_ext" + phase].shape[-1]
        knots, step = E.lut_knots(co[k + "_lwr"][0], co[k + "_upr"][0], nsteps)
        index, fint = E.table_index(r, co[k + "_lwr"][0], step, nsteps)
        assert index.min() == 1 and index.max() == nsteps - 1
        assert (fint == 0).any() and ((index == nsteps - 1) & (fint == 1)).any()
        assert ((fint > 0) & (fint < 1)).any()


@pytest.mark.parametrize("which", ["lw", "sw"])
@pytest.mark.parametrize("lut,nstr,icergh", CO_RUNS)
def test_cloud_optics_oracle_equals_reference(orc, which, lut, nstr, icergh):
    ref, co = _ref(), _co(which)
    p = E.build_cloud_optics(co, which)
    a = orc.cloud_optics(co, *p["args"], nstr=nstr, lut=lut, icergh=icergh)
    b = ref.cloud_optics(co, *p["args"], nstr=nstr, lut=lut, icergh=icergh)
    for x, y, name in zip(a, b, ("tau", "ssa", "g")):
        E.assert_bits(E.co_rows(x), E.co_rows(y), "cloud optics %s %s" % (which, name), p["describe"])


@pytest.mark.parametrize("which", ["lw", "sw"])
@pytest.mark.parametrize("lut,nstr,icergh", CO_RUNS)
def test_cloud_optics_conditions(orc, which, lut, nstr, icergh):
    co = _co(which)
    p = E.build_cloud_optics(co, which)
    out = orc.cloud_optics(co, *p["args"], nstr=nstr, lut=lut, icergh=icergh)
    assert not any(np.isnan(a).any() for a in out)
    assert sum(int(E.is_denormal(a).sum()) for a in out) >= 1000
    if nstr == 2:
        tau, ssa, _ = out
        # max(FLT_EPSILON, t): tau is t itself; max(FLT_EPSILON, ts): ts <= t below the guard, and above it
        # ssa = ts / t to one rounding, so ssa * t > 2 eps puts ts above eps
        assert (tau < E.FLT_EPS).any() and (tau > E.FLT_EPS).any()
        with np.errstate(all="ignore"):
            assert (np.where(np.isfinite(tau), ssa * tau, 0) > F(2) * E.FLT_EPS).any()
    if not lut:
        lwp, iwp, rl, ri = (a.ravel() for a in p["args"])
        clamped = False
        for phase, r, w, coef in (("liq", rl, lwp, co["pade_ssaliq"]), ("ice", ri, iwp, co["pade_ssaice"][icergh - 1])):
            irad = E.pade_irad(r[w > 0], co["pade_sizreg_ssa" + phase])
            # never a regime before the table; dividing by b(3) keeps some arrays from ever reaching regime 3
            assert irad.min() >= 1 and len(set(irad.tolist())) >= 2
            clamped |= bool((E.pade_eval(coef, irad, r[w > 0], 2, 2) < 0).any())
        # the LW coefficients give no negative co-albedo anywhere on these radii: the SW Pade runs take the clamp
        assert clamped == (which == "sw"), "the max(0, .) of the Pade co-albedo"


@pytest.mark.parametrize("which", ["lw", "sw"])
@pytest.mark.parametrize("icergh", [1, 2, 3])
def test_cloud_optics_pade_runs_return_inf_and_negative_values(orc, which, icergh):
    """Why the comparison is on bit patterns: the Pade extinction is negative at some radii, so that ssa and g are the
    quotient of a huge negative value by FLT_EPSILON, -inf."""
    co = _co(which)
    p = E.build_cloud_optics(co, which)
    tau, ssa, g = orc.cloud_optics(co, *p["args"], nstr=2, lut=False, icergh=icergh)
    assert (tau < 0).any() and np.isinf(ssa).any() and np.isinf(g).any()


# ---- heating rates --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k_day", [False, True])
def test_heating_rate_conditions(orc, k_day):
    p = E.build_heating()
    dp = p["plev"][:, 1] - p["plev"][:, 0]
    assert (dp > 0).any() and (dp < 0).any() and not (dp == 0).any()
    assert (np.abs(dp) == np.spacing(F(5e4))).any()
    hr = orc.heating_rate(p["up"], p["dn"], p["plev"], k_day=k_day)
    assert not np.isnan(hr).any()
    assert E.is_denormal(hr).any() and np.isfinite(hr).all()
    up, dn = p["up"], p["dn"]
    d = (up[:, 1] - up[:, 0] - dn[:, 1] + dn[:, 0]) if not k_day else ((dn[:, 1] - up[:, 1]) - (dn[:, 0] - up[:, 0]))
    differs = (up[:, 1] != up[:, 0]) | (dn[:, 1] != dn[:, 0])
    assert ((d == 0) & differs).any(), "no four-term difference cancels exactly"
    assert E.is_denormal(d).any()


# ---- the glue against float64 ---------------------------------------------------------------------------------------------
def _within(got, val, bound, what, p):
    err = np.abs(np.asarray(got, np.float64) - val)
    bad = np.unique(np.nonzero((~(err <= bound)).reshape(err.shape[0], -1))[0])
    assert not bad.size, "%s: beyond the float32 forward-error bound; %s" % (what, p["describe"](bad))


@pytest.mark.parametrize("kind", ["lw_pair", "sw_pair"])
@pytest.mark.parametrize("variant", E.GL_VARIANTS)
def test_nn_inputs_against_float64(orc, kind, variant):
    m = E.models(kind)[0]
    p = E.build_glue(m, kind, variant)
    x = orc.nn_inputs(p["play"], p["tlay"], p["gases"], m)
    val, bound = E.nn_inputs_f64(p, m)
    assert np.isfinite(x).all() and np.abs(x).max() < 2.0 ** 100  # far inside div_softsign's |x| < 2^126
    _within(x, val, bound, "compute_nn_inputs", p)
    assert (x[..., 2] == (F(0) - F(m["input_min"][2])) / (F(m["input_max"][2]) - F(m["input_min"][2]))).any()  # sqrt(sqrt(0))
    assert set(p["forms"].values()) >= ({"scalar", "1d", "2d", "absent"} if kind == "lw_pair" else {"2d"})


def test_glue_forms_cover_every_gas_form():
    for kind in ("lw_pair", "sw_pair"):
        m = E.models(kind)[0]
        seen = set()
        for v in E.GL_VARIANTS:
            seen |= set(E.build_glue(m, kind, v)["forms"].values())
        assert seen == set(E.GL_FORMS)


def test_col_dry_against_float64(orc):
    m = E.models("sw_pair")[0]
    p = E.build_glue(m, "sw_pair", 0)
    h2o = p["gases"][p["names"][2]]
    cd = orc.col_dry(h2o, p["plev"])
    val, bound = E.col_dry_f64(h2o, p["plev"])
    assert np.isfinite(cd).all()
    thin = p["plev"][:, 0] == p["plev"][:, 1]
    assert thin.any() and (cd[thin] == 0).all() and (cd[~thin] > 0).all()  # the zero-thickness layer
    _within(cd, val, bound, "get_col_dry", p)
    # every h2o beside every level pair
    assert len(set(zip(h2o[:, 0].tolist(), map(tuple, p["plev"].tolist())))) == len(E.GL_VMRS) * len(E.GL_PLEVS)


@pytest.mark.parametrize("nlay", [2, 5])
def test_interpolate_tlev_against_float64(orc, nlay):
    p = E.build_tlev(nlay)
    tl = orc.interpolate_tlev(p["play"], p["plev"], p["tlay"])
    val, bound = E.tlev_f64(p)
    assert np.isfinite(tl).all()
    _within(tl, val, bound, "interpolate_tlev", p)
    r = np.maximum(p["play"][:, 1:] / p["play"][:, :-1], p["play"][:, :-1] / p["play"][:, 1:])
    assert r.min() > 1 and r.min() <= 1 + 2.0 ** -22 and r.max() >= 9e5


@pytest.mark.parametrize("kind", sorted(E.NET_KINDS))
def test_network_reference_conditions(orc, kind):
    """The fused entries' reference: finite but for the SW ssa, nan exactly where tau == 0 (0 / 0 under a layer of
    zero thickness); denormal outputs."""
    p, x, cd, o0, o1 = E.network_ref(orc, kind, 0)
    assert o0.shape == (p["ncol"], E.NET_NGPT[kind]) and not np.isnan(o0).any() and (o0 > 0).any()
    if kind.startswith("sw"):
        assert np.array_equal(np.isnan(o1), o0 == 0) and (o0 == 0).any()
    else:
        assert not np.isnan(o1).any()
    assert E.is_denormal(o0).any() or E.is_denormal(x).any()


# ---- the refusal of overlapping band limits --------------------------------------------------------------------------------
def test_increment_bybnd_refuses_overlapping_band_limits():
    """increment_bybnd_kernel gives a g-point the first band that holds it; the reference's inc_*_bybnd increment it once
    per band.  Overlapping limits are RRTMGPNN_ERR_ARGUMENT (1) before anything is launched: the entry judges its band
    limits ahead of the context, so no device is needed here.  A gap stays legal (it then goes on to the context)."""
    from rrtmgpnn import _lib
    L = _lib.lib()
    for lims in ([1, 8, 8, 16], [1, 16, 4, 6], [5, 16, 1, 5]):
        rc = L.rrtmgpnn_increment_bybnd(None, 1, 1, 16, 2, _lib.int_array(lims), None, None, None, None, None, None)
        assert rc == 1 and b"overlap" in L.rrtmgpnn_last_error(), lims
    rc = L.rrtmgpnn_increment_bybnd(None, 1, 1, 16, 2, _lib.int_array([1, 7, 9, 16]), None, None, None, None, None, None)
    assert rc != 0 and b"null context" in L.rrtmgpnn_last_error()
