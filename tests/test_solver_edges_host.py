"""CPU: the conditions under which tests/test_gpu_solver_edges.py cannot hide a failure, checked on the oracle alone.

The edge problems of tests/solver_edges.py must (a) give finite reference fluxes everywhere, (b) not be mostly zeros,
(c) put the lit g-point's flux into the broadband outputs bit for bit, and (d) really reach the value-dependent code
they are built for: the eps branch and the k_min clamp of sw_two_stream, underflowed direct-beam transmittances, single
scattering albedos below the shortened division's numerator bound, both sides of the LW tau threshold for every secant,
subnormal fluxes, and the clamps of the band increment.

Measured with this construction (1344 SW columns, 672 LW columns, 5 layers): zero shares SW up 0.24, down 0.19,
direct 0.46, LW up 0.006, down 0.092 (fused Planck: 0.015 / 0.09); eps branch 484 columns, k_min clamp 280,
exp(-tau/mu0) underflowed 636, 0 < ssa < 2^-100 240, subnormal nonzero fluxes > 3000.  The zero shares are those of the
problem as built (incident diffuse flux present in two thirds of the columns); the GPU test's runs without any
diffuse flux compare more zeros (up 0.31) on top of these.
"""
import numpy as np
import pytest

import solver_edges as E

F = np.float32


@pytest.fixture(scope="module")
def sw():
    return E.build_sw()


@pytest.fixture(scope="module")
def lw():
    return E.build_lw()


def _zero_share(a):
    return float((a == 0).mean())


@pytest.mark.parametrize("top_at_1", [True, False])
def test_sw_reference_is_finite_lit_only_and_not_mostly_zero(orc, sw, top_at_1):
    p = sw
    out = orc.sw_solver(p["tau"], p["ssa"], p["g"], p["mu0"], p["inc"], p["alb_dir"], p["alb_dif"], top_at_1,
                        inc_flux_dif=p["inc_dif"], gpt=True)
    plain = orc.sw_solver(p["tau"], p["ssa"], p["g"], p["mu0"], p["inc"], p["alb_dir"], p["alb_dif"], top_at_1,
                          inc_flux_dif=p["inc_dif"])
    for a in out + plain:
        assert np.isfinite(a).all()
    c = np.arange(p["ncol"])
    for name, bb, bb_plain, gp, cap in zip(("up", "dn", "dir"), out[:3], plain, out[3:], (0.25, 0.25, 0.50)):
        # the broadband flux IS the lit g-point's flux, and the unlit g-points carry exactly zero
        np.testing.assert_array_equal(bb, gp[c, :, p["lit"]], err_msg=name)
        np.testing.assert_array_equal(bb_plain, bb, err_msg=name)
        unlit = gp.copy()
        unlit[c, :, p["lit"]] = 0
        assert not unlit.any(), name
        share = _zero_share(bb)
        print("SW %s top_at_1=%s: share of exact zeros %.3f (cap %.2f)" % (name, top_at_1, share, cap))
        assert share <= cap, (name, share)
    subn = sum(int(((a != 0) & (np.abs(a) < E.FLT_MIN)).sum()) for a in plain)
    print("subnormal nonzero SW reference fluxes:", subn)
    assert subn >= 100
    # without any incident diffuse flux and on absorption-only properties the reference stays finite too
    for a in orc.sw_solver(p["tau"], p["ssa"], p["g"], p["mu0"], p["inc"], p["alb_dir"], p["alb_dif"], top_at_1):
        assert np.isfinite(a).all()
    assert np.isfinite(orc.sw_solver_noscat(p["tau"], p["mu0"], p["inc"], top_at_1)).all()


def test_sw_census_of_the_edge_layers(sw):
    e = sw["edge"]
    _, k2 = E.sw_k(e["ssa"], e["g"])
    with np.errstate(over="ignore"):
        beam = -e["tau"] * (F(1) / e["mu0"])
    census = {"eps branch": int(E.in_eps_branch(e["ssa"], e["g"], e["mu0"]).sum()),
              "k_min clamp": int((k2 < E.K_MIN).sum()),
              "exp(-tau/mu0) underflowed": int((beam < E.EXP_UNDERFLOW).sum()),
              "0 < ssa < 2^-100": int(((e["ssa"] > 0) & (e["ssa"] < F(2.0 ** -100))).sum())}
    print(census)
    for what, n in census.items():
        assert n >= 100, (what, n)
    # the special values themselves
    assert (e["tau"] == 0).sum() >= 50 and (e["ssa"] == 1).sum() >= 50
    assert ((e["ssa"] == 0) & (e["mu0"] == F(0.5))).sum() >= 10  # k mu0 == 1 exactly
    # every residue mod 4 and both halves of a pair are lit, every layer position is an edge layer
    assert set(sw["lit"] % 4) == {0, 1, 2, 3} and set(sw["layer"]) == set(range(E.NLAY))
    # both sides of the stated operand domain are present, and the g == 0 subset (the g = NULL instances) is not small
    assert 100 <= sw["in_domain"].sum() <= sw["ncol"] - 100
    assert len(sw["g0"]) >= 100
    # every column is one case of its own
    assert len({c[1:-2] for c in sw["cases"]}) == sw["ncol"]


def test_sw_band_increment_reaches_its_clamps(orc, sw):
    p = sw
    c = np.arange(p["ncol"])
    per = p["ngpt"] // E.INC_NBND
    t2, w2 = (np.repeat(p[k], per, axis=2)[c, p["layer"], p["lit"]] for k in ("tau_bnd", "ssa_bnd"))
    t1, w1 = (p[k][c, p["layer"], p["lit"]] for k in ("tau", "ssa"))
    tau12, scat12 = t1 + t2, t1 * w1 + t2 * w2
    eps = F(3) * E.FLT_MIN
    both0, under = int((tau12 == 0).sum()), int(((tau12 > 0) & (scat12 < eps)).sum())
    print("band increment: both taus 0 in %d columns, tau*ssa sum below 3*FLT_MIN in %d" % (both0, under))
    assert both0 >= 10 and under >= 100
    io = orc.increment_bybnd(p["band_lims_gpt"], (p["tau"], p["ssa"], p["g"]), (p["tau_bnd"], p["ssa_bnd"], p["g_bnd"]))
    for a in io:
        assert np.isfinite(a).all()
    for top_at_1 in (True, False):
        for a in orc.sw_solver(*io, p["mu0"], p["inc"], p["alb_dir"], p["alb_dif"], top_at_1, inc_flux_dif=p["inc_dif"]):
            assert np.isfinite(a).all()


def _lw_runs(orc, lw, top_at_1):
    from rrtmgpnn import data
    p = lw
    yield "nmus1", orc.lw_solver(p["tau"], p["lay"], p["lev"], p["emis"], p["sfc"], top_at_1, 1, inc_flux=p["inc"])
    yield "nmus3", orc.lw_solver(p["tau"], p["lay"], p["lev"], p["emis"], p["sfc"], top_at_1, 3, inc_flux=p["inc"])
    yield "lw_Ds", orc.lw_solver(p["tau"], p["lay"], p["lev"], p["emis"], p["sfc"], top_at_1, 1, inc_flux=p["inc"],
                                 lw_Ds=p["lw_ds"])
    kd = data.load_kdist("lw")
    lay, lev, sfc, _ = orc.planck_source(kd, p["tlay"], p["tlev"], E.lw_tsfc(p, top_at_1), p["pfrac"],
                                         p["nlay"] if top_at_1 else 1)
    c = np.arange(p["ncol"])
    for a in (lay, lev):  # a zero Planck fraction leaves the unlit g-points without any source
        a = a.copy()
        a[c, :, p["lit"]] = 0
        assert not a.any()
    yield "planck", orc.lw_solver(p["tau"], lay, lev, p["emis"], sfc, top_at_1, 1, inc_flux=p["inc"])


@pytest.mark.parametrize("top_at_1", [True, False])
def test_lw_reference_is_finite_lit_only_and_not_mostly_zero(orc, lw, top_at_1):
    p = lw
    for what, (up, dn) in _lw_runs(orc, lw, top_at_1):
        assert np.isfinite(up).all() and np.isfinite(dn).all(), what
        for name, a in (("up", up), ("dn", dn)):
            share = _zero_share(a)
            print("LW %s %s top_at_1=%s: share of exact zeros %.3f (cap 0.15)" % (what, name, top_at_1, share))
            assert share <= 0.15, (what, name, share)
    up, dn, gu, gd = orc.lw_solver(p["tau"], p["lay"], p["lev"], p["emis"], p["sfc"], top_at_1, 3, inc_flux=p["inc"],
                                   gpt=True)
    c = np.arange(p["ncol"])
    for bb, gp in ((up, gu), (dn, gd)):
        np.testing.assert_array_equal(bb, gp[c, :, p["lit"]])
        unlit = gp.copy()
        unlit[c, :, p["lit"]] = 0
        assert not unlit.any()


def test_lw_census_both_sides_of_tau_thresh_for_every_secant(lw):
    e = lw["edge"]
    taus = np.unique(e["tau"])
    for D in E.lw_secants():
        # the columns that see this secant: all of them for a Gauss secant, the lit lw_Ds value's for the others
        for name, tt in (("gauss", taus), ("lw_Ds", np.unique(e["tau"][e["lw_d"] == D]))):
            if name == "lw_Ds" and D not in E.LW_DS:
                continue
            with np.errstate(over="ignore"):
                t = (tt * F(D)).astype(F)
            below, above = t[t <= E.TAU_THRESH], t[t > E.TAU_THRESH]
            assert below.size and above.size, (D, name)
            # the two products straddle the threshold within a few ulps: the switch itself is exercised
            assert above.min() / below.max() - 1 < 4 * E.FLT_EPS, (D, name, below.max(), above.min())
            # huge optical depths: tau*D beyond 2^126 and overflowed
            assert (t > F(2.0 ** 126)).any(), (D, name)
    assert 100 <= lw["in_domain"].sum() <= lw["ncol"] - 40
    # tau = 1e30 (tau * D below 2^126 for every secant) and tau = 2e38 (beyond it, or inf) are both present, and some of
    # the latter have no level source next to a layer source of order 1 or more: there the quotient (1 - T) / t alone
    # makes the layer's source, so a wrong quotient reaches the flux
    big = ~lw["in_domain"]
    assert (big & ~lw["beyond_2p126"]).sum() >= 20 and lw["beyond_2p126"].sum() >= 20
    dmax, dmin = max(E.lw_secants()), min(E.lw_secants())
    assert F(1e30) * dmax < F(2.0 ** 126) and F(2e38) * dmin > F(2.0 ** 126)
    sharp = np.array([c.lev == 0 and c.src >= 1 for c in lw["cases"]])
    assert (sharp & lw["beyond_2p126"]).sum() >= 4 and (sharp & lw["in_domain"]).sum() >= 50
    assert set(lw["lit"] % 4) == {0, 1, 2, 3} and set(lw["layer"]) == set(range(E.NLAY))
