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

The scattering and fused LW solvers (build_lw_scat, 1224 columns): every reference finite; zeros 0.044-0.051 of the up
and down fluxes together (two-stream without incident flux 0.094; flux_up_Jac below 0.10 outside the emissivity-0
columns, where it is 0 by definition); 0.82-0.87 of the columns change when the edge (ssa, g) gives way to the
background pair (flux_up_Jac 0.65-0.69), 0.82-0.85 when the lit mask bit is flipped; the census of the last test.

The fused SW solvers (build_sw_fused, 1344 columns; {mask} x {aerosol} x {gas g, g = NULL} x both orientations): every
reference and every incremented property finite (the gas tau falls back to the background in the 28 columns where
2e38 + 2e38 would be inf); zero shares all sky up 0.25-0.26, down 0.21, direct 0.48, masked 0.18-0.19 / 0.14-0.15 /
0.43-0.44, clear 0.12 / 0.08 / 0.38-0.39 (caps 0.30 / 0.30 / 0.55); the background cloud triple changes 0.95-0.96 of
the columns without a mask and of the bit-set columns under it, the flipped lit bit 0.58-0.60; census (no mask -
masked): eps branch 313 - 280, k_min clamp 143 - 101, 0 < ssa < 2^-100 136 - 83, tau12 > 0 with tauscat12 < 3 FLT_MIN
328, incremented tau > 1e4 224, tau12 == 0 with the lit bit set 28 and clear 28 (all the case grid holds: 84 columns
have an edge tau of 0, the gas tau is 0 in two thirds of them and the bit halves those); the lit bit set and clear
with every edge tau in at least 42 columns, every edge ssa 40, every mu0 96; classes in_domain / out_of_domain: all sky
1006-1148 / 196-338, clear 1238-1265 / 79-106.
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


# ---- the scattering and fused LW solvers (solver_edges.build_lw_scat) --------------------------------------------------
@pytest.fixture(scope="module")
def scat():
    return E.build_lw_scat()


NMUS = (1, 3)
FUSED = [(nmus, masked, aer, by_band) for nmus in NMUS for masked in (False, True) for aer in (False, True)
         for by_band in (False,)] + [(1, True, False, True), (1, True, True, True)]


def _scat_references(orc, top_at_1):
    """Every reference the GPU file compares with on build_lw_scat(): name -> flux arrays."""
    for n in NMUS:
        yield "1rescl nmus%d" % n, E.ref_rescl(orc, top_at_1, n)
        yield "1rescl_gpt nmus%d" % n, E.ref_rescl(orc, top_at_1, n, gpt=True)
    for with_inc in (True, False):
        for gpt in (False, True):
            yield "2stream inc=%s gpt=%s" % (with_inc, gpt), E.ref_2stream(orc, top_at_1, with_inc, gpt)
    for nmus, masked, aer, by_band in FUSED:
        yield ("fused nmus%d masked=%s aer=%s emis_by_band=%s" % (nmus, masked, aer, by_band),
               E.ref_fused(orc, top_at_1, nmus, masked, aer, by_band)[:4])


def _noscat_fused_references(orc, top_at_1):
    for kind in ("inc", "masked", "clear", "gpt"):
        yield "noscat fused " + kind, E.ref_noscat_fused(orc, top_at_1, 1, kind)[:2 if kind != "gpt" else 4]


def _changed_share(a, b):
    """Share of the columns in which any flux of the lists a and b differs."""
    n = a[0].shape[0]
    diff = np.zeros(n, bool)
    for x, y in zip(a, b):
        diff[E.mismatch_columns(x, y)] = True
    return float(diff.mean())


@pytest.mark.parametrize("top_at_1", [True, False])
def test_lw_scat_references_are_finite_and_not_mostly_zero(orc, scat, top_at_1):
    """Conditions 1 and 2.  The share of exact zeros is taken over the up and down fluxes of a reference together (the
    g-point arrays apart: all but one g-point of them are zero by design).  flux_up_Jac is apart too: a third of the
    columns have emissivity 0 (LW_EMIS), where J = emis * sfc_source_Jac is exactly 0 at every level; its cap holds on
    the other columns."""
    for what, arrs in list(_scat_references(orc, top_at_1)) + list(_noscat_fused_references(orc, top_at_1)):
        for a in arrs:
            assert np.isfinite(a).all(), what
        share = _zero_share(np.concatenate([a.ravel() for a in arrs[:2]]))
        print("%s top_at_1=%s: share of exact zeros %.3f (cap 0.10)" % (what, top_at_1, share))
        assert share <= 0.10, "%s: share of exact zeros %.3f exceeds 0.10" % (what, share)
        if len(arrs) == 4 and "fused" in what and "noscat" not in what:  # the clear set of the dual entry
            share = _zero_share(np.concatenate([a.ravel() for a in arrs[2:]]))
            print("%s clear set: share of exact zeros %.3f (cap 0.10)" % (what, share))
            assert share <= 0.10, "%s clear set: share of exact zeros %.3f exceeds 0.10" % (what, share)
    lit_emis = scat["edge"]["tau"] * 0 + np.array([c.emis for c in scat["cases"]], F)
    for n in NMUS:
        jac = E.ref_rescl_jac(orc, top_at_1, n)
        assert np.isfinite(jac).all()
        assert not jac[lit_emis == 0].any()
        share = _zero_share(jac[lit_emis > 0])
        print("flux_up_Jac nmus%d top_at_1=%s: share of exact zeros %.3f where emis > 0 (cap 0.10)" % (n, top_at_1, share))
        assert share <= 0.10, "flux_up_Jac nmus%d: share of exact zeros %.3f exceeds 0.10" % (n, share)


@pytest.mark.parametrize("top_at_1", [True, False])
def test_lw_scat_broadband_is_the_lit_gpoint(orc, scat, top_at_1):
    """Condition 3: the unlit g-points carry exactly +-0 and the broadband flux is the lit g-point's term bit for bit --
    with three angles and in the two-stream solver the g-point flux itself, with one angle fac * radiance (quirk B-5)."""
    p = scat
    c = np.arange(p["ncol"])
    fac1 = F(2) * F(np.pi) * F(0.5)
    io = E.ref_fused(orc, top_at_1, 3, True, True)[4]
    lay, lev, sfc = E.planck_sources(orc, p, top_at_1)
    for a in (lay, lev):  # a zero Planck fraction leaves the unlit g-points without any source
        a = a.copy()
        a[c, :, p["lit"]] = 0
        assert not a.any()
    runs = [("1rescl nmus1", E.ref_rescl(orc, top_at_1, 1, gpt=True), fac1),
            ("1rescl nmus3", E.ref_rescl(orc, top_at_1, 3, gpt=True), None),
            ("2stream", E.ref_2stream(orc, top_at_1, True, gpt=True), None),
            ("fused masked aer nmus3", orc.lw_solver(io[0], lay, lev, p["emis"], sfc, top_at_1, 3, inc_flux=p["inc"],
                                                     ssa=io[1], g=io[2], gpt=True), None)]
    plain = {"1rescl nmus1": E.ref_rescl(orc, top_at_1, 1), "1rescl nmus3": E.ref_rescl(orc, top_at_1, 3),
             "2stream": E.ref_2stream(orc, top_at_1, True), "fused masked aer nmus3": E.ref_fused(orc, top_at_1, 3, True, True)}
    for what, (up, dn, gu, gd), fac in runs:
        for name, bb, gp, bb_plain in (("up", up, gu, plain[what][0]), ("dn", dn, gd, plain[what][1])):
            term = gp[c, :, p["lit"]]
            np.testing.assert_array_equal(bb, term if fac is None else fac * term, err_msg="%s %s" % (what, name))
            np.testing.assert_array_equal(bb_plain, bb, err_msg="%s %s" % (what, name))
            unlit = gp.copy()
            unlit[c, :, p["lit"]] = 0
            assert not unlit.any(), (what, name)


@pytest.mark.parametrize("top_at_1", [True, False])
def test_lw_scat_edge_operands_show_in_the_fluxes(orc, scat, top_at_1):
    """Condition 4: at least half of the columns change their fluxes when the edge layer's (ssa, g) -- for the fused
    references the edge band operands -- is replaced by the background pair, and when the lit mask bit is flipped."""
    p = scat
    shares = {}
    w, q = E.with_background_pair(p)
    for n in NMUS:
        other = orc.lw_solver(p["tau"], p["lay"], p["lev"], p["emis"], p["sfc"], top_at_1, n, inc_flux=p["inc"], ssa=w, g=q)
        shares["1rescl nmus%d" % n] = _changed_share(E.ref_rescl(orc, top_at_1, n), other)
        import lw_jacobian_ref as J
        other = J.zero_source_flux_up(orc, p["tau"], p["emis"], p["sjac"], top_at_1, n, ssa=w, g=q)
        emis = np.array([c.emis for c in p["cases"]], F) > 0  # with emissivity 0 the Jacobian is 0 whatever the layer
        shares["flux_up_Jac nmus%d (emis > 0)" % n] = _changed_share([E.ref_rescl_jac(orc, top_at_1, n)[emis]], [other[emis]])
    for with_inc in (True, False):
        other = orc.lw_solver_2stream(p["tau"], w, q, p["lev"], p["emis"], p["sfc"], top_at_1, p["inc"] if with_inc else None)
        shares["2stream inc=%s" % with_inc] = _changed_share(E.ref_2stream(orc, top_at_1, with_inc), other)
    wb, gb = E.with_background_pair(p, "ssa_bnd", "g_bnd")
    lay, lev, sfc = E.planck_sources(orc, p, top_at_1)
    for nmus, masked, aer, by_band in FUSED:
        if by_band:
            continue
        ref = E.ref_fused(orc, top_at_1, nmus, masked, aer)
        io = E.fused_props(orc, p, masked, aer, cloud=[p["tau_bnd"], wb, gb])
        other = orc.lw_solver(io[0], lay, lev, p["emis"], sfc, top_at_1, nmus, inc_flux=p["inc"], ssa=io[1], g=io[2])
        name = "fused nmus%d masked=%s aer=%s" % (nmus, masked, aer)
        if masked:  # the edge operands reach the kernel in the columns whose lit bit is set
            lit = p["edge"]["bit"]
            shares[name + " (lit bit set)"] = _changed_share([a[lit] for a in ref[:2]], [a[lit] for a in other])
            io = E.fused_props(orc, p, True, aer, mask=E.flipped_lit_mask(p))
            other = orc.lw_solver(io[0], lay, lev, p["emis"], sfc, top_at_1, nmus, inc_flux=p["inc"], ssa=io[1], g=io[2])
            shares[name + ", lit bit flipped"] = _changed_share(ref[:2], other)
        else:
            shares[name] = _changed_share(ref[:2], other)
    for what, share in shares.items():
        print("%s top_at_1=%s: %.3f of the columns change (at least 0.5)" % (what, top_at_1, share))
    for what, share in shares.items():
        assert share >= 0.5, "%s: only %.3f of the columns change their fluxes" % (what, share)


def test_lw_scat_census_of_the_edge_layers(scat):
    """Condition 5, in float32 with the kernels' operation order: every value-dependent path of rs_layer, l2_layer and
    the in-kernel increments is reached by at least 20 columns."""
    p, e = scat, scat["edge"]
    census = {}
    wb, scale, cn = E.scale_tau(e["ssa"], e["g"])
    with np.errstate(over="ignore"):
        for D in E.rescl_secants():
            t = (e["tau"] * F(D)) * scale
            for name, sel in (("scaleTau != 1", scale != 1), ("scaleTau == 1 (ssa == 0)", e["ssa"] == 0)):
                census["D=%.4f %s, t <= thresh" % (D, name)] = int((sel & (t <= E.TAU_THRESH)).sum())
                census["D=%.4f %s, t > thresh" % (D, name)] = int((sel & (t > E.TAU_THRESH)).sum())
            # the switch itself: the columns built for a pair of THRESH_PAIRS sit one float either side of it
            forced = np.zeros(p["ncol"], bool)
            for w, g in E.THRESH_PAIRS:
                lo, hi = E.tau_at_thresh(D, E.scale_tau(w, g)[1])
                forced |= (e["ssa"] == w) & (e["g"] == g) & ((e["tau"] == lo) | (e["tau"] == hi))
            census["D=%.4f one float below the switch" % D] = int((forced & (t <= E.TAU_THRESH)).sum())
            census["D=%.4f one float above the switch" % D] = int((forced & (t > E.TAU_THRESH)).sum())
    census["Cn == 0"], census["Cn > 0"] = int((cn == 0).sum()), int((cn > 0).sum())
    census["l2: tau <= 1e-8"], census["l2: tau > 1e-8"] = int((e["tau"] <= F(1e-8)).sum()), int((e["tau"] > F(1e-8)).sum())
    k2, emk, em2k = E.l2_terms(e["tau"], e["ssa"], e["g"])
    census["l2: k_min clamp active (w0 == 1)"] = int(((k2 < E.K_MIN) & (e["ssa"] == 1)).sum())
    census["l2: em2k == 0 with emk > 0"] = int(((em2k == 0) & (emk > 0)).sum())
    census["l2: emk == 0"] = int((emk == 0).sum())
    for aer in (False, True):
        with np.errstate(over="ignore"):
            t1 = e["gas_tau"] + e["aer"] if aer else e["gas_tau"]
            tau12, _, _, scat12 = E.inc_2str_gas(t1, e["tau"], e["ssa"], e["g"])
        census["inc_2str aer=%s: max(eps, tauscat12) bites" % aer] = int((scat12 < E.EPS_INC).sum())
        census["inc_2str aer=%s: max(eps, tau12) bites" % aer] = int((tau12 < E.EPS_INC).sum())
        census["inc_2str aer=%s: t1 == 0 with t2 == 0" % aer] = int(((t1 == 0) & (e["tau"] == 0)).sum())
        census["inc_2str aer=%s: t1 == 0 with t2 > 0" % aer] = int(((t1 == 0) & (e["tau"] > 0)).sum())
    census["lit mask bit set"], census["lit mask bit clear"] = int(e["bit"].sum()), int((~e["bit"]).sum())
    census["tau_aer == 0"], census["tau_aer > 0"] = int((e["aer"] == 0).sum()), int((e["aer"] > 0).sum())
    print(census)
    for what, n in census.items():
        # with the aerosol in front t1 is tau_gas + tau_aer, zero in a third of the columns above: 8 where 24 were
        assert n >= (8 if "aer=True" in what else 20), (what, n)
    # the edge values are where the kernels read them
    c = np.arange(p["ncol"])
    b = p["band_of"][p["lit"]]
    for k, kb in (("tau", "tau_bnd"), ("ssa", "ssa_bnd"), ("g", "g_bnd"), ("aer", "tau_aer")):
        np.testing.assert_array_equal(p[kb][c, p["layer"], b], e[k])
    np.testing.assert_array_equal(p["mask"][c, p["layer"], p["lit"]], e["bit"])
    assert not any(w == 1 and g == 1 for w, g in E.SCAT_PAIRS) and len(E.SCAT_PAIRS) == 59
    assert {(float(x.ssa), float(x.g)) for x in p["cases"]} >= {(float(w), float(g)) for w, g in E.SCAT_PAIRS}
    assert set(p["lit"] % 4) == {0, 1, 2, 3} and set(p["layer"]) == set(range(E.NLAY))
    # the three floats around l2_layer's branch, each with its 24 columns
    for t in E.TAUS_1E8:
        assert (e["tau"] == t).sum() >= 20


def test_lw_scat_domain_classes_have_columns(orc, scat):
    """Every class the GPU file compares has at least 20 columns (it asserts so itself; here without a device)."""
    p, e = scat, scat["edge"]
    qs = {"1rescl nmus%d" % n: E.classes(p, e["tau"], E.scale_tau(e["ssa"], e["g"])[1], E.gauss_ds(n)) for n in NMUS}
    for nmus, masked, aer, _ in FUSED:
        ref = E.ref_fused(orc, True, nmus, masked, aer)
        io = ref[4]
        scale = E.scale_tau(E.edge_values(p, io[1]), E.edge_values(p, io[2]))[1]
        qs["fused %d %s %s all" % (nmus, masked, aer)] = E.classes(p, E.edge_values(p, io[0]), scale, E.gauss_ds(nmus))
        qs["fused %d %s %s clr" % (nmus, masked, aer)] = E.classes(p, E.edge_values(p, ref[5]), None, E.gauss_ds(nmus))
    for what, q in qs.items():
        n = (int(q["in_domain"].sum()), int((~q["in_domain"] & ~q["beyond_2p126"]).sum()), int(q["beyond_2p126"].sum()))
        assert min(n) >= 20, (what, n)
        assert not (q["in_domain"] & q["beyond_2p126"]).any()
    q = E.classes(p, e["tau"])
    assert q["in_domain"].sum() >= 20 and (~q["in_domain"]).sum() >= 20
    pl = E.build_lw()
    for kind in ("inc", "masked", "clear"):
        q = E.classes(pl, E.edge_values(pl, E.ref_noscat_fused(orc, True, 1, kind)[2]), None, E.gauss_ds(1))
        n = (int(q["in_domain"].sum()), int((~q["in_domain"] & ~q["beyond_2p126"]).sum()), int(q["beyond_2p126"].sum()))
        assert min(n) >= 20, (kind, n)


# ---- the fused SW solvers (solver_edges.build_sw_fused) -----------------------------------------------------------------
@pytest.fixture(scope="module")
def swf():
    return E.build_sw_fused()


SW_SETS = [(masked, aer, with_g) for masked in (False, True) for aer in (False, True) for with_g in (True, False)]


def _lit_only(p, flux, what):
    """flux: (up, dn, dir, gpt_up, gpt_dn, gpt_dir).  The broadband flux is the lit g-point's, the others are +-0."""
    c = np.arange(p["ncol"])
    for name, bb, gp in zip(("up", "dn", "dir"), flux[:3], flux[3:]):
        np.testing.assert_array_equal(bb, gp[c, :, p["lit"]], err_msg="%s %s" % (what, name))
        unlit = gp.copy()
        unlit[c, :, p["lit"]] = 0
        assert not unlit.any(), (what, name)


@pytest.mark.parametrize("top_at_1", [True, False])
def test_sw_fused_references_are_finite_lit_only_and_not_mostly_zero(orc, swf, top_at_1):
    """Finite everywhere ({mask} x {aerosol} x {gas g, g = NULL}, the all-sky and the clear sets, the incremented
    properties); zero shares up <= 0.30, down <= 0.30, direct <= 0.55; the broadband flux is the lit g-point's flux bit for
    bit and every unlit g-point is exactly zero, under the mask and with the aerosol too."""
    p = swf
    for masked, aer, with_g in SW_SETS:
        allsky, clear, io, clr = E.ref_sw_fused(orc, top_at_1, masked, aer, with_g, gpt=True)
        plain = E.ref_sw_fused(orc, top_at_1, masked, aer, with_g)
        what = "masked=%s aer=%s g=%s top_at_1=%s" % (masked, aer, with_g, top_at_1)
        for a in allsky + clear + tuple(io) + tuple(clr) + plain[0] + plain[1]:
            assert np.isfinite(a).all(), what
        for name, flux, flux_plain in (("all sky", allsky, plain[0]), ("clear", clear, plain[1])):
            _lit_only(p, flux, what + " " + name)
            for x, y in zip(flux[:3], flux_plain):
                np.testing.assert_array_equal(x, y, err_msg=what + " " + name)
            shares = [_zero_share(a) for a in flux[:3]]
            print("SW fused %s %s: share of exact zeros up %.3f down %.3f direct %.3f (caps 0.30 0.30 0.55)"
                  % (what, name, *shares))
            for s, cap in zip(shares, (0.30, 0.30, 0.55)):
                assert s <= cap, (what, name, shares)


def _changed(a, b, cols=None):
    n = a[0].shape[0]
    diff = np.zeros(n, bool)
    for x, y in zip(a, b):
        diff[E.mismatch_columns(x, y)] = True
    return float(diff.mean() if cols is None else diff[cols].mean())


@pytest.mark.parametrize("top_at_1", [True, False])
def test_sw_fused_edge_operands_show_in_the_fluxes(orc, swf, top_at_1):
    """The edge cloud triple gives way to the background triple: at least 0.8 of the columns change without a mask, at
    least 0.8 of the bit-set columns under it; the lit bit flipped: at least 0.5 of the columns."""
    p = swf
    bit = p["edge"]["bit"]
    bg = E.with_background_cloud(p)
    shares = {}
    for aer in (False, True):
        for with_g in (True, False):
            t = "aer=%s g=%s" % (aer, with_g)
            ref = E.ref_sw_fused(orc, top_at_1, False, aer, with_g)[0]
            other = E.sw_fused_solve(orc, p, E.sw_fused_props(orc, p, False, aer, with_g, cloud=bg)[0], top_at_1)
            shares["background cloud, no mask, " + t] = (_changed(ref, other), 0.8)
            ref = E.ref_sw_fused(orc, top_at_1, True, aer, with_g)[0]
            other = E.sw_fused_solve(orc, p, E.sw_fused_props(orc, p, True, aer, with_g, cloud=bg)[0], top_at_1)
            shares["background cloud, masked, bit-set columns, " + t] = (_changed(ref, other, bit), 0.8)
            assert _changed(ref, other, ~bit) == 0  # a clear bit switches either triple off
            other = E.sw_fused_solve(orc, p, E.sw_fused_props(orc, p, True, aer, with_g, mask=E.flipped_lit_mask(p))[0],
                                     top_at_1)
            shares["lit bit flipped, " + t] = (_changed(ref, other), 0.5)
    for what, (share, least) in shares.items():
        print("SW fused top_at_1=%s %s: %.3f of the columns change (at least %.1f)" % (top_at_1, what, share, least))
    for what, (share, least) in shares.items():
        assert share >= least, "%s: only %.3f of the columns change their fluxes" % (what, share)


def test_sw_fused_census_of_the_incremented_edge_operands(orc, swf):
    """In float32, from the oracle's incremented properties at (edge layer, lit g-point), gas g present: every
    value-dependent path of sw_two_stream and of the band increment is reached by at least 50 columns, without and under
    the mask.  The two rows on tau12 == 0 are bounded by the case grid itself: tau12 = tau_gas + tau_cloud is zero only
    in the 84 columns whose edge tau is 0, the gas tau is 0 in two thirds of them (the cycle {0, background, edge}) and
    the lit bit halves those: 28 and 28, which is what they must hold."""
    p, e = swf, swf["edge"]
    census = {}
    for masked in (False, True):
        io = E.ref_sw_fused(orc, True, masked, False, True)[2]
        t, w, q = (E.edge_values(p, a) for a in io)
        tag = "masked" if masked else "no mask"
        census["eps branch, " + tag] = int(E.in_eps_branch(w, q, e["mu0"]).sum())
        census["k_min clamp, " + tag] = int((E.sw_k(w, q)[1] < E.K_MIN).sum())
        census["0 < ssa < 2^-100, " + tag] = int(((w > 0) & (w < F(2.0 ** -100))).sum())
    with np.errstate(over="ignore", under="ignore"):
        tau12 = e["gas_tau"] + e["tau"]
        scat12 = e["gas_tau"] * e["gas_ssa"] + e["tau"] * e["ssa"]
    grid = {"tau12 == 0, bit set": int(((tau12 == 0) & e["bit"]).sum()),
            "tau12 == 0, bit clear": int(((tau12 == 0) & ~e["bit"]).sum())}
    census["tau12 > 0 and tauscat12 < 3 FLT_MIN"] = int(((tau12 > 0) & (scat12 < E.EPS_INC)).sum())
    census["incremented tau > 1e4"] = int((E.edge_values(p, E.ref_sw_fused(orc, True, False, False, True)[2][0]) > F(1e4)).sum())
    print(census, grid)
    for what, n in census.items():
        assert n >= 50, (what, n)
    assert grid == {"tau12 == 0, bit set": 28, "tau12 == 0, bit clear": 28}
    # the lit bit is spread over every edge tau, edge ssa and mu0
    spread = {}
    for k in ("tau", "ssa", "mu0"):
        vals = np.unique(e[k])
        spread[k] = min(min(int(((e[k] == v) & e["bit"]).sum()), int(((e[k] == v) & ~e["bit"]).sum())) for v in vals)
    print("least columns of one edge value with the lit bit set / clear:", spread)
    assert set(np.unique(e["tau"])) == set(E.TAUS) and set(np.unique(e["ssa"])) >= set(E.SSAS)  # + the resonant 0.3
    for k, n in spread.items():
        assert n >= 20, (k, n)
    assert abs(int(e["bit"].sum()) - p["ncol"] // 2) <= 24
    # gas tau and gas ssa cycle independently: all nine pairings of {0, background, edge}
    kt = np.select([e["gas_tau"] == 0, e["gas_tau"] == E.BG_TAU], [0, 1], 2)
    kw = np.select([e["gas_ssa"] == 0, e["gas_ssa"] == E.BG_SSA], [0, 1], 2)
    pairs = np.bincount(3 * kt + kw, minlength=9)
    print("gas (tau, ssa) pairings:", pairs)
    assert pairs.min() >= 50
    # the edge values are where the kernels read them
    c, b = np.arange(p["ncol"]), p["band_of"][p["lit"]]
    for k, kb in (("tau", "tau_bnd"), ("ssa", "ssa_bnd"), ("g", "g_bnd")):
        np.testing.assert_array_equal(p[kb][c, p["layer"], b], e[k])
    for k in ("tau", "ssa", "g"):
        np.testing.assert_array_equal(E.edge_values(p, p[k]), e["gas_" + k])
    np.testing.assert_array_equal(E.edge_values(p, p["mask"]), e["bit"])
    with np.errstate(over="ignore"):
        assert np.isfinite(e["gas_tau"] + e["tau"]).all()
    assert (p["lims"][:, 0] % 2 == 1).all() and p["nb"] == 14  # the band-pair layout


def test_sw_fused_domain_classes_have_columns(orc, swf):
    """Every class the GPU file compares holds at least 20 columns (it asserts so itself; here without a device), and the
    tiled problem repeats the columns."""
    p = swf
    for masked, aer, with_g in SW_SETS:
        _, _, io, clr = E.ref_sw_fused(orc, True, masked, aer, with_g)
        for name, props in (("all sky", io), ("clear", clr)):
            q = E.classes_sw_of(p, props)
            n = (int(q["in_domain"].sum()), int((~q["in_domain"]).sum()))
            print("SW fused masked=%s aer=%s g=%s %s: in_domain %d, out_of_domain %d" % (masked, aer, with_g, name, *n))
            assert min(n) >= 20, (masked, aer, with_g, name, n)
    t = E.tile(p, 2)
    assert t["ncol"] == 2 * p["ncol"] and t["tau"].shape[0] == t["ncol"] and t["lims"].shape == p["lims"].shape
    np.testing.assert_array_equal(t["tau_bnd"][p["ncol"]:], p["tau_bnd"])
    np.testing.assert_array_equal(t["mask"][:p["ncol"]], p["mask"])
