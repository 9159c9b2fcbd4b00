"""GPU: clear-sky and all-sky fluxes from one call (extensions/mo_rrtmgp_clr_all_sky.F90), bit for bit:

* rrtmgpnn_lw_solver_noscat_planck_clr_all -- the dual kernel (one read of tau, pfrac and the band cloud tau, two
  radiances per lane) and its two-launch form -- against the oracle and against the _planck / _planck_inc entries;
* rrtmgpnn.clr_all_sky.rte_lw / rte_sw, the dual path and every fallback, against the oracle;
* ClearSkyStep(clouds=..., clrsky=True), eager and captured, fused and unfused.
"""
import numpy as np
import pytest

import clr_all_sky_ref as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a device"
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def T(a, dev):
    return torch.as_tensor(np.array(a, dtype=np.float32, order="C", copy=True), device=dev)


def nan(dev, *shape):
    return torch.full(shape, float("nan"), device=dev)


@pytest.fixture
def clr_all_mode():
    """Set the clear + all-sky LW mode of the library for one test, then restore the default."""
    from rrtmgpnn import api
    yield api.set_lw_clr_all_default
    api.set_lw_clr_all_default(0)


def _device_case(case, dev):
    return {k: T(case[k], dev) for k in ("tau", "pfrac", "cld", "emis", "emis_band", "inc_flux")} | {
        "tlay": T(case["prob"]["tlay"], dev), "tlev": T(case["tlev"], dev), "tsfc": T(case["prob"]["tsfc"], dev),
        "totplnk": T(case["kd"]["totplnk"], dev)}


def _solve(entry, case, d, dev, top_at_1, nmus=1, inc=False, emis_by_band=False):
    """One of the three entries on the case's arrays: 'clr_all' -> (up, dn, up_clr, dn_clr), 'planck' / 'planck_inc'
    -> (up, dn); outputs pre-filled with nan."""
    from rrtmgpnn import _lib
    from rrtmgpnn._lib import check, float_array, int_array
    from rrtmgpnn.api import GAUSS_DS, GAUSS_WTS, context
    L = _lib.lib()
    kd = case["kd"]
    ncol, nlay, ngpt = case["tau"].shape
    P = lambda t: t.data_ptr()  # noqa: E731
    head = (context(0).h, ngpt, nlay, ncol, int(top_at_1), nmus, float_array(GAUSS_DS[nmus]),
            float_array(GAUSS_WTS[nmus]), P(d["inc_flux"]) if inc else None)
    tail = (kd["nband"], kd["nPlanckTemp"], P(d["tlay"]), P(d["tlev"]), P(d["tsfc"]), case["sfc_lay"],
            int_array(np.asarray(case["lims"]).ravel()), float(kd["temp_ref_min"][0]), float(kd["totplnk_delta"]),
            P(d["totplnk"]), int(emis_by_band), P(d["emis_band"] if emis_by_band else d["emis"]))
    outs = [nan(dev, ncol, nlay + 1) for _ in range(4 if entry == "clr_all" else 2)]
    if entry == "clr_all":
        rc = L.rrtmgpnn_lw_solver_noscat_planck_clr_all(*head, P(d["tau"]), P(d["cld"]), P(d["pfrac"]), *tail,
                                                        *[P(o) for o in outs])
    elif entry == "planck_inc":
        rc = L.rrtmgpnn_lw_solver_noscat_planck_inc(*head, P(d["tau"]), P(d["cld"]), P(d["pfrac"]), *tail,
                                                    *[P(o) for o in outs])
    else:
        rc = L.rrtmgpnn_lw_solver_noscat_planck(*head, P(d["tau"]), P(d["pfrac"]), *tail, *[P(o) for o in outs])
    check(rc, entry)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs]


@pytest.mark.parametrize("nlay", R.NLAYS)
@pytest.mark.parametrize("top_at_1", [True, False])
def test_dual_entry_matches_oracle(dev, orc, clr_all_mode, nlay, top_at_1):
    """The dual kernel on synthetic columns of 1 to 65 layers (below its prefetch depth, at and around its ring of 4 and
    the single kernels' ring of 8, several chunks) in both orientations: the all-sky set is the oracle's solve of
    increment_bybnd(tau, cloud tau), the clear set its solve of tau.  The two sets differ in at least a third of the columns (asserted on the oracle alone)
    and are equal in the cloud-free ones."""
    case = R.solver_case(orc, nlay, top_at_1)
    differ = R.sets_differ(case)
    assert differ.sum() * 3 >= R.NCOL, "the inputs do not tell the two flux sets apart"
    assert not differ[~case["cloudy"]].any()
    (up_a, dn_a), (up_c, dn_c) = case["want"]["plain", 1]
    clr_all_mode(1)
    up, dn, upc, dnc = _solve("clr_all", case, _device_case(case, dev), dev, top_at_1)
    np.testing.assert_array_equal(up, up_a)
    np.testing.assert_array_equal(dn, dn_a)
    np.testing.assert_array_equal(upc, up_c)
    np.testing.assert_array_equal(dnc, dn_c)
    clear = ~case["cloudy"]
    assert clear.any()
    np.testing.assert_array_equal(up[clear], upc[clear])
    np.testing.assert_array_equal(dn[clear], dnc[clear])


def _modes_equal(dev, orc, clr_all_mode, case, top_at_1, key, **kw):
    d = _device_case(case, dev)
    before = d["tau"].clone(), d["pfrac"].clone()
    sep = _solve("planck_inc", case, d, dev, top_at_1, **kw) + _solve("planck", case, d, dev, top_at_1, **kw)
    for mode in (1, 2, 0):
        clr_all_mode(mode)
        got = _solve("clr_all", case, d, dev, top_at_1, **kw)
        for g, s in zip(got, sep):
            np.testing.assert_array_equal(g, s, err_msg="mode %d" % mode)
    assert torch.equal(d["tau"], before[0]) and torch.equal(d["pfrac"], before[1])
    if key is not None:
        (up_a, dn_a), (up_c, dn_c) = case["want"][key]
        for g, w in zip(sep, (up_a, dn_a, up_c, dn_c)):
            np.testing.assert_array_equal(g, w)


@pytest.mark.parametrize("nmus", [1, 2, 3, 4])
@pytest.mark.parametrize("top_at_1", [True, False])
def test_modes_equal_each_angle_count(dev, orc, clr_all_mode, nmus, top_at_1):
    """Mode 1 (dual) == mode 2 (two launches) == mode 0 == the _planck and _planck_inc entries called separately, and
    the oracle, for 1 to 4 angles (several angles always take the two existing kernels); tau and pfrac unchanged."""
    _modes_equal(dev, orc, clr_all_mode, R.solver_case(orc, 17, top_at_1), top_at_1, ("plain", nmus), nmus=nmus)


@pytest.mark.parametrize("emis_by_band", [False, True])
@pytest.mark.parametrize("inc", [False, True])
def test_modes_equal_inc_flux_and_emissivity(dev, orc, clr_all_mode, inc, emis_by_band):
    """The same equalities with an incident flux and with the emissivity by band or by g-point."""
    case = R.solver_case(orc, 9, True)
    _modes_equal(dev, orc, clr_all_mode, case, True, ("inc" if inc else "plain", 1), inc=inc,
                 emis_by_band=emis_by_band)


@pytest.mark.parametrize("nlay", [3, 4, 7, 9])
@pytest.mark.parametrize("top_at_1", [True, False])
def test_modes_equal_ngpt_not_multiple_of_4(dev, orc, clr_all_mode, nlay, top_at_1):
    """254 g-points (the k-distribution cut short, the last band ending at 254): the broadband sums are plain
    sequential sums of the radiances (quirk B-5), for both flux sets."""
    case = R.solver_case(orc, nlay, top_at_1, ngpt=254)
    assert R.sets_differ(case).sum() * 3 >= R.NCOL
    _modes_equal(dev, orc, clr_all_mode, case, top_at_1, ("plain", 1))


def test_byband_request_is_refused_and_cleared(dev, orc, clr_all_mode):
    """A by-band request armed before the entry: the argument error with a last_error text, the outputs untouched, and
    the next plain solver call runs without by-band output."""
    from rrtmgpnn import _lib
    from rrtmgpnn._lib import check, float_array, int_array
    from rrtmgpnn.api import GAUSS_DS, GAUSS_WTS, context
    L = _lib.lib()
    case = R.solver_case(orc, 9, True)
    d = _device_case(case, dev)
    kd = case["kd"]
    ncol, nlay, ngpt = case["tau"].shape
    lims = int_array(np.asarray(case["lims"]).ravel())
    bnd = [nan(dev, ncol, nlay + 1, kd["nband"]) for _ in range(2)]
    check(L.rrtmgpnn_solver_request_byband(context(0).h, kd["nband"], lims, bnd[0].data_ptr(), bnd[1].data_ptr(),
                                           None), "solver_request_byband")
    P = lambda t: t.data_ptr()  # noqa: E731
    outs = [nan(dev, ncol, nlay + 1) for _ in range(4)]
    rc = L.rrtmgpnn_lw_solver_noscat_planck_clr_all(
        context(0).h, ngpt, nlay, ncol, 1, 1, float_array(GAUSS_DS[1]), float_array(GAUSS_WTS[1]), None, P(d["tau"]),
        P(d["cld"]), P(d["pfrac"]), kd["nband"], kd["nPlanckTemp"], P(d["tlay"]), P(d["tlev"]), P(d["tsfc"]),
        case["sfc_lay"], lims, float(kd["temp_ref_min"][0]), float(kd["totplnk_delta"]), P(d["totplnk"]), 0,
        P(d["emis"]), *[P(o) for o in outs])
    assert rc == 1  # RRTMGPNN_ERR_ARGUMENT
    assert b"by-band" in L.rrtmgpnn_last_error()
    torch.cuda.synchronize()
    assert all(torch.isnan(o).all() for o in outs)
    up, dn = _solve("planck", case, d, dev, True)
    (_, _), (up_c, dn_c) = case["want"]["plain", 1]
    np.testing.assert_array_equal(up, up_c)
    np.testing.assert_array_equal(dn, dn_c)
    assert all(torch.isnan(b).all() for b in bnd), "the refused request was still armed"


# ---------------------------------------------------------------------------------------------
# The class layer (rrtmgpnn.clr_all_sky) and the step on 20 RFMIP columns
def _rfmip20(rfmip):
    from conftest import subset
    return subset(rfmip, np.arange(5, 1800, 90))


def _oracle20(orc, rfmip):
    """The oracle's clear and all-sky results on the 20 columns, once per session."""
    def make():
        from rrtmgpnn import data
        prob = _rfmip20(rfmip)
        m = {k: data.load_model(k) for k in ("lw_abs", "lw_pfrac", "sw_abs", "sw_ray")}
        kl, ks = data.load_kdist("lw"), data.load_kdist("sw")
        co_lw, co_sw = data.load_cloud_optics("lw"), data.load_cloud_optics("sw")
        clouds = data.allsky_clouds(prob, co_lw)
        out = dict(prob=prob, clouds=clouds, kl=kl, ks=ks)
        lw, sw = [m["lw_abs"], m["lw_pfrac"]], [m["sw_abs"], m["sw_ray"]]
        out["lw_clr"] = orc.clear_sky_lw(prob, lw, kl)
        out["lw_all"] = orc.all_sky_lw(prob, lw, kl, co_lw, clouds)
        for z in (True, False):
            out["sw_clr", z] = orc.clear_sky_sw(prob, sw, ks, zero_unused=z)
            out["sw_all", z] = orc.all_sky_sw(prob, sw, ks, co_sw, clouds, zero_unused=z)
        # 2str clouds in the LW: the rescaled solver on gas optics with ssa = g = 0, then on the incremented set
        go = out["lw_clr"][2]
        ngpt = go["tau"].shape[-1]
        emis = np.repeat(np.asarray(prob["sfc_emis"], np.float32)[:, None], ngpt, axis=1)
        cld2 = orc.cloud_optics(co_lw, *clouds, nstr=2, icergh=2)
        z0 = np.zeros_like(go["tau"])
        src = (go["lay_source"], go["lev_source"], emis, go["sfc_source"], prob["top_at_1"], 1)
        inc2 = orc.increment_bybnd(kl["band_lims_gpt"], (go["tau"], z0, z0), cld2)
        out["lw2_clr"] = orc.lw_solver(go["tau"], *src, ssa=z0, g=z0)
        out["lw2_all"] = orc.lw_solver(inc2[0], *src, ssa=inc2[1], g=inc2[2])
        out["cld2"] = cld2
        differ = (out["lw_clr"][1] != out["lw_all"][1]).any(axis=1)
        assert differ.sum() * 3 >= prob["ncol"]
        return out
    return R.cached("rfmip20", make)


def _class_setup(dev, which, prob):
    from rrtmgpnn import api, data
    kd = api.GasOpticsRRTMGP()
    api.stop_on_err(kd.load(which))
    names = ("lw_abs", "lw_pfrac") if which == "lw" else ("sw_abs", "sw_ray")
    nets = [api.RrtmgpNetwork(0).load_netcdf(data.path(n)) for n in names]
    gc = api.GasConcs()
    api.stop_on_err(gc.init(list(prob["gases"])))
    for k, v in prob["gases"].items():
        api.stop_on_err(gc.set_vmr(k, T(v, dev)))
    state = [T(prob[k], dev) for k in ("play", "tlay", "plev")]
    return kd, nets, gc, state


def _cloud_props(api, kd, arrays, dev, gpt=False):
    """Cloud properties holding `arrays` ((tau,) or (tau, ssa, g), by band); gpt: expanded to kd's g-points."""
    ncol, nlay, _ = arrays[0].shape
    p = api.OpticalProps1scl() if len(arrays) == 1 else api.OpticalProps2str()
    assert p.init(kd.get_band_lims_wavenumber(), kd.get_band_lims_gpoint() if gpt else None) == ""
    assert (p.alloc_1scl if len(arrays) == 1 else p.alloc_2str)(ncol, nlay, device=dev) == ""
    band = kd.get_gpoint_bands() - 1
    for t, a in zip([p.tau] if len(arrays) == 1 else [p.tau, p.ssa, p.g], arrays):
        t.copy_(T(a[..., band] if gpt else a, dev))
    return p


def _bb(api, dev, ncol, nlev, beam=False):
    return api.FluxesBroadband(flux_up=nan(dev, ncol, nlev), flux_dn=nan(dev, ncol, nlev),
                               flux_dn_dir=nan(dev, ncol, nlev) if beam else None)


@pytest.mark.parametrize("case", ["dual", "dual_tlev_interpolated", "gpoint_clouds", "2str_clouds", "byband_clear",
                                  "byband_all"])
def test_class_rte_lw_matches_oracle(dev, orc, rfmip, case):
    """clr_all_sky.rte_lw: the dual path and each fallback (clouds on g-points, 2str clouds, a FluxesByBand as either
    flux object) against the oracle."""
    from rrtmgpnn import api, clr_all_sky, data
    o = _oracle20(orc, rfmip)
    prob = o["prob"]
    ncol, nlay = prob["ncol"], prob["nlay"]
    kd, nets, gc, (play, tlay, plev) = _class_setup(dev, "lw", prob)
    nb = kd.get_nband()
    emis = T(np.repeat(np.asarray(prob["sfc_emis"], np.float32)[:, None], nb, axis=1), dev)
    cld1 = o["lw_all"][2]["clouds"]
    if case == "2str_clouds":
        clouds = _cloud_props(api, kd, o["cld2"], dev)
        want_clr, want_all = o["lw2_clr"], o["lw2_all"]
    else:
        clouds = _cloud_props(api, kd, cld1, dev, gpt=case == "gpoint_clouds")
        want_clr, want_all = o["lw_clr"][:2], o["lw_all"][:2]
    f_all, f_clr = _bb(api, dev, ncol, nlay + 1), _bb(api, dev, ncol, nlay + 1)
    if case.startswith("byband"):
        fb = api.FluxesByBand(bnd_flux_up=nan(dev, ncol, nlay + 1, nb), bnd_flux_dn=nan(dev, ncol, nlay + 1, nb),
                              flux_up=nan(dev, ncol, nlay + 1), flux_dn=nan(dev, ncol, nlay + 1))
        if case == "byband_clear":
            f_clr = fb
        else:
            f_all = fb
    tlev = None if case == "dual_tlev_interpolated" else T(prob["tlev"], dev)
    if tlev is None:
        m = [data.load_model("lw_abs"), data.load_model("lw_pfrac")]
        go = orc.lw_gas_optics(prob, m, o["kl"], tlev=False)
        ngpt = go["tau"].shape[-1]
        e_g = np.repeat(np.asarray(prob["sfc_emis"], np.float32)[:, None], ngpt, axis=1)
        src = (go["lay_source"], go["lev_source"], e_g, go["sfc_source"], prob["top_at_1"], 1)
        (tau_all,) = orc.increment_bybnd(o["kl"]["band_lims_gpt"], (go["tau"],), cld1)
        want_clr, want_all = orc.lw_solver(go["tau"], *src), orc.lw_solver(tau_all, *src)
    assert clr_all_sky.rte_lw(kd, gc, play, tlay, plev, T(prob["tsfc"], dev), emis, clouds, f_all, f_clr,
                              t_lev=tlev, neural_nets=nets) == ""
    torch.cuda.synchronize()
    np.testing.assert_array_equal(f_clr.flux_up.cpu().numpy(), want_clr[0])
    np.testing.assert_array_equal(f_clr.flux_dn.cpu().numpy(), want_clr[1])
    np.testing.assert_array_equal(f_all.flux_up.cpu().numpy(), want_all[0])
    np.testing.assert_array_equal(f_all.flux_dn.cpu().numpy(), want_all[1])
    if case.startswith("byband"):
        # the by-band arrays against api.rte_lw on hand-assembled gas optics (+ increment)
        op, src = api.OpticalProps1scl(), api.SourceFuncLW()
        assert op.alloc_1scl(ncol, nlay, kd, device=dev) == "" and src.alloc(ncol, nlay, kd, device=dev) == ""
        assert kd.gas_optics(play, plev, tlay, T(prob["tsfc"], dev), gc, op, src, tlev=tlev, neural_nets=nets) == ""
        if case == "byband_all":
            assert clouds.increment(op) == ""
        ref = api.FluxesByBand(bnd_flux_up=nan(dev, ncol, nlay + 1, nb), bnd_flux_dn=nan(dev, ncol, nlay + 1, nb),
                               flux_up=nan(dev, ncol, nlay + 1), flux_dn=nan(dev, ncol, nlay + 1))
        assert api.rte_lw(op, prob["top_at_1"], src, emis, ref) == ""
        torch.cuda.synchronize()
        assert torch.equal(fb.bnd_flux_up, ref.bnd_flux_up) and torch.equal(fb.bnd_flux_dn, ref.bnd_flux_dn)
        assert not torch.isnan(fb.bnd_flux_up).any()


def test_class_rte_sw_matches_oracle(dev, orc, rfmip):
    """clr_all_sky.rte_sw (always two solves) with delta-scaled 2str clouds by band against the oracle, on every column
    (night columns are solved with mu0 = 1, as the driver does)."""
    from rrtmgpnn import api, clr_all_sky, data
    o = _oracle20(orc, rfmip)
    prob = o["prob"]
    ncol, nlay = prob["ncol"], prob["nlay"]
    kd, nets, gc, (play, tlay, plev) = _class_setup(dev, "sw", prob)
    clouds = _cloud_props(api, kd, o["sw_all", False][3]["clouds"], dev)
    alb = T(np.repeat(np.asarray(prob["sfc_alb"], np.float32)[:, None], kd.get_nband(), axis=1), dev)
    f_all, f_clr = _bb(api, dev, ncol, nlay + 1, True), _bb(api, dev, ncol, nlay + 1, True)
    assert clr_all_sky.rte_sw(kd, gc, play, tlay, plev, T(prob["mu0"], dev), alb, alb, clouds, f_all, f_clr,
                              inc_flux=T(data.toa_flux(prob, o["ks"]), dev), neural_nets=nets) == ""
    torch.cuda.synchronize()
    for f, key in ((f_clr, "sw_clr"), (f_all, "sw_all")):
        up, dn, dr = o[key, False][:3]
        np.testing.assert_array_equal(f.flux_up.cpu().numpy(), up, err_msg=key)
        np.testing.assert_array_equal(f.flux_dn.cpu().numpy(), dn, err_msg=key)
        np.testing.assert_array_equal(f.flux_dn_dir.cpu().numpy(), dr, err_msg=key)


def test_class_error_strings(dev, orc, rfmip):
    """The reference's messages for mis-sized t_lev, inc_flux and aer_props, and inc_flux with tsi_scaling."""
    from rrtmgpnn import api, clr_all_sky
    o = _oracle20(orc, rfmip)
    prob = o["prob"]
    ncol, nlay = prob["ncol"], prob["nlay"]
    kd, nets, gc, (play, tlay, plev) = _class_setup(dev, "lw", prob)
    clouds = _cloud_props(api, kd, o["lw_all"][2]["clouds"], dev)
    emis = torch.ones((ncol, kd.get_nband()), device=dev)
    fl = lambda: _bb(api, dev, ncol, nlay + 1)  # noqa: E731
    lw = lambda **kw: clr_all_sky.rte_lw(kd, gc, play, tlay, plev, T(prob["tsfc"], dev), emis, clouds, fl(), fl(),  # noqa: E731
                                         neural_nets=nets, **kw)
    assert lw(t_lev=torch.zeros((ncol, nlay), device=dev)) == "rrtmpg_lw: t_lev inconsistently sized"
    assert lw(inc_flux=torch.zeros((ncol, 3), device=dev)) == "rrtmpg_lw: incident flux inconsistently sized"
    aer = api.OpticalProps1scl()
    assert aer.alloc_1scl(ncol, nlay - 1, kd, device=dev) == ""
    assert lw(aer_props=aer) == "rrtmpg_lw: aerosol properties inconsistently sized"
    ks, nets_s, gcs, _ = _class_setup(dev, "sw", prob)
    c2 = _cloud_props(api, ks, o["sw_all", False][3]["clouds"], dev)
    alb = torch.zeros((ncol, ks.get_nband()), device=dev)
    sw = lambda **kw: clr_all_sky.rte_sw(ks, gcs, play, tlay, plev, T(prob["mu0"], dev), alb, alb, c2, fl(), fl(),  # noqa: E731
                                         neural_nets=nets_s, **kw)
    assert sw(inc_flux=torch.zeros((ncol, ks.get_ngpt()), device=dev), tsi_scaling=1.0) == \
        "rrtmpg_sw: only one of inc_flux, tsi_scaling may be supplied."
    assert sw(inc_flux=torch.zeros((ncol, 3), device=dev)) == "rrtmpg_sw: incident flux inconsistently sized"
    assert sw(tsi_scaling=-1.0) == "rrtmpg_sw: tsi_scaling is < 0"
    aer2 = api.OpticalProps2str()
    assert aer2.alloc_2str(ncol + 1, nlay, ks, device=dev) == ""
    assert sw(aer_props=aer2) == "rrtmpg_sw: aerosol properties inconsistently sized"


def _step_outputs(step):
    torch.cuda.synchronize()
    out = dict(step.fluxes())
    if step.clrsky:
        out.update(step.clrsky_fluxes())
    return out


@pytest.mark.parametrize("fused", [True, False])
def test_step_clrsky(dev, orc, rfmip, fused):
    """ClearSkyStep(clouds, clrsky=True): its all-sky outputs are the step's without the flag, its clear outputs a
    cloud-free step's and the oracle's (SW night columns zeroed / left out as the driver's output step does); eager ==
    captured."""
    from rrtmgpnn.pipeline import ClearSkyStep
    o = _oracle20(orc, rfmip)
    prob, clouds = o["prob"], o["clouds"]
    step = ClearSkyStep(prob, device=0, fused=fused, clouds=clouds, clrsky=True)
    for k in ("lw_up", "lw_dn", "sw_up", "sw_dn", "sw_dir"):
        getattr(step, k).fill_(float("nan"))
        getattr(step, k + "_clr").fill_(float("nan"))
    step.step()
    got = _step_outputs(step)
    plain = ClearSkyStep(prob, device=0, fused=fused, clouds=clouds)
    plain.step()
    clear = ClearSkyStep(prob, device=0, fused=fused)
    clear.step()
    a, c = _step_outputs(plain), _step_outputs(clear)
    for k in a:
        np.testing.assert_array_equal(got[k], a[k], err_msg=k)
        np.testing.assert_array_equal(got[k + "_clr"], c[k], err_msg=k + "_clr")
    use = prob["usecol"]
    assert (~use).any() and use.any()
    for sfx, lw, sw in (("", o["lw_all"], o["sw_all", True]), ("_clr", o["lw_clr"], o["sw_clr", True])):
        np.testing.assert_array_equal(got["lw_up" + sfx], lw[0])
        np.testing.assert_array_equal(got["lw_dn" + sfx], lw[1])
        for k, r in (("sw_up", sw[0]), ("sw_dn", sw[1])):
            g = got[k + sfx].copy()
            g[~use] = 0.0
            np.testing.assert_array_equal(g, r, err_msg=k + sfx)
        np.testing.assert_array_equal(got["sw_dir" + sfx][use], sw[2][use])
    # the flag adds the clear solver calls and nothing else (unfused, the LW increment moves behind the clear solver)
    kept = [n for n, _, _ in step.calls if not n.endswith("_clr")]
    assert sorted(kept) == sorted(n for n, _, _ in plain.calls)
    if fused:
        assert kept == [n for n, _, _ in plain.calls]
        assert [n for n, _, _ in step.calls if n.endswith("_clr")] == ["sw_solver_clr"]
    else:
        names = [n for n, _, _ in step.calls]
        assert names.index("lw_solver_clr") < names.index("increment_lw") < names.index("lw_solver")
        assert names.index("sw_solver_clr") < names.index("increment_sw") < names.index("sw_solver")
    step.capture()
    for k in got:
        getattr(step, k).fill_(float("nan"))
    step.replay()
    rep = _step_outputs(step)
    for k in got:
        np.testing.assert_array_equal(rep[k], got[k], err_msg="replay " + k)
    for s in (step, plain, clear):
        s.close()


def test_step_clrsky_fused_equals_unfused_and_refusals(dev, orc, rfmip):
    from rrtmgpnn.pipeline import ClearSkyStep
    o = _oracle20(orc, rfmip)
    outs = []
    for fused in (True, False):
        st = ClearSkyStep(o["prob"], device=0, fused=fused, clouds=o["clouds"], clrsky=True, overlap=fused)
        st.step()
        outs.append(_step_outputs(st))
        st.close()
    for k in outs[0]:
        np.testing.assert_array_equal(outs[0][k], outs[1][k], err_msg=k)
    with pytest.raises(ValueError, match="byband"):
        ClearSkyStep(o["prob"], device=0, clouds=o["clouds"], clrsky=True, byband=True)
    with pytest.raises(ValueError, match="clouds"):
        ClearSkyStep(o["prob"], device=0, clrsky=True)
