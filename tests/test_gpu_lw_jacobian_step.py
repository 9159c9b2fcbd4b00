"""GPU: flux_up_Jac through the class layer (api.rte_config_jacobian + rte_lw) and ClearSkyStep(jacobian=True), bit for
bit against the oracle's flux_up on zero sources with sfc_source_Jac as the surface source (tests/lw_jacobian_ref.py)."""
import numpy as np
import pytest

import lw_jacobian_ref as J
import mcica_ref as M
import philox_ref as P
import step_plan as SP
from conftest import subset
from test_lw_scattering_oracle import lw_2str_problem

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENTINEL = -4321.25


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a device"
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def T(a, dev):
    return torch.as_tensor(np.array(a, dtype=np.float32, order="C", copy=True), device=dev)


@pytest.fixture
def jacobian_switch():
    """rte_config_jacobian for one test; off again afterwards."""
    from rrtmgpnn import api
    yield api.rte_config_jacobian
    api.rte_config_jacobian(False)


@pytest.fixture(scope="module")
def prob2(orc, rfmip):
    return lw_2str_problem(orc, rfmip, ncol=12)


def _rte_lw(p, dev, scat, nmus=None, use_2stream=False, jac="right", dn_jac=False, fluxes=None):
    """api.rte_lw on the problem's arrays; jac: "right" / "wrong" extents, or None.  -> (message, up, dn, flux_up_Jac,
    flux_dn_Jac) as host arrays."""
    from rrtmgpnn import api
    kd = p["kd"]
    ncol, nlay, ngpt = p["tau"].shape
    op = api.OpticalProps2str() if scat else api.OpticalProps1scl()
    assert op.init(kd["band_lims_wvn"], kd["band_lims_gpt"]) == ""
    assert (op.alloc_2str if scat else op.alloc_1scl)(ncol, nlay, device=dev) == ""
    op.tau.copy_(T(p["tau"], dev))
    if scat:
        op.ssa.copy_(T(p["ssa"], dev)), op.g.copy_(T(p["g"], dev))
    src = api.SourceFuncLW()
    assert src.alloc(ncol, nlay, op, device=dev) == ""
    src.lay_source.copy_(T(p["lay"], dev)), src.lev_source.copy_(T(p["lev"], dev))
    src.sfc_source.copy_(T(p["sfc"], dev)), src.sfc_source_Jac.copy_(T(p["jac"], dev))
    full = lambda *s: torch.full(s, SENTINEL, device=dev)  # noqa: E731
    fl = fluxes(full, ncol, nlay, ngpt, kd["nband"]) if fluxes else api.FluxesBroadband(full(ncol, nlay + 1), full(ncol, nlay + 1))
    uj = None if jac is None else full(ncol, nlay + (1 if jac == "right" else 2))
    dj = full(ncol, nlay + 1) if dn_jac else None
    e = api.rte_lw(op, True, src, T(p["emis_band"], dev), fl, n_gauss_angles=nmus, use_2stream=use_2stream,
                   flux_up_Jac=uj, flux_dn_Jac=dj)
    torch.cuda.synchronize()
    h = lambda t: None if t is None else t.cpu().numpy()  # noqa: E731
    return e, h(fl.flux_up), h(fl.flux_dn), h(uj), h(dj)


@pytest.mark.parametrize("nmus", [1, 3])
@pytest.mark.parametrize("scat", [False, True])
def test_rte_lw_switch_on(dev, orc, prob2, jacobian_switch, scat, nmus):
    """Values on 1scl properties (the no-scattering solver) and on 2str ones (the rescaled solution); flux_dn_Jac stays
    untouched; the fluxes are those of the call with the switch off."""
    p = prob2
    sc = dict(ssa=p["ssa"], g=p["g"]) if scat else {}
    e, up0, dn0, uj0, _ = _rte_lw(p, dev, scat, nmus)
    assert e == "" and (uj0 == SENTINEL).all(), "switch off: accepted and untouched"
    jacobian_switch(True)
    e, up, dn, uj, dj = _rte_lw(p, dev, scat, nmus, dn_jac=True)
    assert e == "", e
    want_up, want_dn = orc.lw_solver(p["tau"], p["lay"], p["lev"], p["emis_gpt"], p["sfc"], True, nmus, **sc)
    np.testing.assert_array_equal(uj, J.zero_source_flux_up(orc, p["tau"], p["emis_gpt"], p["jac"], True, nmus, **sc))
    for got, want in ((up, want_up), (dn, want_dn), (up, up0), (dn, dn0)):
        np.testing.assert_array_equal(got, want)
    assert (dj == SENTINEL).all()


def test_rte_lw_messages(dev, prob2, jacobian_switch):
    from rrtmgpnn import api
    p = prob2
    jacobian_switch(True)
    e, up, _, _, _ = _rte_lw(p, dev, False, jac=None)
    assert e == "rte_lw: compute_Jac=true but Jacobian arrays not provided" and (up == SENTINEL).all()
    e, up, _, uj, _ = _rte_lw(p, dev, False, jac="wrong")
    assert e == "rte_lw: flux Jacobian inconsistently sized" and (up == SENTINEL).all() and (uj == SENTINEL).all()
    e, up, _, uj, _ = _rte_lw(p, dev, True, use_2stream=True)
    assert e == "rte_lw: can't provide Jacobian of fluxes w.r.t surface temperature with 2-stream"
    assert (up == SENTINEL).all() and (uj == SENTINEL).all()
    gpt = lambda full, ncol, nlay, ngpt, nb: api.FluxesFlexible(  # noqa: E731
        full(ncol, nlay + 1), full(ncol, nlay + 1), gpt_flux_up=full(ncol, nlay + 1, ngpt), gpt_flux_dn=full(ncol, nlay + 1, ngpt))
    bnd = lambda full, ncol, nlay, ngpt, nb: api.FluxesByBand(  # noqa: E731
        bnd_flux_up=full(ncol, nlay + 1, nb), bnd_flux_dn=full(ncol, nlay + 1, nb), flux_up=full(ncol, nlay + 1),
        flux_dn=full(ncol, nlay + 1))
    for fluxes, word in ((gpt, "g-point"), (bnd, "by-band")):
        e, up, _, uj, _ = _rte_lw(p, dev, False, fluxes=fluxes)
        assert e.startswith("rte_lw: flux Jacobian together with %s fluxes" % word), e
        assert (up == SENTINEL).all() and (uj == SENTINEL).all()
    # nothing stayed armed: a plain call with the switch off leaves a Jacobian array untouched
    jacobian_switch(False)
    e, up, _, uj, _ = _rte_lw(p, dev, False)
    assert e == "" and (uj == SENTINEL).all() and (up != SENTINEL).all()


# ---- ClearSkyStep(jacobian=True): 12 RFMIP columns ------------------------------------------------------------------

SEED = 20261020


@pytest.fixture(scope="module")
def step_case(orc, rfmip):
    """The problem, its clouds, and the oracle's fluxes and Jacobian for the clear, overcast and seeded-McICA step."""
    from rrtmgpnn import data
    prob = subset(rfmip, np.arange(7, 1800, 150))
    ncol, nlay = prob["ncol"], prob["nlay"]
    assert ncol == 12
    kd = data.load_kdist("lw")
    clouds = data.allsky_clouds(prob, data.load_cloud_optics("lw"))
    cloudy = (clouds[0] > 0) | (clouds[1] > 0)
    assert cloudy.any()
    cf = np.where(cloudy, np.random.default_rng(52).uniform(0.2, 0.9, cloudy.shape), 0).astype(np.float32)
    go = orc.lw_gas_optics(prob, [data.load_model("lw_abs"), data.load_model("lw_pfrac")], kd)
    ng = go["tau"].shape[-1]
    (ct,) = orc.cloud_optics(data.load_cloud_optics("lw"), *clouds, nstr=1, lut=True, icergh=2)
    (overcast,) = orc.increment_bybnd(kd["band_lims_gpt"], (go["tau"],), (ct,))
    ident = np.stack([np.arange(1, ng + 1)] * 2, axis=1).astype(np.int32)
    mask = M.sampled_mask(P.randoms(SEED, 0, 0, ng, nlay, ncol), cf, None)
    (sampled,) = orc.increment_bybnd(ident, (go["tau"],), (M.draw(mask, ct, kd["band_lims_gpt"]),))
    emis = np.repeat(np.asarray(prob["sfc_emis"], np.float32)[:, None], ng, axis=1)
    want = {}
    for mode, tau in (("clear", go["tau"]), ("overcast", overcast), ("mcica", sampled)):
        up, dn = orc.lw_solver(tau, go["lay_source"], go["lev_source"], emis, go["sfc_source"], prob["top_at_1"], 1)
        want[mode] = (up, dn, J.zero_source_flux_up(orc, tau, emis, go["sfc_source_Jac"], prob["top_at_1"], 1))
    assert (want["mcica"][2] != want["clear"][2]).any() and (want["mcica"][2] != want["overcast"][2]).any()
    kw = {"clear": {}, "overcast": {"clouds": clouds},
          "mcica": {"clouds": clouds, "mcica": {"cloud_frac": cf, "overlap_param": None, "seed": SEED}}}
    return {"prob": prob, "clouds": clouds, "want": want, "kw": kw, "cf": cf}


@pytest.mark.parametrize("mode", ["clear", "overcast", "mcica"])
def test_step_fused_unfused_oracle_and_replay(dev, step_case, mode):
    """fused = unfused = oracle, and a captured graph's replay = the eager step, for lw_up, lw_dn and lw_up_jac; the
    other fluxes are those of the step without jacobian=True."""
    from rrtmgpnn.pipeline import ClearSkyStep
    c = step_case
    up, dn, jac = c["want"][mode]
    plain = ClearSkyStep(c["prob"], device=0, **c["kw"][mode])
    plain.step()
    torch.cuda.synchronize()
    base = plain.fluxes()
    plain.close()
    for fused in (True, False):
        s = ClearSkyStep(c["prob"], device=0, fused=fused, jacobian=True, **c["kw"][mode])
        s.step()
        torch.cuda.synchronize()
        got = s.fluxes()
        np.testing.assert_array_equal(s.jacobian_flux(), jac, err_msg="fused %s" % fused)
        np.testing.assert_array_equal(got["lw_up"], up)
        np.testing.assert_array_equal(got["lw_dn"], dn)
        if fused:
            for k, v in base.items():
                np.testing.assert_array_equal(got[k], v, err_msg=k)
            s.capture()
            for t in (s.lw_up, s.lw_dn, s.lw_up_jac, s.sw_up):
                t.fill_(float("nan"))
            s.replay()
            torch.cuda.synchronize()
            np.testing.assert_array_equal(s.jacobian_flux(), jac, err_msg="replay")
            for k, v in s.fluxes().items():
                np.testing.assert_array_equal(v, got[k], err_msg="replay " + k)
        s.close()


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("mode", ["clear", "allsky", "mcica-seeded-maxran", "mcica-arrays-expran"])
def test_step_plan_is_the_plain_plan_plus_one_call_and_one_buffer(dev, rfmip, mode, fused):
    """With tests/step_plan.py's description of a step: jacobian=True adds exactly the request, right before lw_solver
    on the LW stream, and the buffer lw_up_jac; every other call, buffer and schedule attribute is the plain step's."""
    env = SP.environment(rfmip)
    build = dict(SP.MODES)[mode]
    plain = SP.run_case(lambda e: dict(build(e), fused=fused), env)
    withj = SP.run_case(lambda e: dict(build(e), fused=fused, jacobian=True), env)
    extra = [c for c in withj["calls"] if c not in plain["calls"]]
    assert len(extra) == 1 and extra[0].startswith("lw_jacobian rrtmgpnn_solver_request_jacobian lw: ctx, 256, "), extra
    assert extra[0].endswith(", null, lw_up_jac" if fused else ", sfc_jac, lw_up_jac")
    i = withj["calls"].index(extra[0])
    assert withj["calls"][i + 1].startswith("lw_solver ")
    assert withj["calls"][:i] + withj["calls"][i + 1:] == plain["calls"]
    nlay = env["prob"]["nlay"]
    assert {k: v for k, v in withj["buffers"].items() if k not in plain["buffers"]} == {"lw_up_jac": [[4, nlay + 1], "float32"]}
    assert {k: v for k, v in withj["buffers"].items() if k != "lw_up_jac"} == plain["buffers"]
    assert withj["schedule"] == plain["schedule"]


def test_step_refusals(dev, step_case):
    from rrtmgpnn.pipeline import ClearSkyStep
    c = step_case
    mc = c["kw"]["mcica"]["mcica"]
    for kw in ({"byband": True}, {"clouds": c["clouds"], "clrsky": True}, {"clouds": c["clouds"], "byband": True},
               {"clouds": c["clouds"], "mcica": dict(mc, clrsky=True)}, {"clouds": c["clouds"], "mcica": dict(mc, byband=True)}):
        with pytest.raises(ValueError, match="jacobian=True"):
            ClearSkyStep(c["prob"], device=0, jacobian=True, **kw)
    s = ClearSkyStep(c["prob"], device=0)
    assert not hasattr(s, "lw_up_jac") and "lw_jacobian" not in [n for n, _, _ in s.calls]
    with pytest.raises(ValueError):
        s.jacobian_flux()
    s.close()
