"""GPU: ClearSkyStep(clouds=..., lw_scattering=True, lw_dual=True) on 12 RFMIP columns, every comparison bit for bit --
the call plan of every lw_dual option set against tests/golden/step_plan_lw_dual.json; lw_dual on against off, ten flux
arrays, overcast and McICA, in both modes of rrtmgpnn_context_set_lw_scat_clr_all; with aerosols against
clr_all_sky.rte_lw on the step's own cloud, aerosol and mask arrays (its comparison route, LW_SCAT_FUSED = False, too)
and against the composed oracle; a captured graph replayed after set_aerosols against a fresh step; the ValueErrors."""
import json
import os

import numpy as np
import pytest

import mcica_ref as M
import step_plan as P
import step_plan_lw_dual as PD

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "step_plan_lw_dual.json")
FLUX = ("lw_up", "lw_dn", "sw_up", "sw_dn", "sw_dir")
LW4 = ("lw_up", "lw_dn", "lw_up_clr", "lw_dn_clr")
MODES = ("clrsky", "mcica_clrsky")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a device"
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def case(rfmip, orc):
    """12 columns, the all-sky example's clouds, a cloud fraction, overlap parameter and random numbers, two aerosol
    sets; the oracle's gas optics, computed once."""
    from conftest import subset
    from rrtmgpnn import data
    prob = subset(rfmip, np.arange(7, 1800, 150))
    ncol, nlay = prob["ncol"], prob["nlay"]
    kl, ks = data.load_kdist("lw"), data.load_kdist("sw")
    clouds = data.allsky_clouds(prob, data.load_cloud_optics("lw"))
    cloudy = (clouds[0] > 0) | (clouds[1] > 0)
    assert cloudy.any()
    rng = np.random.default_rng(64)
    cf = np.where(cloudy, rng.uniform(0.2, 0.9, cloudy.shape), 0).astype(np.float32)
    ov = rng.uniform(-1, 1, (ncol, nlay - 1)).astype(np.float32)
    r_lw = rng.random((ncol, nlay, kl["ngpt"]), dtype=np.float32)
    r_sw = rng.random((ncol, nlay, ks["ngpt"]), dtype=np.float32)

    def aer(seed):
        r = np.random.default_rng(seed)
        nbl, nbs = kl["nband"], ks["nband"]
        return {"lw_tau": r.lognormal(-2, 1, (ncol, nlay, nbl)).astype(np.float32),
                "sw_tau": r.lognormal(-2, 1, (ncol, nlay, nbs)).astype(np.float32),
                "sw_ssa": r.uniform(0.6, 1, (ncol, nlay, nbs)).astype(np.float32),
                "sw_g": r.uniform(0.3, 0.8, (ncol, nlay, nbs)).astype(np.float32)}

    go = orc.lw_gas_optics(prob, [data.load_model("lw_abs"), data.load_model("lw_pfrac")], kl)
    return dict(prob=prob, clouds=clouds, cf=cf, ov=ov, r_lw=r_lw, r_sw=r_sw, go=go, kl=kl, aer=[aer(101), aer(102)])


def _kwargs(c, mode):
    kw = {"clouds": c["clouds"], "lw_scattering": True}
    if mode == "mcica_clrsky":
        kw["mcica"] = {"cloud_frac": c["cf"], "overlap_param": c["ov"], "randoms_lw": c["r_lw"], "randoms_sw": c["r_sw"],
                       "clrsky": True}
    else:
        kw["clrsky"] = True
    return kw


def _ident(ng):
    return np.stack([np.arange(1, ng + 1)] * 2, axis=1).astype(np.int32)


def _lw_oracle(orc, c, mode, aer):
    """The composed oracle's four LW arrays: the aerosol (1scl into the 2str gas set), then the -- sampled -- cloud, the
    rescaled solver; the clear set: the no-scattering solver on gases plus aerosols."""
    from rrtmgpnn import data
    prob, go, kl = c["prob"], c["go"], c["kl"]
    ng = go["tau"].shape[-1]
    cld = orc.cloud_optics(data.load_cloud_optics("lw"), *c["clouds"], nstr=2, lut=True, icergh=2)
    z = np.zeros_like(go["tau"])
    io = orc.increment_bybnd(kl["band_lims_gpt"], (go["tau"], z, z), (aer["lw_tau"],))
    (tau_a,) = orc.increment_bybnd(kl["band_lims_gpt"], (go["tau"],), (aer["lw_tau"],))
    if mode == "mcica_clrsky":
        mask = M.sampled_mask(c["r_lw"], c["cf"], c["ov"])
        io = orc.increment_bybnd(_ident(ng), io, [M.draw(mask, a, kl["band_lims_gpt"]) for a in cld])
    else:
        io = orc.increment_bybnd(kl["band_lims_gpt"], io, cld)
    emis = np.repeat(np.asarray(prob["sfc_emis"], np.float32)[:, None], ng, axis=1)
    src = (go["lay_source"], go["lev_source"], emis, go["sfc_source"], prob["top_at_1"], 1)
    out = {}
    out["lw_up"], out["lw_dn"] = orc.lw_solver(io[0], *src, ssa=io[1], g=io[2])
    out["lw_up_clr"], out["lw_dn_clr"] = orc.lw_solver(tau_a, *src)
    return out


def _poison(step):
    for k in FLUX:
        getattr(step, k).fill_(float("nan"))
        getattr(step, k + "_clr").fill_(float("nan"))


def _outputs(step):
    torch.cuda.synchronize()
    out = dict(step.fluxes())
    out.update(step.clrsky_fluxes())
    return out


def _run(step):
    _poison(step)
    step.step()
    return _outputs(step)


def _equal(got, want, what, keys=None):
    for k in (keys or want):
        g, w = np.ascontiguousarray(got[k], np.float32), np.ascontiguousarray(want[k], np.float32)
        np.testing.assert_array_equal(g.view(np.uint32), w.view(np.uint32), err_msg="%s %s" % (what, k))


def _set_mode(step, mode):
    from rrtmgpnn import _lib
    assert _lib.lib().rrtmgpnn_context_set_lw_scat_clr_all(step.ctx.h, mode) == 0


@pytest.mark.parametrize("mode", MODES)
def test_lw_dual_on_against_off(dev, case, mode):
    """The new entry as lw_solver, no lw_solver_clr, the mask request right before it; ten flux arrays equal those of the
    step without the option, in both modes of the knob, eager and captured."""
    from rrtmgpnn import _lib
    from rrtmgpnn.pipeline import ClearSkyStep
    c, L = case, _lib.lib()
    off = ClearSkyStep(c["prob"], device=0, **_kwargs(c, mode))
    want = _run(off)
    off.close()
    assert len(want) == 10
    step = ClearSkyStep(c["prob"], device=0, lw_dual=True, **_kwargs(c, mode))
    names = [n for n, _, _ in step.calls]
    fns = {n: f for n, f, _ in step.calls}
    assert fns["lw_solver"] is L.rrtmgpnn_lw_solver_1rescl_planck_clr_all and "lw_solver_clr" not in names
    assert "lw_aerosol" not in names
    if mode == "mcica_clrsky":
        assert names.index("lw_mask") == names.index("lw_solver") - 1
    for knob in (1, 2):
        _set_mode(step, knob)
        _equal(_run(step), want, "lw_dual on against off, mode %d:" % knob)
    _set_mode(step, 0)
    step.capture()
    _poison(step)
    step.replay()
    _equal(_outputs(step), want, "captured against the step without the option:")
    step.close()
    assert (want["lw_dn"] != want["lw_dn_clr"]).any()


@pytest.mark.parametrize("mode", MODES)
def test_lw_dual_with_aerosols(dev, orc, case, mode):
    """aerosols= beside lw_scattering: lw_aerosol right before the solver; the four LW arrays against the composed
    oracle and against clr_all_sky.rte_lw (both of its routes) on the step's own device arrays; a captured graph
    replayed after set_aerosols against a fresh step."""
    from rrtmgpnn import _lib, api, clr_all_sky
    from rrtmgpnn.pipeline import ClearSkyStep
    c, L = case, _lib.lib()
    prob, (aer_a, aer_b) = c["prob"], c["aer"]
    ncol, nlay = prob["ncol"], prob["nlay"]
    step = ClearSkyStep(prob, device=0, lw_dual=True, aerosols=aer_a, **_kwargs(c, mode))
    names = [n for n, _, _ in step.calls]
    fns = {n: f for n, f, _ in step.calls}
    assert fns["lw_solver"] is L.rrtmgpnn_lw_solver_1rescl_planck_clr_all and "lw_solver_clr" not in names
    assert names.index("lw_aerosol") == names.index("lw_solver") - 1
    assert fns["lw_aerosol"] is L.rrtmgpnn_solver_request_aerosol
    if mode == "mcica_clrsky":
        assert names.index("lw_mask") == names.index("lw_solver") - 2
    assert not [n for n in names if n.startswith("increment") or n.startswith("draw_samples")]
    eager = _run(step)
    _equal(eager, _lw_oracle(orc, c, mode, aer_a), "against the composed oracle:", LW4)
    _set_mode(step, 2)
    _equal(_run(step), eager, "mode 2 against mode 0:")
    _set_mode(step, 0)
    # the SW arrays are those of the aerosol step with absorbing LW clouds
    kw = _kwargs(c, mode)
    del kw["lw_scattering"]
    plain = ClearSkyStep(prob, device=0, aerosols=aer_a, **kw)
    base = _run(plain)
    plain.close()
    _equal(eager, base, "the SW arrays:", [k for k in base if k.startswith("sw")])
    _equal(eager, base, "the clear LW set beside the absorbing-cloud step's:", ("lw_up_clr", "lw_dn_clr"))
    assert (eager["lw_dn"] != base["lw_dn"]).any(), "scattering does not show"

    # the class layer on the step's own arrays
    T = lambda a: torch.as_tensor(np.array(a, dtype=np.float32), device=dev)  # noqa: E731
    kd = api.GasOpticsRRTMGP()
    api.stop_on_err(kd.load("lw"))
    from rrtmgpnn import data
    nets = [api.RrtmgpNetwork(0).load_netcdf(data.path(n)) for n in ("lw_abs", "lw_pfrac")]
    gases = api.GasConcs()
    api.stop_on_err(gases.init(list(prob["gases"])))
    for k, v in prob["gases"].items():
        api.stop_on_err(gases.set_vmr(k, T(v)))
    nb, ng = kd.get_nband(), kd.get_ngpt()
    cld = api.OpticalProps2str()
    assert cld.init(kd.get_band_lims_wavenumber()) == "" and cld.alloc_2str(ncol, nlay, device=dev) == ""
    cld.tau.copy_(step.cld_tau_lw)
    cld.ssa.copy_(step.cld_ssa_lw)
    cld.g.copy_(step.cld_g_lw)
    aer = api.OpticalProps1scl()
    assert aer.init(kd.get_band_lims_wavenumber()) == "" and aer.alloc_1scl(ncol, nlay, device=dev) == ""
    aer.tau.copy_(step.aer_tau_lw)
    masks = {}
    if mode == "mcica_clrsky":
        bits = step.mask_bits_lw.clone()
        mask = M.sampled_mask(c["r_lw"], c["cf"], c["ov"])
        assert np.array_equal(M.pack_bits(mask).view(np.int32).ravel(), bits.cpu().numpy().view(np.int32).ravel())
        masks = {"mask_bits": bits, "cloud_mask": torch.as_tensor(np.ascontiguousarray(mask, np.uint8), device=dev)}
    emis = T(np.repeat(np.asarray(prob["sfc_emis"], np.float32)[:, None], nb, axis=1))
    for route in (True, False):
        clr_all_sky.LW_SCAT_FUSED = route
        try:
            a, cl = (api.FluxesBroadband(*[torch.full((ncol, nlay + 1), float("nan"), device=dev) for _ in range(3)])
                     for _ in range(2))
            e = clr_all_sky.rte_lw(kd, gases, T(prob["play"]), T(prob["tlay"]), T(prob["plev"]), T(prob["tsfc"]), emis,
                                   cld, a, cl, aer_props=aer, t_lev=T(prob["tlev"]), neural_nets=nets, **masks)
        finally:
            clr_all_sky.LW_SCAT_FUSED = True
        assert e == "", e
        got = dict(zip(LW4, (t.cpu().numpy() for t in (a.flux_up, a.flux_dn, cl.flux_up, cl.flux_dn))))
        _equal(eager, got, "against clr_all_sky.rte_lw (LW_SCAT_FUSED = %s):" % route, LW4)

    # a captured graph, replayed after set_aerosols, against a fresh step built with the new values
    step.capture()
    _poison(step)
    step.replay()
    _equal(_outputs(step), eager, "captured against eager:")
    step.set_aerosols(**aer_b)
    _poison(step)
    step.replay()
    again = _outputs(step)
    step.close()
    fresh = ClearSkyStep(prob, device=0, lw_dual=True, aerosols=aer_b, **_kwargs(c, mode))
    _equal(again, _run(fresh), "replay after set_aerosols against a fresh step:")
    fresh.close()
    _equal(again, _lw_oracle(orc, c, mode, aer_b), "replay after set_aerosols against the oracle:", LW4)
    assert (again["lw_dn"] != eager["lw_dn"]).any() and (again["lw_dn_clr"] != eager["lw_dn_clr"]).any()


def test_step_refusals(dev, case):
    """Every lw_dual refusal names the option; without it lw_scattering keeps refusing aerosols."""
    from rrtmgpnn.pipeline import ClearSkyStep
    c = case
    mc = {"cloud_frac": c["cf"], "overlap_param": None, "randoms_lw": c["r_lw"], "randoms_sw": c["r_sw"]}
    cl = {"clouds": c["clouds"]}
    for kw in (dict(cl, clrsky=True),                                     # without lw_scattering
               dict(cl, lw_scattering=True),                              # without clear-sky outputs
               dict(cl, lw_scattering=True, mcica=mc),
               dict(cl, lw_scattering=True, clrsky=True, fused=False),
               dict(cl, lw_scattering=True, byband=True),
               dict(cl, lw_scattering=True, clrsky=True, jacobian=True),
               dict(cl, lw_scattering=True, mcica=dict(mc, byband=True, clrsky=True))):
        with pytest.raises(ValueError, match="lw_dual"):
            ClearSkyStep(c["prob"], device=0, lw_dual=True, **kw)
    with pytest.raises(ValueError, match="lw_scattering"):
        ClearSkyStep(c["prob"], device=0, lw_scattering=True, clrsky=True, aerosols=c["aer"][0], **cl)


# ---- the call plan ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def env(dev, rfmip):
    return P.environment(rfmip)


def test_cases_and_fixture_hold_the_same_keys(golden):
    assert sorted(golden) == sorted(k for k, _ in PD.CASES)
    assert {k for k, v in golden.items() if "raises" in v} == {k for k, _ in PD.CASES if k.startswith("refused-")}
    for k, v in golden.items():
        if "raises" in v:
            assert v["raises"] == "ValueError" and "lw_dual" in v["message"], k
        else:
            calls = [s.split()[0] for s in v["calls"]]
            assert "lw_solver_clr" not in calls
            assert any(s.startswith("lw_solver rrtmgpnn_lw_solver_1rescl_planck_clr_all ") for s in v["calls"]), k
            assert ("lw_aerosol" in calls) == ("-aer-" in k), k
            if "lw_aerosol" in calls:
                assert calls.index("lw_aerosol") == calls.index("lw_solver") - 1, k


@pytest.mark.parametrize("cid,build", PD.CASES, ids=[k for k, _ in PD.CASES])
def test_step_plan(cid, build, env, golden):
    want = golden[cid]
    got = json.loads(json.dumps(P.run_case(build, env)))
    if "raises" in want:
        assert got == want
        return
    assert "raises" not in got, got
    assert got["schedule"] == want["schedule"]
    assert got["buffers"] == want["buffers"]
    for g, w in zip(got["calls"], want["calls"]):
        assert g == w
    assert got == want
