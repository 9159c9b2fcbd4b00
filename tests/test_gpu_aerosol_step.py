"""GPU: ClearSkyStep(aerosols=...) on 36 RFMIP columns -- clear sky, overcast clouds, McICA (seeded), McICA with
clear-sky fluxes -- every comparison bit for bit: the fused step against the composed oracle (gas optics, increment by
the aerosol, the clear solve, increment by the -- sampled -- cloud, the all-sky solve), fused=False against fused, a
captured graph against the eager step, set_aerosols between replays against a fresh step built with the new values,
and set_mcica_seed between replays leaving the clear arrays as they were; and the call plan of every aerosols= option set
against tests/golden/step_plan_aerosol.json."""
import json
import os

import numpy as np
import pytest

import mcica_ref as M
import philox_ref as PH
import step_plan as P
import step_plan_aerosol as PA

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "step_plan_aerosol.json")
FLUX = ("lw_up", "lw_dn", "sw_up", "sw_dn", "sw_dir")
CLR = tuple(k + "_clr" for k in FLUX)
SEED_A, SEED_B = 20261020, (5 << 32) | 91
MODES = ("clear", "clouds", "mcica", "mcica_clrsky")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a device"
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def _aerosols(ncol, nlay, seed):
    from rrtmgpnn import data
    nb_lw, nb_sw = data.load_kdist("lw")["nband"], data.load_kdist("sw")["nband"]
    rng = np.random.default_rng(seed)
    return {"lw_tau": rng.lognormal(-2, 1, (ncol, nlay, nb_lw)).astype(np.float32),
            "sw_tau": rng.lognormal(-2, 1, (ncol, nlay, nb_sw)).astype(np.float32),
            "sw_ssa": rng.uniform(0.6, 1, (ncol, nlay, nb_sw)).astype(np.float32),
            "sw_g": rng.uniform(0.3, 0.8, (ncol, nlay, nb_sw)).astype(np.float32)}


@pytest.fixture(scope="module")
def case(rfmip):
    """36 columns (more than one SW block pair), the all-sky example's clouds, a cloud fraction and overlap parameter,
    two aerosol sets."""
    from conftest import subset
    from rrtmgpnn import data
    prob = subset(rfmip, np.arange(0, 1800, 50))
    ncol, nlay = prob["ncol"], prob["nlay"]
    clouds = data.allsky_clouds(prob, data.load_cloud_optics("lw"))
    cloudy = (clouds[0] > 0) | (clouds[1] > 0)
    assert cloudy.any()
    rng = np.random.default_rng(62)
    cf = np.where(cloudy, rng.uniform(0.2, 0.9, cloudy.shape), 0).astype(np.float32)
    ov = rng.uniform(-1, 1, (ncol, nlay - 1)).astype(np.float32)
    return dict(prob=prob, clouds=clouds, cf=cf, ov=ov, use=prob["usecol"], aer=[_aerosols(ncol, nlay, 98),
                                                                              _aerosols(ncol, nlay, 99)])


def _kwargs(c, mode, seed=SEED_A):
    kw = {}
    if mode != "clear":
        kw["clouds"] = c["clouds"]
    if mode.startswith("mcica"):
        kw["mcica"] = {"cloud_frac": c["cf"], "overlap_param": c["ov"], "seed": seed}
        if mode == "mcica_clrsky":
            kw["mcica"]["clrsky"] = True
    return kw


def _ident(ng):
    return np.stack([np.arange(1, ng + 1)] * 2, axis=1).astype(np.int32)


def _oracle(orc, c, mode, aer, seed=SEED_A):
    """The composed oracle: the clear set (gases plus aerosols) and, with clouds, the all-sky set; a clear-sky step's
    fluxes are the clear set."""
    from rrtmgpnn import data
    prob, clouds = c["prob"], c["clouds"]
    ncol, nlay = prob["ncol"], prob["nlay"]
    m = {k: data.load_model(k) for k in ("lw_abs", "lw_pfrac", "sw_abs", "sw_ray")}
    kl, ks = data.load_kdist("lw"), data.load_kdist("sw")
    out = {}
    # LW
    go = orc.lw_gas_optics(prob, [m["lw_abs"], m["lw_pfrac"]], kl)
    ng = go["tau"].shape[-1]
    (tau_a,) = orc.increment_bybnd(kl["band_lims_gpt"], (go["tau"],), (aer["lw_tau"],))
    emis = np.repeat(np.asarray(prob["sfc_emis"], np.float32)[:, None], ng, axis=1)
    solve = lambda t: orc.lw_solver(t, go["lay_source"], go["lev_source"], emis, go["sfc_source"], prob["top_at_1"], 1)  # noqa: E731
    out["lw_up_clr"], out["lw_dn_clr"] = solve(tau_a)
    if mode != "clear":
        (ct,) = orc.cloud_optics(data.load_cloud_optics("lw"), *clouds, nstr=1, lut=True, icergh=2)
        if mode.startswith("mcica"):
            mask = M.sampled_mask(PH.randoms(seed, 0, 0, ng, nlay, ncol), c["cf"], c["ov"])
            (tau,) = orc.increment_bybnd(_ident(ng), (tau_a,), (M.draw(mask, ct, kl["band_lims_gpt"]),))
        else:
            (tau,) = orc.increment_bybnd(kl["band_lims_gpt"], (tau_a,), (ct,))
        out["lw_up"], out["lw_dn"] = solve(tau)
    # SW
    go = orc.sw_gas_optics(prob, [m["sw_abs"], m["sw_ray"]])
    ng = go["tau"].shape[-1]
    io_a = orc.increment_bybnd(ks["band_lims_gpt"], (go["tau"], go["ssa"], go["g"]),
                               (aer["sw_tau"], aer["sw_ssa"], aer["sw_g"]))
    alb = np.repeat(np.asarray(prob["sfc_alb"], np.float32)[:, None], ng, axis=1)
    solve = lambda io: orc.sw_solver(*io, prob["mu0"], data.toa_flux(prob, ks), alb, alb, prob["top_at_1"])  # noqa: E731
    out["sw_up_clr"], out["sw_dn_clr"], out["sw_dir_clr"] = solve(io_a)
    if mode != "clear":
        cld = orc.delta_scale(*orc.cloud_optics(data.load_cloud_optics("sw"), *clouds, nstr=2, lut=True, icergh=2))
        if mode.startswith("mcica"):
            mask = M.sampled_mask(PH.randoms(seed, 1, 0, ng, nlay, ncol), c["cf"], c["ov"])
            io = orc.increment_bybnd(_ident(ng), io_a, [M.draw(mask, a, ks["band_lims_gpt"]) for a in cld])
        else:
            io = orc.increment_bybnd(ks["band_lims_gpt"], io_a, cld)
        out["sw_up"], out["sw_dn"], out["sw_dir"] = solve(io)
    if mode == "clear":
        return {k: out[k + "_clr"] for k in FLUX}
    if mode != "mcica_clrsky":
        return {k: out[k] for k in FLUX}
    return out


def _poison(step):
    for k in FLUX:
        getattr(step, k).fill_(float("nan"))
        if step.clrsky:
            getattr(step, k + "_clr").fill_(float("nan"))


def _outputs(step):
    torch.cuda.synchronize()
    out = dict(step.fluxes())
    if step.clrsky:
        out.update(step.clrsky_fluxes())
    return out


def _run(step):
    _poison(step)
    step.step()
    return _outputs(step)


def _equal(got, want, what, use=None, keys=None):
    """Bitwise; use: the SW arrays on the sunlit columns only (the oracle solves the others with the driver's mu0)."""
    for k in (keys or want):
        g, w = got[k], want[k]
        if use is not None and k.startswith("sw"):
            g, w = g[use], w[use]
        np.testing.assert_array_equal(g, w, err_msg="%s %s" % (what, k))


@pytest.mark.parametrize("mode", MODES)
def test_step_with_aerosols(dev, orc, case, mode):
    from rrtmgpnn import _lib
    from rrtmgpnn.pipeline import ClearSkyStep
    c, L = case, _lib.lib()
    prob, use, (aer_a, aer_b) = c["prob"], c["use"], c["aer"]
    step = ClearSkyStep(prob, device=0, aerosols=aer_a, **_kwargs(c, mode))
    names = [n for n, _, _ in step.calls]
    fns = {n: f for n, f, _ in step.calls}
    if mode == "clear":  # the aerosol is the solver calls' own increment: no request
        assert "lw_aerosol" not in names and "sw_aerosol" not in names
        assert fns["lw_solver"] is L.rrtmgpnn_lw_solver_noscat_planck_inc
    else:  # the requests, right before their solvers
        assert names.index("lw_aerosol") == names.index("lw_solver") - 1
        assert names.index("sw_aerosol") == names.index("sw_solver") - 1
        assert fns["lw_aerosol"] is L.rrtmgpnn_solver_request_aerosol
    assert not [n for n in names if n.startswith("increment")], "the fused step materialises an increment"
    eager = _run(step)
    want = _oracle(orc, c, mode, aer_a)
    assert set(eager) == set(want)
    _equal(eager, want, "fused eager against the oracle:", use)
    bare = ClearSkyStep(prob, device=0, **_kwargs(c, mode))
    assert (_run(bare)["lw_dn"] != eager["lw_dn"]).any(), "the aerosols do not show"
    bare.close()
    step.capture()
    _poison(step)
    step.replay()
    _equal(_outputs(step), eager, "captured against eager:")
    if mode == "mcica_clrsky":  # a new seed between replays: the clear arrays stay, bit for bit
        step.set_mcica_seed(seed=SEED_B)
        _poison(step)
        step.replay()
        again = _outputs(step)
        _equal(again, eager, "the clear set after a new seed:", keys=CLR)
        assert (again["lw_dn"] != eager["lw_dn"]).any() and (again["sw_dn"] != eager["sw_dn"]).any()
        step.set_mcica_seed(seed=SEED_A)
    # new aerosols between replays: a fresh step built with them
    step.set_aerosols(**aer_b)
    _poison(step)
    step.replay()
    again = _outputs(step)
    step.close()
    fresh = ClearSkyStep(prob, device=0, aerosols=aer_b, **_kwargs(c, mode))
    _equal(again, _run(fresh), "replay after set_aerosols against a fresh step:")
    fresh.close()
    assert (again["lw_dn"] != eager["lw_dn"]).any() and (again["sw_dn"][use] != eager["sw_dn"][use]).any()
    unf = ClearSkyStep(prob, device=0, aerosols=aer_a, fused=False, **_kwargs(c, mode))
    un = [n for n, _, _ in unf.calls]
    assert un.index("predict_nn_lw") < un.index("increment_aer_lw") < un.index("lw_solver")
    assert un.index("predict_nn_sw") < un.index("increment_aer_sw") < un.index("sw_solver")
    if mode == "mcica_clrsky":
        assert un.index("increment_aer_lw") < un.index("lw_solver_clr") < un.index("increment_lw")
        assert un.index("increment_aer_sw") < un.index("sw_solver_clr") < un.index("increment_sw")
    got = _run(unf)
    unf.close()
    _equal(got, want, "fused=False against the oracle:", use)
    _equal(got, eager, "fused=False against fused:")


def test_step_refusals(dev, case):
    from rrtmgpnn.pipeline import ClearSkyStep
    c = case
    aer = c["aer"][0]
    for kw in ({"byband": True}, {"jacobian": True},
               {"clouds": c["clouds"], "mcica": {"cloud_frac": c["cf"], "overlap_param": None, "seed": 1, "byband": True}}):
        with pytest.raises(ValueError, match="aerosols"):
            ClearSkyStep(c["prob"], device=0, aerosols=aer, **kw)
    with pytest.raises(ValueError, match="keys"):
        ClearSkyStep(c["prob"], device=0, aerosols={"lw_tau": aer["lw_tau"]})
    with pytest.raises(ValueError, match="shape"):
        ClearSkyStep(c["prob"], device=0, aerosols=dict(aer, sw_g=aer["sw_g"][:, 1:]))
    plain = ClearSkyStep(c["prob"], device=0)
    with pytest.raises(ValueError, match="aerosols"):
        plain.set_aerosols(lw_tau=aer["lw_tau"])
    plain.close()


# ---- the call plan ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def env(dev, rfmip):
    return P.environment(rfmip)


@pytest.mark.parametrize("cid,build", PA.CASES, ids=[k for k, _ in PA.CASES])
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
