"""GPU: ClearSkyStep(clouds=..., mcica={..., "daylit": True}), the McICA SW chain on the daylit columns of the block, bit
for bit.

On the first 36 RFMIP columns (16 of them at night) with a cloud fraction per layer, three configurations -- seeded
max-ran; the array route with exp-ran and aerosols=; seeded with "clrsky" and aerosols= on the g128 / g112 models -- each
against the same step without "daylit" (the full-extent McICA route, which the existing McICA, seeded and aerosol tests
hold to the oracle; tests/test_mcica_daylit_host.py shows on the oracle alone that solving the daylit columns by
themselves changes no bit): the SW fluxes equal on the daylit columns and exactly 0 at night, sw_dir and the clear set
included; the LW fluxes equal everywhere; eager equal to the captured graph.  One capture serves any sun, a new seed,
new random numbers and new aerosols without recapture."""
import ctypes
import os

import numpy as np
import pytest

from conftest import subset

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES = os.path.join(ROOT, "tests", "golden", "reference_files")
PATHS = {"lw_abs": os.path.join(FILES, "lw-g128-210809_absorption_BEST.nc"),
         "lw_pfrac": os.path.join(FILES, "lw-g128-210809_planck_frac_BEST.nc"),
         "sw_abs": os.path.join(FILES, "sw-g112-210809_absorption_BEST.nc"),
         "sw_ray": os.path.join(FILES, "sw-g112-210809_rayleigh_BEST.nc")}
SPECTRAL = {"lw_models": (PATHS["lw_abs"], PATHS["lw_pfrac"]), "sw_models": (PATHS["sw_abs"], PATHS["sw_ray"]),
            "ngpt_lw": 128, "ngpt_sw": 112}
FLUX = ("lw_up", "lw_dn", "sw_up", "sw_dn", "sw_dir")
CLR = ("lw_up_clr", "lw_dn_clr", "sw_up_clr", "sw_dn_clr", "sw_dir_clr")
SEED_A, SEED_B = 20261021, (5 << 32) | 91
# rrtmgpnn_context_get_solver_path of the SW context: family 8 with the band-pair increment, the transmittance plane and
# the count (2 | 8 | 32 | 2048) beside the mask (128) and the aerosol (256); the clear launch runs family 7, the
# small-grid instance (1024 | 8 | 16 | 2048) or, with the aerosol as its increment, 2 | 8 | 32 | 2048
PATH_MASK, PATH_MASK_AER, PATH_CLR_AER = [8, 2218], [8, 2474], [7, 2090]
F_ACTIVE = 16


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a device"
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def aerosols(ncol, nlay, seed, nb_lw, nb_sw):
    rng = np.random.default_rng(seed)
    return {"lw_tau": rng.lognormal(-2, 1, (ncol, nlay, nb_lw)).astype(np.float32),
            "sw_tau": rng.lognormal(-2, 1, (ncol, nlay, nb_sw)).astype(np.float32),
            "sw_ssa": rng.uniform(0.6, 1, (ncol, nlay, nb_sw)).astype(np.float32),
            "sw_g": rng.uniform(0.3, 0.8, (ncol, nlay, nb_sw)).astype(np.float32)}


@pytest.fixture(scope="module")
def case(rfmip):
    """The first 36 RFMIP columns (16 of them night columns), the all-sky example's clouds with a cloud fraction per
    layer, an overlap parameter, random numbers for both chains and two aerosol sets"""
    from rrtmgpnn import data
    prob = subset(rfmip, np.arange(36))
    ncol, nlay = prob["ncol"], prob["nlay"]
    assert int((~prob["usecol"]).sum()) == 16
    clouds = data.allsky_clouds(prob, data.load_cloud_optics("lw"))
    cloudy = (clouds[0] > 0) | (clouds[1] > 0)
    assert cloudy[prob["usecol"]].any()
    rng = np.random.default_rng(83)
    cf = np.where(cloudy, rng.uniform(0.2, 0.9, cloudy.shape), 0).astype(np.float32)
    ov = rng.uniform(-1, 1, (ncol, nlay - 1)).astype(np.float32)
    kl, ks = data.load_kdist("lw"), data.load_kdist("sw")
    return dict(prob=prob, use=prob["usecol"], clouds=clouds, cf=cf, ov=ov,
                r_lw=rng.random((ncol, nlay, kl["ngpt"]), dtype=np.float32),
                r_sw=[rng.random((ncol, nlay, ks["ngpt"]), dtype=np.float32) for _ in range(2)],
                aer=[aerosols(ncol, nlay, s, kl["nband"], ks["nband"]) for s in (98, 99)])


def kwargs(c, config, daylit, seed=SEED_A, sza=None):
    """The constructor's arguments of a configuration, with or without the "daylit" key"""
    mc = {"cloud_frac": c["cf"]}
    kw = {"device": 0, "clouds": c["clouds"], "mcica": mc}
    if config == "seeded-maxran":
        mc.update(overlap_param=None, seed=seed)
    elif config == "arrays-expran-aer":
        mc.update(overlap_param=c["ov"], randoms_lw=c["r_lw"], randoms_sw=c["r_sw"][0])
        kw["aerosols"] = c["aer"][0]
    else:   # seeded-clrsky-aer-g112
        mc.update(overlap_param=c["ov"], seed=seed, clrsky=True)
        kw.update(aerosols=c["aer"][0], spectral=SPECTRAL)
    if daylit:
        mc["daylit"] = True
    return kw


CONFIGS = ("seeded-maxran", "arrays-expran-aer", "seeded-clrsky-aer-g112")


def names(step):
    return FLUX + (CLR if step.clrsky else ())


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(got, want, msg):
    np.testing.assert_array_equal(bits(got), bits(want), err_msg=msg)


def run(step, how="eager"):
    for k in names(step):
        getattr(step, k).fill_(float("nan"))
    torch.cuda.synchronize()
    if how == "eager":
        step.step()
    else:
        if step.graph is None:
            step.capture()
            for k in names(step):
                getattr(step, k).fill_(float("nan"))
            torch.cuda.synchronize()
        step.replay()
    torch.cuda.synchronize()
    return {k: getattr(step, k).cpu().numpy() for k in names(step)}


def paths(step):
    from rrtmgpnn import _lib
    c = step.ctx2 if step.ctx2 is not None else step.ctx
    s, m = (ctypes.c_int * 4)(), (ctypes.c_int * 8)()
    _lib.check(_lib.lib().rrtmgpnn_context_get_solver_path(c.h, s), "get_solver_path")
    _lib.check(_lib.lib().rrtmgpnn_context_get_mlp_path(c.h, m), "get_mlp_path")
    return list(s)[:2], list(m)


def against_the_full_extent_step(got, ref, use, what):
    """SW: the full-extent step's on the daylit columns (its night columns hold the mu0 = 1 solve), exactly 0 at night;
    LW: the full-extent step's everywhere"""
    for k in got:
        if k.startswith("lw"):
            same(got[k], ref[k], "%s: %s" % (what, k))
        else:
            same(got[k][use], ref[k][use], "%s: %s on the daylit columns" % (what, k))
            assert not got[k][~use].any(), "%s: %s is not exactly 0 at night" % (what, k)
            assert (got[k][use] > 0).any(), "%s: %s is 0 in daylight" % (what, k)


@pytest.fixture(scope="module")
def reference(dev, case):
    """The fluxes of each configuration's step without "daylit" (computed once, never modified)"""
    from rrtmgpnn.pipeline import ClearSkyStep
    out = {}
    for config in CONFIGS:
        step = ClearSkyStep(case["prob"], **kwargs(case, config, False))
        out[config] = run(step)
        out[config + "/calls"] = [n for n, _, _ in step.calls]
        step.close()
    return out


@pytest.mark.parametrize("config", CONFIGS)
def test_step_equals_the_full_extent_mcica_step(dev, case, reference, config):
    from rrtmgpnn.pipeline import SW_CHAIN, ClearSkyStep
    c = case
    step = ClearSkyStep(c["prob"], **kwargs(c, config, True))
    try:
        eager = run(step)
        sp, mp = paths(step)
        # the all-sky launch's path: the SW chain again, without the clear launch behind it
        if step.clrsky:
            for name, fn, args in step.calls:
                if name in SW_CHAIN and name not in ("sw_active_clr", "sw_solver_clr", "daylit_scatter"):
                    assert fn(*args) == 0, name
            torch.cuda.synchronize()
            sky, _ = paths(step)
            assert sky == PATH_MASK_AER and sp == PATH_CLR_AER, (sky, sp)
        else:
            assert sp == (PATH_MASK_AER if "aer" in config else PATH_MASK), sp
        assert mp[7] & F_ACTIVE, mp
        graph = run(step, "graph")
        assert int(step.nday.item()) == int(c["use"].sum())
        calls = [n for n, _, _ in step.calls]
        assert ("sw_aerosol" in calls) == ("aer" in config) and ("sw_active_clr" in calls) == step.clrsky
        assert not hasattr(step, "d_cloud_frac") and not hasattr(step, "d_randoms_sw"), "sampling inputs were gathered"
    finally:
        step.close()
    against_the_full_extent_step(eager, reference[config], c["use"], config)
    for k in eager:
        same(graph[k], eager[k], "%s: %s, graph against eager" % (config, k))
    # the step without the key is the parent's: no daylit call in its list
    assert not [n for n in reference[config + "/calls"] if n.startswith("daylit") or n.startswith("sw_active")]


@pytest.mark.parametrize("config", ["seeded-maxran", "seeded-clrsky-aer-g112"])
def test_one_capture_three_suns(dev, case, config):
    """Capture once; replay with every column at night, every column in daylight, and the original angles reversed.
    Each replay equals a freshly built (eager) step on those angles."""
    from rrtmgpnn.pipeline import ClearSkyStep
    c = case
    prob, ncol = c["prob"], c["prob"]["ncol"]
    step = ClearSkyStep(prob, **kwargs(c, config, True))
    first = run(step, "graph")
    graph = step.graph
    suns = {"night": np.full(ncol, 120.0, np.float32), "day": np.linspace(0.0, 89.0, ncol).astype(np.float32),
            "reversed": np.ascontiguousarray(prob["sza"][::-1])}
    try:
        for name, sza in suns.items():
            step.set_sza(sza)
            got = run(step, "graph")
            assert step.graph is graph, "set_sza recaptured"
            kw = kwargs(c, config, True)
            fresh = ClearSkyStep(dict(prob, sza=sza), **kw)
            want = run(fresh)
            nday = int(fresh.nday.item())
            fresh.close()
            assert int(step.nday.item()) == nday == {"night": 0, "day": ncol}.get(name, nday)
            for k in got:
                same(got[k], want[k], "%s: %s" % (name, k))
            if name == "night":
                assert all(not got[k].any() for k in got if k.startswith("sw")), "a night block's SW fluxes are exactly 0"
            if name == "day":
                assert all((got[k][:, 0] > 0).all() for k in got if k.startswith("sw_d"))
        step.set_sza(prob["sza"])
        again = run(step, "graph")
        for k in first:
            same(again[k], first[k], "back to the first sun: " + k)
    finally:
        step.close()


def test_all_night_block_gives_exact_zeros(dev, case):
    from rrtmgpnn.pipeline import ClearSkyStep
    c = case
    prob = dict(c["prob"], sza=np.full(c["prob"]["ncol"], 100.0, np.float32))
    step = ClearSkyStep(prob, **kwargs(c, "seeded-clrsky-aer-g112", True))
    try:
        got = run(step)
        assert int(step.nday.item()) == 0
    finally:
        step.close()
    for k in got:
        if k.startswith("sw"):
            assert not got[k].any() and np.isfinite(got[k]).all(), k
        else:
            assert np.isfinite(got[k]).all() and (got[k] > 0).any(), k


def test_new_seed_randoms_and_aerosols_between_replays(dev, case):
    """set_mcica_seed, set_mcica_randoms and set_aerosols between replays of one capture: each equals a freshly built
    step with those values, and the clouds (or the aerosol) did change."""
    from rrtmgpnn.pipeline import ClearSkyStep
    c = case
    step = ClearSkyStep(c["prob"], **kwargs(c, "seeded-maxran", True))
    try:
        a = run(step, "graph")
        graph = step.graph
        step.set_mcica_seed(seed=SEED_B)
        b = run(step, "graph")
        assert step.graph is graph
    finally:
        step.close()
    fresh = ClearSkyStep(c["prob"], **kwargs(c, "seeded-maxran", True, seed=SEED_B))
    want = run(fresh)
    fresh.close()
    for k in b:
        same(b[k], want[k], "after set_mcica_seed: " + k)
    assert (a["sw_dn"] != b["sw_dn"]).any() and (a["lw_dn"] != b["lw_dn"]).any()

    step = ClearSkyStep(c["prob"], **kwargs(c, "arrays-expran-aer", True))
    try:
        a = run(step, "graph")
        graph = step.graph
        step.set_mcica_randoms(randoms_sw=c["r_sw"][1])
        step.set_aerosols(**c["aer"][1])
        b = run(step, "graph")
        assert step.graph is graph
    finally:
        step.close()
    kw = kwargs(c, "arrays-expran-aer", True)
    kw["mcica"]["randoms_sw"] = c["r_sw"][1]
    kw["aerosols"] = c["aer"][1]
    fresh = ClearSkyStep(c["prob"], **kw)
    want = run(fresh)
    fresh.close()
    for k in b:
        same(b[k], want[k], "after set_mcica_randoms and set_aerosols: " + k)
    assert (a["sw_dn"] != b["sw_dn"]).any()


@pytest.mark.parametrize("more", [dict(nmus=3), dict(jacobian=True), dict(lw_scattering=True)],
                         ids=["nmus3", "jacobian", "lw_scattering"])
def test_lw_options_pass_through(dev, case, more):
    from rrtmgpnn.pipeline import ClearSkyStep
    c = case
    out = {}
    for daylit in (False, True):
        kw = kwargs(c, "seeded-maxran", daylit)
        step = ClearSkyStep(c["prob"], **dict(kw, **more))
        out[daylit] = dict(run(step), **({"jac": step.jacobian_flux()} if "jacobian" in more else {}))
        step.close()
    for k in ("lw_up", "lw_dn") + (("jac",) if "jacobian" in more else ()):
        same(out[True][k], out[False][k], k)
    for k in ("sw_up", "sw_dn", "sw_dir"):
        same(out[True][k][c["use"]], out[False][k][c["use"]], k)
        assert not out[True][k][~c["use"]].any()


def test_refused_combinations_and_chain_capture(dev, case):
    from rrtmgpnn.pipeline import ClearSkyStep
    c = case
    kw = kwargs(c, "seeded-maxran", True)
    for more, word in ((dict(sw_dual=True), "sw_dual"), (dict(fused=False), "fused=False")):
        with pytest.raises(ValueError, match=r"mcica\['daylit'\] with .*" + word):
            ClearSkyStep(c["prob"], **dict(kw, **more))
    with pytest.raises(ValueError, match=r"mcica\['daylit'\] with .*byband"):
        ClearSkyStep(c["prob"], **dict(kw, mcica=dict(kw["mcica"], byband=True)))
    with pytest.raises(ValueError, match="daylit=True with .*mcica"):
        ClearSkyStep(c["prob"], daylit=True, **kw)
    step = ClearSkyStep(c["prob"], **kw)
    try:
        with pytest.raises(ValueError, match=r"mcica\['daylit'\] with capture_chains / run_blocks"):
            step.capture_chains()
        with pytest.raises(ValueError, match=r"mcica\['daylit'\] with capture_chains / run_blocks"):
            step.run_blocks(1)
    finally:
        step.close()
