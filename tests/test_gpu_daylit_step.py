"""GPU: ClearSkyStep(daylit=True), the SW chain on the daylit columns of the block, bit for bit.

The step's sw_up / sw_dn are the oracle's with the driver's zeroing (rrtmgp_rfmip_sw.F90:456-463) on every column,
sw_dir the oracle's on the daylit columns and 0 at night, and the LW fluxes those of the default step
(tests/test_daylit_host.py shows on the oracle alone that solving the daylit columns by themselves changes no bit).  One
capture serves any sun: after set_sza a replay equals a freshly built step on those angles, all night included."""
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
SW = FLUX[2:]
# the SW context's last solver launch: family 7, the small-grid instance with its planes (1024 | 8 | 16 | 2048) or the
# band-pair increment with the transmittance plane (2 | 8 | 32 | 2048)
PATH_CLEAR, PATH_OVERCAST = [7, 3096], [7, 2090]
F_ACTIVE = 16


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a device"
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def case(rfmip):
    """The first 36 RFMIP columns (16 of them night columns, usecol false) and the all-sky example's clouds"""
    from rrtmgpnn import data
    prob = subset(rfmip, np.arange(36))
    assert int((~prob["usecol"]).sum()) == 16
    clouds = data.allsky_clouds(prob, data.load_cloud_optics("lw"))
    assert any((c[prob["usecol"]] > 0).any() for c in clouds[:2])
    return dict(prob=prob, use=prob["usecol"], clouds=clouds)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(got, want, msg):
    np.testing.assert_array_equal(bits(got), bits(want), err_msg=msg)


def poison(step):
    for k in FLUX:
        getattr(step, k).fill_(float("nan"))
    torch.cuda.synchronize()


def run(step, how="eager"):
    poison(step)
    if how == "eager":
        step.step()
    else:
        if step.graph is None:
            step.capture()
            poison(step)
        step.replay()
    torch.cuda.synchronize()
    return step.fluxes()


def paths(step):
    from rrtmgpnn import _lib
    c = step.ctx2 if step.ctx2 is not None else step.ctx
    s, m = (ctypes.c_int * 4)(), (ctypes.c_int * 8)()
    _lib.check(_lib.lib().rrtmgpnn_context_get_solver_path(c.h, s), "get_solver_path")
    _lib.check(_lib.lib().rrtmgpnn_context_get_mlp_path(c.h, m), "get_mlp_path")
    return list(s)[:2], list(m)


def models(spectral):
    from rrtmgpnn import data
    if spectral is None:
        return [data.load_model("sw_abs"), data.load_model("sw_ray")], data.load_kdist("sw")
    return [data.load_model(PATHS["sw_abs"]), data.load_model(PATHS["sw_ray"])], data.load_kdist("sw", 112)


def expected_sw(orc, c, spectral, overcast):
    from rrtmgpnn import data
    ms, kd = models(spectral)
    if overcast:
        up, dn, dr, _ = orc.all_sky_sw(c["prob"], ms, kd, data.load_cloud_optics("sw"), c["clouds"], zero_unused=True)
    else:
        up, dn, dr, _ = orc.clear_sky_sw(c["prob"], ms, kd, zero_unused=True)
    dr = np.where(c["use"][:, None], dr, np.float32(0))   # the direct flux of a night column: defined as 0 here
    assert (up[c["use"]] > 0).any() and not up[~c["use"]].any()
    return dict(sw_up=up, sw_dn=dn, sw_dir=dr)


@pytest.mark.parametrize("overcast", [False, True], ids=["clear", "overcast"])
@pytest.mark.parametrize("spectral", [None, SPECTRAL], ids=["g256-g224", "g128-g112"])
def test_step_equals_the_oracle_with_the_drivers_zeroing(dev, orc, case, spectral, overcast):
    from rrtmgpnn.pipeline import ClearSkyStep
    c = case
    kw = dict(device=0, spectral=spectral, clouds=c["clouds"] if overcast else None)
    default = ClearSkyStep(c["prob"], **kw)
    ref = run(default)
    default.close()
    step = ClearSkyStep(c["prob"], daylit=True, **kw)
    eager = run(step)
    sp, mp = paths(step)
    graph = run(step, "graph")
    nday = int(step.nday.item())
    step.close()
    assert nday == int(c["use"].sum())
    assert sp == (PATH_OVERCAST if overcast else PATH_CLEAR) and mp[7] & F_ACTIVE, (sp, mp)
    want = expected_sw(orc, c, spectral, overcast)
    for k in SW:
        same(eager[k], want[k], k + " against the oracle")
    for k in ("lw_up", "lw_dn"):
        same(eager[k], ref[k], k + " against the default step")
    for k in SW:   # the default step on the daylit columns (its night columns hold the mu0 = 1 solve)
        same(eager[k][c["use"]], ref[k][c["use"]], k + " against the default step, daylit columns")
    for k in FLUX:
        same(graph[k], eager[k], k + ": graph against eager")


@pytest.mark.parametrize("nmus", [3])
def test_step_lw_options_pass_through(dev, orc, case, nmus):
    from rrtmgpnn.pipeline import ClearSkyStep
    c = case
    default = ClearSkyStep(c["prob"], device=0, nmus=nmus, jacobian=True)
    ref = dict(run(default), jac=default.jacobian_flux())
    default.close()
    step = ClearSkyStep(c["prob"], device=0, nmus=nmus, jacobian=True, daylit=True)
    got = dict(run(step), jac=step.jacobian_flux())
    step.close()
    want = expected_sw(orc, c, None, False)
    for k in SW:
        same(got[k], want[k], k)
    for k in ("lw_up", "lw_dn", "jac"):
        same(got[k], ref[k], k)


@pytest.mark.parametrize("overcast", [False, True], ids=["clear", "overcast"])
def test_one_capture_three_suns(dev, case, overcast):
    """Capture once; replay with every column at night, every column in daylight, and the original angles reversed.
    Each replay equals a freshly built (eager) step on those angles."""
    from rrtmgpnn.pipeline import ClearSkyStep
    c = case
    prob, ncol = c["prob"], c["prob"]["ncol"]
    kw = dict(device=0, daylit=True, clouds=c["clouds"] if overcast else None)
    step = ClearSkyStep(prob, **kw)
    first = run(step, "graph")
    graph = step.graph
    suns = {"night": np.full(ncol, 120.0, np.float32), "day": np.linspace(0.0, 89.0, ncol).astype(np.float32),
            "reversed": np.ascontiguousarray(prob["sza"][::-1])}
    try:
        for name, sza in suns.items():
            step.set_sza(sza)
            got = run(step, "graph")
            assert step.graph is graph, "set_sza recaptured"
            fresh = ClearSkyStep(dict(prob, sza=sza), **kw)
            want = run(fresh)
            nday = int(fresh.nday.item())
            fresh.close()
            assert int(step.nday.item()) == nday == {"night": 0, "day": ncol}.get(name, nday)
            for k in FLUX:
                same(got[k], want[k], "%s: %s" % (name, k))
            if name == "night":
                assert all(not got[k].any() for k in SW), "a night block's SW fluxes are exactly 0"
            if name == "day":
                assert all((got[k][:, 0] > 0).all() for k in ("sw_dn", "sw_dir"))
        step.set_sza(prob["sza"])
        again = run(step, "graph")
        for k in FLUX:
            same(again[k], first[k], "back to the first sun: " + k)
    finally:
        step.close()


@pytest.mark.parametrize("kw, word", [(dict(mcica={"cloud_frac": None}), "mcica"), (dict(aerosols={}), "aerosols"),
                                      (dict(clrsky=True), "clrsky"), (dict(byband=True), "byband"),
                                      (dict(sw_dual=True), "sw_dual"), (dict(fused=False), "fused=False"),
                                      (dict(sw=False), "sw=False")])
def test_refused_combinations(dev, case, kw, word):
    from rrtmgpnn.pipeline import ClearSkyStep
    with pytest.raises(ValueError, match="daylit=True with .*" + word):
        ClearSkyStep(case["prob"], device=0, daylit=True, clouds=case["clouds"], **kw)


def test_refused_chain_capture(dev, case):
    from rrtmgpnn.pipeline import ClearSkyStep
    step = ClearSkyStep(case["prob"], device=0, daylit=True)
    try:
        with pytest.raises(ValueError, match="daylit=True with capture_chains / run_blocks"):
            step.capture_chains()
        with pytest.raises(ValueError, match="daylit=True with capture_chains / run_blocks"):
            step.run_blocks(1)
    finally:
        step.close()
