"""GPU: ClearSkyStep(..., sw_dual=True) -- the SW chain's clear and all-sky solves as one call of
rrtmgpnn_sw_solver_2stream_rfmip_clr_all -- against the same step without sw_dual, on all ten flux arrays, bit for bit,
eager and captured, in both modes of rrtmgpnn_context_set_sw_clr_all; its call list; the constructor's refusals.  And
the class layer: clr_all_sky.rte_sw through the new entry against its two-solve route.  4 RFMIP columns, the
environment of tests/step_plan.py."""
import numpy as np
import pytest

import step_plan as P

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
FLUX = ("lw_up", "lw_dn", "sw_up", "sw_dn", "sw_dir")
ALL = FLUX + tuple(k + "_clr" for k in FLUX)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a device"
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def env(rfmip):
    return P.environment(rfmip)


@pytest.fixture
def mode():
    from rrtmgpnn import api
    yield api.set_sw_clr_all_default
    api.set_sw_clr_all_default(0)


def _aerosols(ncol, nlay, seed):
    from rrtmgpnn import data
    nb_lw, nb_sw = data.load_kdist("lw")["nband"], data.load_kdist("sw")["nband"]
    rng = np.random.default_rng(seed)
    return {"lw_tau": rng.lognormal(-2, 1, (ncol, nlay, nb_lw)).astype(np.float32),
            "sw_tau": rng.lognormal(-2, 1, (ncol, nlay, nb_sw)).astype(np.float32),
            "sw_ssa": rng.uniform(0.6, 1, (ncol, nlay, nb_sw)).astype(np.float32),
            "sw_g": rng.uniform(0.3, 0.8, (ncol, nlay, nb_sw)).astype(np.float32)}


def _kwargs(e, variant):
    kw = {"clouds": e["clouds"]}
    if variant == "allsky":
        kw["clrsky"] = True
    else:
        kw["mcica"] = {"cloud_frac": e["cloud_frac"], "overlap_param": e["overlap_param"], "seed": 2026, "clrsky": True}
    if variant == "aerosols":
        kw["aerosols"] = _aerosols(e["prob"]["ncol"], e["prob"]["nlay"], 98)
    return kw


def _poison(step):
    for k in ALL:
        getattr(step, k).fill_(float("nan"))


def _out(step):
    torch.cuda.synchronize()
    out = dict(step.fluxes())
    out.update(step.clrsky_fluxes())
    assert set(out) == set(ALL) and not any(np.isnan(v).any() for v in out.values())
    return out


def _run(step, how="step"):
    _poison(step)
    getattr(step, how)()
    return _out(step)


def _equal(got, want, what):
    for k in ALL:
        np.testing.assert_array_equal(got[k], want[k], err_msg="%s %s" % (what, k))


@pytest.mark.parametrize("m", [1, 2], ids=["dual", "two_launches"])
@pytest.mark.parametrize("variant", ["allsky", "mcica", "aerosols"])
def test_sw_dual_step_equals_the_two_launch_step(dev, env, mode, variant, m):
    from rrtmgpnn import _lib
    from rrtmgpnn.pipeline import ClearSkyStep
    mode(m)
    kw = _kwargs(env, variant)
    ref = ClearSkyStep(env["prob"], device=0, **kw)
    step = ClearSkyStep(env["prob"], device=0, sw_dual=True, **kw)
    try:
        names = [n for n, _, _ in step.calls]
        assert names.count("sw_solver") == 1 and "sw_solver_clr" not in names
        assert [f for n, f, _ in step.calls if n == "sw_solver"] == [_lib.lib().rrtmgpnn_sw_solver_2stream_rfmip_clr_all]
        assert "sw_solver_clr" in [n for n, _, _ in ref.calls]
        assert [(n, f) for n, f, _ in step.calls if not n.startswith("sw_solver")] == \
            [(n, f) for n, f, _ in ref.calls if not n.startswith("sw_solver")]
        want = _run(ref)
        assert (want["sw_dn"] != want["sw_dn_clr"]).any(), "the clouds do not show"
        _equal(_run(step), want, "eager")
        step.capture()
        _equal(_run(step, "replay"), want, "captured")
        if variant == "aerosols":
            other = _aerosols(env["prob"]["ncol"], env["prob"]["nlay"], 99)
            ref.set_aerosols(**other)
            step.set_aerosols(**other)
            want2 = _run(ref)
            assert (want2["sw_dn_clr"] != want["sw_dn_clr"]).any(), "the new aerosols do not show"
            _equal(_run(step, "replay"), want2, "replay after set_aerosols")
    finally:
        step.close()
        ref.close()


def test_constructor_refusals(dev, env):
    from rrtmgpnn.pipeline import ClearSkyStep
    e = env
    for kw in ({"clouds": e["clouds"]}, {},
               {"clouds": e["clouds"], "clrsky": True, "sw": False},
               {"clouds": e["clouds"], "clrsky": True, "fused": False},
               {"clouds": e["clouds"], "byband": True},
               {"clouds": e["clouds"], "mcica": {"cloud_frac": e["cloud_frac"], "seed": 1, "byband": True}}):
        with pytest.raises(ValueError, match="sw_dual"):
            ClearSkyStep(e["prob"], device=0, sw_dual=True, **kw)


# ---- the class layer ------------------------------------------------------------------------------------------------------
def T(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=dev)


def _band_props(api, kd, arrays, dev):
    op = api.OpticalProps2str()
    assert op.init(kd.get_band_lims_wavenumber()) == ""
    ncol, nlay = arrays[0].shape[:2]
    assert op.alloc_2str(ncol, nlay, device=dev) == ""
    for k, a in zip(("tau", "ssa", "g"), arrays):
        getattr(op, k).copy_(T(a, dev))
    return op


@pytest.fixture(scope="module")
def class_case(dev, env):
    from rrtmgpnn import api, data
    import mcica_ref as M
    p = env["prob"]
    ncol, nlay = p["ncol"], p["nlay"]
    kd = api.GasOpticsRRTMGP()
    api.stop_on_err(kd.load("sw"))
    nets = [api.RrtmgpNetwork(0).load_netcdf(data.path(n)) for n in ("sw_abs", "sw_ray")]
    gc = api.GasConcs()
    api.stop_on_err(gc.init(list(p["gases"])))
    for k, v in p["gases"].items():
        api.stop_on_err(gc.set_vmr(k, T(v, dev)))
    nb, ng = kd.get_nband(), kd.get_ngpt()
    r = np.random.default_rng(196)
    shape = (ncol, nlay, nb)
    cloudy = (r.uniform(size=(ncol, nlay, 1)) < 0.6) & (np.arange(ncol) != 1)[:, None, None]
    cld = _band_props(api, kd, [np.where(cloudy, r.lognormal(0, 1, shape), 0), r.uniform(0.5, 1, shape),
                                r.uniform(0, 0.9, shape)], dev)
    aer = _band_props(api, kd, [r.lognormal(-2, 1, shape), r.uniform(0.6, 1, shape), r.uniform(0.3, 0.8, shape)], dev)
    mask = r.random((ncol, nlay, ng)) < 0.5
    return dict(kd=kd, nets=nets, gc=gc, cld=cld, aer=aer, nb=nb, ng=ng,
                bits=torch.as_tensor(M.pack_bits(mask).view(np.int32), device=dev),
                bytes=torch.as_tensor(mask.astype(np.uint8), device=dev),
                state=[T(p[k], dev) for k in ("play", "tlay", "plev")], mu0=T(p["mu0"], dev),
                alb=T(np.repeat(np.asarray(p["sfc_alb"], np.float32)[:, None], nb, axis=1), dev),
                toa=T(data.toa_flux(p, data.load_kdist("sw")), dev), ncol=ncol, nlay=nlay)


def _class_call(c, dev, fused, counts, masked=False, aer=False, fluxes=None, net=False):
    """clr_all_sky.rte_sw with SW_CLR_ALL_FUSED = fused -> the six arrays (and the two nets); counts: the number of
    calls of the new entry, seen from outside through the library's function table."""
    from rrtmgpnn import _lib, api, clr_all_sky
    nan = lambda: torch.full((c["ncol"], c["nlay"] + 1), float("nan"), device=dev)  # noqa: E731
    mk = fluxes or (lambda: api.FluxesBroadband(nan(), nan(), nan(), nan() if net else None))
    f_all, f_clr = mk(), mk()
    L = _lib.lib()
    inner = L.rrtmgpnn_sw_solver_2stream_clr_all

    def counted(*a):
        counts.append(1)
        return inner(*a)
    clr_all_sky.SW_CLR_ALL_FUSED = fused
    L.rrtmgpnn_sw_solver_2stream_clr_all = counted
    try:
        e = clr_all_sky.rte_sw(c["kd"], c["gc"], *c["state"], c["mu0"], c["alb"], c["alb"], c["cld"], f_all, f_clr,
                               aer_props=c["aer"] if aer else None, inc_flux=c["toa"], neural_nets=c["nets"],
                               **(masked if isinstance(masked, dict) else {"mask_bits": c["bits"]} if masked else {}))
    finally:
        L.rrtmgpnn_sw_solver_2stream_clr_all = inner
        clr_all_sky.SW_CLR_ALL_FUSED = True
    assert e == "", e
    torch.cuda.synchronize()
    out = [f_all.flux_up, f_all.flux_dn, f_all.flux_dn_dir, f_clr.flux_up, f_clr.flux_dn, f_clr.flux_dn_dir]
    if net:
        out += [f_all.flux_net, f_clr.flux_net]
    return [o.cpu().numpy() for o in out], (f_all, f_clr)


@pytest.mark.parametrize("m", [1, 2], ids=["dual", "two_launches"])
@pytest.mark.parametrize("aer", [False, True], ids=["noaer", "aer"])
@pytest.mark.parametrize("masked", [False, True], ids=["overcast", "masked"])
def test_class_rte_sw_one_call_equals_the_two_solves(dev, class_case, mode, masked, aer, m):
    mode(m)
    n_new, n_old = [], []
    got, _ = _class_call(class_case, dev, True, n_new, masked, aer, net=True)
    want, _ = _class_call(class_case, dev, False, n_old, masked, aer, net=True)
    assert (len(n_new), len(n_old)) == (1, 0), "rte_sw took the other route"
    assert all(np.isfinite(g).all() for g in got) and (got[1] != got[4]).any()
    for i, (g, w) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(g, w, err_msg="array %d" % i)


def test_class_rte_sw_other_cases_keep_the_old_route(dev, class_case):
    """By-band flux objects, and a byte mask without mask_bits, do not take the new entry."""
    from rrtmgpnn import api
    c = class_case
    nan = lambda *s: torch.full(s, float("nan"), device=dev)  # noqa: E731
    lev = (c["ncol"], c["nlay"] + 1)
    byband = lambda: api.FluxesByBand(bnd_flux_up=nan(*lev, c["nb"]), bnd_flux_dn=nan(*lev, c["nb"]),  # noqa: E731
                                      flux_up=nan(*lev), flux_dn=nan(*lev), flux_dn_dir=nan(*lev))
    n = []
    got, (f_all, _) = _class_call(c, dev, True, n, fluxes=byband)
    assert n == [] and torch.isfinite(f_all.bnd_flux_up).all()
    plain, _ = _class_call(c, dev, True, n)
    assert len(n) == 1
    for g, w in zip(got, plain):
        np.testing.assert_array_equal(g, w)
    del n[:]
    bytes_only, _ = _class_call(c, dev, True, n, masked={"cloud_mask": c["bytes"]})
    assert n == []
    bits, _ = _class_call(c, dev, True, n, masked=True)
    assert len(n) == 1
    for g, w in zip(bytes_only, bits):
        np.testing.assert_array_equal(g, w)
