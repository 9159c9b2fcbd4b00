"""GPU: ClearSkyStep(..., sfc_byband=True), the SW fluxes at the surface by band from the step's all-sky launch, bit for
bit, on the first 36 RFMIP columns (16 of them at night) with a cloud fraction per layer.

  * seeded McICA without aerosols: the surface level of sw_bnd_* of the existing mcica={..., "byband": True} step;
  * with aerosols: the class layer's composition on the step's own arrays -- arm_cloud_mask + arm_aerosol +
    arm_sfc_byband + rte_sw(band_inc=) behind rrtmgpnn_sw_boundary_rfmip;
  * with mcica["daylit"] on a half-night sza: zeros at night, the full-extent step's values in daylight, and after
    capture() a set_sza to another pattern and replay() give that pattern's values without recapture;
  * the broadband fluxes of each step are those of the same step without sfc_byband;
  * every refused combination raises ValueError naming the pair."""
import ctypes

import numpy as np
import pytest

from conftest import subset

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FLUX = ("lw_up", "lw_dn", "sw_up", "sw_dn", "sw_dir")
CLR = ("lw_up_clr", "lw_dn_clr", "sw_up_clr", "sw_dn_clr", "sw_dir_clr")
SFC = ("sw_sfc_bnd_up", "sw_sfc_bnd_dn", "sw_sfc_bnd_dir")
SEED = 20261021
SW_CK_SFC_BAND, CK_SFC, CK_ACTIVE = 9, 4096, 2048


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a device"
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def case(rfmip):
    from rrtmgpnn import data
    prob = subset(rfmip, np.arange(36))
    ncol, nlay = prob["ncol"], prob["nlay"]
    assert int((~prob["usecol"]).sum()) == 16
    clouds = data.allsky_clouds(prob, data.load_cloud_optics("lw"))
    cloudy = (clouds[0] > 0) | (clouds[1] > 0)
    assert cloudy[prob["usecol"]].any()
    rng = np.random.default_rng(83)
    cf = np.where(cloudy, rng.uniform(0.2, 0.9, cloudy.shape), 0).astype(np.float32)
    kl, ks = data.load_kdist("lw"), data.load_kdist("sw")
    aer = {"lw_tau": rng.lognormal(-2, 1, (ncol, nlay, kl["nband"])).astype(np.float32),
           "sw_tau": rng.lognormal(-2, 1, (ncol, nlay, ks["nband"])).astype(np.float32),
           "sw_ssa": rng.uniform(0.6, 1, (ncol, nlay, ks["nband"])).astype(np.float32),
           "sw_g": rng.uniform(0.3, 0.8, (ncol, nlay, ks["nband"])).astype(np.float32)}
    # another sun: the angles reversed, so other columns are at night
    sza2 = np.ascontiguousarray(prob["sza"][::-1])
    use2 = np.ascontiguousarray(prob["usecol"][::-1])
    assert (use2 != prob["usecol"]).any()
    return dict(prob=prob, use=prob["usecol"], clouds=clouds, cf=cf, aer=aer, sza2=sza2, use2=use2)


def make(c, aerosols=False, **mcica):
    from rrtmgpnn.pipeline import ClearSkyStep
    sfc = mcica.pop("sfc_byband", False)
    kw = {"device": 0, "clouds": c["clouds"], "mcica": dict(cloud_frac=c["cf"], overlap_param=None, seed=SEED, **mcica)}
    if aerosols:
        kw["aerosols"] = c["aer"]
    return ClearSkyStep(c["prob"], sfc_byband=sfc, **kw) if sfc else ClearSkyStep(c["prob"], **kw)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(got, want, msg):
    np.testing.assert_array_equal(bits(got), bits(want), err_msg=msg)


def names(step):
    return FLUX + (CLR if step.clrsky else ()) + (SFC if getattr(step, "sfc_byband", False) else ())


def run(step, how="eager"):
    for k in names(step):
        getattr(step, k).fill_(float("nan"))
    torch.cuda.synchronize()
    if how == "eager":
        step.step()
    else:
        step.replay()
    torch.cuda.synchronize()
    return {k: getattr(step, k).cpu().numpy() for k in names(step)}


def sw_path(step):
    from rrtmgpnn import _lib
    c = step.ctx2 if step.ctx2 is not None else step.ctx
    s = (ctypes.c_int * 4)()
    _lib.check(_lib.lib().rrtmgpnn_context_get_solver_path(c.h, s), "get_solver_path")
    return list(s)


def test_mcica_step_equals_the_surface_level_of_the_byband_step(dev, case):
    step = make(case, sfc_byband=True)
    got = run(step)
    assert [n for n, _, _ in step.calls].count("sw_sfc_byband") == 1
    names_ = [n for n, _, _ in step.calls]
    assert names_.index("sw_sfc_byband") + 1 == names_.index("sw_solver")
    path = sw_path(step)
    assert path[0] == SW_CK_SFC_BAND and path[1] & CK_SFC and path[3] == 12, path
    assert sorted(step.sfc_byband_fluxes()) == sorted(SFC)
    step.close()
    ref = make(case, byband=True)
    run(ref)
    bnd = ref.byband_fluxes()
    sfc = ref.nlay if ref.top_at_1 else 0
    ref.close()
    for k in ("up", "dn", "dir"):
        want = bnd["sw_bnd_" + k][:, sfc]
        assert want.shape == got["sw_sfc_bnd_" + k].shape and (want > 0).any()
        same(got["sw_sfc_bnd_" + k], want, "sw_sfc_bnd_" + k)
    plain = make(case)
    want = run(plain)
    calls = [n for n, _, _ in plain.calls]
    plain.close()
    assert calls == [n for n in names_ if n != "sw_sfc_byband"]
    for k in FLUX:
        same(got[k], want[k], k + ": the step without sfc_byband")


def test_aerosol_step_equals_the_class_layer_composition(dev, case):
    from rrtmgpnn import _lib, api, cloud_sampling as cs
    step = make(case, aerosols=True, sfc_byband=True)
    got = run(step)
    ctx = api.context(0)
    L = _lib.lib()
    ncol, nlay, ngpt, nb = step.ncol, step.nlay, step.ng_sw, step.nb_sw
    kd = step.kd_sw
    toa, alb = (torch.zeros(ncol, ngpt, device=dev) for _ in range(2))
    mu0 = torch.zeros(ncol, device=dev)
    _lib.check(L.rrtmgpnn_sw_boundary_rfmip(ctx.h, ngpt, ncol, step.solar_source.data_ptr(), step.tsi.data_ptr(),
                                            step.sfc_alb.data_ptr(), step.sza.data_ptr(), toa.data_ptr(), alb.data_ptr(),
                                            mu0.data_ptr()), "sw_boundary_rfmip")

    def props(t, w, g, gpt):
        op = api.OpticalProps2str()
        assert (op.init(kd["band_lims_wvn"], kd["band_lims_gpt"]) if gpt else op.init(kd["band_lims_wvn"])) == ""
        op.tau, op.ssa, op.g = t, w, g
        return op

    fl3 = [torch.full((ncol, nlay + 1), float("nan"), device=dev) for _ in range(3)]
    so = [torch.full((ncol, nb), float("nan"), device=dev) for _ in range(3)]
    cs.arm_cloud_mask(ctx, ngpt, step.mask_bits_sw)
    cs.arm_aerosol(ctx, props(step.aer_tau_sw, step.aer_ssa_sw, step.aer_g_sw, False))
    cs.arm_sfc_byband(ctx, kd["band_lims_gpt"], *so)
    assert api.rte_sw(props(step.tau_sw, step.ssa_sw, None, True), bool(step.top_at_1), mu0, toa, alb, alb,
                      api.FluxesBroadband(flux_up=fl3[0], flux_dn=fl3[1], flux_dn_dir=fl3[2]),
                      band_inc=props(step.cld_tau_sw, step.cld_ssa_sw, step.cld_g_sw, False)) == ""
    torch.cuda.synchronize()
    for k, t in zip(("up", "dn", "dir"), so):
        same(got["sw_sfc_bnd_" + k], t.cpu().numpy(), "sw_sfc_bnd_" + k)
        assert (got["sw_sfc_bnd_" + k] > 0).any()
    for k, t in zip(("sw_up", "sw_dn", "sw_dir"), fl3):
        same(got[k], t.cpu().numpy(), k)
    step.close()
    plain = make(case, aerosols=True)
    want = run(plain)
    plain.close()
    for k in FLUX:
        same(got[k], want[k], k + ": the step without sfc_byband")


def test_daylit_step_follows_the_sun_without_recapture(dev, case):
    use, use2 = case["use"], case["use2"]
    full = make(case, aerosols=True, clrsky=True, sfc_byband=True)
    ref = run(full)
    full.set_sza(case["sza2"])
    ref2 = run(full)
    full.close()
    step = make(case, aerosols=True, clrsky=True, daylit=True, sfc_byband=True)
    names_ = [n for n, _, _ in step.calls]
    assert names_.count("daylit_scatter_sfc") == 1 and names_.index("sw_sfc_byband") + 1 == names_.index("sw_solver")
    got = run(step)
    path = sw_path(step)   # the last SW launch is the clear one (family 7); the all-sky launch is checked through its outputs
    assert path[0] in (7, SW_CK_SFC_BAND), path

    def check(got, ref, use, what):
        for k in SFC:
            same(got[k][use], ref[k][use], "%s: %s on the daylit columns" % (what, k))
            assert not got[k][~use].any(), "%s: %s is not exactly 0 at night" % (what, k)
            assert (got[k][use] > 0).any()

    check(got, ref, use, "eager")
    plain = make(case, aerosols=True, clrsky=True, daylit=True)
    want = run(plain)
    plain.close()
    for k in FLUX + CLR:
        same(got[k], want[k], k + ": the daylit step without sfc_byband")
    step.capture()
    check(run(step, "replay"), ref, use, "replay")
    step.set_sza(case["sza2"])
    got2 = run(step, "replay")
    check(got2, ref2, use2, "replay after set_sza")
    assert any((bits(got2[k]) != bits(got[k])).any() for k in SFC)
    step.close()


def test_refused_combinations(case):
    from rrtmgpnn.pipeline import ClearSkyStep
    c = case
    mc = dict(cloud_frac=c["cf"], overlap_param=None, seed=SEED)
    base = dict(device=0, clouds=c["clouds"], mcica=mc, sfc_byband=True)
    for word, kw in (("byband", dict(base, mcica=None, aerosols=None, byband=True)),
                     ("mcica['byband']", dict(base, mcica=dict(mc, byband=True))),
                     ("sw_dual", dict(base, mcica=dict(mc, clrsky=True), sw_dual=True)),
                     ("fused=False", dict(base, fused=False)),
                     ("sw=False", dict(base, sw=False)),
                     ("daylit=True", dict(base, mcica=None, daylit=True)),
                     ("neither mcica nor aerosols", dict(base, mcica=None)),
                     ("no clouds", dict(base, clouds=None, mcica=None, aerosols=c["aer"]))):
        with pytest.raises(ValueError, match="sfc_byband=True with .*" + word.replace("[", r"\[").replace("]", r"\]")):
            ClearSkyStep(c["prob"], **kw)
    step_off = ClearSkyStep(c["prob"], device=0, clouds=c["clouds"], mcica=mc)
    with pytest.raises(ValueError, match="sfc_byband"):
        step_off.sfc_byband_fluxes()
    step_off.close()
