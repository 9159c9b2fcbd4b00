"""GPU: by-band fluxes (ty_fluxes_byband) summed inside the solvers (rrtmgpnn_solver_request_byband), the standalone
rrtmgpnn_sum_byband, the request's lifetime, the class layer and ClearSkyStep(byband=True) -- all bit for bit against
the oracle's g-point outputs (pinned to the reference's rte_lw / rte_sw by tests/test_oracle.py) reduced by the
sequential float32 sum_byband of tests/byband_ref.py."""
import numpy as np
import pytest

import byband_ref as R
from conftest import subset

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a device"
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def T(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=dev)


def P(t):
    return t.data_ptr() if t is not None else None


def nan(dev, *shape):
    return torch.full(shape, NAN, device=dev)


def arm(lims, up, dn, dr):
    from rrtmgpnn import _lib
    from rrtmgpnn._lib import check, int_array
    from rrtmgpnn.api import context
    lims = np.asarray(lims).reshape(-1, 2)
    check(_lib.lib().rrtmgpnn_solver_request_byband(context(0).h, len(lims), int_array(lims.ravel()), P(up), P(dn),
                                                    P(dr)), "solver_request_byband")


def layouts(ngpt, shipped=None):
    out = {"irregular": R.irregular_limits(ngpt), "one": R.one_band(ngpt)}
    if shipped is not None:
        out["shipped"] = np.asarray(shipped, np.int32).reshape(-1, 2)
    return out


_cache = {}


def cached(key, fn):
    """References are computed once and shared among the cases that need them."""
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


# ---- SW two-stream -------------------------------------------------------------------------------------------------
def _sw_case(ngpt, nlay, with_g, ncol=5):
    rng = np.random.default_rng(5 + ngpt + nlay)
    tau = rng.lognormal(-2, 2, size=(ncol, nlay, ngpt)).astype(np.float32)
    ssa = rng.uniform(0, 1, size=(ncol, nlay, ngpt)).astype(np.float32)
    g = rng.uniform(0, 0.9, size=(ncol, nlay, ngpt)).astype(np.float32) if with_g else np.zeros_like(tau)
    mu0 = rng.uniform(0.05, 1, size=ncol).astype(np.float32)
    inc = rng.uniform(0, 10, size=(ncol, ngpt)).astype(np.float32)
    ad, af = (rng.uniform(0, 1, size=(ncol, ngpt)).astype(np.float32) for _ in range(2))
    return tau, ssa, g, mu0, inc, ad, af


def _sw_call(dev, a, ngpt, nlay, ncol, top_at_1, with_g, outs):
    from rrtmgpnn import _lib
    from rrtmgpnn._lib import check
    from rrtmgpnn.api import context
    check(_lib.lib().rrtmgpnn_sw_solver_2stream(
        context(0).h, ngpt, nlay, ncol, int(top_at_1), P(a[4]), None, P(a[0]), P(a[1]), P(a[2]) if with_g else None,
        P(a[3]), P(a[5]), P(a[6]), *[P(t) for t in outs]), "sw_solver_2stream")


@pytest.mark.parametrize("top_at_1", [True, False])
@pytest.mark.parametrize("with_g", [True, False])
@pytest.mark.parametrize("nlay", [4, 10, 19])
@pytest.mark.parametrize("ngpt", [224, 223, 222])
def test_sw_2stream_byband(dev, orc, sw_kernel, ngpt, nlay, with_g, top_at_1):
    """ncol = 5: the last block of the two-columns-per-block kernels holds an absent column; nlay 4 / 10 / 19: a chunk
    remainder of 1 with K = 3, one and two ring refills; 223: the one-g-point-per-lane kernel whatever the mode; 222:
    the sequential broadband sums.  One band over the whole spectrum differs from the broadband flux in its order."""
    from rrtmgpnn import data
    case = _sw_case(ngpt, nlay, with_g)
    ncol = case[0].shape[0]
    want = cached(("sw", ngpt, nlay, with_g, top_at_1), lambda: orc.sw_solver(*case, top_at_1, gpt=True))
    a = [T(x, dev) for x in case]
    plain = [nan(dev, ncol, nlay + 1) for _ in range(3)]
    _sw_call(dev, a, ngpt, nlay, ncol, top_at_1, with_g, plain)
    shipped = data.load_kdist("sw")["band_lims_gpt"] if ngpt == 224 else None
    for name, lims in layouts(ngpt, shipped).items():
        nb = len(lims)
        outs = [nan(dev, ncol, nlay + 1) for _ in range(3)]
        bnd = [nan(dev, ncol, nlay + 1, nb) for _ in range(3)]
        arm(lims, *bnd)
        _sw_call(dev, a, ngpt, nlay, ncol, top_at_1, with_g, outs)
        torch.cuda.synchronize()
        for x, y, what in zip(bnd, want[3:], ("bnd_up", "bnd_dn", "bnd_dir")):
            np.testing.assert_array_equal(x.cpu().numpy(), R.sum_byband(y, lims), err_msg="%s %s" % (name, what))
        for x, y, what in zip(outs, plain, ("up", "dn", "dir")):  # the broadband outputs do not move
            np.testing.assert_array_equal(x.cpu().numpy(), y.cpu().numpy(), err_msg="%s %s" % (name, what))
    # the plain call itself is the oracle's broadband without g-point outputs
    ref = cached(("swbb", ngpt, nlay, with_g, top_at_1), lambda: orc.sw_solver(*case, top_at_1))
    for x, y in zip(plain, ref):
        np.testing.assert_array_equal(x.cpu().numpy(), y)


def test_sw_2stream_byband_large_grid(dev, orc):
    """More columns than one round of resident waves holds (64 * 16 lanes per CU at two g-points per lane), g = NULL:
    the checkpointed kernel's large-grid clear-sky instance instead of the small-grid one the 5-column cases run.
    An odd column count, so the last block holds an absent column."""
    from rrtmgpnn import data
    ngpt, nlay = 224, 4
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    ncol = 64 * 16 * cus // (ngpt // 2) + 2
    ncol += 1 - ncol % 2
    case = _sw_case(ngpt, nlay, False, ncol=ncol)
    want = orc.sw_solver(*case, True, gpt=True)
    lims = np.asarray(data.load_kdist("sw")["band_lims_gpt"], np.int32).reshape(-1, 2)
    a = [T(x, dev) for x in case]
    plain = [nan(dev, ncol, nlay + 1) for _ in range(3)]
    outs = [nan(dev, ncol, nlay + 1) for _ in range(3)]
    bnd = [nan(dev, ncol, nlay + 1, len(lims)) for _ in range(3)]
    _sw_call(dev, a, ngpt, nlay, ncol, True, False, plain)
    arm(lims, *bnd)
    _sw_call(dev, a, ngpt, nlay, ncol, True, False, outs)
    torch.cuda.synchronize()
    for x, y, what in zip(bnd, want[3:], ("bnd_up", "bnd_dn", "bnd_dir")):
        np.testing.assert_array_equal(x.cpu().numpy(), R.sum_byband(y, lims), err_msg=what)
    for x, y, what in zip(outs, plain, ("up", "dn", "dir")):
        np.testing.assert_array_equal(x.cpu().numpy(), y.cpu().numpy(), err_msg=what)


def test_one_band_differs_from_broadband_in_bits(orc):
    """The whole-spectrum band is a sequential sum, the broadband flux four interleaved partials: not the same bits
    (so the one-band cases above do check the band walk)."""
    case = _sw_case(224, 10, True)
    w = orc.sw_solver(*case, True, gpt=True)
    assert (R.sum_byband(w[3], R.one_band(224))[..., 0] != w[0]).any()


@pytest.mark.parametrize("layout", ["shipped", "irregular"])
@pytest.mark.parametrize("with_g", [True, False])
def test_sw_2stream_inc_byband(dev, orc, sw_kernel, layout, with_g):
    """The fused cloud increment: band limits that start at even g-points (the band-pair instance of the checkpointed
    kernel) and irregular ones (the general instance); the increment's bands are also the by-band request's."""
    from rrtmgpnn import _lib, data
    from rrtmgpnn._lib import check, int_array
    from rrtmgpnn.api import context
    ngpt, nlay, top_at_1 = 224, 10, True
    case = _sw_case(ngpt, nlay, with_g)
    tau, ssa, g, mu0, inc, ad, af = case
    ncol = tau.shape[0]
    lims = np.asarray(data.load_kdist("sw")["band_lims_gpt"], np.int32).reshape(-1, 2) if layout == "shipped" \
        else R.irregular_limits(ngpt)
    nb = len(lims)
    rng = np.random.default_rng(17)
    s = (ncol, nlay, nb)
    cl = rng.uniform(size=s) < 0.5
    cld = [np.where(cl, rng.lognormal(0, 1, s), 0).astype(np.float32),
           np.where(cl, rng.uniform(0.5, 1, s), 0).astype(np.float32),
           np.where(cl, rng.uniform(0, 0.9, s), 0).astype(np.float32)]

    def ref():
        t2, w2, g2 = orc.increment_bybnd(lims, (tau, ssa, g), cld)
        return orc.sw_solver(t2, w2, g2, mu0, inc, ad, af, top_at_1, gpt=True), \
            orc.sw_solver(t2, w2, g2, mu0, inc, ad, af, top_at_1)
    want, bb = cached(("swinc", layout, with_g), ref)
    a = [T(x, dev) for x in case]
    c = [T(x, dev) for x in cld]
    outs = [nan(dev, ncol, nlay + 1) for _ in range(3)]
    bnd = [nan(dev, ncol, nlay + 1, nb) for _ in range(3)]
    arm(lims, *bnd)
    check(_lib.lib().rrtmgpnn_sw_solver_2stream_inc(
        context(0).h, ngpt, nlay, ncol, int(top_at_1), P(a[4]), None, P(a[0]), P(a[1]), P(a[2]) if with_g else None, nb,
        int_array(lims.ravel()), P(c[0]), P(c[1]), P(c[2]), P(a[3]), P(a[5]), P(a[6]), *[P(t) for t in outs]),
        "sw_solver_2stream_inc")
    torch.cuda.synchronize()
    for x, y, what in zip(bnd, want[3:], ("bnd_up", "bnd_dn", "bnd_dir")):
        np.testing.assert_array_equal(x.cpu().numpy(), R.sum_byband(y, lims), err_msg=what)
    for x, y, what in zip(outs, bb, ("up", "dn", "dir")):
        np.testing.assert_array_equal(x.cpu().numpy(), y, err_msg=what)


def test_sw_rfmip_entry_byband(dev, orc, rfmip, sw_kernel):
    """rrtmgpnn_sw_solver_2stream_rfmip (the boundary conditions formed in the solver) on RFMIP columns."""
    from rrtmgpnn import _lib, data
    from rrtmgpnn._lib import check
    from rrtmgpnn.api import context
    prob = subset(rfmip, np.arange(3, 1800, 263))
    kd = data.load_kdist("sw")
    ncol, nlay, ngpt = prob["ncol"], prob["nlay"], int(kd["ngpt"])
    lims = np.asarray(kd["band_lims_gpt"], np.int32).reshape(-1, 2)
    nb = len(lims)

    def ref():
        go = orc.sw_gas_optics(prob, [data.load_model("sw_abs"), data.load_model("sw_ray")])
        alb = np.repeat(np.asarray(prob["sfc_alb"], np.float32)[:, None], ngpt, axis=1)
        return go, orc.sw_solver(go["tau"], go["ssa"], go["g"], prob["mu0"], data.toa_flux(prob, kd), alb, alb,
                                 prob["top_at_1"], gpt=True)
    go, want = cached("swrfmip", ref)
    sol = T(data.set_tsi(kd["solar_source"], 1361.0), dev)
    ins = [T(prob[k], dev) for k in ("tsi", "sfc_alb", "sza")]
    tau, ssa = T(go["tau"], dev), T(go["ssa"], dev)
    toa, albg, mu0 = nan(dev, ncol, ngpt), nan(dev, ncol, ngpt), nan(dev, ncol)
    outs = [nan(dev, ncol, nlay + 1) for _ in range(3)]
    bnd = [nan(dev, ncol, nlay + 1, nb) for _ in range(3)]
    arm(lims, *bnd)
    check(_lib.lib().rrtmgpnn_sw_solver_2stream_rfmip(
        context(0).h, ngpt, nlay, ncol, int(bool(prob["top_at_1"])), P(sol), *[P(t) for t in ins], P(tau), P(ssa), None,
        0, None, None, None, None, P(toa), P(albg), P(mu0), *[P(t) for t in outs]), "sw_solver_2stream_rfmip")
    torch.cuda.synchronize()
    for x, y, what in zip(bnd, want[3:], ("bnd_up", "bnd_dn", "bnd_dir")):
        np.testing.assert_array_equal(x.cpu().numpy(), R.sum_byband(y, lims), err_msg=what)


@pytest.mark.parametrize("top_at_1", [True, False])
def test_sw_noscat_byband(dev, orc, top_at_1):
    from rrtmgpnn import _lib
    from rrtmgpnn._lib import check
    from rrtmgpnn.api import context
    ngpt, nlay, ncol = 223, 19, 3
    rng = np.random.default_rng(23)
    tau = rng.lognormal(-2, 2, size=(ncol, nlay, ngpt)).astype(np.float32)
    mu0 = rng.uniform(0.05, 1, size=ncol).astype(np.float32)
    inc = rng.uniform(0, 10, size=(ncol, ngpt)).astype(np.float32)
    dr, gdir = orc.sw_solver_noscat(tau, mu0, inc, top_at_1, gpt=True)
    a = [T(x, dev) for x in (inc, tau, mu0)]
    for name, lims in layouts(ngpt).items():
        out, bnd = nan(dev, ncol, nlay + 1), nan(dev, ncol, nlay + 1, len(lims))
        arm(lims, None, None, bnd)
        check(_lib.lib().rrtmgpnn_sw_solver_noscat(context(0).h, ngpt, nlay, ncol, int(top_at_1), P(a[0]), P(a[1]),
                                                   P(a[2]), P(out)), "sw_solver_noscat")
        torch.cuda.synchronize()
        np.testing.assert_array_equal(bnd.cpu().numpy(), R.sum_byband(gdir, lims), err_msg=name)
        np.testing.assert_array_equal(out.cpu().numpy(), dr, err_msg=name)
    # only the direct beam is an output here
    up = nan(dev, ncol, nlay + 1, 1)
    arm(R.one_band(ngpt), up, None, None)
    rc = _lib.lib().rrtmgpnn_sw_solver_noscat(context(0).h, ngpt, nlay, ncol, int(top_at_1), P(a[0]), P(a[1]), P(a[2]),
                                              P(out))
    assert rc == 1 and b"bnd_flux_dn_dir" in _lib.lib().rrtmgpnn_last_error()


# ---- LW ------------------------------------------------------------------------------------------------------------
def _lw_case(ngpt, nlay, ncol=3):
    rng = np.random.default_rng(31 + ngpt + nlay)
    tau = rng.lognormal(-1, 1.5, size=(ncol, nlay, ngpt)).astype(np.float32)
    lay = rng.uniform(1, 50, size=(ncol, nlay, ngpt)).astype(np.float32)
    lev = rng.uniform(1, 50, size=(ncol, nlay + 1, ngpt)).astype(np.float32)
    emis = rng.uniform(0.8, 1.0, size=(ncol, ngpt)).astype(np.float32)
    sfc = rng.uniform(1, 50, size=(ncol, ngpt)).astype(np.float32)
    return tau, lay, lev, emis, sfc


def _lw_gpt_fluxes(orc, case, top_at_1, nmus, ds=None, ssa=None, g=None):
    """The oracle's broadband fluxes and the g-point values the by-band sums add: the g-point fluxes with several
    angles, fac * radiance (or the bare radiance, ngpt % 4 != 0) with one."""
    from oracle import gauss
    tau, lay, lev, emis, sfc = case
    ngpt = tau.shape[-1]
    up, dn, gu, gd = orc.lw_solver(tau, lay, lev, emis, sfc, top_at_1, nmus, lw_Ds=ds, ssa=ssa, g=g, gpt=True)
    if nmus == 1:
        w = gauss(1)[1][0]
        gu, gd = R.lw_one_angle_terms(gu, w, ngpt), R.lw_one_angle_terms(gd, w, ngpt)
    return up, dn, gu, gd


@pytest.mark.parametrize("top_at_1", [True, False])
@pytest.mark.parametrize("mode", ["nmus1", "nmus2", "nmus3", "lw_ds"])
@pytest.mark.parametrize("nlay", [4, 10, 19])
@pytest.mark.parametrize("ngpt", [256, 130])
def test_lw_noscat_byband(dev, orc, ngpt, nlay, mode, top_at_1):
    """256: the lane-per-partial flush over padded ring rows; 130 (not a multiple of 4): the float4-free walk, and at
    one angle the broadband sum of bare radiances, which the by-band values follow."""
    from rrtmgpnn import _lib
    from rrtmgpnn._lib import check, float_array
    from rrtmgpnn.api import GAUSS_DS, GAUSS_WTS, context
    case = _lw_case(ngpt, nlay)
    ncol = case[0].shape[0]
    nmus = int(mode[-1]) if mode.startswith("nmus") else 1
    ds = np.random.default_rng(3).uniform(1.0, 2.5, size=ngpt * ncol).astype(np.float32) if mode == "lw_ds" else None
    up, dn, gu, gd = cached(("lw", ngpt, nlay, mode, top_at_1), lambda: _lw_gpt_fluxes(orc, case, top_at_1, nmus, ds))
    a = [T(x, dev) for x in case]
    dsd = T(ds, dev) if ds is not None else None
    for name, lims in layouts(ngpt, R.even_limits(ngpt) if ngpt == 256 else None).items():
        nb = len(lims)
        o_up, o_dn = nan(dev, ncol, nlay + 1), nan(dev, ncol, nlay + 1)
        b_up, b_dn = nan(dev, ncol, nlay + 1, nb), nan(dev, ncol, nlay + 1, nb)
        arm(lims, b_up, b_dn, None)
        check(_lib.lib().rrtmgpnn_lw_solver_noscat_gpt(
            context(0).h, ngpt, nlay, ncol, int(top_at_1), nmus, float_array(GAUSS_DS[nmus]),
            float_array(GAUSS_WTS[nmus]), P(dsd), None, *[P(t) for t in a], P(o_up), P(o_dn), None, None),
            "lw_solver_noscat_gpt")
        torch.cuda.synchronize()
        np.testing.assert_array_equal(b_up.cpu().numpy(), R.sum_byband(gu, lims), err_msg=name + " bnd_up")
        np.testing.assert_array_equal(b_dn.cpu().numpy(), R.sum_byband(gd, lims), err_msg=name + " bnd_dn")
        np.testing.assert_array_equal(o_up.cpu().numpy(), up, err_msg=name + " up")
        np.testing.assert_array_equal(o_dn.cpu().numpy(), dn, err_msg=name + " dn")


def _rfmip_lw(orc, rfmip, top_at_1):
    from rrtmgpnn import data
    prob = subset(rfmip, np.arange(4, 1800, 601))
    if not top_at_1:
        prob = dict(prob)
        for k in ("play", "plev", "tlay", "tlev"):
            prob[k] = np.ascontiguousarray(prob[k][:, ::-1])
        prob["gases"] = {k: np.ascontiguousarray(v[:, ::-1]) for k, v in prob["gases"].items()}
        prob["top_at_1"] = False
    kd = data.load_kdist("lw")
    go = orc.lw_gas_optics(prob, [data.load_model("lw_abs"), data.load_model("lw_pfrac")], kd)
    return prob, kd, go


@pytest.mark.parametrize("top_at_1", [True, False])
@pytest.mark.parametrize("nmus", [1, 2])
@pytest.mark.parametrize("entry", ["plain", "planck", "planck_inc"])
def test_lw_rfmip_entries_byband(dev, orc, rfmip, entry, nmus, top_at_1):
    """The plain, fused-Planck and fused-Planck + increment entries on RFMIP columns, shipped and irregular limits."""
    from rrtmgpnn import _lib
    from rrtmgpnn._lib import check, float_array, int_array
    from rrtmgpnn.api import GAUSS_DS, GAUSS_WTS, context
    prob, kd, go = cached(("rfmip_lw", top_at_1), lambda: _rfmip_lw(orc, rfmip, top_at_1))
    ncol, nlay, ngpt = go["tau"].shape
    nbk = int(kd["nband"])
    klims = np.asarray(kd["band_lims_gpt"], np.int32).reshape(-1, 2)
    emis = np.repeat(np.asarray(prob["sfc_emis"], np.float32)[:, None], ngpt, axis=1)
    rng = np.random.default_rng(41)
    cld = np.where(rng.uniform(size=(ncol, nlay, nbk)) < 0.5, rng.lognormal(0, 1, (ncol, nlay, nbk)), 0).astype(np.float32)
    tau = go["tau"]
    if entry == "planck_inc":
        tau = cached(("rfmip_lw_inc", top_at_1), lambda: orc.increment_bybnd(klims, (go["tau"],), (cld,))[0])
    case = (tau, go["lay_source"], go["lev_source"], emis, go["sfc_source"])
    up, dn, gu, gd = cached(("rfmip_lw_sol", entry == "planck_inc", nmus, top_at_1),
                            lambda: _lw_gpt_fluxes(orc, case, top_at_1, nmus))
    sfc_lay = 1 if prob["play"][0, 0] > prob["play"][0, nlay - 1] else nlay
    L, c = _lib.lib(), context(0).h
    head = (c, ngpt, nlay, ncol, int(top_at_1), nmus, float_array(GAUSS_DS[nmus]), float_array(GAUSS_WTS[nmus]), None)
    d = {k: T(v, dev) for k, v in dict(tau=go["tau"], pfrac=go["pfrac"], tlay=prob["tlay"], tlev=prob["tlev"],
                                       tsfc=prob["tsfc"], totplnk=kd["totplnk"], emis=emis, cld=cld,
                                       tau_inc=tau, lay=go["lay_source"], lev=go["lev_source"],
                                       sfc=go["sfc_source"]).items()}
    for name, lims in (("shipped", klims), ("irregular", R.irregular_limits(ngpt))):
        nb = len(lims)
        o_up, o_dn = nan(dev, ncol, nlay + 1), nan(dev, ncol, nlay + 1)
        b_up, b_dn = nan(dev, ncol, nlay + 1, nb), nan(dev, ncol, nlay + 1, nb)
        arm(lims, b_up, b_dn, None)
        planck_tail = (P(d["pfrac"]), nbk, int(kd["nPlanckTemp"]), P(d["tlay"]), P(d["tlev"]), P(d["tsfc"]), sfc_lay,
                       int_array(klims.ravel()), float(kd["temp_ref_min"][0]), float(kd["totplnk_delta"]),
                       P(d["totplnk"]), 0, P(d["emis"]), P(o_up), P(o_dn))
        if entry == "plain":
            check(L.rrtmgpnn_lw_solver_noscat(*head, P(d["tau"]), P(d["lay"]), P(d["lev"]), P(d["emis"]), P(d["sfc"]),
                                              P(o_up), P(o_dn)), "lw_solver_noscat")
        elif entry == "planck":
            check(L.rrtmgpnn_lw_solver_noscat_planck(*head, P(d["tau"]), *planck_tail), "lw_solver_noscat_planck")
        else:
            check(L.rrtmgpnn_lw_solver_noscat_planck_inc(*head, P(d["tau"]), P(d["cld"]), *planck_tail),
                  "lw_solver_noscat_planck_inc")
        torch.cuda.synchronize()
        np.testing.assert_array_equal(b_up.cpu().numpy(), R.sum_byband(gu, lims), err_msg=name + " bnd_up")
        np.testing.assert_array_equal(b_dn.cpu().numpy(), R.sum_byband(gd, lims), err_msg=name + " bnd_dn")
        np.testing.assert_array_equal(o_up.cpu().numpy(), up, err_msg=name + " up")
        np.testing.assert_array_equal(o_dn.cpu().numpy(), dn, err_msg=name + " dn")


@pytest.fixture(scope="module")
def prob2str(orc, rfmip):
    from test_lw_scattering_oracle import lw_2str_problem
    return lw_2str_problem(orc, rfmip, ncol=6)


@pytest.mark.parametrize("top_at_1", [True, False])
@pytest.mark.parametrize("mode", ["rescl1", "rescl3", "2stream"])
def test_lw_scattering_byband(dev, orc, prob2str, mode, top_at_1):
    """The rescaled solution (one angle: the ring; several: the accumulators) and lw_solver_2stream."""
    from rrtmgpnn import _lib
    from rrtmgpnn._lib import check, float_array
    from rrtmgpnn.api import GAUSS_DS, GAUSS_WTS, context
    from test_lw_scattering_oracle import _flip
    p = prob2str if top_at_1 else _flip(prob2str)
    ncol, nlay, ngpt = p["tau"].shape
    lims = np.asarray(p["kd"]["band_lims_gpt"], np.int32).reshape(-1, 2)
    d = {k: T(p[k], dev) for k in ("tau", "ssa", "g", "lay", "lev", "emis_gpt", "sfc")}
    L, c = _lib.lib(), context(0).h
    if mode == "2stream":
        up, dn, gu, gd = orc.lw_solver_2stream(p["tau"], p["ssa"], p["g"], p["lev"], p["emis_gpt"], p["sfc"], top_at_1,
                                               gpt=True)
    else:
        nmus = int(mode[-1])
        up, dn, gu, gd = _lw_gpt_fluxes(orc, (p["tau"], p["lay"], p["lev"], p["emis_gpt"], p["sfc"]), top_at_1, nmus,
                                        ssa=p["ssa"], g=p["g"])
    for name, lims in (("shipped", lims), ("irregular", R.irregular_limits(ngpt))):
        nb = len(lims)
        o_up, o_dn = nan(dev, ncol, nlay + 1), nan(dev, ncol, nlay + 1)
        b_up, b_dn = nan(dev, ncol, nlay + 1, nb), nan(dev, ncol, nlay + 1, nb)
        arm(lims, b_up, b_dn, None)
        if mode == "2stream":
            check(L.rrtmgpnn_lw_solver_2stream(c, ngpt, nlay, ncol, int(top_at_1), None, P(d["tau"]), P(d["ssa"]),
                                               P(d["g"]), P(d["lev"]), P(d["emis_gpt"]), P(d["sfc"]), P(o_up), P(o_dn)),
                  "lw_solver_2stream")
        else:
            check(L.rrtmgpnn_lw_solver_1rescl(c, ngpt, nlay, ncol, int(top_at_1), nmus, float_array(GAUSS_DS[nmus]),
                                              float_array(GAUSS_WTS[nmus]), None, P(d["tau"]), P(d["ssa"]), P(d["g"]),
                                              P(d["lay"]), P(d["lev"]), P(d["emis_gpt"]), P(d["sfc"]), P(o_up),
                                              P(o_dn)), "lw_solver_1rescl")
        torch.cuda.synchronize()
        np.testing.assert_array_equal(b_up.cpu().numpy(), R.sum_byband(gu, lims), err_msg=name + " bnd_up")
        np.testing.assert_array_equal(b_dn.cpu().numpy(), R.sum_byband(gd, lims), err_msg=name + " bnd_dn")
        np.testing.assert_array_equal(o_up.cpu().numpy(), up, err_msg=name + " up")
        np.testing.assert_array_equal(o_dn.cpu().numpy(), dn, err_msg=name + " dn")


# ---- rrtmgpnn_sum_byband ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ngpt", [224, 37])
def test_sum_byband_entry(dev, ngpt):
    """37 rows of 5 columns: more than one block, a short last one; limits that leave g-points uncovered."""
    from rrtmgpnn import _lib
    from rrtmgpnn._lib import check, int_array
    from rrtmgpnn.api import context
    rng = np.random.default_rng(2)
    ncol, nlev = 5, 37
    x = (rng.uniform(0, 1, size=(ncol, nlev, ngpt)) * 10.0 ** rng.integers(-3, 4, size=(ncol, nlev, ngpt))).astype(np.float32)
    xd = T(x, dev)
    for lims in (R.irregular_limits(ngpt), R.uncovered_limits(ngpt), R.one_band(ngpt)):
        out = nan(dev, ncol, nlev, len(lims))
        check(_lib.lib().rrtmgpnn_sum_byband(context(0).h, ngpt, nlev, ncol, len(lims), int_array(lims.ravel()), P(xd),
                                             P(out)), "sum_byband")
        torch.cuda.synchronize()
        np.testing.assert_array_equal(out.cpu().numpy(), R.sum_byband(x, lims))


# ---- request lifetime ------------------------------------------------------------------------------------------------
def test_request_lifetime(dev):
    from rrtmgpnn import _lib
    from rrtmgpnn.api import context
    L, c = _lib.lib(), context(0).h
    ngpt, nlay = 222, 4
    case = _sw_case(ngpt, nlay, True)
    ncol = case[0].shape[0]
    a = [T(x, dev) for x in case]
    lims = R.irregular_limits(ngpt)
    nb = len(lims)
    outs = [nan(dev, ncol, nlay + 1) for _ in range(3)]
    first = [nan(dev, ncol, nlay + 1, nb) for _ in range(3)]
    arm(lims, *first)
    _sw_call(dev, a, ngpt, nlay, ncol, True, True, outs)
    torch.cuda.synchronize()
    assert not torch.isnan(first[0]).any()
    # a second solver call does not see the request: NaN-filled arrays stay untouched
    for t in first:
        t.fill_(NAN)
    _sw_call(dev, a, ngpt, nlay, ncol, True, True, outs)
    torch.cuda.synchronize()
    assert all(torch.isnan(t).all() for t in first)
    # an armed request followed by a failing call (bad argument) is cleared
    arm(lims, *first)
    rc = L.rrtmgpnn_sw_solver_2stream(c, ngpt, nlay, ncol, 1, None, None, P(a[0]), P(a[1]), P(a[2]), P(a[3]), P(a[5]),
                                      P(a[6]), *[P(t) for t in outs])
    assert rc == 1
    _sw_call(dev, a, ngpt, nlay, ncol, True, True, outs)
    torch.cuda.synchronize()
    assert all(torch.isnan(t).all() for t in first)
    # band limits past the call's ngpt are an argument error of the consuming call
    arm(np.asarray([(1, ngpt + 1)], np.int32), nan(dev, ncol, nlay + 1, 1), None, None)
    rc = L.rrtmgpnn_sw_solver_2stream(c, ngpt, nlay, ncol, 1, P(a[4]), None, P(a[0]), P(a[1]), P(a[2]), P(a[3]),
                                      P(a[5]), P(a[6]), *[P(t) for t in outs])
    assert rc == 1 and b"band limits" in L.rrtmgpnn_last_error()
    # by-band + g-point outputs in one C call: unsupported, with a message of its own
    L.rrtmgpnn_sum_byband(c, 0, 0, 0, 0, None, None, None)  # leaves another error text behind
    stale = L.rrtmgpnn_last_error()
    gp = [nan(dev, ncol, nlay + 1, ngpt) for _ in range(3)]
    arm(lims, *first)
    rc = L.rrtmgpnn_sw_solver_2stream_gpt(c, ngpt, nlay, ncol, 1, P(a[4]), None, P(a[0]), P(a[1]), P(a[2]), P(a[3]),
                                          P(a[5]), P(a[6]), *[P(t) for t in outs + gp])
    msg = L.rrtmgpnn_last_error()
    assert rc == 4 and msg != stale and b"by-band" in msg
    torch.cuda.synchronize()
    assert all(torch.isnan(t).all() for t in first)
    # an LW entry refuses a direct-beam array
    lw = _lw_case(32, 4)
    b = [T(x, dev) for x in lw]
    from rrtmgpnn._lib import float_array
    from rrtmgpnn.api import GAUSS_DS, GAUSS_WTS
    arm(R.one_band(32), None, None, nan(dev, 3, 5, 1))
    rc = L.rrtmgpnn_lw_solver_noscat(c, 32, 4, 3, 1, 1, float_array(GAUSS_DS[1]), float_array(GAUSS_WTS[1]), None,
                                     *[P(t) for t in b], P(nan(dev, 3, 5)), P(nan(dev, 3, 5)))
    assert rc == 1 and b"bnd_flux_dn_dir" in L.rrtmgpnn_last_error()


# ---- class layer -------------------------------------------------------------------------------------------------------
def _lw_class_setup(dev, orc, rfmip):
    from rrtmgpnn import api
    prob, kd, go = cached(("rfmip_lw", True), lambda: _rfmip_lw(orc, rfmip, True))
    ncol, nlay, ngpt = go["tau"].shape
    op = api.OpticalProps1scl()
    assert op.init(kd["band_lims_wvn"], kd["band_lims_gpt"]) == ""
    assert op.alloc_1scl(ncol, nlay) == ""
    op.tau = T(go["tau"], dev)
    src = api.SourceFuncLW()
    assert src.alloc(ncol, nlay, op) == ""
    src.lay_source, src.lev_source, src.sfc_source = T(go["lay_source"], dev), T(go["lev_source"], dev), \
        T(go["sfc_source"], dev)
    emis_band = np.repeat(np.asarray(prob["sfc_emis"], np.float32)[:, None], kd["nband"], axis=1)
    emis_gpt = np.repeat(np.asarray(prob["sfc_emis"], np.float32)[:, None], ngpt, axis=1)
    return prob, kd, go, op, src, emis_band, emis_gpt


@pytest.mark.parametrize("nmus", [1, 2])
@pytest.mark.parametrize("with_gpt", [False, True])
def test_class_layer_rte_lw_byband(dev, orc, rfmip, nmus, with_gpt):
    from rrtmgpnn import api
    prob, kd, go, op, src, emis_band, emis_gpt = _lw_class_setup(dev, orc, rfmip)
    ncol, nlay, ngpt = go["tau"].shape
    nb = int(kd["nband"])
    lims = np.asarray(kd["band_lims_gpt"], np.int32).reshape(-1, 2)
    case = (go["tau"], go["lay_source"], go["lev_source"], emis_gpt, go["sfc_source"])
    up, dn, gu, gd = cached(("rfmip_lw_sol", False, nmus, True), lambda: _lw_gpt_fluxes(orc, case, True, nmus))
    kw = dict(flux_up=nan(dev, ncol, nlay + 1), flux_dn=nan(dev, ncol, nlay + 1))
    if with_gpt:
        kw.update(gpt_flux_up=nan(dev, ncol, nlay + 1, ngpt), gpt_flux_dn=nan(dev, ncol, nlay + 1, ngpt))
    fl = api.FluxesByBand(bnd_flux_up=nan(dev, ncol, nlay + 1, nb), bnd_flux_dn=nan(dev, ncol, nlay + 1, nb),
                          bnd_flux_net=nan(dev, ncol, nlay + 1, nb), **kw)
    assert api.rte_lw(op, True, src, T(emis_band, dev), fl, n_gauss_angles=nmus) == ""
    torch.cuda.synchronize()
    wu, wd = R.sum_byband(gu, lims), R.sum_byband(gd, lims)
    np.testing.assert_array_equal(fl.bnd_flux_up.cpu().numpy(), wu)
    np.testing.assert_array_equal(fl.bnd_flux_dn.cpu().numpy(), wd)
    np.testing.assert_array_equal(fl.bnd_flux_net.cpu().numpy(), wd - wu)
    np.testing.assert_array_equal(fl.flux_up.cpu().numpy(), up)
    np.testing.assert_array_equal(fl.flux_dn.cpu().numpy(), dn)
    if with_gpt:  # the g-point arrays are the _gpt entry's (radiances at one angle)
        raw = orc.lw_solver(*case, True, nmus, gpt=True)
        np.testing.assert_array_equal(fl.gpt_flux_up.cpu().numpy(), raw[2])
        np.testing.assert_array_equal(fl.gpt_flux_dn.cpu().numpy(), raw[3])


def test_class_layer_error_strings(dev, orc, rfmip):
    from rrtmgpnn import api
    prob, kd, go, op, src, emis_band, emis_gpt = _lw_class_setup(dev, orc, rfmip)
    ncol, nlay, ngpt = go["tau"].shape
    nb = int(kd["nband"])
    e = T(emis_band, dev)
    f = lambda *s: nan(dev, *s)  # noqa: E731
    bad = api.FluxesByBand(flux_up=f(ncol, nlay + 1), bnd_flux_up=f(ncol, nlay + 1, nb + 1))
    assert api.rte_lw(op, True, src, e, bad) == \
        "reduce: bnd_flux_up array incorrectly sized (can't compute net flux either)"
    bad = api.FluxesByBand(flux_up=f(ncol, nlay + 1), bnd_flux_dn=f(ncol, nlay, nb))
    assert api.rte_lw(op, True, src, e, bad) == \
        "reduce: bnd_flux_dn array incorrectly sized (can't compute net flux either)"
    bad = api.FluxesByBand(flux_up=f(ncol, nlay + 1), bnd_flux_dn_dir=f(ncol, nlay + 1, nb))
    assert api.rte_lw(op, True, src, e, bad) == \
        "reduce: requesting bnd_flux_dn_dir but direct flux hasn't been supplied"
    bad = api.FluxesByBand(flux_up=f(ncol, nlay + 1), bnd_flux_dn_dir=f(ncol + 1, nlay + 1, nb))
    assert api.rte_lw(op, True, src, e, bad) == "reduce: bnd_flux_dn_dir array incorrectly sized"
    bad = api.FluxesByBand(flux_up=f(ncol, nlay + 1), bnd_flux_up=f(ncol, nlay + 1, nb),
                           bnd_flux_net=f(ncol, nlay + 1, nb))
    assert api.rte_lw(op, True, src, e, bad) == api.BYBAND_NET_ERROR
    # nothing stays armed after an error return: a plain call leaves NaN-filled by-band arrays of an earlier object alone
    fl = api.FluxesBroadband(f(ncol, nlay + 1), f(ncol, nlay + 1))
    assert api.rte_lw(op, True, src, e, fl) == ""
    torch.cuda.synchronize()
    assert not torch.isnan(fl.flux_up).any()


@pytest.mark.parametrize("with_gpt", [False, True])
def test_class_layer_rte_sw_byband(dev, orc, with_gpt):
    from rrtmgpnn import api, data
    kd = data.load_kdist("sw")
    ngpt, nlay = int(kd["ngpt"]), 10
    case = _sw_case(ngpt, nlay, True)
    tau, ssa, g, mu0, inc, ad, af = case
    ncol = tau.shape[0]
    nb = int(kd["nband"])
    lims = np.asarray(kd["band_lims_gpt"], np.int32).reshape(-1, 2)
    want = cached(("sw", ngpt, nlay, True, True), lambda: orc.sw_solver(*case, True, gpt=True))
    op = api.OpticalProps2str()
    assert op.init(kd["band_lims_wvn"], kd["band_lims_gpt"]) == ""
    assert op.alloc_2str(ncol, nlay, device=dev) == ""
    op.tau.copy_(T(tau, dev)), op.ssa.copy_(T(ssa, dev)), op.g.copy_(T(g, dev))
    f = lambda *s: nan(dev, *s)  # noqa: E731
    kw = dict(flux_up=f(ncol, nlay + 1), flux_dn=f(ncol, nlay + 1), flux_dn_dir=f(ncol, nlay + 1))
    if with_gpt:
        kw.update(gpt_flux_up=f(ncol, nlay + 1, ngpt), gpt_flux_dn=f(ncol, nlay + 1, ngpt),
                  gpt_flux_dn_dir=f(ncol, nlay + 1, ngpt))
    fl = api.FluxesByBand(bnd_flux_up=f(ncol, nlay + 1, nb), bnd_flux_dn=f(ncol, nlay + 1, nb),
                          bnd_flux_dn_dir=f(ncol, nlay + 1, nb), bnd_flux_net=f(ncol, nlay + 1, nb), **kw)
    assert api.rte_sw(op, True, T(mu0, dev), T(inc, dev), T(ad, dev), T(af, dev), fl) == ""
    torch.cuda.synchronize()
    w = [R.sum_byband(y, lims) for y in want[3:]]
    np.testing.assert_array_equal(fl.bnd_flux_up.cpu().numpy(), w[0])
    np.testing.assert_array_equal(fl.bnd_flux_dn.cpu().numpy(), w[1])
    np.testing.assert_array_equal(fl.bnd_flux_dn_dir.cpu().numpy(), w[2])
    np.testing.assert_array_equal(fl.bnd_flux_net.cpu().numpy(), w[1] - w[0])
    bb = want[:3] if with_gpt else cached(("swbb", ngpt, nlay, True, True), lambda: orc.sw_solver(*case, True))
    for x, y in zip((fl.flux_up, fl.flux_dn, fl.flux_dn_dir), bb):
        np.testing.assert_array_equal(x.cpu().numpy(), y)
    bad = api.FluxesByBand(flux_up=f(ncol, nlay + 1), bnd_flux_net=f(ncol, nlay + 1, nb + 2))
    assert api.rte_sw(op, True, T(mu0, dev), T(inc, dev), T(ad, dev), T(af, dev), bad) == \
        "reduce: bnd_flux_net array incorrectly sized (can't compute net flux either)"


# ---- pipeline ----------------------------------------------------------------------------------------------------------
def test_clear_sky_step_byband(dev, orc, rfmip):
    """ClearSkyStep(byband=True) on 12 RFMIP columns: eager = graph replay = the oracle's solvers on the step's own
    optical properties, by-band and broadband; byband=False issues today's call list."""
    from rrtmgpnn import data
    from rrtmgpnn.pipeline import ClearSkyStep
    from oracle import gauss
    prob = subset(rfmip, np.arange(7, 1800, 150))
    assert prob["ncol"] == 12
    plain = ClearSkyStep(prob, device=0)
    step = ClearSkyStep(prob, device=0, byband=True)
    names = [n for n, _, _ in step.calls]
    assert [n for n in names if not n.endswith("_byband")] == [n for n, _, _ in plain.calls]
    assert names.index("lw_byband") + 1 == names.index("lw_solver")
    assert names.index("sw_byband") + 1 == names.index("sw_solver")
    assert not any(n.endswith("_byband") for n, _, _ in plain.calls)
    keys = ("lw_up", "lw_dn", "sw_up", "sw_dn", "sw_dir")
    bkeys = ("lw_bnd_up", "lw_bnd_dn", "sw_bnd_up", "sw_bnd_dn", "sw_bnd_dir")
    for k in keys + bkeys:
        getattr(step, k).fill_(NAN)
    plain.step()
    step.step()
    torch.cuda.synchronize()
    eager, eager_b, base = step.fluxes(), step.byband_fluxes(), plain.fluxes()
    for k in keys:  # the request does not move the broadband outputs
        np.testing.assert_array_equal(eager[k], base[k], err_msg=k)
    step.capture()
    for k in keys + bkeys:
        getattr(step, k).fill_(NAN)
    step.replay()
    torch.cuda.synchronize()
    rep, rep_b = step.fluxes(), step.byband_fluxes()
    for k in keys:
        np.testing.assert_array_equal(rep[k], eager[k], err_msg=k)
    for k in bkeys:
        np.testing.assert_array_equal(rep_b[k], eager_b[k], err_msg=k)
    # the oracle's solvers on the step's own optical properties
    kl, ks = data.load_kdist("lw"), data.load_kdist("sw")
    tau_lw, pfrac = step.tau_lw.cpu().numpy(), step.lay_src.cpu().numpy()
    nlay = prob["nlay"]
    sfc_lay = 1 if prob["play"][0, 0] > prob["play"][0, nlay - 1] else nlay
    lay, lev, sfc, _ = orc.planck_source(kl, prob["tlay"], prob["tlev"], prob["tsfc"], pfrac, sfc_lay)
    emis = np.repeat(np.asarray(prob["sfc_emis"], np.float32)[:, None], kl["ngpt"], axis=1)
    up, dn, gu, gd = orc.lw_solver(tau_lw, lay, lev, emis, sfc, prob["top_at_1"], 1, gpt=True)
    w = gauss(1)[1][0]
    ll = np.asarray(kl["band_lims_gpt"], np.int32).reshape(-1, 2)
    np.testing.assert_array_equal(eager["lw_up"], up)
    np.testing.assert_array_equal(eager["lw_dn"], dn)
    np.testing.assert_array_equal(eager_b["lw_bnd_up"], R.sum_byband(R.lw_one_angle_terms(gu, w, kl["ngpt"]), ll))
    np.testing.assert_array_equal(eager_b["lw_bnd_dn"], R.sum_byband(R.lw_one_angle_terms(gd, w, kl["ngpt"]), ll))
    tau_sw, ssa_sw = step.tau_sw.cpu().numpy(), step.ssa_sw.cpu().numpy()
    alb = np.repeat(np.asarray(prob["sfc_alb"], np.float32)[:, None], ks["ngpt"], axis=1)
    args = (tau_sw, ssa_sw, np.zeros_like(tau_sw), prob["mu0"], data.toa_flux(prob, ks), alb, alb, prob["top_at_1"])
    sw = orc.sw_solver(*args, gpt=True)
    sl = np.asarray(ks["band_lims_gpt"], np.int32).reshape(-1, 2)
    for k, y in zip(("sw_bnd_up", "sw_bnd_dn", "sw_bnd_dir"), sw[3:]):
        np.testing.assert_array_equal(eager_b[k], R.sum_byband(y, sl), err_msg=k)
    for k, y in zip(("sw_up", "sw_dn", "sw_dir"), orc.sw_solver(*args)):
        np.testing.assert_array_equal(eager[k], y, err_msg=k)
    step.close()
    plain.close()
