"""GPU: rrtmgpnn_compute_bc_lw / _sw (extensions/mo_compute_bc.F90) against the CPU comparator
(tests/compute_bc_ref.py), bit for bit: every input set (7, 1 and 65 RFMIP columns, nlay 2 and 5 under the removed top
layers, both orientations, gases as arrays / an (nlay) profile / a scalar / absent), one and three angles, radiance and
flux units; against the composed route through the existing entries on the GPU (host gather, gas optics at nlay = 1, the
g-point solver); the zero-thickness layer of the unmodified reversed columns; the three-kernel fallback of a network
without an in-kernel instance; the entries' refusals (host-side returns); and the Python class layer."""
import numpy as np
import pytest

import compute_bc_ref as B

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a device"
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def kit(dev):
    """The k-distributions and networks of both streams."""
    from rrtmgpnn import api, data
    kd = {}
    for w in ("lw", "sw"):
        kd[w] = api.GasOpticsRRTMGP()
        assert kd[w].load(w) == ""
    nets = {"lw": [api.RrtmgpNetwork(0).load(data.path(n)) for n in ("lw_abs", "lw_pfrac")],
            "sw": [api.RrtmgpNetwork(0).load(data.path(n)) for n in ("sw_abs", "sw_ray")]}
    return kd, nets


_WANT = {}


def want(orc, rfmip, s):
    """The comparator's arrays of an input set, computed once: the set's problem, LW at one and three angles, SW."""
    if s not in _WANT:
        cols, trunc, top_at_1 = s
        prob = B.truncated(rfmip, B.COLS[cols], *B.TRUNC[trunc], top_at_1)
        w = {"prob": prob, "lw1": B.lw(orc, prob, 1), "lw3": B.lw(orc, prob, 3), "sw": B.sw(orc, prob)}
        for a in w.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _WANT[s] = w
    return _WANT[s]


def T(a, dev):
    return torch.as_tensor(np.array(a, dtype=np.float32, order="C", copy=True), device=dev)


def gas_concs(gases, dev):
    from rrtmgpnn import api
    gc = api.GasConcs()
    assert gc.init(list(gases)) == ""
    for k, v in gases.items():
        assert gc.set_vmr(k, float(v) if np.ndim(v) == 0 else np.asarray(v), device=dev) == ""
    return gc


def entry(which, kit, prob, dev, nmus=1, as_flux=0, nets=None):
    """One call of the C entry on a host problem; returns flux_bc (ncol, ngpt) as a host array."""
    from rrtmgpnn import _lib
    from rrtmgpnn._lib import check, float_array, int_array, ptr_array
    from rrtmgpnn.api import GAUSS_DS, GAUSS_WTS, context
    from rrtmgpnn.compute_bc import gas_arguments
    kd, nets = kit[0][which], nets or kit[1][which]
    ncol, nlay = prob["play"].shape
    play, plev, tlay, mu0 = (T(prob[k], dev) for k in ("play", "plev", "tlay", "mu0"))
    gc = gas_concs(prob["gases"], dev)
    ptrs, nds, e = gas_arguments(nets[0], gc)
    assert e == ""
    out = torch.full((ncol, kd.get_ngpt()), float("nan"), device=dev)
    head = (context(0).h, ncol, nlay, kd.get_ngpt(), nets[0].dims[0], int(prob["top_at_1"]), kd.get_press_min(),
            play.data_ptr(), plev.data_ptr(), tlay.data_ptr(), gc.concs["h2o"].data_ptr(), ptr_array(ptrs),
            int_array(nds), ptr_array([n.h.value for n in nets]))
    L = _lib.lib()
    if which == "lw":
        check(L.rrtmgpnn_compute_bc_lw(
            *head, len(nets), kd.get_nband(), kd.get_nPlanckTemp(), int_array(kd.band_lims_gpt.ravel()),
            kd.temp_ref_min, kd.totplnk_delta, kd.totplnk.data_ptr(), nmus, float_array(GAUSS_DS[nmus]),
            float_array(GAUSS_WTS[nmus]), as_flux, out.data_ptr()), "compute_bc_lw")
    else:
        src = T(kd.solar_source, dev)
        check(L.rrtmgpnn_compute_bc_sw(*head, src.data_ptr(), mu0.data_ptr(), out.data_ptr()), "compute_bc_sw")
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("s", B.SETS, ids=B.set_id)
def test_entries_equal_the_comparator(dev, kit, orc, rfmip, s):
    w = want(orc, rfmip, s)
    prob = w["prob"]
    for nmus in (1, 3):
        radn = w["lw%d" % nmus]
        for as_flux in (0, 1):
            got = entry("lw", kit, prob, dev, nmus, as_flux)
            np.testing.assert_array_equal(got, B.in_flux_units(radn, nmus) if as_flux else radn,
                                          err_msg="lw nmus %d as_flux %d" % (nmus, as_flux))
    np.testing.assert_array_equal(entry("sw", kit, prob, dev), w["sw"], err_msg="sw")


def composed(which, kit, prob, dev, nmus=1):
    """The route a host can compose from the existing entries: the one-layer problem gathered on the host, gas optics at
    nlay = 1, the g-point solver into (ncol, 2, ngpt) arrays, one level of them."""
    from rrtmgpnn import _lib
    from rrtmgpnn._lib import check, float_array, int_array, ptr_array
    from rrtmgpnn.api import GAUSS_DS, GAUSS_WTS, context
    from rrtmgpnn.compute_bc import gas_arguments
    kd, nets = kit[0][which], kit[1][which]
    p1 = B.one_layer(prob, kd.get_press_min())
    ncol, ngpt, top_at_1 = p1["ncol"], kd.get_ngpt(), int(prob["top_at_1"])
    play, plev, tlay, tlev, mu0 = (T(p1[k], dev) for k in ("play", "plev", "tlay", "tlev", "mu0"))
    gc = gas_concs(p1["gases"], dev)
    ptrs, nds, e = gas_arguments(nets[0], gc)
    assert e == ""
    L, c = _lib.lib(), context(0).h
    tau, second = (torch.empty((ncol, 1, ngpt), device=dev) for _ in range(2))
    head = (c, ncol, 1, ngpt, nets[0].dims[0], play.data_ptr(), tlay.data_ptr(), plev.data_ptr(),
            gc.concs["h2o"].data_ptr(), ptr_array(ptrs), int_array(nds), ptr_array([n.h.value for n in nets]))
    flux = [torch.empty((ncol, 2), device=dev) for _ in range(3)]
    gpt = [torch.empty((ncol, 2, ngpt), device=dev) for _ in range(3)]
    ones = torch.ones((ncol, ngpt), device=dev)
    if which == "lw":
        check(L.rrtmgpnn_gas_optics_lw_nn(*head, len(nets), tau.data_ptr(), second.data_ptr()), "gas_optics_lw_nn")
        check(L.rrtmgpnn_lw_solver_noscat_planck_gpt(
            c, ngpt, 1, ncol, top_at_1, nmus, float_array(GAUSS_DS[nmus]), float_array(GAUSS_WTS[nmus]), None, None,
            tau.data_ptr(), second.data_ptr(), kd.get_nband(), kd.get_nPlanckTemp(), tlay.data_ptr(), tlev.data_ptr(),
            tlay.data_ptr(), 1, int_array(kd.band_lims_gpt.ravel()), kd.temp_ref_min, kd.totplnk_delta,
            kd.totplnk.data_ptr(), 0, ones.data_ptr(), flux[0].data_ptr(), flux[1].data_ptr(), gpt[0].data_ptr(),
            gpt[1].data_ptr()), "lw_solver_noscat_planck_gpt")
        res = gpt[1]
    else:
        check(L.rrtmgpnn_gas_optics_sw_nn(*head, tau.data_ptr(), second.data_ptr(), None), "gas_optics_sw_nn")
        inc = T(np.broadcast_to(kd.solar_source, (ncol, ngpt)), dev)
        check(L.rrtmgpnn_sw_solver_2stream_gpt(
            c, ngpt, 1, ncol, top_at_1, inc.data_ptr(), None, tau.data_ptr(), second.data_ptr(), None, mu0.data_ptr(),
            ones.data_ptr(), ones.data_ptr(), *[t.data_ptr() for t in flux + gpt]), "sw_solver_2stream_gpt")
        res = gpt[2]
    torch.cuda.synchronize()
    return res[:, 1 if top_at_1 else 0].cpu().numpy()


@pytest.mark.parametrize("s", [("c7", "n2", True), ("c65", "n5", False)], ids=B.set_id)
def test_entries_equal_the_composed_route(dev, kit, orc, rfmip, s):
    prob = want(orc, rfmip, s)["prob"]
    for nmus in (1, 3):
        np.testing.assert_array_equal(entry("lw", kit, prob, dev, nmus), composed("lw", kit, prob, dev, nmus),
                                      err_msg="lw nmus %d" % nmus)
    np.testing.assert_array_equal(entry("sw", kit, prob, dev), composed("sw", kit, prob, dev), err_msg="sw")


def test_zero_thickness_layer(dev, kit, orc, rfmip):
    """The unmodified columns reversed to top_at_1 = False: the reference's check reads plev(:, nlay) = 20 Pa and passes,
    and the layer is press_min .. press_min + eps.  Finite, and the comparator's bits."""
    from conftest import subset
    from rrtmgpnn.compute_bc import pressure_check
    prob = B.flip(subset(rfmip, B.COLS["c7"]))
    nlay = prob["nlay"]
    assert pressure_check(prob["plev"][:, nlay - 1], kit[0]["lw"].get_press_min()) == ""
    assert (prob["plev"][:, nlay] - np.float32(kit[0]["lw"].get_press_min()) < 1e-5).all()
    for nmus in (1, 3):
        got = entry("lw", kit, prob, dev, nmus)
        assert np.isfinite(got).all()
        np.testing.assert_array_equal(got, B.lw(orc, prob, nmus))
    got = entry("sw", kit, prob, dev)
    assert np.isfinite(got).all()
    np.testing.assert_array_equal(got, B.sw(orc, prob))


class _Kd128:
    """The LW k-distribution's Planck table on 128 g-points, 8 per band: the spectral grid of the g128 model."""

    def __init__(self, kd):
        self._kd = kd
        self.band_lims_gpt = np.array([[8 * b + 1, 8 * b + 8] for b in range(kd.get_nband())], np.int32)
        self.temp_ref_min, self.totplnk_delta, self.totplnk = kd.temp_ref_min, kd.totplnk_delta, kd.totplnk

    def get_ngpt(self):
        return 128

    def __getattr__(self, name):
        return getattr(self._kd, name)


def test_fallback_without_an_in_kernel_instance(dev, kit, orc, rfmip):
    """The g128 single-output LW model has no in-kernel-input instance: compute_nn_inputs and get_col_dry run on the
    gathered layer in the workspace, then the network.  Against the oracle's single-model branch, bit for bit."""
    from rrtmgpnn import api, data
    model = data.load_model("lw_g128_both")
    both = [api.RrtmgpNetwork(0).load(data.path("lw_g128_both"))]
    k128 = _Kd128(kit[0]["lw"])
    assert k128.get_nband() * 8 == 128
    kd = dict(data.load_kdist("lw"), band_lims_gpt=k128.band_lims_gpt, ngpt=128)
    for top_at_1 in (True, False):
        prob = want(orc, rfmip, ("c7", "n5", top_at_1))["prob"]
        go = orc.lw_gas_optics(B.one_layer(prob, kd["press_ref_min"][0]), [model], kd)
        ones = np.ones(go["sfc_source"].shape, np.float32)
        for nmus in (1, 3):
            ref = orc.lw_solver(go["tau"], go["lay_source"], go["lev_source"], ones, go["sfc_source"], top_at_1, nmus,
                                gpt=True)[3]
            got = entry("lw", ({"lw": k128}, None), prob, dev, nmus, nets=both)
            np.testing.assert_array_equal(got, ref[:, 1 if top_at_1 else 0], err_msg="nmus %d" % nmus)


def test_entry_refusals_are_host_side(dev, kit, orc, rfmip):
    """Bad arguments come back as RRTMGPNN_ERR_ARGUMENT with a message before anything is launched, and the context
    serves the next call."""
    from rrtmgpnn import api
    from rrtmgpnn._lib import RrtmgpnnError
    w = want(orc, rfmip, ("c7", "n2", True))
    prob = w["prob"]
    api.GAUSS_DS[5], api.GAUSS_WTS[5] = [1.0] * 5, [0.2] * 5
    try:
        with pytest.raises(RrtmgpnnError, match="nmus must be 1..4"):
            entry("lw", kit, prob, dev, nmus=5)
    finally:
        del api.GAUSS_DS[5], api.GAUSS_WTS[5]

    class NoNetwork:
        class h:
            value = None

    with pytest.raises(RrtmgpnnError, match="Rayleigh networks missing or inconsistent"):
        entry("sw", kit, prob, dev, nets=[kit[1]["sw"][0], NoNetwork])
    with pytest.raises(RrtmgpnnError, match="network sizes do not match"):
        entry("lw", kit, prob, dev, nets=[kit[1]["lw"][0], kit[1]["sw"][0]])
    np.testing.assert_array_equal(entry("sw", kit, prob, dev), w["sw"])


def test_class_layer(dev, kit, orc, rfmip):
    """rrtmgpnn.compute_bc.compute_bc: the reference's behaviour by default (one angle, the radiance), as_flux for the
    solvers' units, the solar problem with mu0; and its refusal of the unmodified columns."""
    from conftest import subset
    from rrtmgpnn.compute_bc import compute_bc
    kd, nets = kit
    for s in (("c7", "n5", True), ("c7", "n5", False)):
        w = want(orc, rfmip, s)
        prob = w["prob"]
        play, plev, tlay, mu0 = (T(prob[k], dev) for k in ("play", "plev", "tlay", "mu0"))
        gc = gas_concs(prob["gases"], dev)
        out = torch.full((prob["ncol"], 256), float("nan"), device=dev)
        assert compute_bc(kd["lw"], play, plev, tlay, gc, out, neural_nets=nets["lw"]) == ""
        np.testing.assert_array_equal(out.cpu().numpy(), w["lw1"])
        assert compute_bc(kd["lw"], play, plev, tlay, gc, out, as_flux=True, neural_nets=nets["lw"]) == ""
        np.testing.assert_array_equal(out.cpu().numpy(), B.in_flux_units(w["lw1"]))
        out = torch.full((prob["ncol"], 224), float("nan"), device=dev)
        assert compute_bc(kd["sw"], play, plev, tlay, gc, out, mu0=mu0, neural_nets=nets["sw"]) == ""
        np.testing.assert_array_equal(out.cpu().numpy(), w["sw"])
        assert compute_bc(kd["sw"], play, plev, tlay, gc, out[:, 1:], mu0=mu0, neural_nets=nets["sw"]) == \
            "compute_bc: array flux_bc has wrong dimensions"
    full = subset(rfmip, B.COLS["c7"])
    play, plev, tlay = (T(full[k], dev) for k in ("play", "plev", "tlay"))
    assert compute_bc(kd["lw"], play, plev, tlay, gas_concs(full["gases"], dev), out, neural_nets=nets["lw"]) == \
        "compute_bc: pressures are too close to (or less than) min in gas optics "
