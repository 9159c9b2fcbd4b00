"""GPU: the fused all-sky LW solve with scattering clouds (rrtmgpnn_lw_solver_1rescl_planck_inc), every comparison bit
for bit.

1. against the composed oracle of tests/lw_scat_cases.py: both orientations x one and three angles x unmasked / sampled /
   all-ones / all-zero masks over every case, outputs pre-filled with NaN;
2. against the GPU composition of the existing entries on the same device arrays (compute_planck_source_nn, zeroed
   ssa / g, [draw_samples,] increment[_bybnd], lw_solver_1rescl); tau and pfrac compared before and after;
3. an all-zero mask equals rrtmgpnn_lw_solver_noscat_planck on the same arguments;
4. emis_by_band 0 and 1;  5. a non-NULL inc_flux;
6. the request's lifetime and every refusal, with codes and the entry's name in rrtmgpnn_last_error;
7. clr_all_sky.rte_lw with by-band 2str clouds, LW_SCAT_FUSED True against False, masked and unmasked.

That the expectations tell masks, ssa_bnd and g_bnd apart is established on the CPU in tests/test_lw_scat_allsky_host.py."""
import numpy as np
import pytest

import lw_scat_cases as S
import mcica_ref as M
from lw_scat_cases import NCOL

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
ERR_ARGUMENT, ERR_UNSUPPORTED = 1, 4
NAN = float("nan")
ENTRY = "rrtmgpnn_lw_solver_1rescl_planck_inc"
NAME = "lw_solver_1rescl_planck_inc"
ORIENT = pytest.mark.parametrize("top_at_1", [True, False], ids=["top1", "top0"])
NMUS = pytest.mark.parametrize("nmus", [1, 3])
CASES = pytest.mark.parametrize("ng,nlay", S.CASES)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a device"
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def T(a, dev):
    return torch.as_tensor(np.array(a, dtype=np.float32), device=dev)


def P(t):
    return t.data_ptr() if t is not None else None


def _bits_t(mask, dev):
    return torch.as_tensor(M.pack_bits(mask).view(np.int32), device=dev)


def _ctx():
    from rrtmgpnn.api import context
    return context(0).h


def _L():
    from rrtmgpnn import _lib
    return _lib.lib()


def _last_error():
    return _L().rrtmgpnn_last_error().decode()


def _same(got, want, what):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(g, w, err_msg="%s [%d]" % (what, i))


_dev_cases = {}


def case(ng, nlay, dev):
    """The case's inputs on the host and the device, built once and never modified."""
    if (ng, nlay) not in _dev_cases:
        c = dict(S.case(ng, nlay))
        c["dev"] = {k: T(c[k], dev) for k in ("tau", "pfrac", "tb", "wb", "gb", "tlay", "tlev", "tsfc", "emis_bnd",
                                             "emis_gpt", "inc")}
        c["dev"]["totplnk"] = T(c["kd"]["totplnk"], dev)
        _dev_cases[(ng, nlay)] = c
    return _dev_cases[(ng, nlay)]


def _planck_tail(c, top_at_1, emis_by_band=True):
    from rrtmgpnn._lib import int_array
    d, kd, nlay = c["dev"], c["kd"], c["nlay"]
    return (P(d["pfrac"]), c["nb"], kd["nPlanckTemp"], P(d["tlay"]), P(d["tlev"]), P(d["tsfc"]), nlay if top_at_1 else 1,
            int_array(np.asarray(c["lims"]).ravel()), float(kd["temp_ref_min"][0]), float(kd["totplnk_delta"]),
            P(d["totplnk"]), int(emis_by_band), P(d["emis_bnd"] if emis_by_band else d["emis_gpt"]))


def _head(c, top_at_1, nmus, inc=False, nlay=None, ncol=NCOL):
    from rrtmgpnn._lib import float_array
    from rrtmgpnn.api import GAUSS_DS, GAUSS_WTS
    return (_ctx(), c["ng"], c["nlay"] if nlay is None else nlay, ncol, int(top_at_1), nmus, float_array(GAUSS_DS[nmus]),
            float_array(GAUSS_WTS[nmus]), P(c["dev"]["inc"]) if inc else None, P(c["dev"]["tau"]))


def _arm_mask(c, bits):
    assert _L().rrtmgpnn_solver_request_cloud_mask(_ctx(), c["ng"], c["nlay"], NCOL, P(bits)) == 0, _last_error()


def _call(c, dev, top_at_1, nmus=1, bits=None, emis_by_band=True, inc=False, check=True, cloud=None, ncol=NCOL):
    """The entry on the case, outputs pre-filled with NaN.  bits: armed as the cloud mask; cloud: (tau_bnd, ssa_bnd,
    g_bnd) other than the case's (None entries: NULL) -> the 2 flux arrays, or (rc, arrays) with check=False."""
    d = c["dev"]
    outs = [torch.full((NCOL, c["nlay"] + 1), NAN, device=dev) for _ in range(2)]
    cloud = (d["tb"], d["wb"], d["gb"]) if cloud is None else cloud
    if bits is not None:
        _arm_mask(c, bits)
    rc = getattr(_L(), ENTRY)(*_head(c, top_at_1, nmus, inc, ncol=ncol), *[P(a) for a in cloud],
                              *_planck_tail(c, top_at_1, emis_by_band), *[P(o) for o in outs])
    torch.cuda.synchronize()
    res = [o.cpu().numpy() for o in outs]
    if check:
        assert rc == 0, _last_error()
        return res
    return rc, res


def _composition(c, dev, top_at_1, nmus, mask):
    """The existing entries on copies of the same device arrays: the Planck sources, zeroed ssa / g, the (sampled)
    increment, the rescaled solver."""
    from rrtmgpnn._lib import int_array
    L, d, kd, ng, nlay, nb = _L(), c["dev"], c["kd"], c["ng"], c["nlay"], c["nb"]
    lims = int_array(np.asarray(c["lims"]).ravel())
    lay = d["pfrac"].clone()
    lev = torch.empty((NCOL, nlay + 1, ng), device=dev)
    sfc, jac, emis = (torch.empty((NCOL, ng), device=dev) for _ in range(3))
    assert L.rrtmgpnn_compute_planck_source_nn(
        _ctx(), NCOL, nlay, nb, ng, kd["nPlanckTemp"], P(d["tlay"]), P(d["tlev"]), P(d["tsfc"]), nlay if top_at_1 else 1,
        lims, float(kd["temp_ref_min"][0]), float(kd["totplnk_delta"]), P(d["totplnk"]), P(sfc), P(jac), P(lay),
        P(lev)) == 0, _last_error()
    tau, ssa, g = d["tau"].clone(), torch.zeros_like(d["tau"]), torch.zeros_like(d["tau"])
    if mask is None:
        assert L.rrtmgpnn_increment_bybnd(_ctx(), NCOL, nlay, ng, nb, lims, P(tau), P(ssa), P(g), P(d["tb"]), P(d["wb"]),
                                          P(d["gb"])) == 0, _last_error()
    else:
        bytes_ = torch.as_tensor(np.ascontiguousarray(mask, np.uint8), device=dev)
        smp = [torch.empty_like(d["tau"]) for _ in range(3)]
        assert L.rrtmgpnn_draw_samples(_ctx(), ng, nlay, NCOL, nb, lims, P(bytes_), P(d["tb"]), P(d["wb"]), P(d["gb"]),
                                       *[P(s) for s in smp]) == 0, _last_error()
        assert L.rrtmgpnn_increment(_ctx(), NCOL, nlay, ng, P(tau), P(ssa), P(g), *[P(s) for s in smp]) == 0, _last_error()
    assert L.rrtmgpnn_expand_band_to_gpt(_ctx(), nb, ng, NCOL, lims, P(d["emis_bnd"]), P(emis)) == 0, _last_error()
    outs = [torch.full((NCOL, nlay + 1), NAN, device=dev) for _ in range(2)]
    assert L.rrtmgpnn_lw_solver_1rescl(*_head(c, top_at_1, nmus)[:-1], P(tau), P(ssa), P(g), P(lay), P(lev), P(emis),
                                       P(sfc), *[P(o) for o in outs]) == 0, _last_error()
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs]


def _noscat_planck(c, dev, top_at_1, nmus):
    outs = [torch.full((NCOL, c["nlay"] + 1), NAN, device=dev) for _ in range(2)]
    assert _L().rrtmgpnn_lw_solver_noscat_planck(*_head(c, top_at_1, nmus), *_planck_tail(c, top_at_1),
                                                 *[P(o) for o in outs]) == 0, _last_error()
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs]


@CASES
@ORIENT
@NMUS
def test_against_the_composed_oracle(dev, orc, ng, nlay, top_at_1, nmus):
    """1 and 3: every mask kind against the oracle; all ones is the unmasked call, all zeros the clear entry."""
    c = case(ng, nlay, dev)
    got = {}
    for kind in S.MASKS:
        mask = S.mask_for(c, kind)
        got[kind] = _call(c, dev, top_at_1, nmus, bits=None if mask is None else _bits_t(mask, dev))
        _same(got[kind], S.expect(orc, c, kind, top_at_1, nmus), "%s against the oracle" % (kind,))
    _same(got["ones"], got[None], "all ones against the unmasked call")
    _same(got["zeros"], _noscat_planck(c, dev, top_at_1, nmus), "all zeros against lw_solver_noscat_planck")
    assert (got["sampled"][1] != got[None][1]).any() and (got["sampled"][1] != got["zeros"][1]).any()


@CASES
@ORIENT
@NMUS
def test_against_the_gpu_composition(dev, ng, nlay, top_at_1, nmus):
    """2: the existing entries on the same device arrays; the caller's tau and pfrac (and band arrays) are only read."""
    c = case(ng, nlay, dev)
    d = c["dev"]
    before = {k: d[k].clone() for k in ("tau", "pfrac", "tb", "wb", "gb")}
    for kind in (None, "sampled"):
        mask = S.mask_for(c, kind)
        got = _call(c, dev, top_at_1, nmus, bits=None if mask is None else _bits_t(mask, dev))
        _same(got, _composition(c, dev, top_at_1, nmus, mask), "%s against the composition" % (kind,))
    assert all(torch.equal(d[k], v) for k, v in before.items()), "an input was modified"


@pytest.mark.parametrize("ng,nlay", [(256, 11), (30, 7)])
@ORIENT
@NMUS
def test_emissivity_per_gpoint_and_incident_flux(dev, orc, ng, nlay, top_at_1, nmus):
    """4 and 5: emis_by_band = 0 (a per-g-point emissivity) and a non-NULL inc_flux, unmasked and sampled."""
    c = case(ng, nlay, dev)
    for kind in (None, "sampled"):
        mask = S.mask_for(c, kind)
        bits = None if mask is None else _bits_t(mask, dev)
        plain = S.expect(orc, c, kind, top_at_1, nmus)
        for by_band, inc in ((False, False), (True, True), (False, True)):
            got = _call(c, dev, top_at_1, nmus, bits=bits, emis_by_band=by_band, inc=inc)
            want = S.expect(orc, c, kind, top_at_1, nmus, emis_by_band=by_band, inc=inc)
            _same(got, want, "%s, emis_by_band=%d, inc_flux=%s" % (kind, by_band, inc))
            assert (want[0] != plain[0]).any() and (not inc or (want[1] != plain[1]).any())


def test_request_lifetime_and_refusals(dev, orc):
    """6: the mask request belongs to one call; by-band (separate and paired), Jacobian and aerosol requests are refused
    with the entry's name, write nothing and leave nothing armed; NULL band arrays and foreign mask extents are
    argument errors; ncol == 0 is OK; the other rescaled entries keep refusing a mask."""
    from rrtmgpnn._lib import int_array
    L = _L()
    c = case(72, 7, dev)
    d, ng, nlay, nb = c["dev"], c["ng"], c["nlay"], c["nb"]
    plain = _call(c, dev, True)
    _same(plain, S.expect(orc, c, None, True, 1), "the plain call")
    bits = _bits_t(S.mask_for(c, "sampled"), dev)
    masked = _call(c, dev, True, bits=bits)
    assert (masked[1] != plain[1]).any()
    _same(_call(c, dev, True), plain, "the mask outlived its call")
    lims = int_array(np.asarray(c["lims"]).ravel())
    bnd = [torch.full((NCOL, nlay + 1, nb), NAN, device=dev) for _ in range(2)]
    jac = torch.full((NCOL, nlay + 1), NAN, device=dev)

    def byband():
        return L.rrtmgpnn_solver_request_byband(_ctx(), nb, lims, P(bnd[0]), P(bnd[1]), None)

    def paired():
        return L.rrtmgpnn_solver_request_byband_mcica(_ctx(), nb, lims, P(bnd[0]), P(bnd[1]), None, ng, nlay, NCOL, P(bits))

    def jacobian():
        return L.rrtmgpnn_solver_request_jacobian(_ctx(), ng, nlay, NCOL, None, P(jac))

    def aerosol():
        return L.rrtmgpnn_solver_request_aerosol(_ctx(), nb, nlay, NCOL, P(d["tb"]), None, None)

    def wrong_mask():
        return L.rrtmgpnn_solver_request_cloud_mask(_ctx(), ng, nlay + 1, NCOL, P(bits))

    for arm in (byband, paired, jacobian, aerosol, wrong_mask):
        assert arm() == 0, _last_error()
        rc, out = _call(c, dev, True, check=False)
        assert rc == ERR_ARGUMENT, (arm.__name__, rc, _last_error())
        assert NAME in _last_error(), (arm.__name__, _last_error())
        assert all(np.isnan(o).all() for o in out), "a refused call wrote (%s)" % arm.__name__
        _same(_call(c, dev, True), plain, "something stayed armed after the %s refusal" % arm.__name__)
    assert all(torch.isnan(b).all() for b in bnd) and torch.isnan(jac).all(), "a refused call wrote a requested output"
    # all three band arrays are required
    for k in range(3):
        cloud = [d["tb"], d["wb"], d["gb"]]
        cloud[k] = None
        rc, out = _call(c, dev, True, check=False, cloud=cloud)
        assert rc == ERR_ARGUMENT and NAME in _last_error(), (k, rc, _last_error())
        assert all(np.isnan(o).all() for o in out)
    rc, _ = _call(c, dev, True, check=False, ncol=-1)
    assert rc == ERR_ARGUMENT
    # ncol == 0: OK, nothing written, and an armed mask of those extents is cleared
    assert L.rrtmgpnn_solver_request_cloud_mask(_ctx(), ng, nlay, 0, P(bits)) == 0
    rc, out = _call(c, dev, True, check=False, ncol=0)
    assert rc == 0, _last_error()
    assert all(np.isnan(o).all() for o in out)
    _same(_call(c, dev, True), plain, "the mask of the empty call stayed armed")
    # the unfused rescaled entry keeps refusing a mask
    _arm_mask(c, bits)
    outs = [torch.full((NCOL, nlay + 1), NAN, device=dev) for _ in range(2)]
    z = torch.zeros_like(d["tau"])
    lev = torch.zeros((NCOL, nlay + 1, ng), device=dev)
    rc = L.rrtmgpnn_lw_solver_1rescl(*_head(c, True, 1), P(z), P(z), P(d["pfrac"]), P(lev), P(d["emis_gpt"]),
                                     P(d["emis_gpt"]), *[P(o) for o in outs])
    torch.cuda.synchronize()
    assert rc == ERR_ARGUMENT and "cloud mask" in _last_error()
    _same(_call(c, dev, True), plain, "something stayed armed after lw_solver_1rescl's refusal")


# ---- the class layer --------------------------------------------------------------------------------------------------
def test_class_layer_fused_against_the_sequence(dev, rfmip, monkeypatch):
    """7: clr_all_sky.rte_lw with by-band 2str clouds: LW_SCAT_FUSED True against False, masked (mask_bits and cloud_mask
    of one mask) and unmasked, all four flux arrays bit for bit.  The fused route allocates one 1scl gas object and no
    two-stream one (no g-point ssa / g arrays are allocated or zeroed)."""
    from conftest import subset
    from rrtmgpnn import api, clr_all_sky, data
    p = subset(rfmip, np.arange(4) * 400)
    ncol, nlay = p["ncol"], p["nlay"]
    play, tlay, plev = (T(p[k], dev) for k in ("play", "tlay", "plev"))
    kd = api.GasOpticsRRTMGP()
    api.stop_on_err(kd.load("lw"))
    nets = [api.RrtmgpNetwork(0).load_netcdf(data.path(n)) for n in ("lw_abs", "lw_pfrac")]
    gases = api.GasConcs()
    api.stop_on_err(gases.init(list(p["gases"])))
    for k, v in p["gases"].items():
        api.stop_on_err(gases.set_vmr(k, T(v, dev)))
    nb, ng = kd.get_nband(), kd.get_ngpt()
    rng = np.random.default_rng(97)
    cld = api.OpticalProps2str()
    assert cld.init(kd.get_band_lims_wavenumber()) == "" and cld.alloc_2str(ncol, nlay, device=dev) == ""
    cld.tau.copy_(T(rng.lognormal(0, 1, (ncol, nlay, nb)), dev))
    cld.ssa.copy_(T(rng.uniform(0.2, 0.9, (ncol, nlay, nb)), dev))
    cld.g.copy_(T(rng.uniform(0.5, 0.95, (ncol, nlay, nb)), dev))
    mask = rng.random((ncol, nlay, ng)) < 0.5
    bits = _bits_t(mask, dev)
    bytes_ = torch.as_tensor(np.ascontiguousarray(mask, np.uint8), device=dev)
    emis = T(np.repeat(np.asarray(p["sfc_emis"], np.float32)[:, None], nb, axis=1), dev)

    def fl():
        return api.FluxesBroadband(*[torch.full((ncol, nlay + 1), NAN, device=dev) for _ in range(3)])

    # what each rte_lw call allocates: the fused route one 1scl object (tau), never (ncol, nlay, ngpt) ssa / g arrays
    allocs = []
    orig = {"2str": api.OpticalProps2str.alloc_2str, "1scl": api.OpticalProps1scl.alloc_1scl}

    def spy(kind):
        def alloc(self, *args, **kw):
            allocs.append(kind)
            return orig[kind](self, *args, **kw)
        return alloc

    monkeypatch.setattr(api.OpticalProps2str, "alloc_2str", spy("2str"))
    monkeypatch.setattr(api.OpticalProps1scl, "alloc_1scl", spy("1scl"))
    res = {}
    for route in (True, False):
        clr_all_sky.LW_SCAT_FUSED = route
        try:
            for masked in (False, True):
                for nmu in (1, 3):
                    a, cl = fl(), fl()
                    del allocs[:]
                    e = clr_all_sky.rte_lw(kd, gases, play, tlay, plev, T(p["tsfc"], dev), emis, cld, a, cl,
                                           t_lev=T(p["tlev"], dev), neural_nets=nets, n_gauss_angles=nmu,
                                           mask_bits=bits if masked else None, cloud_mask=bytes_ if masked else None)
                    assert e == "", e
                    if route:
                        assert allocs == ["1scl"], "the fused route allocated %s" % allocs
                    else:
                        assert "2str" in allocs and "1scl" not in allocs, "the sequence allocated %s" % allocs
                    res[(masked, nmu, route)] = [t.cpu().numpy() for t in (a.flux_up, a.flux_dn, cl.flux_up, cl.flux_dn)]
        finally:
            clr_all_sky.LW_SCAT_FUSED = True
    for masked in (False, True):
        for nmu in (1, 3):
            fused, seq = res[(masked, nmu, True)], res[(masked, nmu, False)]
            assert all(np.isfinite(v).all() for v in fused)
            _same(fused, seq, "rte_lw masked=%s nmu=%d" % (masked, nmu))
            assert (fused[1] != fused[3]).any(), "the cloud does not show"
    assert (res[(True, 1, True)][1] != res[(False, 1, True)][1]).any(), "the mask does not show"
