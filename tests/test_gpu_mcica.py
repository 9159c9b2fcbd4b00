"""GPU: McICA cloud sampling (extensions/cloud_optics/mo_cloud_sampling.F90), everything bit for bit.

* the mask kernels (bytes and packed bits) against the numpy restatement tests/mcica_ref.py and the fixture made from
  the reference's own module (tests/golden/mcica_masks.npz);
* draw_samples for 1scl and 2str, and the class layer's error strings;
* the packed mask inside the fused solvers (rrtmgpnn_solver_request_cloud_mask): against the composed oracle
  (restated mask -> merge -> same-resolution increment -> solver) and against this library's own unfused route
  (draw_samples -> increment -> solver);
* the request's semantics: cleared after success and after failure, extents, every refusing entry and combination.
"""
import os

import numpy as np
import pytest

import mcica_ref as M

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARGUMENT, ERR_UNSUPPORTED = 1, 4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a device"
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def T(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=dev)


def _masks_gpu(dev, r, cf, ov, want_bytes=True, want_bits=True):
    """Both outputs of one mask call through the class layer, as numpy (None where not asked for)."""
    from rrtmgpnn import cloud_sampling as cs
    ncol, nlay, ngpt = r.shape
    # poisoned outputs: every element must be written (the packed words' unused high bits with zeros)
    mb = torch.full((ncol, nlay, ngpt), 7, dtype=torch.uint8, device=dev) if want_bytes else None
    bits = torch.full((ncol, nlay, (ngpt + 31) // 32), -1, dtype=torch.int32, device=dev) if want_bits else None
    if ov is None:
        e = cs.sampled_mask_max_ran(T(r, dev), T(cf, dev), mb, bits)
    else:
        e = cs.sampled_mask_exp_ran(T(r, dev), T(cf, dev), T(ov, dev), mb, bits)
    assert e == ""
    torch.cuda.synchronize()
    return (None if mb is None else mb.cpu().numpy(),
            None if bits is None else bits.cpu().numpy().view(np.uint32))


@pytest.mark.parametrize("overlap", ["max_ran", "exp_ran"])
@pytest.mark.parametrize("shape", M.CASES, ids=lambda s: "g%d-l%d-c%d" % s)
def test_mask_kernels_match_restatement(dev, shape, overlap):
    ngpt, nlay, ncol = shape
    r, cf, ov = M.build(ngpt, nlay, ncol, M.case_seed(*shape))
    ov = ov if overlap == "exp_ran" else None
    want = M.sampled_mask(r, cf, ov)
    mb, bits = _masks_gpu(dev, r, cf, ov)
    np.testing.assert_array_equal(mb, want.astype(np.uint8))
    np.testing.assert_array_equal(bits, M.pack_bits(want))


@pytest.mark.parametrize("overlap", ["max_ran", "exp_ran"])
@pytest.mark.parametrize("outputs", ["bytes", "bits", "both"])
def test_mask_kernels_match_reference_fixture(dev, overlap, outputs):
    """The fixture's 36 columns (every designed situation, tests/test_mcica_host.py), with and without each output;
    clear layers' randoms are NaN here: the reference reads randoms only where cloud_frac > 0."""
    d = np.load(os.path.join(ROOT, "tests", "golden", "mcica_masks.npz"))
    r, cf = d["randoms"].copy(), d["cloud_frac"]
    r[cf == 0] = np.nan
    ov = d["overlap_param"] if overlap == "exp_ran" else None
    want = d["mask_" + overlap]
    mb, bits = _masks_gpu(dev, r, cf, ov, outputs != "bits", outputs != "bytes")
    if mb is not None:
        np.testing.assert_array_equal(mb, want)
    if bits is not None:
        np.testing.assert_array_equal(bits, M.pack_bits(want.astype(bool)))
    assert (mb is None) == (outputs == "bits") and (bits is None) == (outputs == "bytes")


def test_mask_error_strings(dev):
    from rrtmgpnn import api, cloud_sampling as cs
    r, cf, ov = (T(a, dev) for a in M.build(40, 7, 3, 1))
    mb = torch.zeros((3, 7, 40), dtype=torch.uint8, device=dev)
    pre = "sampled_mask_max_ran: "  # exp_ran carries max_ran's prefix in the reference too
    assert cs.sampled_mask_max_ran(r, cf[:, :6], mb) == \
        pre + "sizes of randoms(ngpt,nlay,ncol) and cloud_frac(ncol,nlay) are inconsistent"
    assert cs.sampled_mask_max_ran(r, cf, mb[:2]) == \
        pre + "sizes of randoms(ngpt,nlay,ncol) and cloud_mask(ncol,nlay,ngpt) are inconsistent"
    assert cs.sampled_mask_exp_ran(r, cf[:, :6], ov, mb) == \
        pre + "sizes of randoms(ngpt,nlay,ncol) and cloud_frac(ncol,nlay) are inconsistent"
    assert cs.sampled_mask_exp_ran(r, cf, ov[:, :4], mb) == \
        pre + "sizes of randoms(ngpt,nlay,ncol) and overlap_param(ncol,nlay-1) are inconsistent"
    assert cs.sampled_mask_exp_ran(r, cf, ov, mb[:, :, :39]) == \
        pre + "sizes of randoms(ngpt,nlay,ncol) and cloud_mask(ncol,nlay,ngpt) are inconsistent"
    assert cs.sampled_mask_max_ran(r, cf) != ""  # no output at all
    api.rte_config_checks(True)
    try:
        hi, lo = cf.clone(), cf.clone()
        hi[1, 2], lo[0, 0] = 1.5, -0.1
        for bad in (hi, lo):
            assert cs.sampled_mask_max_ran(r, bad, mb) == pre + "cloud fraction values out of range [0,1]"
            assert cs.sampled_mask_exp_ran(r, bad, ov, mb) == pre + "cloud fraction values out of range [0,1]"
        for v in (1.25, -1.25):
            bad = ov.clone()
            bad[2, 3] = v
            assert cs.sampled_mask_exp_ran(r, cf, bad, mb) == pre + "overlap_param values out of range [-1,1]"
        assert cs.sampled_mask_exp_ran(r, cf, ov, mb) == ""
    finally:
        api.rte_config_checks(False)


# ---------------------------------------------------------------------------------------------
def _props(api, nstr, wvn, ncol, nlay, dev, gpt=None):
    p = api.OpticalProps1scl() if nstr == 1 else api.OpticalProps2str()
    assert p.init(wvn, gpt) == ""
    assert (p.alloc_1scl(ncol, nlay, device=dev) if nstr == 1 else p.alloc_2str(ncol, nlay, device=dev)) == ""
    return p


@pytest.mark.parametrize("nstr", [1, 2])
def test_draw_samples(dev, nstr):
    from rrtmgpnn import api, cloud_sampling as cs, data
    kd = data.load_kdist("sw")
    ngpt, nb, ncol, nlay = kd["ngpt"], kd["nband"], 5, 7
    rng = np.random.default_rng(nstr)
    mask = rng.random((ncol, nlay, ngpt)) < 0.5
    clouds = _props(api, nstr, kd["band_lims_wvn"], ncol, nlay, dev)
    sampled = _props(api, nstr, kd["band_lims_wvn"], ncol, nlay, dev, kd["band_lims_gpt"])
    vals = [rng.lognormal(0, 1, (ncol, nlay, nb)).astype(np.float32) for _ in range(3 if nstr == 2 else 1)]
    names = ("tau", "ssa", "g")[:len(vals)]
    for n, v in zip(names, vals):
        getattr(clouds, n).copy_(T(v, dev))
        getattr(sampled, n).fill_(float("nan"))
    mt = torch.as_tensor(mask.astype(np.uint8), device=dev)
    assert cs.draw_samples(mt, clouds, sampled) == ""
    for n, v in zip(names, vals):
        np.testing.assert_array_equal(getattr(sampled, n).cpu().numpy(), M.draw(mask, v, kd["band_lims_gpt"]), err_msg=n)
    # the reference's error strings
    other = _props(api, 3 - nstr, kd["band_lims_wvn"], ncol, nlay, dev, kd["band_lims_gpt"])
    assert cs.draw_samples(mt, clouds, other) == \
        "draw_samples: by-band and sampled cloud properties need to be the same variable type"
    assert cs.draw_samples(mt, type(clouds)(), sampled) == "draw_samples: cloud optical properties are not initialized"
    assert cs.draw_samples(mt, clouds, type(sampled)()) == \
        "draw_samples: sampled cloud optical properties are not initialized"
    lw = data.load_kdist("lw")
    assert cs.draw_samples(mt, clouds, _props(api, nstr, lw["band_lims_wvn"], ncol, nlay, dev, lw["band_lims_gpt"])) \
        == "draw_samples: by-band and sampled cloud properties spectral structure is different"
    assert cs.draw_samples(mt[:, :6], clouds, sampled) == \
        "draw_samples: cloud mask and cloud optical properties have different ncol and/or nlay"
    assert cs.draw_samples(mt[:4].contiguous(), _props(api, nstr, kd["band_lims_wvn"], 4, nlay, dev), sampled) == \
        "draw_samples: sampled/unsampled cloud optical properties have different ncol and/or nlay"

    class Nstr(api._OpticalPropsArry):
        pass
    n = Nstr()
    assert n.init(kd["band_lims_wvn"]) == ""
    assert cs.draw_samples(mt, n, sampled) == "draw_samples: sampling isn't implemented yet for ty_optical_props_nstr"


# ---------------------------------------------------------------------------------------------
# The packed mask inside the fused solvers.  Shapes: 3 columns (odd: the SW block of two columns has a ragged last
# block) x 7 layers (no multiple of the LW ring, the prefetch depths or the SW checkpoint stride of 3).
NCOL, NLAY = 3, 7


def _mask_for(ngpt, seed, kind="sampled"):
    if kind == "ones":
        return np.ones((NCOL, NLAY, ngpt), bool)
    if kind == "zeros":
        return np.zeros((NCOL, NLAY, ngpt), bool)
    r, cf, ov = M.build(ngpt, NLAY, NCOL, seed)
    return M.sampled_mask(r, cf, ov)


def _bits_t(mask, dev):
    return torch.as_tensor(M.pack_bits(mask).view(np.int32), device=dev)


@pytest.fixture(scope="module")
def lw_case(dev):
    """LW inputs shared by the fused-LW tests (never modified)."""
    from rrtmgpnn import data
    kl = data.load_kdist("lw")
    rng = np.random.default_rng(77)
    ng, nb = kl["ngpt"], kl["nband"]
    c = {"kd": kl, "ng": ng, "nb": nb}
    c["tau"] = rng.lognormal(-2, 2, (NCOL, NLAY, ng)).astype(np.float32)
    c["pfrac"] = rng.uniform(0, 0.2, (NCOL, NLAY, ng)).astype(np.float32)
    c["tb"] = rng.lognormal(0, 1, (NCOL, NLAY, nb)).astype(np.float32)  # every layer cloudy: the mask decides
    c["tlay"] = rng.uniform(200, 300, (NCOL, NLAY)).astype(np.float32)
    c["tlev"] = rng.uniform(200, 300, (NCOL, NLAY + 1)).astype(np.float32)
    c["tsfc"] = rng.uniform(250, 310, NCOL).astype(np.float32)
    c["emis_gpt"] = rng.uniform(0.9, 1, (NCOL, ng)).astype(np.float32)
    c["emis_bnd"] = rng.uniform(0.9, 1, (NCOL, nb)).astype(np.float32)
    c["dev"] = {k: T(c[k], dev) for k in ("tau", "pfrac", "tb", "tlay", "tlev", "tsfc", "emis_gpt", "emis_bnd")}
    c["dev"]["totplnk"] = T(kl["totplnk"], dev)
    return c


def _lw_call(c, dev, entry, top_at_1, nmus, by_band, tau=None, with_tb=True):
    """One of the fused-Planck LW entries on the shared inputs -> (up, dn) numpy."""
    from rrtmgpnn import _lib
    from rrtmgpnn._lib import float_array, int_array
    from rrtmgpnn.api import GAUSS_DS, GAUSS_WTS, context
    L, d, kl = _lib.lib(), c["dev"], c["kd"]
    up, dn = (torch.full((NCOL, NLAY + 1), float("nan"), device=dev) for _ in range(2))
    emis = d["emis_bnd"] if by_band else d["emis_gpt"]
    common = (c["nb"], kl["nPlanckTemp"], d["tlay"].data_ptr(), d["tlev"].data_ptr(), d["tsfc"].data_ptr(),
              NLAY if top_at_1 else 1, int_array(kl["band_lims_gpt"].ravel()), float(kl["temp_ref_min"][0]),
              float(kl["totplnk_delta"]), d["totplnk"].data_ptr(), int(by_band), emis.data_ptr())
    t = d["tau"] if tau is None else tau
    head = (context(0).h, c["ng"], NLAY, NCOL, int(top_at_1), nmus, float_array(GAUSS_DS[nmus]),
            float_array(GAUSS_WTS[nmus]), None, t.data_ptr())
    mid = (d["tb"].data_ptr(),) if with_tb else ()
    rc = getattr(L, entry)(*head, *mid, d["pfrac"].data_ptr(), *common, up.data_ptr(), dn.data_ptr())
    torch.cuda.synchronize()
    return rc, up.cpu().numpy(), dn.cpu().numpy()


def _arm(ngpt, bits, nlay=NLAY, ncol=NCOL):
    from rrtmgpnn import _lib
    from rrtmgpnn.api import context
    _lib.check(_lib.lib().rrtmgpnn_solver_request_cloud_mask(context(0).h, ngpt, nlay, ncol, bits.data_ptr()))


def _expand(bnd, lims, ngpt):
    out = np.zeros(bnd.shape[:-1] + (ngpt,), np.float32)
    for ib, (lo, hi) in enumerate(np.asarray(lims).reshape(-1, 2)):
        out[..., lo - 1:hi] = bnd[..., ib:ib + 1]
    return out


@pytest.mark.parametrize("by_band", [False, True], ids=["emis_gpt", "emis_bnd"])
@pytest.mark.parametrize("top_at_1", [True, False])
@pytest.mark.parametrize("nmus", [1, 3])
def test_fused_lw_mask(dev, orc, lw_case, nmus, top_at_1, by_band):
    from rrtmgpnn import _lib
    from rrtmgpnn._lib import int_array
    from rrtmgpnn.api import context
    c, L, ctx = lw_case, _lib.lib(), context(0).h
    ng, nb, kl = c["ng"], c["nb"], c["kd"]
    mask = _mask_for(ng, 5)
    bits = _bits_t(mask, dev)
    tau0 = c["dev"]["tau"].clone()
    _arm(ng, bits)
    rc, up, dn = _lw_call(c, dev, "rrtmgpnn_lw_solver_noscat_planck_inc", top_at_1, nmus, by_band)
    assert rc == 0 and torch.equal(tau0, c["dev"]["tau"])
    # (1) the composed oracle: restated mask -> merge -> same-resolution increment -> Planck sources -> solver
    ident = np.stack([np.arange(1, ng + 1)] * 2, axis=1).astype(np.int32)
    (tau_all,) = orc.increment_bybnd(ident, [c["tau"]], [M.draw(mask, c["tb"], kl["band_lims_gpt"])])
    lay, lev, sfc, _ = orc.planck_source(kl, c["tlay"], c["tlev"], c["tsfc"], c["pfrac"], NLAY if top_at_1 else 1)
    emis = _expand(c["emis_bnd"], kl["band_lims_gpt"], ng) if by_band else c["emis_gpt"]
    wup, wdn = orc.lw_solver(tau_all, lay, lev, emis, sfc, top_at_1=top_at_1, nmus=nmus)
    np.testing.assert_array_equal(up, wup)
    np.testing.assert_array_equal(dn, wdn)
    # (2) this library's unfused route: draw_samples -> increment -> the plain fused-Planck solver
    samp = torch.empty((NCOL, NLAY, ng), device=dev)
    mb = torch.as_tensor(mask.astype(np.uint8), device=dev)
    _lib.check(L.rrtmgpnn_draw_samples(ctx, ng, NLAY, NCOL, nb, int_array(kl["band_lims_gpt"].ravel()), mb.data_ptr(),
                                       c["dev"]["tb"].data_ptr(), None, None, samp.data_ptr(), None, None))
    tau2 = c["dev"]["tau"].clone()
    _lib.check(L.rrtmgpnn_increment(ctx, NCOL, NLAY, ng, tau2.data_ptr(), None, None, samp.data_ptr(), None, None))
    rc, up2, dn2 = _lw_call(c, dev, "rrtmgpnn_lw_solver_noscat_planck", top_at_1, nmus, by_band, tau=tau2, with_tb=False)
    assert rc == 0
    np.testing.assert_array_equal(up, up2)
    np.testing.assert_array_equal(dn, dn2)
    # the mask matters: neither the overcast nor the clear fluxes
    _, oup, odn = _lw_call(c, dev, "rrtmgpnn_lw_solver_noscat_planck_inc", top_at_1, nmus, by_band)
    _, cup, cdn = _lw_call(c, dev, "rrtmgpnn_lw_solver_noscat_planck", top_at_1, nmus, by_band, with_tb=False)
    assert (dn != odn).any() and (dn != cdn).any()
    # all ones == the unmasked _inc call; all zeros == _planck
    ones_bits = _bits_t(_mask_for(ng, 0, "ones"), dev)  # kept alive until its solver call has run
    _arm(ng, ones_bits)
    _, up1, dn1 = _lw_call(c, dev, "rrtmgpnn_lw_solver_noscat_planck_inc", top_at_1, nmus, by_band)
    np.testing.assert_array_equal(up1, oup)
    np.testing.assert_array_equal(dn1, odn)
    zero_bits = _bits_t(_mask_for(ng, 0, "zeros"), dev)
    _arm(ng, zero_bits)
    _, up0, dn0 = _lw_call(c, dev, "rrtmgpnn_lw_solver_noscat_planck_inc", top_at_1, nmus, by_band)
    np.testing.assert_array_equal(up0, cup)
    np.testing.assert_array_equal(dn0, cdn)


# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sw_case(dev):
    from rrtmgpnn import data
    ks = data.load_kdist("sw")
    rng = np.random.default_rng(78)
    ng, nb = ks["ngpt"], ks["nband"]
    c = {"kd": ks, "ng": ng, "nb": nb}
    c["tau"] = rng.lognormal(-2, 2, (NCOL, NLAY, ng)).astype(np.float32)
    c["ssa"] = rng.uniform(0, 1, (NCOL, NLAY, ng)).astype(np.float32)
    c["g"] = rng.uniform(0, 0.8, (NCOL, NLAY, ng)).astype(np.float32)
    c["bt"] = rng.lognormal(0, 1, (NCOL, NLAY, nb)).astype(np.float32)
    c["bw"] = rng.uniform(0.5, 1, (NCOL, NLAY, nb)).astype(np.float32)
    c["bg"] = rng.uniform(0, 0.9, (NCOL, NLAY, nb)).astype(np.float32)
    c["mu0"] = rng.uniform(0.1, 1, NCOL).astype(np.float32)
    c["inc"] = rng.uniform(0, 5, (NCOL, ng)).astype(np.float32)
    c["alb"] = rng.uniform(0, 1, (NCOL, ng)).astype(np.float32)
    # the RFMIP form's inputs: sza below and above the usecol bound, spectrally constant albedo
    c["solar"] = rng.uniform(0.1, 5, ng).astype(np.float32)
    c["tsi"] = rng.uniform(1300, 1400, NCOL).astype(np.float32)
    c["sfc_alb"] = rng.uniform(0, 1, NCOL).astype(np.float32)
    c["sza"] = np.array([10.0, 60.0, 85.0], np.float32)
    bl = np.array(ks["band_lims_gpt"], dtype=np.int64).reshape(-1, 2)
    odd = bl.copy()
    odd[0, 1] -= 1
    odd[1, 0] -= 1
    c["lims"] = {"pair": bl, "general": odd}
    c["dev"] = {k: T(c[k], dev) for k in ("tau", "ssa", "g", "bt", "bw", "bg", "mu0", "inc", "alb", "solar", "tsi",
                                         "sfc_alb", "sza")}
    return c


def _sw_inc(c, dev, lims, with_g, top_at_1, tau=None, ssa=None, g=None, plain=False):
    """rrtmgpnn_sw_solver_2stream_inc (or, plain, rrtmgpnn_sw_solver_2stream on the given arrays) -> rc, 3 fluxes."""
    from rrtmgpnn import _lib
    from rrtmgpnn._lib import int_array
    from rrtmgpnn.api import context
    L, d = _lib.lib(), c["dev"]
    outs = [torch.full((NCOL, NLAY + 1), float("nan"), device=dev) for _ in range(3)]
    t, w = (d["tau"] if tau is None else tau), (d["ssa"] if ssa is None else ssa)
    gg = g if g is not None else (d["g"] if with_g else None)
    head = (context(0).h, c["ng"], NLAY, NCOL, int(top_at_1), d["inc"].data_ptr(), None, t.data_ptr(), w.data_ptr(),
            None if gg is None else gg.data_ptr())
    tail = (d["mu0"].data_ptr(), d["alb"].data_ptr(), d["alb"].data_ptr(), *[o.data_ptr() for o in outs])
    if plain:
        rc = L.rrtmgpnn_sw_solver_2stream(*head, *tail)
    else:
        rc = L.rrtmgpnn_sw_solver_2stream_inc(*head, c["nb"], int_array(lims.ravel()), d["bt"].data_ptr(),
                                              d["bw"].data_ptr(), d["bg"].data_ptr(), *tail)
    torch.cuda.synchronize()
    return rc, [o.cpu().numpy() for o in outs]


def _sw_rfmip(c, dev, lims, with_g, top_at_1, nbnd=None):
    from rrtmgpnn import _lib
    from rrtmgpnn._lib import int_array
    from rrtmgpnn.api import context
    L, d = _lib.lib(), c["dev"]
    outs = [torch.full((NCOL, NLAY + 1), float("nan"), device=dev) for _ in range(3)]
    scr = [torch.empty((NCOL, c["ng"]), device=dev), torch.empty((NCOL, c["ng"]), device=dev),
           torch.empty(NCOL, device=dev)]
    nb = c["nb"] if nbnd is None else nbnd
    rc = L.rrtmgpnn_sw_solver_2stream_rfmip(
        context(0).h, c["ng"], NLAY, NCOL, int(top_at_1), d["solar"].data_ptr(), d["tsi"].data_ptr(),
        d["sfc_alb"].data_ptr(), d["sza"].data_ptr(), d["tau"].data_ptr(), d["ssa"].data_ptr(),
        d["g"].data_ptr() if with_g else None, nb, int_array(lims.ravel()), d["bt"].data_ptr(), d["bw"].data_ptr(),
        d["bg"].data_ptr(), *[s.data_ptr() for s in scr], *[o.data_ptr() for o in outs])
    torch.cuda.synchronize()
    return rc, [o.cpu().numpy() for o in outs], [s.cpu().numpy() for s in scr]


def _sw_sampled(c, mask, lims):
    """The composed oracle's optical properties: merge, then the same-resolution increment."""
    return [M.draw(mask, c[k], lims) for k in ("bt", "bw", "bg")]


@pytest.mark.parametrize("layout", ["pair", "general"])
@pytest.mark.parametrize("with_g", [True, False], ids=["g", "nog"])
@pytest.mark.parametrize("top_at_1", [True, False])
def test_fused_sw_mask_inc(dev, orc, sw_case, top_at_1, with_g, layout):
    from rrtmgpnn import _lib
    from rrtmgpnn._lib import int_array
    from rrtmgpnn.api import context
    c, L, ctx = sw_case, _lib.lib(), context(0).h
    ng, nb, lims = c["ng"], c["nb"], c["lims"][layout]
    mask = _mask_for(ng, 9)
    saved = [c["dev"][k].clone() for k in ("tau", "ssa", "g")]
    bits = _bits_t(mask, dev)
    _arm(ng, bits)
    rc, got = _sw_inc(c, dev, lims, with_g, top_at_1)
    assert rc == 0, _lib.lib().rrtmgpnn_last_error()
    assert all(torch.equal(a, c["dev"][k]) for a, k in zip(saved, ("tau", "ssa", "g")))
    # (1) the composed oracle
    ident = np.stack([np.arange(1, ng + 1)] * 2, axis=1).astype(np.int32)
    g_in = c["g"] if with_g else np.zeros_like(c["g"])
    io = orc.increment_bybnd(ident, [c["tau"], c["ssa"], g_in], _sw_sampled(c, mask, lims))
    want = orc.sw_solver(*io, c["mu0"], c["inc"], c["alb"], c["alb"], top_at_1=top_at_1)
    for a, b, n in zip(got, want, ("up", "dn", "dir")):
        np.testing.assert_array_equal(a, b, err_msg=n)
    # (2) this library's unfused route
    samp = [torch.empty((NCOL, NLAY, ng), device=dev) for _ in range(3)]
    mb = torch.as_tensor(mask.astype(np.uint8), device=dev)
    d = c["dev"]
    _lib.check(L.rrtmgpnn_draw_samples(ctx, ng, NLAY, NCOL, nb, int_array(lims.ravel()), mb.data_ptr(),
                                       d["bt"].data_ptr(), d["bw"].data_ptr(), d["bg"].data_ptr(),
                                       *[s.data_ptr() for s in samp]))
    t2, w2 = d["tau"].clone(), d["ssa"].clone()
    g2 = d["g"].clone() if with_g else torch.zeros_like(d["g"])
    _lib.check(L.rrtmgpnn_increment(ctx, NCOL, NLAY, ng, t2.data_ptr(), w2.data_ptr(), g2.data_ptr(),
                                    *[s.data_ptr() for s in samp]))
    rc, unf = _sw_inc(c, dev, lims, True, top_at_1, tau=t2, ssa=w2, g=g2, plain=True)
    assert rc == 0
    for a, b, n in zip(got, unf, ("up", "dn", "dir")):
        np.testing.assert_array_equal(a, b, err_msg=n)
    # all ones == the unmasked _inc call, and the sampled mask gives neither that nor the all-zero result
    _, over = _sw_inc(c, dev, lims, with_g, top_at_1)
    ones_bits = _bits_t(_mask_for(ng, 0, "ones"), dev)  # kept alive until its solver call has run
    _arm(ng, ones_bits)
    _, ones = _sw_inc(c, dev, lims, with_g, top_at_1)
    for a, b in zip(ones, over):
        np.testing.assert_array_equal(a, b)
    assert (got[1] != over[1]).any()
    # all zeros == the oracle's increment BY ZEROS (which still rounds tau * ssa / max(eps, tau)), asserted as such:
    # it is not required to be the clear solve
    zero_bits = _bits_t(_mask_for(ng, 0, "zeros"), dev)
    _arm(ng, zero_bits)
    _, zeros = _sw_inc(c, dev, lims, with_g, top_at_1)
    z = np.zeros_like(c["tau"])
    io0 = orc.increment_bybnd(ident, [c["tau"], c["ssa"], g_in], [z, z, z])
    for a, b in zip(zeros, orc.sw_solver(*io0, c["mu0"], c["inc"], c["alb"], c["alb"], top_at_1=top_at_1)):
        np.testing.assert_array_equal(a, b)
    assert (got[1] != zeros[1]).any()


@pytest.mark.parametrize("layout", ["pair", "general"])
@pytest.mark.parametrize("with_g", [True, False], ids=["g", "nog"])
def test_fused_sw_mask_rfmip(dev, orc, sw_case, with_g, layout):
    """The _rfmip entry with nbnd > 0: the boundary conditions it forms (read back from an unmasked run on the
    workspace-plane kernel, which stores them) feed the composed oracle."""
    from rrtmgpnn import api
    c = sw_case
    ng, lims = c["ng"], c["lims"][layout]
    mask = _mask_for(ng, 11)
    api.set_sw_kernel_default(2)
    try:
        rc, _, (toa, alb, mu0) = _sw_rfmip(c, dev, lims, with_g, True)
    finally:
        api.set_sw_kernel_default(0)
    assert rc == 0
    bits = _bits_t(mask, dev)
    for top_at_1 in (True, False):
        _arm(ng, bits)
        rc, got, _ = _sw_rfmip(c, dev, lims, with_g, top_at_1)
        assert rc == 0
        ident = np.stack([np.arange(1, ng + 1)] * 2, axis=1).astype(np.int32)
        g_in = c["g"] if with_g else np.zeros_like(c["g"])
        io = orc.increment_bybnd(ident, [c["tau"], c["ssa"], g_in], _sw_sampled(c, mask, lims))
        want = orc.sw_solver(*io, mu0, toa, alb, alb, top_at_1=top_at_1)
        for a, b, n in zip(got, want, ("up", "dn", "dir")):
            np.testing.assert_array_equal(a, b, err_msg=n)
        _, over, _ = _sw_rfmip(c, dev, lims, with_g, top_at_1)
        assert (got[1] != over[1]).any()


# ---------------------------------------------------------------------------------------------
def _last_error():
    from rrtmgpnn import _lib
    return _lib.lib().rrtmgpnn_last_error().decode()


def test_request_semantics_lw(dev, lw_case):
    """Cleared after success and after failure; extents; the by-band combination; the call after a consumed request is
    the plain one."""
    from rrtmgpnn import _lib
    from rrtmgpnn._lib import int_array
    from rrtmgpnn.api import context
    c, L, ctx = lw_case, _lib.lib(), context(0).h
    ng = c["ng"]
    bits = _bits_t(_mask_for(ng, 5), dev)
    inc = "rrtmgpnn_lw_solver_noscat_planck_inc"
    _, oup, odn = _lw_call(c, dev, inc, True, 1, False)
    _arm(ng, bits)
    rc, mup, mdn = _lw_call(c, dev, inc, True, 1, False)
    assert rc == 0 and (mdn != odn).any()
    rc, up, dn = _lw_call(c, dev, inc, True, 1, False)  # consumed: the plain call again
    assert rc == 0
    np.testing.assert_array_equal(dn, odn)
    np.testing.assert_array_equal(up, oup)
    # extents that are not the call's: refused, and cleared by the failing call
    for ext in ((ng - 32, NLAY, NCOL), (ng, NLAY + 1, NCOL), (ng, NLAY, NCOL + 1)):
        _lib.check(L.rrtmgpnn_solver_request_cloud_mask(ctx, *ext, bits.data_ptr()))
        rc, _, _ = _lw_call(c, dev, inc, True, 1, False)
        assert rc == ERR_ARGUMENT and "cloud mask" in _last_error()
        rc, up, dn = _lw_call(c, dev, inc, True, 1, False)
        assert rc == 0
        np.testing.assert_array_equal(dn, odn)
    # a failing honoured call (bad argument after the request was taken) clears it too
    _arm(ng, bits)
    rc = getattr(L, inc)(ctx, ng, NLAY, NCOL, 1, 1, None, None, None, None, None, None, 0, 0, None, None, None, 1, None,
                         0.0, 0.0, None, 0, None, None, None)
    assert rc == ERR_ARGUMENT
    rc, up, dn = _lw_call(c, dev, inc, True, 1, False)
    assert rc == 0
    np.testing.assert_array_equal(dn, odn)
    # a NULL mask disarms
    _arm(ng, bits)
    _lib.check(L.rrtmgpnn_solver_request_cloud_mask(ctx, 0, 0, 0, None))
    rc, up, dn = _lw_call(c, dev, inc, True, 1, False)
    np.testing.assert_array_equal(dn, odn)
    # together with a by-band request: unsupported, both cleared
    bnd = torch.empty((NCOL, NLAY + 1, c["nb"]), device=dev)
    _arm(ng, bits)
    _lib.check(L.rrtmgpnn_solver_request_byband(ctx, c["nb"], int_array(c["kd"]["band_lims_gpt"].ravel()),
                                                bnd.data_ptr(), None, None))
    rc, _, _ = _lw_call(c, dev, inc, True, 1, False)
    assert rc == ERR_UNSUPPORTED
    rc, up, dn = _lw_call(c, dev, inc, True, 1, False)
    assert rc == 0
    np.testing.assert_array_equal(dn, odn)


def test_refusing_entries(dev, lw_case, sw_case):
    """Every solver entry without a masked instance refuses an armed mask with RRTMGPNN_ERR_ARGUMENT (before it looks
    at its other arguments, so these calls pass none) and clears it."""
    from rrtmgpnn import _lib
    from rrtmgpnn.api import context
    L, ctx = _lib.lib(), context(0).h
    ng = lw_case["ng"]
    bits = _bits_t(_mask_for(ng, 5), dev)
    refusing = ["rrtmgpnn_lw_solver_noscat", "rrtmgpnn_lw_solver_noscat_planck",
                "rrtmgpnn_lw_solver_noscat_planck_clr_all", "rrtmgpnn_lw_solver_1rescl", "rrtmgpnn_lw_solver_2stream",
                "rrtmgpnn_sw_solver_2stream", "rrtmgpnn_sw_solver_noscat", "rrtmgpnn_lw_solver_noscat_gpt",
                "rrtmgpnn_lw_solver_noscat_planck_gpt", "rrtmgpnn_sw_solver_2stream_gpt",
                "rrtmgpnn_lw_solver_1rescl_gpt", "rrtmgpnn_lw_solver_2stream_gpt", "rrtmgpnn_sw_solver_noscat_gpt"]
    for name in refusing:
        _arm(ng, bits)
        argt = _lib.SIGNATURES[name][1]
        args = [ctx, ng, NLAY, NCOL] + [0 if a is _lib.c_int else 0.0 if a is _lib.c_float else None for a in argt[4:]]
        rc = getattr(L, name)(*args)
        assert rc == ERR_ARGUMENT and "takes no cloud mask" in _last_error(), name
        # cleared: the honoured entry runs the plain increment afterwards
    _, oup, odn = _lw_call(lw_case, dev, "rrtmgpnn_lw_solver_noscat_planck_inc", True, 1, False)
    _arm(ng, bits)
    rc = L.rrtmgpnn_lw_solver_noscat(ctx, ng, NLAY, NCOL, 1, 1, None, None, None, None, None, None, None, None, None,
                                     None)
    assert rc == ERR_ARGUMENT
    rc, up, dn = _lw_call(lw_case, dev, "rrtmgpnn_lw_solver_noscat_planck_inc", True, 1, False)
    assert rc == 0
    np.testing.assert_array_equal(dn, odn)


def test_request_semantics_sw(dev, sw_case):
    from rrtmgpnn import api
    c = sw_case
    ng, lims = c["ng"], c["lims"]["pair"]
    bits = _bits_t(_mask_for(ng, 9), dev)
    _, over = _sw_inc(c, dev, lims, True, True)
    _arm(ng, bits)
    rc, got = _sw_inc(c, dev, lims, True, True)
    assert rc == 0 and (got[1] != over[1]).any()
    rc, again = _sw_inc(c, dev, lims, True, True)
    for a, b in zip(again, over):
        np.testing.assert_array_equal(a, b)
    _arm(ng, bits, nlay=NLAY - 1)
    rc, _ = _sw_inc(c, dev, lims, True, True)
    assert rc == ERR_ARGUMENT and "cloud mask" in _last_error()
    # _rfmip without the band increment
    _arm(ng, bits)
    rc, _, _ = _sw_rfmip(c, dev, lims, True, True, nbnd=0)
    assert rc == ERR_ARGUMENT and "cloud mask" in _last_error()
    # the other SW kernels have no masked instance
    for mode in (1, 2):
        api.set_sw_kernel_default(mode)
        try:
            _arm(ng, bits)
            rc, _ = _sw_inc(c, dev, lims, True, True)
            assert rc == ERR_UNSUPPORTED, mode
            rc, plain = _sw_inc(c, dev, lims, True, True)  # cleared: the unmasked call on that kernel
            assert rc == 0
            for a, b in zip(plain, over):
                np.testing.assert_array_equal(a, b)
        finally:
            api.set_sw_kernel_default(0)
    for mode in (0, 3):
        api.set_sw_kernel_default(mode)
        try:
            _arm(ng, bits)
            rc, g2 = _sw_inc(c, dev, lims, True, True)
            assert rc == 0
            for a, b in zip(g2, got):
                np.testing.assert_array_equal(a, b)
        finally:
            api.set_sw_kernel_default(0)


# ---------------------------------------------------------------------------------------------
# ClearSkyStep(mcica=...): 12 RFMIP columns, the all-sky recipe's clouds with a cloud fraction per layer
def _check_step(got, want, use):
    np.testing.assert_array_equal(got["lw_up"], want["lw_up"])
    np.testing.assert_array_equal(got["lw_dn"], want["lw_dn"])
    for k in ("sw_up", "sw_dn", "sw_dir"):
        np.testing.assert_array_equal(got[k][use], want[k][use], err_msg=k)


@pytest.mark.parametrize("overlap_kind", ["max_ran", "exp_ran"])
def test_step_mcica(dev, orc, rfmip, overlap_kind):
    from conftest import subset
    from rrtmgpnn import data
    from rrtmgpnn.pipeline import ClearSkyStep
    ncol = 12
    prob = subset(rfmip, np.arange(ncol) * (rfmip["ncol"] // ncol))
    clouds = data.allsky_clouds(prob, data.load_cloud_optics("lw"))
    cloudy = (clouds[0] > 0) | (clouds[1] > 0)
    assert cloudy.any()
    rng = np.random.default_rng(31)
    nlay = prob["nlay"]
    cf = np.where(cloudy, rng.uniform(0.2, 0.9, cloudy.shape), 0).astype(np.float32)
    ov = rng.uniform(-1, 1, (ncol, nlay - 1)).astype(np.float32) if overlap_kind == "exp_ran" else None
    kl, ks = data.load_kdist("lw"), data.load_kdist("sw")
    draws = [(rng.random((ncol, nlay, kl["ngpt"]), dtype=np.float32), rng.random((ncol, nlay, ks["ngpt"]), dtype=np.float32))
             for _ in range(2)]
    mc = {"cloud_frac": cf, "randoms_lw": draws[0][0], "randoms_sw": draws[0][1], "overlap_param": ov}
    use = prob["usecol"]
    want = [M.step_oracle(orc, prob, clouds, cf, ov, *d) for d in draws]
    assert (want[0]["lw_dn"] != want[1]["lw_dn"]).any()  # refilled randoms change the fluxes
    step = ClearSkyStep(prob, device=0, clouds=clouds, mcica=mc)
    names = [n for n, _, _ in step.calls]
    assert names.index("lw_mask") == names.index("lw_solver") - 1 and names.index("sw_mask") == names.index("sw_solver") - 1
    step.step()
    torch.cuda.synchronize()
    eager = step.fluxes()
    _check_step(eager, want[0], use)
    step.capture()
    for t in (step.lw_up, step.lw_dn, step.sw_up, step.sw_dn, step.sw_dir):
        t.fill_(float("nan"))
    step.replay()
    torch.cuda.synchronize()
    _check_step(step.fluxes(), want[0], use)
    step.set_mcica_randoms(*draws[1])  # refill between replays: same graph, new masks
    step.replay()
    torch.cuda.synchronize()
    _check_step(step.fluxes(), want[1], use)
    step.close()
    unf = ClearSkyStep(prob, device=0, clouds=clouds, mcica=mc, fused=False)
    unf.step()
    torch.cuda.synchronize()
    _check_step(unf.fluxes(), want[0], use)
    unf.close()
    # partially cloudy columns: neither the overcast nor the clear step's fluxes
    over, clr = ClearSkyStep(prob, device=0, clouds=clouds), ClearSkyStep(prob, device=0)
    for s in (over, clr):
        s.step()
    torch.cuda.synchronize()
    fo, fc = over.fluxes(), clr.fluxes()
    cols = cloudy.any(axis=1)
    assert cols.any()
    assert (np.abs(eager["lw_dn"][cols] - fo["lw_dn"][cols]).max(axis=1) > 0).all()
    assert (np.abs(eager["lw_dn"][cols] - fc["lw_dn"][cols]).max(axis=1) > 0).all()
    np.testing.assert_array_equal(eager["lw_dn"][~cols], fc["lw_dn"][~cols])
    over.close(), clr.close()


def test_step_mcica_refusals_and_default_call_list(dev, rfmip):
    from conftest import subset
    from rrtmgpnn import data
    from rrtmgpnn.pipeline import ClearSkyStep
    prob = subset(rfmip, np.arange(4) * 400)
    clouds = data.allsky_clouds(prob, data.load_cloud_optics("lw"))
    nlay = prob["nlay"]
    mc = {"cloud_frac": np.zeros((4, nlay), np.float32), "randoms_lw": np.zeros((4, nlay, 256), np.float32),
          "randoms_sw": np.zeros((4, nlay, 224), np.float32), "overlap_param": None}
    for kw in ({"clrsky": True}, {"byband": True}):
        with pytest.raises(ValueError, match="mcica"):
            ClearSkyStep(prob, device=0, clouds=clouds, mcica=mc, **kw)
    with pytest.raises(ValueError, match="mcica"):
        ClearSkyStep(prob, device=0, mcica=mc)
    with pytest.raises(ValueError, match="cloud_frac"):
        ClearSkyStep(prob, device=0, clouds=clouds, mcica=dict(mc, cloud_frac=np.zeros((4, nlay + 1), np.float32)))
    # without mcica the call list holds none of the new calls
    for fused in (True, False):
        s = ClearSkyStep(prob, device=0, clouds=clouds, fused=fused)
        assert not [n for n, _, _ in s.calls if "mask" in n or "draw_samples" in n]
        with pytest.raises(ValueError):
            s.mcica_randoms()
        s.close()
