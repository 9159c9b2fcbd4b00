"""GPU: clear-sky fluxes beside McICA all-sky fluxes, everything bit for bit.

* rrtmgpnn_lw_solver_noscat_planck_clr_all_mcica -- the masked dual kernel (both of its instances: the wave-uniform mask
  pair in SGPRs for full waves, the per-lane word otherwise) and its two-launch form -- against the _planck entry, the
  armed _planck_inc entry and the composed oracle (the oracle's solve of tau and of tau + the sampled band cloud);
* the entry's refusals: a NULL mask, an armed cloud-mask request, an armed by-band request;
* ClearSkyStep(clouds=..., mcica={..., "clrsky": True}): fused eager, captured, fused=False, the composed oracle, the
  steps that have only one of the two features, and reseeding / refilling between replays;
* rrtmgpnn.clr_all_sky.rte_lw / rte_sw with mask_bits and with the byte mask.
"""
import numpy as np
import pytest

import mcica_ref as M
import philox_ref as P

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
ERR_ARGUMENT = 1
NCOL = 3
# layer counts: levels 2, 4, 5, 10 straddle the dual ring's depth of 4 and its prefetch of 2
NLAYS = (1, 3, 4, 9)
# spectral shapes (band limits, 1-based inclusive; None: the shipped 256-g-point set).  256 and 128: full waves, the
# mask pair of a wave read by a scalar load; 72: three words, a partial second wave, the lane-per-partial flush; 30:
# ngpt % 4 != 0 (plain sums of the radiances, the float4-free flush) with a partly used last word
SPECS = {"g256": None, "g128": [(1, 50), (51, 128)], "g72": [(1, 10), (11, 40), (41, 64), (65, 72)],
         "g30": [(1, 8), (9, 19), (20, 30)]}
FLUX = ("lw_up", "lw_dn", "sw_up", "sw_dn", "sw_dir")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a device"
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


@pytest.fixture
def clr_all_mode():
    """Set the clear + all-sky LW mode of the library for one test, then restore the default."""
    from rrtmgpnn import api
    yield api.set_lw_clr_all_default
    api.set_lw_clr_all_default(0)


def T(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=dev)


def _bits_t(mask, dev):
    return torch.as_tensor(M.pack_bits(mask).view(np.int32), device=dev)


def _expand(bnd, lims, ngpt):
    out = np.zeros(bnd.shape[:-1] + (ngpt,), np.float32)
    for ib, (lo, hi) in enumerate(np.asarray(lims).reshape(-1, 2)):
        out[..., lo - 1:hi] = bnd[..., ib:ib + 1]
    return out


_cases = {}


def lw_case(spec, nlay, dev):
    """Inputs of one (spectral shape, layer count), host and device, built once and never modified: synthetic band
    limits on the first rows of the shipped Planck table, every layer cloudy (the mask decides)."""
    key = (spec, nlay)
    if key in _cases:
        return _cases[key]
    from rrtmgpnn import data
    kl = data.load_kdist("lw")
    lims = np.array(kl["band_lims_gpt"] if SPECS[spec] is None else SPECS[spec], np.int32).reshape(-1, 2)
    nb, ng = len(lims), int(lims[-1, 1])
    kd = {"nband": nb, "ngpt": ng, "band_lims_gpt": lims, "nPlanckTemp": kl["nPlanckTemp"],
          "temp_ref_min": kl["temp_ref_min"], "totplnk_delta": kl["totplnk_delta"],
          "totplnk": np.ascontiguousarray(kl["totplnk"][:nb])}
    rng = np.random.default_rng(1000 * ng + nlay)
    c = {"kd": kd, "ng": ng, "nb": nb, "nlay": nlay, "lims": lims}
    c["tau"] = rng.lognormal(-2, 2, (NCOL, nlay, ng)).astype(np.float32)
    c["pfrac"] = rng.uniform(0, 0.2, (NCOL, nlay, ng)).astype(np.float32)
    c["tb"] = rng.lognormal(0, 1, (NCOL, nlay, nb)).astype(np.float32)
    c["tlay"] = rng.uniform(200, 300, (NCOL, nlay)).astype(np.float32)
    c["tlev"] = rng.uniform(200, 300, (NCOL, nlay + 1)).astype(np.float32)
    c["tsfc"] = rng.uniform(250, 310, NCOL).astype(np.float32)
    c["emis_gpt"] = rng.uniform(0.9, 1, (NCOL, ng)).astype(np.float32)
    c["emis_bnd"] = rng.uniform(0.9, 1, (NCOL, nb)).astype(np.float32)
    # the masks: a McICA sample at cloud fraction 1/2 in every layer (maximum-random overlap; about half the bits),
    # none, all, and one bit per layer, walking over the word and wave boundaries (31, 32, 63, 64, ...)
    r = rng.random((NCOL, nlay, ng), dtype=np.float32)
    one = np.zeros((NCOL, nlay, ng), bool)
    for ic in range(NCOL):
        for il in range(nlay):
            one[ic, il, (31 + 33 * il + ic) % ng] = True
    c["masks"] = {"sampled": M.sampled_mask(r, np.full((NCOL, nlay), 0.5, np.float32)),
                  "zeros": np.zeros((NCOL, nlay, ng), bool), "ones": np.ones((NCOL, nlay, ng), bool), "one_bit": one}
    assert 0.3 < c["masks"]["sampled"].mean() < 0.7
    c["dev"] = {k: T(c[k], dev) for k in ("tau", "pfrac", "tb", "tlay", "tlev", "tsfc", "emis_gpt", "emis_bnd")}
    c["dev"]["totplnk"] = T(kd["totplnk"], dev)
    c["bits"] = {k: _bits_t(m, dev) for k, m in c["masks"].items()}
    _cases[key] = c
    return c


def _solve(c, dev, entry, top_at_1, nmus=1, by_band=False, bits=None, check=True):
    """One of the fused-Planck LW entries on the case's arrays; outputs pre-filled with nan so that an unwritten level
    shows.  'planck' / 'inc' -> (up, dn); 'clr_all' / 'mcica' -> (up, dn, up_clr, dn_clr).  'inc' with bits: armed."""
    from rrtmgpnn import _lib
    from rrtmgpnn._lib import float_array, int_array
    from rrtmgpnn.api import GAUSS_DS, GAUSS_WTS, context
    L, d, kd, nlay = _lib.lib(), c["dev"], c["kd"], c["nlay"]
    ctx = context(0).h
    P_ = lambda t: t.data_ptr()  # noqa: E731
    head = (ctx, c["ng"], nlay, NCOL, int(top_at_1), nmus, float_array(GAUSS_DS[nmus]), float_array(GAUSS_WTS[nmus]),
            None, P_(d["tau"]))
    tail = (c["nb"], kd["nPlanckTemp"], P_(d["tlay"]), P_(d["tlev"]), P_(d["tsfc"]), nlay if top_at_1 else 1,
            int_array(c["lims"].ravel()), float(kd["temp_ref_min"][0]), float(kd["totplnk_delta"]), P_(d["totplnk"]),
            int(by_band), P_(d["emis_bnd"] if by_band else d["emis_gpt"]))
    outs = [torch.full((NCOL, nlay + 1), float("nan"), device=dev) for _ in range(2 if entry in ("planck", "inc") else 4)]
    op = [P_(o) for o in outs]
    if entry == "planck":
        rc = L.rrtmgpnn_lw_solver_noscat_planck(*head, P_(d["pfrac"]), *tail, *op)
    elif entry == "inc":
        if bits is not None:
            _lib.check(L.rrtmgpnn_solver_request_cloud_mask(ctx, c["ng"], nlay, NCOL, P_(bits)))
        rc = L.rrtmgpnn_lw_solver_noscat_planck_inc(*head, P_(d["tb"]), P_(d["pfrac"]), *tail, *op)
    elif entry == "clr_all":
        rc = L.rrtmgpnn_lw_solver_noscat_planck_clr_all(*head, P_(d["tb"]), P_(d["pfrac"]), *tail, *op)
    else:
        rc = L.rrtmgpnn_lw_solver_noscat_planck_clr_all_mcica(*head, P_(d["tb"]), P_(d["pfrac"]), *tail, *op,
                                                              None if bits is None else P_(bits))
    torch.cuda.synchronize()
    if check:
        _lib.check(rc, entry)
        return [o.cpu().numpy() for o in outs]
    return rc, outs


def _same(got, want, what):
    assert len(got) == len(want)
    for g, w, n in zip(got, want, ("up", "dn", "up_clr", "dn_clr")):
        np.testing.assert_array_equal(g, w, err_msg="%s %s" % (what, n))


@pytest.mark.parametrize("by_band", [False, True], ids=["emis_gpt", "emis_bnd"])
@pytest.mark.parametrize("top_at_1", [True, False], ids=["top1", "top0"])
@pytest.mark.parametrize("nlay", NLAYS)
@pytest.mark.parametrize("spec", list(SPECS))
def test_entry_matches_the_two_entries_and_the_oracle(dev, orc, clr_all_mode, spec, nlay, top_at_1, by_band):
    c = lw_case(spec, nlay, dev)
    ng, kd = c["ng"], c["kd"]
    before = c["dev"]["tau"].clone(), c["dev"]["pfrac"].clone()
    kw = dict(top_at_1=top_at_1, by_band=by_band)
    clear = _solve(c, dev, "planck", **kw)
    clear3 = _solve(c, dev, "planck", nmus=3, **kw)
    # the composed oracle: Planck sources, then the solve of tau and of tau + the sampled band cloud
    lay, lev, sfc, _ = orc.planck_source(kd, c["tlay"], c["tlev"], c["tsfc"], c["pfrac"], nlay if top_at_1 else 1)
    emis = _expand(c["emis_bnd"], c["lims"], ng) if by_band else c["emis_gpt"]
    ident = np.stack([np.arange(1, ng + 1)] * 2, axis=1).astype(np.int32)
    want_clear = orc.lw_solver(c["tau"], lay, lev, emis, sfc, top_at_1=top_at_1, nmus=1)
    _same(clear, want_clear, "_planck against the oracle")
    sets = {}
    for kind, mask in c["masks"].items():
        bits = c["bits"][kind]
        armed = _solve(c, dev, "inc", bits=bits, **kw)
        (tau_all,) = orc.increment_bybnd(ident, [c["tau"]], [M.draw(mask, c["tb"], c["lims"])])
        want = list(orc.lw_solver(tau_all, lay, lev, emis, sfc, top_at_1=top_at_1, nmus=1)) + list(want_clear)
        for mode in (1, 2, 0):
            clr_all_mode(mode)
            got = _solve(c, dev, "mcica", bits=bits, **kw)
            _same(got[2:], clear, "%s mode %d: clear set against _planck," % (kind, mode))
            _same(got[:2], armed, "%s mode %d: all-sky set against the armed _planck_inc," % (kind, mode))
            _same(got, want, "%s mode %d: against the oracle," % (kind, mode))
        sets[kind] = got
        # three angles: the two existing launches, whatever the mode
        clr_all_mode(1)
        got3 = _solve(c, dev, "mcica", nmus=3, bits=bits, **kw)
        _same(got3[2:], clear3, "%s nmus 3: clear set" % kind)
        _same(got3[:2], _solve(c, dev, "inc", nmus=3, bits=bits, **kw), "%s nmus 3: all-sky set" % kind)
    # no bit set: the all-sky set is the clear one; every bit set: the unmasked dual entry's four arrays
    _same(sets["zeros"][:2], clear, "all-zero mask")
    _same(sets["ones"], _solve(c, dev, "clr_all", **kw), "all-ones mask against _clr_all")
    # the mask matters, bit by bit
    assert (sets["sampled"][1] != sets["ones"][1]).any() and (sets["sampled"][1] != sets["zeros"][1]).any()
    assert (sets["one_bit"][1] != sets["zeros"][1]).any()
    assert torch.equal(c["dev"]["tau"], before[0]) and torch.equal(c["dev"]["pfrac"], before[1])


@pytest.mark.parametrize("top_at_1", [True, False], ids=["top1", "top0"])
def test_mask_at_an_odd_word_address_takes_the_per_lane_instance(dev, clr_all_mode, top_at_1):
    """256 g-points with the mask 4 bytes off an 8-byte boundary: the scalar pair cannot be read, the per-lane instance
    runs; and the mask's extents are the call's -- the words around it (all set) are never looked at."""
    c = lw_case("g256", 9, dev)
    bits = c["bits"]["sampled"]
    buf = torch.full((bits.numel() + 3,), -1, dtype=torch.int32, device=dev)
    for off in (1, 2):
        view = buf[off:off + bits.numel()]
        view.copy_(bits.reshape(-1))
        assert view.data_ptr() % 8 == (4 if off == 1 else 0)
        clr_all_mode(1)
        got = _solve(c, dev, "mcica", top_at_1=top_at_1, bits=view)
        _same(got[:2], _solve(c, dev, "inc", top_at_1=top_at_1, bits=bits), "offset %d all-sky" % off)
        _same(got[2:], _solve(c, dev, "planck", top_at_1=top_at_1), "offset %d clear" % off)
        buf.fill_(-1)


def _last_error():
    from rrtmgpnn import _lib
    return _lib.lib().rrtmgpnn_last_error().decode()


def test_entry_refusals(dev, clr_all_mode):
    """A NULL mask; an armed cloud-mask request (refused and cleared: the next plain _planck_inc is unmasked); an armed
    by-band request (refused and cleared).  A refused call writes nothing."""
    from rrtmgpnn import _lib
    from rrtmgpnn._lib import int_array
    from rrtmgpnn.api import context
    L, ctx = _lib.lib(), context(0).h
    c = lw_case("g256", 4, dev)
    bits = c["bits"]["sampled"]
    plain = _solve(c, dev, "inc", top_at_1=True)
    rc, outs = _solve(c, dev, "mcica", top_at_1=True, bits=None, check=False)
    assert rc == ERR_ARGUMENT and "mask_bits" in _last_error()
    assert all(torch.isnan(o).all() for o in outs)
    _lib.check(L.rrtmgpnn_solver_request_cloud_mask(ctx, c["ng"], c["nlay"], NCOL, bits.data_ptr()))
    rc, outs = _solve(c, dev, "mcica", top_at_1=True, bits=bits, check=False)
    assert rc == ERR_ARGUMENT and "cloud mask" in _last_error()
    assert all(torch.isnan(o).all() for o in outs)
    _same(_solve(c, dev, "inc", top_at_1=True), plain, "the refused request was still armed:")
    bnd = [torch.full((NCOL, c["nlay"] + 1, c["nb"]), float("nan"), device=dev) for _ in range(2)]
    _lib.check(L.rrtmgpnn_solver_request_byband(ctx, c["nb"], int_array(c["lims"].ravel()), bnd[0].data_ptr(),
                                                bnd[1].data_ptr(), None))
    rc, outs = _solve(c, dev, "mcica", top_at_1=True, bits=bits, check=False)
    assert rc == ERR_ARGUMENT and "by-band" in _last_error()
    assert all(torch.isnan(o).all() for o in outs)
    _same(_solve(c, dev, "inc", top_at_1=True), plain, "after the refused by-band request:")
    assert all(torch.isnan(b).all() for b in bnd), "the refused by-band request was still armed"
    # and the entry itself runs afterwards
    got = _solve(c, dev, "mcica", top_at_1=True, bits=bits)
    _same(got[:2], _solve(c, dev, "inc", top_at_1=True, bits=bits), "after the refusals")


# ---------------------------------------------------------------------------------------------
# ClearSkyStep(clouds=..., mcica={..., "clrsky": True})
SEED_A, SEED_B = 20261019, (3 << 32) | 77
LW_ENTRY = "rrtmgpnn_lw_solver_noscat_planck_clr_all_mcica"


def _problem(rfmip, idx, overlap_kind, route):
    """Problem, clouds and the mcica dict of a route ("array": caller-filled random numbers; "seed"), with the random
    numbers the composed oracle needs (for a seed: the restated Philox draws) for two draws / seeds."""
    from conftest import subset
    from rrtmgpnn import data
    prob = subset(rfmip, idx)
    ncol, nlay = prob["ncol"], prob["nlay"]
    clouds = data.allsky_clouds(prob, data.load_cloud_optics("lw"))
    cloudy = (clouds[0] > 0) | (clouds[1] > 0)
    assert cloudy.any()
    rng = np.random.default_rng(61)
    cf = np.where(cloudy, rng.uniform(0.2, 0.9, cloudy.shape), 0).astype(np.float32)
    ov = rng.uniform(-1, 1, (ncol, nlay - 1)).astype(np.float32) if overlap_kind == "exp_ran" else None
    ng_lw, ng_sw = data.load_kdist("lw")["ngpt"], data.load_kdist("sw")["ngpt"]
    if route == "seed":
        draws = [(P.randoms(s, 0, 0, ng_lw, nlay, ncol), P.randoms(s, 1, 0, ng_sw, nlay, ncol)) for s in (SEED_A, SEED_B)]
        mcs = [{"cloud_frac": cf, "overlap_param": ov, "seed": s} for s in (SEED_A, SEED_B)]
    else:
        draws = [(rng.random((ncol, nlay, ng_lw), dtype=np.float32), rng.random((ncol, nlay, ng_sw), dtype=np.float32))
                 for _ in range(2)]
        mcs = [{"cloud_frac": cf, "overlap_param": ov, "randoms_lw": d[0], "randoms_sw": d[1]} for d in draws]
    return dict(prob=prob, clouds=clouds, cf=cf, ov=ov, draws=draws, mcs=mcs, use=prob["usecol"], route=route)


def _oracle(orc, p, draw):
    """The composed oracle's ten arrays: the McICA all-sky set of mcica_ref.step_oracle and the clear-sky set."""
    from rrtmgpnn import data
    want = dict(M.step_oracle(orc, p["prob"], p["clouds"], p["cf"], p["ov"], *p["draws"][draw]))
    lw = orc.clear_sky_lw(p["prob"], [data.load_model("lw_abs"), data.load_model("lw_pfrac")], data.load_kdist("lw"))
    sw = orc.clear_sky_sw(p["prob"], [data.load_model("sw_abs"), data.load_model("sw_ray")], data.load_kdist("sw"),
                          zero_unused=False)
    want.update(lw_up_clr=lw[0], lw_dn_clr=lw[1], sw_up_clr=sw[0], sw_dn_clr=sw[1], sw_dir_clr=sw[2])
    return want


def _outputs(step):
    torch.cuda.synchronize()
    out = dict(step.fluxes())
    if step.clrsky:
        out.update(step.clrsky_fluxes())
    return out


def _poison(step):
    for k in FLUX:
        getattr(step, k).fill_(float("nan"))
        if step.clrsky:
            getattr(step, k + "_clr").fill_(float("nan"))


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


ALL = FLUX
CLR = tuple(k + "_clr" for k in FLUX)


def _check_step(orc, p):
    from rrtmgpnn import _lib
    from rrtmgpnn.pipeline import ClearSkyStep
    prob, clouds, use = p["prob"], p["clouds"], p["use"]
    mc = dict(p["mcs"][0], clrsky=True)
    step = ClearSkyStep(prob, device=0, clouds=clouds, mcica=mc)
    names = [n for n, _, _ in step.calls]
    fns = {n: f for n, f, _ in step.calls}
    # LW: the mask call, then the new entry in place of _planck_inc, no request; SW: mask, request, the masked solve,
    # the clear solve
    assert "lw_mask" not in names and names.index("mcica_mask_lw") < names.index("lw_solver")
    assert fns["lw_solver"] is getattr(_lib.lib(), LW_ENTRY)
    assert names.index("sw_mask") == names.index("sw_solver") - 1
    assert names.index("mcica_mask_sw") < names.index("sw_mask") and names.index("sw_solver") < names.index("sw_solver_clr")
    eager = _run(step)
    assert set(eager) == set(ALL + CLR)
    want = _oracle(orc, p, 0)
    _equal(eager, want, "fused eager against the oracle:", use)
    step.capture()
    _poison(step)
    step.replay()
    _equal(_outputs(step), eager, "captured against eager:")
    # between replays: new random numbers change the all-sky set and leave the clear one as it is, bit for bit
    if p["route"] == "seed":
        step.set_mcica_seed(seed=SEED_B)
    else:
        step.set_mcica_randoms(*p["draws"][1])
    _poison(step)
    step.replay()
    again = _outputs(step)
    step.close()
    fresh = ClearSkyStep(prob, device=0, clouds=clouds, mcica=dict(p["mcs"][1], clrsky=True))
    _equal(again, _run(fresh), "replay after new random numbers against a fresh step:")
    fresh.close()
    _equal(again, eager, "the clear set after new random numbers:", keys=CLR)
    assert (again["lw_dn"] != eager["lw_dn"]).any() and (again["sw_dn"] != eager["sw_dn"]).any()
    unf = ClearSkyStep(prob, device=0, clouds=clouds, mcica=mc, fused=False)
    un = [n for n, _, _ in unf.calls]
    assert un.index("lw_solver_clr") < un.index("mcica_mask_lw") < un.index("draw_samples_lw") \
        < un.index("increment_lw") < un.index("lw_solver")
    assert un.index("sw_solver_clr") < un.index("mcica_mask_sw") < un.index("draw_samples_sw") \
        < un.index("increment_sw") < un.index("sw_solver")
    got = _run(unf)
    unf.close()
    _equal(got, want, "fused=False against the oracle:", use)
    _equal(got, eager, "fused=False against fused:")
    # each feature alone: the all-sky set of the McICA step without the key, the clear set of a clrsky step
    plain = ClearSkyStep(prob, device=0, clouds=clouds, mcica=p["mcs"][0])
    assert not plain.clrsky
    pn = [n for n, _, _ in plain.calls]
    assert not [n for n in pn if n.endswith("_clr")] and "lw_mask" in pn
    assert all(f is not getattr(_lib.lib(), LW_ENTRY) for _, f, _ in plain.calls)
    _equal(eager, _run(plain), "against the step without the key:", keys=ALL)
    plain.close()
    clr = ClearSkyStep(prob, device=0, clouds=clouds, clrsky=True)
    _equal(eager, _run(clr), "against the clrsky step without mcica:", keys=CLR)
    clr.close()
    # cloud radiative effect is there to be had: the sets differ in the cloudy columns, and only there
    cols = (p["cf"] > 0).any(axis=1)
    assert ((eager["lw_dn"] != eager["lw_dn_clr"]).any(axis=1) == cols).all()


@pytest.mark.parametrize("route", ["array", "seed"])
@pytest.mark.parametrize("overlap_kind", ["max_ran", "exp_ran"])
def test_step_4_columns(dev, orc, rfmip, overlap_kind, route):
    _check_step(orc, _problem(rfmip, np.arange(4) * 400, overlap_kind, route))


def test_step_36_columns(dev, orc, rfmip):
    """More columns than one SW block pair and a ragged split over the mask kernels' blocks."""
    _check_step(orc, _problem(rfmip, np.arange(0, 1800, 50), "exp_ran", "seed"))


def test_step_refusals(dev, rfmip):
    from rrtmgpnn.pipeline import ClearSkyStep
    p = _problem(rfmip, np.arange(4) * 400, "max_ran", "array")
    with pytest.raises(ValueError, match="mcica"):  # the top-level flag keeps raising; the message names the key
        ClearSkyStep(p["prob"], device=0, clouds=p["clouds"], mcica=p["mcs"][0], clrsky=True)
    with pytest.raises(ValueError, match="'clrsky': True"):
        ClearSkyStep(p["prob"], device=0, clouds=p["clouds"], mcica=p["mcs"][0], clrsky=True)
    with pytest.raises(ValueError, match="byband"):
        ClearSkyStep(p["prob"], device=0, clouds=p["clouds"], mcica=dict(p["mcs"][0], clrsky=True), byband=True)
    s = ClearSkyStep(p["prob"], device=0, clouds=p["clouds"], mcica=dict(p["mcs"][0], clrsky=False))
    assert not s.clrsky
    with pytest.raises(ValueError):
        s.clrsky_fluxes()
    s.close()


# ---------------------------------------------------------------------------------------------
# The class layer: clr_all_sky.rte_lw / rte_sw with a mask, on the 4 columns
def _class_setup(dev, which, prob):
    from rrtmgpnn import api, data
    kd = api.GasOpticsRRTMGP()
    api.stop_on_err(kd.load(which))
    names = ("lw_abs", "lw_pfrac") if which == "lw" else ("sw_abs", "sw_ray")
    nets = [api.RrtmgpNetwork(0).load_netcdf(data.path(n)) for n in names]
    gc = api.GasConcs()
    api.stop_on_err(gc.init(list(prob["gases"])))
    for k, v in prob["gases"].items():
        api.stop_on_err(gc.set_vmr(k, T(v, dev)))
    return kd, nets, gc, [T(prob[k], dev) for k in ("play", "tlay", "plev")]


def _cloud_props(api, kd, arrays, dev):
    ncol, nlay, _ = arrays[0].shape
    p = api.OpticalProps1scl() if len(arrays) == 1 else api.OpticalProps2str()
    assert p.init(kd.get_band_lims_wavenumber()) == ""
    assert (p.alloc_1scl if len(arrays) == 1 else p.alloc_2str)(ncol, nlay, device=dev) == ""
    for t, a in zip([p.tau] if len(arrays) == 1 else [p.tau, p.ssa, p.g], arrays):
        t.copy_(T(a, dev))
    return p


def _bb(api, dev, ncol, nlev, beam=False):
    nan = lambda: torch.full((ncol, nlev), float("nan"), device=dev)  # noqa: E731
    return api.FluxesBroadband(flux_up=nan(), flux_dn=nan(), flux_dn_dir=nan() if beam else None)


@pytest.fixture(scope="module")
def class_case(dev, orc, rfmip):
    """The 4-column problem, the step's ten arrays (array route, maximum-random overlap) and the oracle's."""
    from rrtmgpnn.pipeline import ClearSkyStep
    p = _problem(rfmip, np.arange(4) * 400, "max_ran", "array")
    step = ClearSkyStep(p["prob"], device=0, clouds=p["clouds"], mcica=dict(p["mcs"][0], clrsky=True))
    p["step"] = _run(step)
    step.close()
    p["want"] = _oracle(orc, p, 0)
    p["mask_lw"] = M.sampled_mask(p["draws"][0][0], p["cf"], p["ov"])
    p["mask_sw"] = M.sampled_mask(p["draws"][0][1], p["cf"], p["ov"])
    return p


@pytest.mark.parametrize("route", ["mask_bits", "cloud_mask"])
def test_class_rte_lw(dev, orc, class_case, route):
    from rrtmgpnn import api, clr_all_sky, data
    p = class_case
    prob = p["prob"]
    ncol, nlay = prob["ncol"], prob["nlay"]
    kd, nets, gc, (play, tlay, plev) = _class_setup(dev, "lw", prob)
    (ct,) = orc.cloud_optics(data.load_cloud_optics("lw"), *p["clouds"], nstr=1, lut=True, icergh=2)
    clouds = _cloud_props(api, kd, (ct,), dev)
    emis = T(np.repeat(np.asarray(prob["sfc_emis"], np.float32)[:, None], kd.get_nband(), axis=1), dev)
    kw = {"mask_bits": _bits_t(p["mask_lw"], dev)} if route == "mask_bits" else \
        {"cloud_mask": torch.as_tensor(p["mask_lw"].astype(np.uint8), device=dev)}
    f_all, f_clr = _bb(api, dev, ncol, nlay + 1), _bb(api, dev, ncol, nlay + 1)
    assert clr_all_sky.rte_lw(kd, gc, play, tlay, plev, T(prob["tsfc"], dev), emis, clouds, f_all, f_clr,
                              t_lev=T(prob["tlev"], dev), neural_nets=nets, **kw) == ""
    torch.cuda.synchronize()
    got = {"lw_up": f_all.flux_up, "lw_dn": f_all.flux_dn, "lw_up_clr": f_clr.flux_up, "lw_dn_clr": f_clr.flux_dn}
    got = {k: v.cpu().numpy() for k, v in got.items()}
    _equal(got, p["step"], route + " against the step:", keys=list(got))
    _equal(got, p["want"], route + " against the oracle:", keys=list(got))
    if route == "mask_bits":
        bad = torch.zeros((ncol, nlay, 7), dtype=torch.int32, device=dev)
        assert clr_all_sky.rte_lw(kd, gc, play, tlay, plev, T(prob["tsfc"], dev), emis, clouds, f_all, f_clr,
                                  neural_nets=nets, mask_bits=bad) == \
            "rte_lw: mask_bits is not (ncol, nlay, ceil(ngpt/32)) 32-bit words"
        # a flux object that wants flux_net cannot take the fused entry, and the sampled sequence needs the byte mask
        e = clr_all_sky.rte_lw(kd, gc, play, tlay, plev, T(prob["tsfc"], dev), emis, clouds, f_all,
                               api.FluxesBroadband(flux_up=f_clr.flux_up, flux_dn=f_clr.flux_dn,
                                                   flux_net=torch.empty_like(f_clr.flux_up)),
                               neural_nets=nets, **kw)
        assert e.startswith("rte_lw: this case runs the sampled sequence")


@pytest.mark.parametrize("route", ["mask_bits", "cloud_mask"])
def test_class_rte_sw(dev, orc, class_case, route):
    from rrtmgpnn import api, clr_all_sky, data
    p = class_case
    prob, use = p["prob"], p["use"]
    ncol, nlay = prob["ncol"], prob["nlay"]
    kd, nets, gc, (play, tlay, plev) = _class_setup(dev, "sw", prob)
    cld = orc.delta_scale(*orc.cloud_optics(data.load_cloud_optics("sw"), *p["clouds"], nstr=2, lut=True, icergh=2))
    clouds = _cloud_props(api, kd, cld, dev)
    alb = T(np.repeat(np.asarray(prob["sfc_alb"], np.float32)[:, None], kd.get_nband(), axis=1), dev)
    kw = {"mask_bits": _bits_t(p["mask_sw"], dev)} if route == "mask_bits" else \
        {"cloud_mask": torch.as_tensor(p["mask_sw"].astype(np.uint8), device=dev)}
    f_all, f_clr = _bb(api, dev, ncol, nlay + 1, True), _bb(api, dev, ncol, nlay + 1, True)
    assert clr_all_sky.rte_sw(kd, gc, play, tlay, plev, T(prob["mu0"], dev), alb, alb, clouds, f_all, f_clr,
                              inc_flux=T(data.toa_flux(prob, data.load_kdist("sw")), dev), neural_nets=nets,
                              **kw) == ""
    torch.cuda.synchronize()
    got = {"sw_up": f_all.flux_up, "sw_dn": f_all.flux_dn, "sw_dir": f_all.flux_dn_dir, "sw_up_clr": f_clr.flux_up,
           "sw_dn_clr": f_clr.flux_dn, "sw_dir_clr": f_clr.flux_dn_dir}
    got = {k: v.cpu().numpy() for k, v in got.items()}
    _equal(got, p["step"], route + " against the step:", use, keys=list(got))
    _equal(got, p["want"], route + " against the oracle:", use, keys=list(got))
    if route == "mask_bits":
        bad = torch.zeros((ncol, nlay + 1, 7), dtype=torch.int32, device=dev)
        assert clr_all_sky.rte_sw(kd, gc, play, tlay, plev, T(prob["mu0"], dev), alb, alb, clouds, f_all, f_clr,
                                  neural_nets=nets, mask_bits=bad) == \
            "rte_sw: mask_bits is not (ncol, nlay, ceil(ngpt/32)) 32-bit words"
