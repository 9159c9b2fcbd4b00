"""GPU: by-band fluxes under a McICA-sampled cloud from the fused solvers (rrtmgpnn_solver_request_byband_mcica),
every comparison bit for bit.

* the LW entry (_planck_inc, one and three angles) and the SW entries (_inc and _rfmip) with the paired request, against
  the composed oracle (restated mask -> merge -> same-resolution increment -> solver with g-point outputs ->
  tests/byband_ref.py's sequential band sums) and against this library's unfused route (draw_samples -> increment -> the
  plain solver with rrtmgpnn_solver_request_byband);
* the broadband outputs equal the masked call's; all ones == the unmasked _inc call, all zeros (LW) == _planck;
* poisoned outputs with guard floats behind them; band layouts that differ from the cloud bands, with odd starts and with
  g-points outside every band;
* the request's semantics, and ClearSkyStep(mcica={..., "byband": True}).

Shapes and inputs: tests/mcica_byband_cases.py; that its masks matter is established in tests/test_mcica_byband_host.py."""
import numpy as np
import pytest

import byband_ref as R
import mcica_byband_cases as C
import mcica_ref as M
from mcica_byband_cases import NCOL, NLAY

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
ERR_ARGUMENT, ERR_UNSUPPORTED = 1, 4
NAN = float("nan")
GUARD, NGUARD = 12345.0, 16


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a device"
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def T(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=dev)


def P(t):
    return t.data_ptr() if t is not None else None


def _bits_t(mask, dev):
    return torch.as_tensor(M.pack_bits(mask).view(np.int32), device=dev)


class Guarded:
    """A by-band output (NCOL, NLAY + 1, nb), pre-filled with NaN, with guard floats right behind it."""

    def __init__(self, dev, nb):
        n = NCOL * (NLAY + 1) * nb
        self.whole = torch.full((n + NGUARD,), GUARD, device=dev)
        self.t = self.whole[:n].view(NCOL, NLAY + 1, nb)
        self.t.fill_(NAN)

    def get(self):
        """The array, every element written; the guards intact."""
        a = self.t.cpu().numpy()
        assert not np.isnan(a).any(), "a by-band element inside a requested band was not written"
        assert (self.whole[-NGUARD:].cpu().numpy() == np.float32(GUARD)).all(), "written past the by-band array"
        return a


def _ctx():
    from rrtmgpnn.api import context
    return context(0).h


def _arm_pair(lims, up, dn, dr, ngpt, bits, nlay=NLAY, ncol=NCOL):
    from rrtmgpnn import _lib
    from rrtmgpnn._lib import int_array
    lims = np.asarray(lims).reshape(-1, 2)
    return _lib.lib().rrtmgpnn_solver_request_byband_mcica(_ctx(), len(lims), int_array(lims.ravel()), P(up), P(dn), P(dr),
                                                           ngpt, nlay, ncol, P(bits))


def _arm_mask(ngpt, bits, nlay=NLAY, ncol=NCOL):
    from rrtmgpnn import _lib
    _lib.check(_lib.lib().rrtmgpnn_solver_request_cloud_mask(_ctx(), ngpt, nlay, ncol, P(bits)))


def _arm_byband(lims, up, dn, dr):
    from rrtmgpnn import _lib
    from rrtmgpnn._lib import int_array
    lims = np.asarray(lims).reshape(-1, 2)
    _lib.check(_lib.lib().rrtmgpnn_solver_request_byband(_ctx(), len(lims), int_array(lims.ravel()), P(up), P(dn), P(dr)))


def _last_error():
    from rrtmgpnn import _lib
    return _lib.lib().rrtmgpnn_last_error().decode()


# ---- LW ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lw_case(dev):
    """LW inputs shared by the LW tests (never modified)."""
    c = C.lw_inputs()
    c["dev"] = {k: T(c[k], dev) for k in ("tau", "pfrac", "tb", "tlay", "tlev", "tsfc", "emis_bnd")}
    c["dev"]["totplnk"] = T(c["kd"]["totplnk"], dev)
    return c


def _lw_call(c, dev, entry, top_at_1, nmus, tau=None, with_tb=True):
    """One of the fused-Planck LW entries on the shared inputs (emissivity by band) -> rc, up, dn (numpy)."""
    from rrtmgpnn import _lib
    from rrtmgpnn._lib import float_array, int_array
    from rrtmgpnn.api import GAUSS_DS, GAUSS_WTS
    L, d, kl = _lib.lib(), c["dev"], c["kd"]
    up, dn = (torch.full((NCOL, NLAY + 1), NAN, device=dev) for _ in range(2))
    common = (c["nb"], kl["nPlanckTemp"], P(d["tlay"]), P(d["tlev"]), P(d["tsfc"]), NLAY if top_at_1 else 1,
              int_array(kl["band_lims_gpt"].ravel()), float(kl["temp_ref_min"][0]), float(kl["totplnk_delta"]),
              P(d["totplnk"]), 1, P(d["emis_bnd"]))
    t = d["tau"] if tau is None else tau
    head = (_ctx(), c["ng"], NLAY, NCOL, int(top_at_1), nmus, float_array(GAUSS_DS[nmus]), float_array(GAUSS_WTS[nmus]),
            None, P(t))
    mid = (P(d["tb"]),) if with_tb else ()
    rc = getattr(L, entry)(*head, *mid, P(d["pfrac"]), *common, P(up), P(dn))
    torch.cuda.synchronize()
    return rc, up.cpu().numpy(), dn.cpu().numpy()


INC, PLANCK = "rrtmgpnn_lw_solver_noscat_planck_inc", "rrtmgpnn_lw_solver_noscat_planck"


def _lw_paired(c, dev, lims, bits, top_at_1, nmus):
    bu, bd = Guarded(dev, len(lims)), Guarded(dev, len(lims))
    assert _arm_pair(lims, bu.t, bd.t, None, c["ng"], bits) == 0, _last_error()
    rc, up, dn = _lw_call(c, dev, INC, top_at_1, nmus)
    assert rc == 0, _last_error()
    return up, dn, bu.get(), bd.get()


def _lw_byband(c, dev, lims, entry, top_at_1, nmus, **kw):
    """The separate by-band request ahead of an unmasked entry."""
    bu, bd = Guarded(dev, len(lims)), Guarded(dev, len(lims))
    _arm_byband(lims, bu.t, bd.t, None)
    rc, up, dn = _lw_call(c, dev, entry, top_at_1, nmus, **kw)
    assert rc == 0, _last_error()
    return up, dn, bu.get(), bd.get()


@pytest.mark.parametrize("top_at_1", [True, False])
@pytest.mark.parametrize("nmus", [1, 3])
def test_fused_lw_mask_byband(dev, orc, lw_case, nmus, top_at_1):
    from rrtmgpnn import _lib
    from rrtmgpnn._lib import int_array
    c, L, ctx = lw_case, _lib.lib(), _ctx()
    ng, nb, kl = c["ng"], c["nb"], c["kd"]
    mask = C.mask_for(ng, C.LW_MASK_SEED)
    bits = _bits_t(mask, dev)
    ones_bits, zero_bits = _bits_t(C.mask_for(ng, 0, "ones"), dev), _bits_t(C.mask_for(ng, 0, "zeros"), dev)
    tau0 = c["dev"]["tau"].clone()
    wup, wdn, gu, gd = C.lw_expect(orc, c, mask, top_at_1, nmus)  # (1) the composed oracle, once for the layouts
    # the masked call without by-band outputs
    _arm_mask(ng, bits)
    rc, mup, mdn = _lw_call(c, dev, INC, top_at_1, nmus)
    assert rc == 0
    np.testing.assert_array_equal(mup, wup)
    np.testing.assert_array_equal(mdn, wdn)
    # (2) this library's unfused route: draw_samples -> increment -> the plain fused-Planck solver with the request
    samp = torch.empty((NCOL, NLAY, ng), device=dev)
    mb = torch.as_tensor(mask.astype(np.uint8), device=dev)
    _lib.check(L.rrtmgpnn_draw_samples(ctx, ng, NLAY, NCOL, nb, int_array(kl["band_lims_gpt"].ravel()), P(mb),
                                       P(c["dev"]["tb"]), None, None, P(samp), None, None))
    tau2 = c["dev"]["tau"].clone()
    _lib.check(L.rrtmgpnn_increment(ctx, NCOL, NLAY, ng, P(tau2), None, None, P(samp), None, None))
    differs = False
    for name, lims in C.byband_layouts(kl).items():
        up, dn, bu, bd = _lw_paired(c, dev, lims, bits, top_at_1, nmus)
        assert torch.equal(tau0, c["dev"]["tau"]), "tau was modified"
        np.testing.assert_array_equal(bu, R.sum_byband(gu, lims), err_msg=name + " bnd_up")
        np.testing.assert_array_equal(bd, R.sum_byband(gd, lims), err_msg=name + " bnd_dn")
        np.testing.assert_array_equal(up, mup, err_msg=name + " up: the broadband flux moved")
        np.testing.assert_array_equal(dn, mdn, err_msg=name + " dn: the broadband flux moved")
        up2, dn2, bu2, bd2 = _lw_byband(c, dev, lims, PLANCK, top_at_1, nmus, tau=tau2, with_tb=False)
        for a, b, what in ((up, up2, "up"), (dn, dn2, "dn"), (bu, bu2, "bnd_up"), (bd, bd2, "bnd_dn")):
            np.testing.assert_array_equal(a, b, err_msg="%s %s against the unfused route" % (name, what))
        # all ones == the unmasked _inc call with the by-band request; all zeros == _planck with it
        one = _lw_paired(c, dev, lims, ones_bits, top_at_1, nmus)
        for a, b in zip(one, _lw_byband(c, dev, lims, INC, top_at_1, nmus)):
            np.testing.assert_array_equal(a, b, err_msg=name + " all ones")
        zero = _lw_paired(c, dev, lims, zero_bits, top_at_1, nmus)
        for a, b in zip(zero, _lw_byband(c, dev, lims, PLANCK, top_at_1, nmus, with_tb=False)):
            np.testing.assert_array_equal(a, b, err_msg=name + " all zeros")
        # the mask matters: a band whose down flux is neither the overcast nor the clear one
        differs |= bool(((bd != one[3]).reshape(-1, len(lims)).any(axis=0)
                         & (bd != zero[3]).reshape(-1, len(lims)).any(axis=0)).any())
    assert differs


# ---- SW ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sw_case(dev):
    c = C.sw_inputs()
    c["dev"] = {k: T(c[k], dev) for k in ("tau", "ssa", "g", "bt", "bw", "bg", "mu0", "inc", "alb", "solar", "tsi",
                                         "sfc_alb", "sza")}
    return c


def _sw_inc(c, dev, lims, with_g, top_at_1, tau=None, ssa=None, g=None, plain=False):
    """rrtmgpnn_sw_solver_2stream_inc (or, plain, rrtmgpnn_sw_solver_2stream on the given arrays) -> rc, 3 fluxes."""
    from rrtmgpnn import _lib
    from rrtmgpnn._lib import int_array
    L, d = _lib.lib(), c["dev"]
    outs = [torch.full((NCOL, NLAY + 1), NAN, device=dev) for _ in range(3)]
    t, w = (d["tau"] if tau is None else tau), (d["ssa"] if ssa is None else ssa)
    gg = g if g is not None else (d["g"] if with_g else None)
    head = (_ctx(), c["ng"], NLAY, NCOL, int(top_at_1), P(d["inc"]), None, P(t), P(w), P(gg))
    tail = (P(d["mu0"]), P(d["alb"]), P(d["alb"]), *[P(o) for o in outs])
    if plain:
        rc = L.rrtmgpnn_sw_solver_2stream(*head, *tail)
    else:
        rc = L.rrtmgpnn_sw_solver_2stream_inc(*head, c["nb"], int_array(lims.ravel()), P(d["bt"]), P(d["bw"]),
                                              P(d["bg"]), *tail)
    torch.cuda.synchronize()
    return rc, [o.cpu().numpy() for o in outs]


def _sw_rfmip(c, dev, lims, with_g, top_at_1, nbnd=None, tau=None, ssa=None, g=None):
    """rrtmgpnn_sw_solver_2stream_rfmip on the shared inputs, or on the given (already incremented) arrays -> rc, the 3
    fluxes, the boundary conditions it stored."""
    from rrtmgpnn import _lib
    from rrtmgpnn._lib import int_array
    L, d = _lib.lib(), c["dev"]
    outs = [torch.full((NCOL, NLAY + 1), NAN, device=dev) for _ in range(3)]
    scr = [torch.empty((NCOL, c["ng"]), device=dev), torch.empty((NCOL, c["ng"]), device=dev),
           torch.empty(NCOL, device=dev)]
    nb = c["nb"] if nbnd is None else nbnd
    rc = L.rrtmgpnn_sw_solver_2stream_rfmip(
        _ctx(), c["ng"], NLAY, NCOL, int(top_at_1), P(d["solar"]), P(d["tsi"]), P(d["sfc_alb"]), P(d["sza"]),
        P(d["tau"] if tau is None else tau), P(d["ssa"] if ssa is None else ssa),
        P(g) if g is not None else (P(d["g"]) if with_g else None), nb, int_array(lims.ravel()), P(d["bt"]), P(d["bw"]),
        P(d["bg"]), *[P(s) for s in scr], *[P(o) for o in outs])
    torch.cuda.synchronize()
    return rc, [o.cpu().numpy() for o in outs], [s.cpu().numpy() for s in scr]


def _with_bnd(dev, lims, arm, call):
    """arm(bnd tensors), call() -> the call's 3 broadband fluxes + the 3 by-band arrays (checked for poison, guards)."""
    bnd = [Guarded(dev, len(lims)) for _ in range(3)]
    arm(*[b.t for b in bnd])
    out = call()
    assert out[0] == 0, _last_error()
    return list(out[1]) + [b.get() for b in bnd]


NAMES = ("up", "dn", "dir", "bnd_up", "bnd_dn", "bnd_dir")


@pytest.mark.parametrize("layout", ["pair", "general"])
@pytest.mark.parametrize("with_g", [True, False], ids=["g", "nog"])
@pytest.mark.parametrize("top_at_1", [True, False])
def test_fused_sw_mask_byband_inc(dev, orc, sw_case, top_at_1, with_g, layout):
    from rrtmgpnn import _lib
    from rrtmgpnn._lib import int_array
    c, L, ctx = sw_case, _lib.lib(), _ctx()
    ng, nb, cl = c["ng"], c["nb"], c["lims"][layout]
    mask = C.mask_for(ng, C.SW_MASK_SEED)
    bits, ones_bits = _bits_t(mask, dev), _bits_t(C.mask_for(ng, 0, "ones"), dev)
    zero_bits = _bits_t(C.mask_for(ng, 0, "zeros"), dev)
    saved = [c["dev"][k].clone() for k in ("tau", "ssa", "g")]
    want_bb, want_gpt = C.sw_expect(orc, c, mask, cl, with_g, top_at_1)  # (1) the composed oracle
    _arm_mask(ng, bits)
    rc, masked = _sw_inc(c, dev, cl, with_g, top_at_1)  # the masked call without by-band outputs
    assert rc == 0
    for a, b, n in zip(masked, want_bb, NAMES):
        np.testing.assert_array_equal(a, b, err_msg=n)
    # (2) this library's unfused route
    d = c["dev"]
    samp = [torch.empty((NCOL, NLAY, ng), device=dev) for _ in range(3)]
    mb = torch.as_tensor(mask.astype(np.uint8), device=dev)
    _lib.check(L.rrtmgpnn_draw_samples(ctx, ng, NLAY, NCOL, nb, int_array(cl.ravel()), P(mb), P(d["bt"]), P(d["bw"]),
                                       P(d["bg"]), *[P(s) for s in samp]))
    t2, w2 = d["tau"].clone(), d["ssa"].clone()
    g2 = d["g"].clone() if with_g else torch.zeros_like(d["g"])
    _lib.check(L.rrtmgpnn_increment(ctx, NCOL, NLAY, ng, P(t2), P(w2), P(g2), *[P(s) for s in samp]))
    differs = False
    for name, lims in C.byband_layouts(c["kd"]).items():
        got = _with_bnd(dev, lims, lambda *b: _arm_pair(lims, *b, ng, bits) == 0 or pytest.fail(_last_error()),
                        lambda: _sw_inc(c, dev, cl, with_g, top_at_1))
        assert all(torch.equal(a, c["dev"][k]) for a, k in zip(saved, ("tau", "ssa", "g")))
        for a, y, n in zip(got[3:], want_gpt, NAMES[3:]):
            np.testing.assert_array_equal(a, R.sum_byband(y, lims), err_msg="%s %s" % (name, n))
        for a, b, n in zip(got[:3], masked, NAMES):
            np.testing.assert_array_equal(a, b, err_msg="%s %s: the broadband flux moved" % (name, n))
        unf = _with_bnd(dev, lims, lambda *b: _arm_byband(lims, *b),
                        lambda: _sw_inc(c, dev, cl, True, top_at_1, tau=t2, ssa=w2, g=g2, plain=True))
        for a, b, n in zip(got, unf, NAMES):
            np.testing.assert_array_equal(a, b, err_msg="%s %s against the unfused route" % (name, n))
        # all ones == the unmasked _inc call with the by-band request
        one = _with_bnd(dev, lims, lambda *b: _arm_pair(lims, *b, ng, ones_bits) == 0 or pytest.fail(_last_error()),
                        lambda: _sw_inc(c, dev, cl, with_g, top_at_1))
        over = _with_bnd(dev, lims, lambda *b: _arm_byband(lims, *b), lambda: _sw_inc(c, dev, cl, with_g, top_at_1))
        for a, b, n in zip(one, over, NAMES):
            np.testing.assert_array_equal(a, b, err_msg="%s %s all ones" % (name, n))
        zero = _with_bnd(dev, lims, lambda *b: _arm_pair(lims, *b, ng, zero_bits) == 0 or pytest.fail(_last_error()),
                         lambda: _sw_inc(c, dev, cl, with_g, top_at_1))
        differs |= bool(((got[4] != one[4]).reshape(-1, len(lims)).any(axis=0)
                         & (got[4] != zero[4]).reshape(-1, len(lims)).any(axis=0)).any())
    assert differs


@pytest.mark.parametrize("layout", ["pair", "general"])
@pytest.mark.parametrize("with_g", [True, False], ids=["g", "nog"])
def test_fused_sw_mask_byband_rfmip(dev, orc, sw_case, with_g, layout):
    """The _rfmip entry with nbnd > 0: the boundary conditions it forms (read back from an unmasked run on the
    workspace-plane kernel, which stores them) feed the composed oracle; the unfused route is draw_samples -> increment
    on copies -> the same entry with nbnd = 0 and rrtmgpnn_solver_request_byband."""
    from rrtmgpnn import _lib, api
    from rrtmgpnn._lib import int_array
    c, L, ctx, d = sw_case, _lib.lib(), _ctx(), sw_case["dev"]
    ng, cl = c["ng"], c["lims"][layout]
    mask = C.mask_for(ng, C.RFMIP_MASK_SEED)
    api.set_sw_kernel_default(2)
    try:
        rc, _, (toa, alb, mu0) = _sw_rfmip(c, dev, cl, with_g, True)
    finally:
        api.set_sw_kernel_default(0)
    assert rc == 0
    bits, ones_bits = _bits_t(mask, dev), _bits_t(C.mask_for(ng, 0, "ones"), dev)
    zero_bits = _bits_t(C.mask_for(ng, 0, "zeros"), dev)
    # (2) this library's unfused route: the sampled cloud arrays added to copies of the gas arrays
    samp = [torch.empty((NCOL, NLAY, ng), device=dev) for _ in range(3)]
    mb = torch.as_tensor(mask.astype(np.uint8), device=dev)
    _lib.check(L.rrtmgpnn_draw_samples(ctx, ng, NLAY, NCOL, c["nb"], int_array(cl.ravel()), P(mb), P(d["bt"]), P(d["bw"]),
                                       P(d["bg"]), *[P(s) for s in samp]))
    t2, w2 = d["tau"].clone(), d["ssa"].clone()
    g2 = d["g"].clone() if with_g else torch.zeros_like(d["g"])
    _lib.check(L.rrtmgpnn_increment(ctx, NCOL, NLAY, ng, P(t2), P(w2), P(g2), *[P(s) for s in samp]))
    for top_at_1 in (True, False):
        want_bb, want_gpt = C.sw_expect(orc, c, mask, cl, with_g, top_at_1, bc=(mu0, toa, alb))
        _arm_mask(ng, bits)
        rc, masked, _ = _sw_rfmip(c, dev, cl, with_g, top_at_1)
        assert rc == 0
        for name, lims in C.byband_layouts(c["kd"]).items():
            got = _with_bnd(dev, lims, lambda *b: _arm_pair(lims, *b, ng, bits) == 0 or pytest.fail(_last_error()),
                            lambda: _sw_rfmip(c, dev, cl, with_g, top_at_1)[:2])
            for a, y, n in zip(got[3:], want_gpt, NAMES[3:]):
                np.testing.assert_array_equal(a, R.sum_byband(y, lims), err_msg="%s %s" % (name, n))
            for a, b, w, n in zip(got[:3], masked, want_bb, NAMES):
                np.testing.assert_array_equal(a, b, err_msg="%s %s: the broadband flux moved" % (name, n))
                np.testing.assert_array_equal(a, w, err_msg="%s %s" % (name, n))
            unf = _with_bnd(dev, lims, lambda *b: _arm_byband(lims, *b),
                            lambda: _sw_rfmip(c, dev, cl, True, top_at_1, nbnd=0, tau=t2, ssa=w2, g=g2)[:2])
            for a, b, n in zip(got, unf, NAMES):
                np.testing.assert_array_equal(a, b, err_msg="%s %s against the unfused route" % (name, n))
            one = _with_bnd(dev, lims, lambda *b: _arm_pair(lims, *b, ng, ones_bits) == 0 or pytest.fail(_last_error()),
                            lambda: _sw_rfmip(c, dev, cl, with_g, top_at_1)[:2])
            over = _with_bnd(dev, lims, lambda *b: _arm_byband(lims, *b),
                             lambda: _sw_rfmip(c, dev, cl, with_g, top_at_1)[:2])
            for a, b, n in zip(one, over, NAMES):
                np.testing.assert_array_equal(a, b, err_msg="%s %s all ones" % (name, n))
            zero = _with_bnd(dev, lims, lambda *b: _arm_pair(lims, *b, ng, zero_bits) == 0 or pytest.fail(_last_error()),
                             lambda: _sw_rfmip(c, dev, cl, with_g, top_at_1)[:2])
            # the mask matters: a band whose down flux is neither the overcast nor the all-zeros one
            assert ((got[4] != one[4]).reshape(-1, len(lims)).any(axis=0)
                    & (got[4] != zero[4]).reshape(-1, len(lims)).any(axis=0)).any(), name


# ---- the request --------------------------------------------------------------------------------------------------------
def test_request_semantics_lw(dev, lw_case):
    from rrtmgpnn import _lib
    from rrtmgpnn._lib import int_array
    c, L, ctx = lw_case, _lib.lib(), _ctx()
    ng, lims = c["ng"], np.asarray(c["kd"]["band_lims_gpt"], np.int32).reshape(-1, 2)
    nb = len(lims)
    bits = _bits_t(C.mask_for(ng, C.LW_MASK_SEED), dev)
    _, oup, odn = _lw_call(c, dev, INC, True, 1)
    bu, bd = Guarded(dev, nb), Guarded(dev, nb)

    def plain_again():
        """The next call is the plain one and writes no by-band output."""
        bu.t.fill_(NAN), bd.t.fill_(NAN)
        rc, up, dn = _lw_call(c, dev, INC, True, 1)
        assert rc == 0
        np.testing.assert_array_equal(up, oup)
        np.testing.assert_array_equal(dn, odn)
        assert torch.isnan(bu.t).all() and torch.isnan(bd.t).all()

    # consumed by a successful call
    assert _arm_pair(lims, bu.t, bd.t, None, ng, bits) == 0
    rc, up, dn = _lw_call(c, dev, INC, True, 1)
    assert rc == 0 and (dn != odn).any()
    bu.get(), bd.get()
    plain_again()
    # consumed by a failing call (bad argument after the request was taken)
    assert _arm_pair(lims, bu.t, bd.t, None, ng, bits) == 0
    rc = getattr(L, INC)(ctx, ng, NLAY, NCOL, 1, 1, None, None, None, None, None, None, 0, 0, None, None, None, 1, None,
                         0.0, 0.0, None, 0, None, None, None)
    assert rc == ERR_ARGUMENT
    plain_again()
    # extents that are not the call's: refused by the call, and cleared
    for ext in ((ng - 32, NLAY, NCOL), (ng, NLAY + 1, NCOL), (ng, NLAY, NCOL + 1)):
        small = lims[lims[:, 1] <= ext[0]]
        assert L.rrtmgpnn_solver_request_byband_mcica(ctx, len(small), int_array(small.ravel()), P(bu.t), P(bd.t), None,
                                                      *ext, P(bits)) == 0
        rc, _, _ = _lw_call(c, dev, INC, True, 1)
        assert rc == ERR_ARGUMENT, ext
        plain_again()
    # bad arguments: RRTMGPNN_ERR_ARGUMENT, nothing armed, and what was armed is cleared
    li = int_array(lims.ravel())
    bad_lims = lims.copy()
    bad_lims[3] = (bad_lims[3, 1], bad_lims[3, 0])  # first > last
    past = lims.copy()
    past[-1, 1] = ng + 1
    for args in ((nb, li, P(bu.t), P(bd.t), None, ng, NLAY, NCOL, None),       # NULL mask
                 (nb, li, None, None, None, ng, NLAY, NCOL, P(bits)),          # no output
                 (nb, li, P(bu.t), P(bd.t), None, 0, NLAY, NCOL, P(bits)),     # extents
                 (nb, li, P(bu.t), P(bd.t), None, ng, 0, NCOL, P(bits)),
                 (nb, li, P(bu.t), P(bd.t), None, ng, NLAY, -1, P(bits)),
                 (0, li, P(bu.t), P(bd.t), None, ng, NLAY, NCOL, P(bits)),     # band limits
                 (65, li, P(bu.t), P(bd.t), None, ng, NLAY, NCOL, P(bits)),
                 (nb, None, P(bu.t), P(bd.t), None, ng, NLAY, NCOL, P(bits)),
                 (nb, int_array(bad_lims.ravel()), P(bu.t), P(bd.t), None, ng, NLAY, NCOL, P(bits)),
                 (nb, int_array(past.ravel()), P(bu.t), P(bd.t), None, ng, NLAY, NCOL, P(bits))):
        assert _arm_pair(lims, bu.t, bd.t, None, ng, bits) == 0  # armed, then cleared by the refused request
        assert L.rrtmgpnn_solver_request_byband_mcica(ctx, *args) == ERR_ARGUMENT, args
        assert "solver_request_byband_mcica" in _last_error()
        plain_again()
    # bnd_flux_dir is not a longwave output
    bdir = Guarded(dev, nb)
    assert _arm_pair(lims, bu.t, bd.t, bdir.t, ng, bits) == 0
    rc, _, _ = _lw_call(c, dev, INC, True, 1)
    assert rc == ERR_ARGUMENT
    plain_again()
    # a separate request of either half drops the pairing: refused as the two separate requests are, and cleared
    assert _arm_pair(lims, bu.t, bd.t, None, ng, bits) == 0
    _arm_mask(ng, bits)
    rc, _, _ = _lw_call(c, dev, INC, True, 1)
    assert rc == ERR_UNSUPPORTED
    plain_again()
    assert _arm_pair(lims, bu.t, bd.t, None, ng, bits) == 0
    _arm_byband(lims, bu.t, bd.t, None)
    rc, _, _ = _lw_call(c, dev, INC, True, 1)
    assert rc == ERR_UNSUPPORTED
    plain_again()


def test_refusing_entries(dev, lw_case):
    """Every solver entry that refuses a cloud mask refuses the pair (before it looks at its other arguments, so these
    calls pass none) and clears it."""
    from rrtmgpnn import _lib
    c, L, ctx = lw_case, _lib.lib(), _ctx()
    ng, lims = c["ng"], np.asarray(c["kd"]["band_lims_gpt"], np.int32).reshape(-1, 2)
    bits = _bits_t(C.mask_for(ng, C.LW_MASK_SEED), dev)
    bu, bd = Guarded(dev, len(lims)), Guarded(dev, len(lims))
    _, oup, odn = _lw_call(c, dev, INC, True, 1)
    refusing = ["rrtmgpnn_lw_solver_noscat", "rrtmgpnn_lw_solver_noscat_planck",
                "rrtmgpnn_lw_solver_noscat_planck_clr_all", "rrtmgpnn_lw_solver_noscat_planck_clr_all_mcica",
                "rrtmgpnn_lw_solver_1rescl", "rrtmgpnn_lw_solver_2stream", "rrtmgpnn_sw_solver_2stream",
                "rrtmgpnn_sw_solver_noscat", "rrtmgpnn_lw_solver_noscat_gpt", "rrtmgpnn_lw_solver_noscat_planck_gpt",
                "rrtmgpnn_sw_solver_2stream_gpt", "rrtmgpnn_lw_solver_1rescl_gpt", "rrtmgpnn_lw_solver_2stream_gpt",
                "rrtmgpnn_sw_solver_noscat_gpt"]
    for name in refusing:
        assert _arm_pair(lims, bu.t, bd.t, None, ng, bits) == 0
        argt = _lib.SIGNATURES[name][1]
        args = [ctx, ng, NLAY, NCOL] + [0 if a is _lib.c_int else 0.0 if a is _lib.c_float else None for a in argt[4:]]
        assert getattr(L, name)(*args) == ERR_ARGUMENT, name
        rc, up, dn = _lw_call(c, dev, INC, True, 1)  # cleared: the plain increment, no by-band output
        assert rc == 0, name
        np.testing.assert_array_equal(dn, odn, err_msg=name)
        assert torch.isnan(bu.t).all() and torch.isnan(bd.t).all(), name


def test_request_semantics_sw(dev, sw_case):
    from rrtmgpnn import api
    c = sw_case
    ng, cl = c["ng"], c["lims"]["pair"]
    lims = C.byband_layouts(c["kd"])["irregular"]
    bits = _bits_t(C.mask_for(ng, C.SW_MASK_SEED), dev)
    _, over = _sw_inc(c, dev, cl, True, True)
    bnd = [Guarded(dev, len(lims)) for _ in range(3)]
    assert _arm_pair(lims, *[b.t for b in bnd], ng, bits) == 0
    rc, got = _sw_inc(c, dev, cl, True, True)
    assert rc == 0 and (got[1] != over[1]).any()
    ref = [b.get() for b in bnd]
    for b in bnd:
        b.t.fill_(NAN)
    rc, again = _sw_inc(c, dev, cl, True, True)  # consumed: the plain call
    assert rc == 0 and all(torch.isnan(b.t).all() for b in bnd)
    for a, b in zip(again, over):
        np.testing.assert_array_equal(a, b)
    assert _arm_pair(lims, *[b.t for b in bnd], ng, bits, nlay=NLAY - 1) == 0
    rc, _ = _sw_inc(c, dev, cl, True, True)
    assert rc == ERR_ARGUMENT and "cloud mask" in _last_error()
    # _rfmip without the band increment
    assert _arm_pair(lims, *[b.t for b in bnd], ng, bits) == 0
    rc, _, _ = _sw_rfmip(c, dev, cl, True, True, nbnd=0)
    assert rc == ERR_ARGUMENT
    for b in bnd:
        b.t.fill_(NAN)
    rc, plain = _sw_inc(c, dev, cl, True, True)  # cleared: the unmasked call, no by-band output
    assert rc == 0 and all(torch.isnan(b.t).all() for b in bnd)
    for a, b in zip(plain, over):
        np.testing.assert_array_equal(a, b)
    # the other SW kernels have no masked instance
    for mode in (1, 2):
        api.set_sw_kernel_default(mode)
        try:
            assert _arm_pair(lims, *[b.t for b in bnd], ng, bits) == 0
            rc, _ = _sw_inc(c, dev, cl, True, True)
            assert rc == ERR_UNSUPPORTED, mode
            rc, plain = _sw_inc(c, dev, cl, True, True)  # cleared: the unmasked call on that kernel
            assert rc == 0 and all(torch.isnan(b.t).all() for b in bnd)
            for a, b in zip(plain, over):
                np.testing.assert_array_equal(a, b)
        finally:
            api.set_sw_kernel_default(0)
    for mode in (0, 3):
        api.set_sw_kernel_default(mode)
        try:
            assert _arm_pair(lims, *[b.t for b in bnd], ng, bits) == 0
            rc, g2 = _sw_inc(c, dev, cl, True, True)
            assert rc == 0
            for a, b in zip(g2 + [b.get() for b in bnd], got + ref):
                np.testing.assert_array_equal(a, b)
        finally:
            api.set_sw_kernel_default(0)


def test_class_layer_arm(dev, lw_case):
    """cloud_sampling.arm_cloud_mask_byband is the request."""
    from rrtmgpnn import cloud_sampling as cs
    from rrtmgpnn.api import context
    c = lw_case
    ng, lims = c["ng"], C.byband_layouts(c["kd"])["uncovered"]
    bits = _bits_t(C.mask_for(ng, C.LW_MASK_SEED), dev)
    want = _lw_paired(c, dev, lims, bits, True, 1)
    bu, bd = Guarded(dev, len(lims)), Guarded(dev, len(lims))
    cs.arm_cloud_mask_byband(context(0), ng, bits, lims, bu.t, bd.t)
    rc, up, dn = _lw_call(c, dev, INC, True, 1)
    assert rc == 0
    for a, b in zip((up, dn, bu.get(), bd.get()), want):
        np.testing.assert_array_equal(a, b)


# ---- ClearSkyStep(mcica={..., "byband": True}) -------------------------------------------------------------------------
KEYS = ("lw_up", "lw_dn", "sw_up", "sw_dn", "sw_dir")
BKEYS = ("lw_bnd_up", "lw_bnd_dn", "sw_bnd_up", "sw_bnd_dn", "sw_bnd_dir")


def _all_fluxes(s):
    out = dict(s.fluxes())
    out.update(s.byband_fluxes())
    return {k: out[k] for k in KEYS + BKEYS}


def _same(got, want, use, what, keys=KEYS + BKEYS):
    for k in keys:
        a, b = (got[k][use], want[k][use]) if k.startswith("sw") else (got[k], want[k])  # night columns: unspecified
        assert not np.isnan(a).any(), what + k
        np.testing.assert_array_equal(a, b, err_msg=what + k)


def test_step_mcica_byband(dev, rfmip):
    from conftest import subset
    from rrtmgpnn import cloud_sampling as cs, data
    from rrtmgpnn.pipeline import ClearSkyStep
    prob = subset(rfmip, np.arange(4) * 400)
    ncol, nlay, use = 4, prob["nlay"], prob["usecol"]
    assert use.any()
    clouds = data.allsky_clouds(prob, data.load_cloud_optics("lw"))
    cloudy = (clouds[0] > 0) | (clouds[1] > 0)
    assert cloudy.any()
    rng = np.random.default_rng(41)
    cf = np.where(cloudy, rng.uniform(0.2, 0.9, cloudy.shape), 0).astype(np.float32)
    ov = rng.uniform(-1, 1, (ncol, nlay - 1)).astype(np.float32)
    seed = 2026
    base = {"cloud_frac": cf, "overlap_param": ov}
    # the seeded route, eager and as a captured and replayed graph
    s = ClearSkyStep(prob, device=0, clouds=clouds, mcica=dict(base, seed=seed, byband=True))
    names = [n for n, _, _ in s.calls]
    assert names.index("lw_mask_byband") == names.index("lw_solver") - 1
    assert names.index("sw_mask_byband") == names.index("sw_solver") - 1
    assert not {"lw_mask", "sw_mask", "lw_byband", "sw_byband"} & set(names)
    for k in KEYS + BKEYS:
        getattr(s, k).fill_(NAN)
    s.step()
    torch.cuda.synchronize()
    seeded = _all_fluxes(s)
    s.capture()
    for k in KEYS + BKEYS:
        getattr(s, k).fill_(NAN)
    s.replay()
    torch.cuda.synchronize()
    _same(_all_fluxes(s), seeded, use, "replay ")
    s.close()
    # the array route fed with the generator's numbers
    zl, zs = np.zeros((ncol, nlay, 256), np.float32), np.zeros((ncol, nlay, 224), np.float32)
    arrays = dict(base, randoms_lw=zl, randoms_sw=zs)

    def run(**kw):
        mc = dict(arrays)
        mc.update(kw.pop("mc", {}))
        st = ClearSkyStep(prob, device=0, clouds=clouds, mcica=mc, **kw)
        r_lw, r_sw = st.mcica_randoms()
        assert cs.mcica_randoms(seed, 0, 0, r_lw) == "" and cs.mcica_randoms(seed, 1, 0, r_sw) == ""
        st.step()
        torch.cuda.synchronize()
        return st

    a = run(mc={"byband": True})
    _same(_all_fluxes(a), seeded, use, "array route ")
    a.close()
    # fused == unfused on all ten arrays
    u = run(mc={"byband": True}, fused=False)
    un = [n for n, _, _ in u.calls]
    assert un.index("lw_byband") == un.index("lw_solver") - 1 and un.index("sw_byband") == un.index("sw_solver") - 1
    assert "draw_samples_lw" in un and "increment_sw" in un and not [n for n in un if n.endswith("mask_byband")]
    _same(_all_fluxes(u), seeded, use, "unfused ")
    u.close()
    # the broadband fluxes are those of the same step without the key, whose call list holds no new name
    p = run()
    pn = [n for n, _, _ in p.calls]
    assert not [n for n in pn if "byband" in n] and "lw_mask" in pn and "sw_mask" in pn
    assert [n for n in names if not n.endswith("_mask_byband")] == [n for n in pn if n not in ("lw_mask", "sw_mask")]
    _same(p.fluxes(), seeded, use, "without the key ", KEYS)
    assert not p.byband
    p.close()
    # the clouds matter to the by-band fluxes: not the overcast step's
    o = ClearSkyStep(prob, device=0, clouds=clouds, byband=True)
    o.step()
    torch.cuda.synchronize()
    assert (o.byband_fluxes()["lw_bnd_dn"] != seeded["lw_bnd_dn"]).any()
    o.close()
    # refusals
    with pytest.raises(ValueError, match="clrsky"):
        ClearSkyStep(prob, device=0, clouds=clouds, mcica=dict(arrays, byband=True, clrsky=True))
    with pytest.raises(ValueError, match="mcica"):
        ClearSkyStep(prob, device=0, clouds=clouds, mcica=dict(arrays, byband=True), byband=True)
