"""GPU: clear-sky beside all-sky LW fluxes for scattering clouds, with aerosols
(rrtmgpnn_lw_solver_1rescl_planck_clr_all), every comparison bit for bit on uint32 views and the mode
(rrtmgpnn_context_set_lw_scat_clr_all: 1 the dual kernel, 2 the two launches) set explicitly in every test.

1. against the composed oracle of tests/lw_scat_dual_cases.py, four arrays: one angle over every case x orientation x
   mask kind x aerosol off / on x mode; three angles at (256, 11) and (30, 7);
2. against the GPU's own composition: aerosol off rrtmgpnn_lw_solver_noscat_planck + _1rescl_planck_inc, aerosol on
   increment_bybnd twice on materialised arrays + compute_planck_source_nn + lw_solver_1rescl and _noscat_planck_inc;
3. emissivity per g-point and a non-zero inc_flux;
4. an all-zero mask: the all-sky arrays equal the clear ones; a sampled mask leaves the clear set the unmasked call's;
5. buffer safety: outputs one float off alignment between intact guards, inputs unchanged, the workspace shared with
   the single entry on one context;
6. the requests' lifetime and every refusal;  7. the modes agree at one and three angles.

That the expectations tell the aerosol, the increment order and the mask apart is established on the CPU in
tests/test_lw_scat_dual_host.py."""
import numpy as np
import pytest

import lw_scat_cases as S
import lw_scat_dual_cases as D
import mcica_ref as M
from lw_scat_cases import NCOL

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
ERR_ARGUMENT, ERR_UNSUPPORTED = 1, 4
NAN = float("nan")
ENTRY = "rrtmgpnn_lw_solver_1rescl_planck_clr_all"
NAME = "lw_solver_1rescl_planck_clr_all"
ORIENT = pytest.mark.parametrize("top_at_1", [True, False], ids=["top1", "top0"])
MODES = pytest.mark.parametrize("mode", [1, 2], ids=["dual", "two"])
AER = pytest.mark.parametrize("aer", [False, True], ids=["noaer", "aer"])
CASES = pytest.mark.parametrize("ng,nlay", S.CASES)
TWO = pytest.mark.parametrize("ng,nlay", [(256, 11), (30, 7)])


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


def _set_mode(mode, expect=0):
    rc = _L().rrtmgpnn_context_set_lw_scat_clr_all(_ctx(), mode)
    assert rc == expect, (mode, rc, _last_error())


@pytest.fixture(autouse=True)
def _default_mode_afterwards():
    yield
    _set_mode(0)


def _same(got, want, what):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        g, w = np.ascontiguousarray(g, np.float32), np.ascontiguousarray(w, np.float32)
        np.testing.assert_array_equal(g.view(np.uint32), w.view(np.uint32), err_msg="%s [%d]" % (what, i))


_dev_cases = {}


def case(ng, nlay, dev):
    """The case's inputs on the host and the device, built once and never modified."""
    if (ng, nlay) not in _dev_cases:
        c = dict(S.case(ng, nlay))
        c["aer"] = D.aerosol(ng, nlay)
        c["dev"] = {k: T(c[k], dev) for k in ("tau", "pfrac", "tb", "wb", "gb", "tlay", "tlev", "tsfc", "emis_bnd",
                                             "emis_gpt", "inc", "aer")}
        c["dev"]["totplnk"] = T(c["kd"]["totplnk"], dev)
        c["bits"] = {k: _bits_t(S.mask_for(c, k), dev) for k in S.MASKS if k is not None}
        c["bits"][None] = None
        _dev_cases[(ng, nlay)] = c
    return _dev_cases[(ng, nlay)]


def _planck_tail(c, top_at_1, emis_by_band=True):
    from rrtmgpnn._lib import int_array
    d, kd, nlay = c["dev"], c["kd"], c["nlay"]
    return (P(d["pfrac"]), c["nb"], kd["nPlanckTemp"], P(d["tlay"]), P(d["tlev"]), P(d["tsfc"]), nlay if top_at_1 else 1,
            int_array(np.asarray(c["lims"]).ravel()), float(kd["temp_ref_min"][0]), float(kd["totplnk_delta"]),
            P(d["totplnk"]), int(emis_by_band), P(d["emis_bnd"] if emis_by_band else d["emis_gpt"]))


def _head(c, top_at_1, nmus, inc=False, ncol=NCOL, ng=None):
    from rrtmgpnn._lib import float_array
    from rrtmgpnn.api import GAUSS_DS, GAUSS_WTS
    return (_ctx(), c["ng"] if ng is None else ng, c["nlay"], ncol, int(top_at_1), nmus, float_array(GAUSS_DS[nmus]),
            float_array(GAUSS_WTS[nmus]), P(c["dev"]["inc"]) if inc else None, P(c["dev"]["tau"]))


def _arm_mask(c, bits):
    assert _L().rrtmgpnn_solver_request_cloud_mask(_ctx(), c["ng"], c["nlay"], NCOL, P(bits)) == 0, _last_error()


def _arm_aer(c, tau_aer=None):
    t = c["dev"]["aer"] if tau_aer is None else tau_aer
    assert _L().rrtmgpnn_solver_request_aerosol(_ctx(), c["nb"], c["nlay"], NCOL, P(t), None, None) == 0, _last_error()


def _nan_outs(c, dev, n):
    return [torch.full((NCOL, c["nlay"] + 1), NAN, device=dev) for _ in range(n)]


def _call(c, dev, top_at_1, nmus=1, kind=None, aer=False, emis_by_band=True, inc=False, check=True, cloud=None,
          ncol=NCOL, outs=None, ng=None, drop_clr=None):
    """The entry on the case, outputs pre-filled with NaN, the mask `kind` and the aerosol armed -> the 4 flux arrays
    (up, dn, up_clr, dn_clr), or (rc, arrays) with check=False.  cloud: other band arrays (None entries: NULL);
    drop_clr: index (2 or 3) of a clear-sky output passed as NULL."""
    d = c["dev"]
    outs = _nan_outs(c, dev, 4) if outs is None else outs
    cloud = (d["tb"], d["wb"], d["gb"]) if cloud is None else cloud
    if c["bits"][kind] is not None:
        _arm_mask(c, c["bits"][kind])
    if aer:
        _arm_aer(c)
    ptrs = [P(o) for o in outs]
    if drop_clr is not None:
        ptrs[drop_clr] = None
    rc = getattr(_L(), ENTRY)(*_head(c, top_at_1, nmus, inc, ncol=ncol, ng=ng), *[P(a) for a in cloud],
                              *_planck_tail(c, top_at_1, emis_by_band), *ptrs)
    torch.cuda.synchronize()
    res = [o.cpu().numpy() for o in outs]
    if check:
        assert rc == 0, _last_error()
        return res
    return rc, res


def _single(c, dev, top_at_1, nmus, kind):
    """rrtmgpnn_lw_solver_1rescl_planck_inc under the same mask request."""
    d = c["dev"]
    outs = _nan_outs(c, dev, 2)
    if c["bits"][kind] is not None:
        _arm_mask(c, c["bits"][kind])
    assert _L().rrtmgpnn_lw_solver_1rescl_planck_inc(*_head(c, top_at_1, nmus), P(d["tb"]), P(d["wb"]), P(d["gb"]),
                                                    *_planck_tail(c, top_at_1), *[P(o) for o in outs]) == 0, _last_error()
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs]


def _noscat(c, dev, top_at_1, nmus, aer):
    """rrtmgpnn_lw_solver_noscat_planck, or _noscat_planck_inc with tau_aer as its band increment."""
    outs = _nan_outs(c, dev, 2)
    L = _L()
    if aer:
        rc = L.rrtmgpnn_lw_solver_noscat_planck_inc(*_head(c, top_at_1, nmus), P(c["dev"]["aer"]),
                                                    *_planck_tail(c, top_at_1), *[P(o) for o in outs])
    else:
        rc = L.rrtmgpnn_lw_solver_noscat_planck(*_head(c, top_at_1, nmus), *_planck_tail(c, top_at_1),
                                                *[P(o) for o in outs])
    assert rc == 0, _last_error()
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs]


def _materialised(c, dev, top_at_1, nmus, kind):
    """The all-sky set with an aerosol from the existing entries on materialised arrays: increment_bybnd by the aerosol
    (1scl into 2str), the (sampled) cloud increment, compute_planck_source_nn, lw_solver_1rescl."""
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
    assert L.rrtmgpnn_increment_bybnd(_ctx(), NCOL, nlay, ng, nb, lims, P(tau), P(ssa), P(g), P(d["aer"]), None,
                                      None) == 0, _last_error()
    mask = S.mask_for(c, kind)
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
    outs = _nan_outs(c, dev, 2)
    assert L.rrtmgpnn_lw_solver_1rescl(*_head(c, top_at_1, nmus)[:-1], P(tau), P(ssa), P(g), P(lay), P(lev), P(emis),
                                       P(sfc), *[P(o) for o in outs]) == 0, _last_error()
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs]


def _oracle_sweep(dev, orc, c, top_at_1, nmus, aer, mode):
    _set_mode(mode)
    got = {}
    for kind in S.MASKS:
        got[kind] = _call(c, dev, top_at_1, nmus, kind=kind, aer=aer)
        _same(got[kind], D.expect(orc, c, kind, aer, top_at_1, nmus), "mask %s against the oracle" % (kind,))
    _same(got["ones"], got[None], "all ones against the unmasked call")
    assert (got["sampled"][1] != got[None][1]).any() and (got["sampled"][1] != got["zeros"][1]).any()


@CASES
@ORIENT
@AER
@MODES
def test_against_the_composed_oracle(dev, orc, ng, nlay, top_at_1, aer, mode):
    """1: one angle, every mask kind."""
    _oracle_sweep(dev, orc, case(ng, nlay, dev), top_at_1, 1, aer, mode)


@TWO
@ORIENT
@AER
@MODES
def test_against_the_composed_oracle_three_angles(dev, orc, ng, nlay, top_at_1, aer, mode):
    """1: three angles (two launches in either mode; the non-dual aerosol instance's accumulator path)."""
    _oracle_sweep(dev, orc, case(ng, nlay, dev), top_at_1, 3, aer, mode)


@CASES
@ORIENT
@AER
@MODES
def test_against_the_gpu_composition(dev, ng, nlay, top_at_1, aer, mode):
    """2: the existing entries on the same device arrays, unmasked and sampled, one and three angles."""
    c = case(ng, nlay, dev)
    _set_mode(mode)
    for nmus in (1, 3):
        clear = _noscat(c, dev, top_at_1, nmus, aer)
        for kind in (None, "sampled"):
            got = _call(c, dev, top_at_1, nmus, kind=kind, aer=aer)
            all_sky = _materialised(c, dev, top_at_1, nmus, kind) if aer else _single(c, dev, top_at_1, nmus, kind)
            _same(got, all_sky + clear, "nmus %d, mask %s against the composition" % (nmus, kind))


@TWO
@ORIENT
@AER
@MODES
def test_emissivity_per_gpoint_and_incident_flux(dev, orc, ng, nlay, top_at_1, aer, mode):
    """3: emis_by_band = 0 and a non-NULL inc_flux, unmasked and sampled."""
    c = case(ng, nlay, dev)
    _set_mode(mode)
    for kind in (None, "sampled"):
        plain = D.expect(orc, c, kind, aer, top_at_1, 1)
        for by_band, inc in ((False, False), (True, True), (False, True)):
            got = _call(c, dev, top_at_1, 1, kind=kind, aer=aer, emis_by_band=by_band, inc=inc)
            want = D.expect(orc, c, kind, aer, top_at_1, 1, emis_by_band=by_band, inc=inc)
            _same(got, want, "%s, emis_by_band=%d, inc_flux=%s" % (kind, by_band, inc))
            assert (want[0] != plain[0]).any() and (want[2] != plain[2]).any()
            assert not inc or ((want[1] != plain[1]).any() and (want[3] != plain[3]).any())


@CASES
@AER
@MODES
def test_zero_mask_is_the_clear_sky_and_masks_leave_the_clear_set(dev, ng, nlay, aer, mode):
    """4."""
    c = case(ng, nlay, dev)
    _set_mode(mode)
    for nmus in (1, 3):
        zeros = _call(c, dev, True, nmus, kind="zeros", aer=aer)
        _same(zeros[:2], zeros[2:], "all-zero mask: all-sky against clear")
        plain = _call(c, dev, True, nmus, aer=aer)
        sampled = _call(c, dev, True, nmus, kind="sampled", aer=aer)
        _same(sampled[2:], plain[2:], "the mask reached the clear set")
        _same(zeros[2:], plain[2:], "the mask reached the clear set")
        assert (sampled[1] != plain[1]).any() and (plain[1] != plain[3]).any()


@AER
@MODES
def test_buffer_safety(dev, aer, mode):
    """5: outputs one float off alignment with their guard floats intact; inputs unchanged; the workspace shared on one
    context by the single entry, the dual at a larger shape, the single again (only mode 1's dual launch grows the
    workspace between the single calls; in mode 2 the sequence repeats the existing launchers)."""
    nlay = 7
    c = case(72, nlay, dev)
    big = case(256, 11, dev)
    d = c["dev"]
    _set_mode(mode)
    keys = ("tau", "pfrac", "tb", "wb", "gb", "aer")
    before = {k: d[k].clone() for k in keys}
    n = NCOL * (nlay + 1)
    GUARD = 12345.0
    bufs = [torch.full((n + 3,), GUARD, device=dev) for _ in range(4)]
    outs = [b[1:n + 1].view(NCOL, nlay + 1) for b in bufs]
    assert all(o.data_ptr() % 8 == 4 for o in outs)
    for kind in (None, "sampled"):
        want = _call(c, dev, True, 1, kind=kind, aer=aer)
        for o in outs:
            o.fill_(NAN)
        got = _call(c, dev, True, 1, kind=kind, aer=aer, outs=outs)
        _same(got, want, "misaligned outputs")
        for b in bufs:
            assert float(b[0]) == GUARD and (b[n + 1:] == GUARD).all(), "a guard float was written"
    assert all(torch.equal(d[k], v) for k, v in before.items()), "an input was modified"
    first = _single(c, dev, True, 1, "sampled")
    ref = _call(big, dev, True, 1, kind="sampled", aer=aer)
    _same(_single(c, dev, True, 1, "sampled"), first, "the single entry after the dual one")
    _same(_call(big, dev, True, 1, kind="sampled", aer=aer), ref, "the dual entry after the single one")
    _same(_call(big, dev, True, 3, kind="sampled", aer=aer)[2:], _noscat(big, dev, True, 3, aer), "three angles")


@MODES
def test_request_lifetime_and_refusals(dev, orc, mode):
    """6: the mask and aerosol requests belong to one call; by-band (separate and paired), Jacobian and 2str-aerosol
    requests, foreign mask and aerosol extents, NULL arrays and ngpt > 256 are refused with their status and the entry's
    name, write nothing and leave nothing armed; the knob rejects mode 3; ncol == 0 is OK."""
    from rrtmgpnn._lib import int_array
    L = _L()
    c = case(72, 7, dev)
    d, ng, nlay, nb = c["dev"], c["ng"], c["nlay"], c["nb"]
    _set_mode(mode)
    plain = _call(c, dev, True)
    _same(plain, D.expect(orc, c, None, False, True, 1), "the plain call")
    both = _call(c, dev, True, kind="sampled", aer=True)
    assert (both[1] != plain[1]).any() and (both[3] != plain[3]).any()
    _same(_call(c, dev, True), plain, "a request outlived its call")
    bits = c["bits"]["sampled"]
    lims = int_array(np.asarray(c["lims"]).ravel())
    bnd = [torch.full((NCOL, nlay + 1, nb), NAN, device=dev) for _ in range(2)]
    jac = torch.full((NCOL, nlay + 1), NAN, device=dev)

    def byband():
        return L.rrtmgpnn_solver_request_byband(_ctx(), nb, lims, P(bnd[0]), P(bnd[1]), None)

    def paired():
        return L.rrtmgpnn_solver_request_byband_mcica(_ctx(), nb, lims, P(bnd[0]), P(bnd[1]), None, ng, nlay, NCOL, P(bits))

    def jacobian():
        return L.rrtmgpnn_solver_request_jacobian(_ctx(), ng, nlay, NCOL, None, P(jac))

    def aerosol_2str():
        return L.rrtmgpnn_solver_request_aerosol(_ctx(), nb, nlay, NCOL, P(d["aer"]), P(d["wb"]), P(d["gb"]))

    def wrong_aerosol():
        return L.rrtmgpnn_solver_request_aerosol(_ctx(), nb, nlay + 1, NCOL, P(d["aer"]), None, None)

    def wrong_mask():
        return L.rrtmgpnn_solver_request_cloud_mask(_ctx(), ng, nlay + 1, NCOL, P(bits))

    def aerosol_and_wrong_mask():
        return wrong_mask() or L.rrtmgpnn_solver_request_aerosol(_ctx(), nb, nlay, NCOL, P(d["aer"]), None, None)

    for arm in (byband, paired, jacobian, aerosol_2str, wrong_aerosol, wrong_mask, aerosol_and_wrong_mask):
        assert arm() == 0, _last_error()
        rc, out = _call(c, dev, True, check=False)
        assert rc == ERR_ARGUMENT, (arm.__name__, rc, _last_error())
        assert NAME in _last_error(), (arm.__name__, _last_error())
        assert all(np.isnan(o).all() for o in out), "a refused call wrote (%s)" % arm.__name__
        _same(_call(c, dev, True), plain, "something stayed armed after the %s refusal" % arm.__name__)
    assert all(torch.isnan(b).all() for b in bnd) and torch.isnan(jac).all(), "a refused call wrote a requested output"
    # all three band arrays and both clear-sky arrays are required
    for k in range(3):
        cloud = [d["tb"], d["wb"], d["gb"]]
        cloud[k] = None
        rc, out = _call(c, dev, True, check=False, cloud=cloud, kind="sampled", aer=True)
        assert rc == ERR_ARGUMENT and NAME in _last_error(), (k, rc, _last_error())
        assert all(np.isnan(o).all() for o in out)
        _same(_call(c, dev, True), plain, "something stayed armed after a NULL band array")
    for k in (2, 3):
        rc, out = _call(c, dev, True, check=False, drop_clr=k)
        assert rc == ERR_ARGUMENT and NAME in _last_error(), (k, rc, _last_error())
        assert all(np.isnan(o).all() for o in out)
    # more than 256 g-points (nothing is read: the refusal comes before the launch)
    _arm_aer(c)
    rc, out = _call(c, dev, True, check=False, ng=260)
    assert rc == ERR_UNSUPPORTED and NAME in _last_error(), (rc, _last_error())
    assert all(np.isnan(o).all() for o in out)
    _same(_call(c, dev, True), plain, "the aerosol of the refused call stayed armed")
    rc, _ = _call(c, dev, True, check=False, ncol=-1)
    assert rc == ERR_ARGUMENT
    # ncol == 0: OK, nothing written, and requests of those extents are cleared
    assert L.rrtmgpnn_solver_request_cloud_mask(_ctx(), ng, nlay, 0, P(bits)) == 0
    rc, out = _call(c, dev, True, check=False, ncol=0)
    assert rc == 0, _last_error()
    assert all(np.isnan(o).all() for o in out)
    _same(_call(c, dev, True), plain, "the mask of the empty call stayed armed")
    # the knob
    _set_mode(3, expect=ERR_ARGUMENT)
    _set_mode(-1, expect=ERR_ARGUMENT)
    assert L.rrtmgpnn_context_set_lw_scat_clr_all(None, 3) == ERR_ARGUMENT
    _same(_call(c, dev, True), plain, "a rejected mode changed the call")
    # the single entry keeps refusing an aerosol
    _arm_aer(c)
    outs = _nan_outs(c, dev, 2)
    rc = L.rrtmgpnn_lw_solver_1rescl_planck_inc(*_head(c, True, 1), P(d["tb"]), P(d["wb"]), P(d["gb"]),
                                                *_planck_tail(c, True), *[P(o) for o in outs])
    torch.cuda.synchronize()
    assert rc == ERR_ARGUMENT and "lw_solver_1rescl_planck_inc" in _last_error()
    assert all(torch.isnan(o).all() for o in outs)


@CASES
@ORIENT
@AER
def test_modes_agree(dev, ng, nlay, top_at_1, aer):
    """7: modes 0, 1 and 2 at one and three angles under a sampled mask; ctx == NULL is accepted."""
    c = case(ng, nlay, dev)
    L = _L()
    res = {}
    for nmus in (1, 3):
        for mode in (0, 1, 2):
            _set_mode(mode)
            res[(nmus, mode)] = _call(c, dev, top_at_1, nmus, kind="sampled", aer=aer)
        _same(res[(nmus, 1)], res[(nmus, 2)], "mode 1 against mode 2, nmus %d" % nmus)
        _same(res[(nmus, 0)], res[(nmus, 2)], "mode 0 against mode 2, nmus %d" % nmus)
    # ctx == NULL sets the default of contexts never set themselves: accepted, and this context keeps its own mode
    try:
        assert L.rrtmgpnn_context_set_lw_scat_clr_all(None, 1) == 0
        _same(_call(c, dev, top_at_1, 1, kind="sampled", aer=aer), res[(1, 2)], "after the process default was set")
    finally:
        assert L.rrtmgpnn_context_set_lw_scat_clr_all(None, 0) == 0


# ---- the class layer --------------------------------------------------------------------------------------------------
def test_class_layer_aerosol_route_against_the_sequence(dev, rfmip, monkeypatch):
    """clr_all_sky.rte_lw with by-band 2str clouds and by-band 1scl aerosols: the entry with the aerosol request
    (LW_SCAT_FUSED True) against the materialising sequence (False), masked and unmasked, one and three angles, all four
    flux arrays bit for bit; the new route never calls aer_props.increment."""
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
    rng = np.random.default_rng(98)
    cld = api.OpticalProps2str()
    assert cld.init(kd.get_band_lims_wavenumber()) == "" and cld.alloc_2str(ncol, nlay, device=dev) == ""
    cld.tau.copy_(T(rng.lognormal(0, 1, (ncol, nlay, nb)), dev))
    cld.ssa.copy_(T(rng.uniform(0.2, 0.9, (ncol, nlay, nb)), dev))
    cld.g.copy_(T(rng.uniform(0.5, 0.95, (ncol, nlay, nb)), dev))
    aer = api.OpticalProps1scl()
    assert aer.init(kd.get_band_lims_wavenumber()) == "" and aer.alloc_1scl(ncol, nlay, device=dev) == ""
    aer.tau.copy_(T(rng.lognormal(-1, 1, (ncol, nlay, nb)), dev))
    mask = rng.random((ncol, nlay, ng)) < 0.5
    bits = _bits_t(mask, dev)
    bytes_ = torch.as_tensor(np.ascontiguousarray(mask, np.uint8), device=dev)
    emis = T(np.repeat(np.asarray(p["sfc_emis"], np.float32)[:, None], nb, axis=1), dev)
    incs = []
    orig = api.OpticalProps1scl.increment

    def spy(self, *args, **kw):
        if self is aer:
            incs.append(1)
        return orig(self, *args, **kw)

    monkeypatch.setattr(api.OpticalProps1scl, "increment", spy)

    def fl():
        return api.FluxesBroadband(*[torch.full((ncol, nlay + 1), NAN, device=dev) for _ in range(3)])

    def run(masked, nmu, with_aer=True):
        a, cl = fl(), fl()
        e = clr_all_sky.rte_lw(kd, gases, play, tlay, plev, T(p["tsfc"], dev), emis, cld, a, cl,
                               aer_props=aer if with_aer else None, t_lev=T(p["tlev"], dev), neural_nets=nets,
                               n_gauss_angles=nmu, mask_bits=bits if masked else None,
                               cloud_mask=bytes_ if masked else None)
        assert e == "", e
        return [t.cpu().numpy() for t in (a.flux_up, a.flux_dn, cl.flux_up, cl.flux_dn)]

    res = {}
    for mode in (1, 2):
        _set_mode(mode)
        for route in (True, False):
            clr_all_sky.LW_SCAT_FUSED = route
            try:
                for masked in (False, True):
                    for nmu in (1, 3):
                        del incs[:]
                        res[(masked, nmu, route)] = run(masked, nmu)
                        assert len(incs) == (0 if route else 1), "rte_lw took the other aerosol route"
                        # without aerosols the same entry serves (the knob reaches the class layer there too)
                        res[(masked, nmu, route, "bare")] = run(masked, nmu, with_aer=False)
            finally:
                clr_all_sky.LW_SCAT_FUSED = True
        for masked in (False, True):
            for nmu in (1, 3):
                for bare in ((), ("bare",)):
                    fused, seq = res[(masked, nmu, True) + bare], res[(masked, nmu, False) + bare]
                    assert all(np.isfinite(v).all() for v in fused)
                    _same(fused, seq, "rte_lw mode=%d masked=%s nmu=%d %s" % (mode, masked, nmu, bare))
                    assert (fused[1] != fused[3]).any(), "the cloud does not show"
    assert (res[(True, 1, True)][1] != res[(False, 1, True)][1]).any(), "the mask does not show"
    no_aer = res[(False, 1, True, "bare")]
    assert all((x != y).any() for x, y in zip(no_aer, res[(False, 1, True)])), "the aerosol does not show"
    # the no-aerosol route issues the one entry, not the pair of before
    called = []
    L = _L()
    for name in ("rrtmgpnn_lw_solver_1rescl_planck_clr_all", "rrtmgpnn_lw_solver_1rescl_planck_inc",
                 "rrtmgpnn_lw_solver_noscat_planck"):
        fn = getattr(L, name)
        monkeypatch.setattr(L, name, lambda *a, _f=fn, _n=name: (called.append(_n), _f(*a))[1])
    run(True, 1, with_aer=False)
    assert called == ["rrtmgpnn_lw_solver_1rescl_planck_clr_all"], called
