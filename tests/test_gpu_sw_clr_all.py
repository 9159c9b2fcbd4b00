"""GPU: clear-sky beside all-sky SW fluxes from one call -- rrtmgpnn_sw_solver_2stream_clr_all and
rrtmgpnn_sw_solver_2stream_rfmip_clr_all (the dual checkpointed kernel, mode 1 of rrtmgpnn_context_set_sw_clr_all, and
the two launches of mode 2) -- bit for bit against the oracle and against the existing single-sky entries.  Inputs and
expectations: tests/sw_clr_all_cases.py.  Every comparison is assert_array_equal; outputs are pre-filled with NaN."""
import numpy as np
import pytest

import mcica_ref as M
import sw_clr_all_cases as S

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
ERR_ARGUMENT, ERR_UNSUPPORTED = 1, 4
NAN = float("nan")
GUARD = 8
DEV_KEYS = ("tau", "ssa", "g", "bt", "bw", "bg", "at", "aw", "ag", "mu0", "inc", "inc_dif", "alb", "solar", "tsi",
            "sfc_alb", "sza")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a device"
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


@pytest.fixture
def mode():
    """Sets the library-wide mode of the clear + all-sky SW entries; restores the default afterwards."""
    from rrtmgpnn import api
    yield api.set_sw_clr_all_default
    api.set_sw_clr_all_default(0)


def T(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=dev)


def P(t):
    return t.data_ptr() if t is not None else None


def _L():
    from rrtmgpnn import _lib
    return _lib.lib()


def _ctx():
    from rrtmgpnn.api import context
    return context(0).h


def _err():
    return _L().rrtmgpnn_last_error().decode()


def _dev(c, dev):
    if "dev" not in c:
        c["dev"] = {k: T(c[k], dev) for k in DEV_KEYS}
        c["dev"]["bits"] = [torch.as_tensor(M.pack_bits(m).view(np.int32), device=dev) for m in c["masks"]]
    return c["dev"]


def _outs(c, dev, n):
    """n flux arrays inside one NaN buffer with GUARD floats before, between and after them."""
    m = c["ncol"] * (c["nlay"] + 1)
    buf = torch.full((n * m + (n + 1) * GUARD,), NAN, device=dev)
    return buf, [buf[GUARD + i * (m + GUARD):GUARD + i * (m + GUARD) + m].view(c["ncol"], c["nlay"] + 1) for i in range(n)]


def _guards_intact(buf, c, n):
    m = c["ncol"] * (c["nlay"] + 1)
    b = buf.cpu().numpy()
    keep = np.ones(b.size, bool)
    for i in range(n):
        keep[GUARD + i * (m + GUARD):GUARD + i * (m + GUARD) + m] = False
    return np.isnan(b[keep]).all() and keep.sum() == (n + 1) * GUARD


def _arm(c, d, aer, mask):
    L = _L()
    if aer:
        assert L.rrtmgpnn_solver_request_aerosol(_ctx(), c["nb"], c["nlay"], c["ncol"], P(d["at"]), P(d["aw"]),
                                                 P(d["ag"])) == 0, _err()
    if mask is not None:
        assert L.rrtmgpnn_solver_request_cloud_mask(_ctx(), c["ng"], c["nlay"], c["ncol"], P(d["bits"][mask])) == 0, _err()


def dual(c, dev, top_at_1, with_g=False, aer=False, mask=None, dif=False, rfmip=False, check=True, guards=False):
    """The new entry -> the six arrays (up, dn, dir, up_clr, dn_clr, dir_clr).  mask: index into the case's masks."""
    from rrtmgpnn._lib import int_array
    L, d = _L(), _dev(c, dev)
    buf, outs = _outs(c, dev, 6)
    _arm(c, d, aer, mask)
    gg = P(d["g"]) if with_g else None
    lims = int_array(c["lims"].ravel())
    if rfmip:
        scr = [torch.empty((c["ncol"], c["ng"]), device=dev), torch.empty((c["ncol"], c["ng"]), device=dev),
               torch.empty(c["ncol"], device=dev)]
        rc = L.rrtmgpnn_sw_solver_2stream_rfmip_clr_all(
            _ctx(), c["ng"], c["nlay"], c["ncol"], int(top_at_1), P(d["solar"]), P(d["tsi"]), P(d["sfc_alb"]),
            P(d["sza"]), P(d["tau"]), P(d["ssa"]), gg, c["nb"], lims, P(d["bt"]), P(d["bw"]), P(d["bg"]),
            *[P(s) for s in scr], *[P(o) for o in outs])
    else:
        rc = L.rrtmgpnn_sw_solver_2stream_clr_all(
            _ctx(), c["ng"], c["nlay"], c["ncol"], int(top_at_1), P(d["inc"]), P(d["inc_dif"]) if dif else None,
            P(d["tau"]), P(d["ssa"]), gg, c["nb"], lims, P(d["bt"]), P(d["bw"]), P(d["bg"]), P(d["mu0"]), P(d["alb"]),
            P(d["alb"]), *[P(o) for o in outs])
    torch.cuda.synchronize()
    res = [o.cpu().numpy() for o in outs]
    if not check:
        return rc, res
    assert rc == 0, _err()
    if guards:
        assert _guards_intact(buf, c, 6), "a store outside the six flux arrays"
    return res


def single(c, dev, top_at_1, with_g=False, inc=None, aer=False, mask=None, dif=False, bc=None):
    """The existing entries: sw_solver_2stream (inc None) or _2stream_inc with the band triple `inc` ("cloud" or "aer"),
    with the aerosol / mask requests -> (up, dn, dir).  bc: device (mu0, inc_flux, alb) instead of the case's."""
    from rrtmgpnn._lib import int_array
    L, d = _L(), _dev(c, dev)
    _, outs = _outs(c, dev, 3)
    gg = P(d["g"]) if with_g else None
    mu0, toa, alb = (d["mu0"], d["inc"], d["alb"]) if bc is None else bc
    head = (_ctx(), c["ng"], c["nlay"], c["ncol"], int(top_at_1), P(toa), P(d["inc_dif"]) if dif else None,
            P(d["tau"]), P(d["ssa"]), gg)
    if inc is None:
        rc = L.rrtmgpnn_sw_solver_2stream(*head, P(mu0), P(alb), P(alb), *[P(o) for o in outs])
    else:
        _arm(c, d, aer, mask)
        b = (d["bt"], d["bw"], d["bg"]) if inc == "cloud" else (d["at"], d["aw"], d["ag"])
        rc = L.rrtmgpnn_sw_solver_2stream_inc(*head, c["nb"], int_array(c["lims"].ravel()), *[P(x) for x in b], P(mu0),
                                              P(alb), P(alb), *[P(o) for o in outs])
    torch.cuda.synchronize()
    assert rc == 0, _err()
    return [o.cpu().numpy() for o in outs]


def same(got, want, what):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(g, w, err_msg="%s [%d]" % (what, i))


# ---- against the oracle, mode 1 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncol", [1, S.NCOL])
@pytest.mark.parametrize("top_at_1", [True, False], ids=["top1", "top0"])
@pytest.mark.parametrize("nlay", S.NLAYS)
def test_dual_against_the_oracle(dev, orc, mode, nlay, top_at_1, ncol):
    mode(1)
    c = S.nn_case(orc, nlay, ncol)
    assert c["ng"] == 224
    same(dual(c, dev, top_at_1, guards=True), S.expect(orc, c, top_at_1), "nlay %d" % nlay)


def test_dual_with_a_diffuse_incident_flux(dev, orc, mode):
    mode(1)
    c = S.nn_case(orc, 10)
    for top_at_1 in (True, False):
        same(dual(c, dev, top_at_1, dif=True), S.expect(orc, c, top_at_1, dif=True), "inc_flux_dif")


# ---- against the existing entries ---------------------------------------------------------------------------------------
VARIANTS = {"plain": {}, "gas_g": {"with_g": True}, "mask": {"mask": 0}, "aer": {"aer": True},
            "mask_aer": {"mask": 0, "aer": True}, "gas_g_mask_aer": {"with_g": True, "mask": 0, "aer": True}}


def _existing(c, dev, top_at_1, with_g=False, aer=False, mask=None, bc=None):
    alls = single(c, dev, top_at_1, with_g, "cloud", aer, mask, bc=bc)
    clear = single(c, dev, top_at_1, with_g, "aer" if aer else None, bc=bc)
    return alls + clear


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("top_at_1", [True, False], ids=["top1", "top0"])
@pytest.mark.parametrize("nlay", [7, 19])
def test_dual_against_the_existing_entries(dev, orc, mode, nlay, top_at_1, variant):
    mode(1)
    c = S.nn_case(orc, nlay)
    kw = VARIANTS[variant]
    got = dual(c, dev, top_at_1, **kw)
    same(got, _existing(c, dev, top_at_1, **kw), variant)
    m = None if kw.get("mask") is None else c["masks"][kw["mask"]]
    same(got, S.expect(orc, c, top_at_1, kw.get("with_g", False), kw.get("aer", False), m), variant + " (oracle)")


@pytest.mark.parametrize("aer", [False, True], ids=["noaer", "aer"])
def test_the_mask_leaves_the_clear_set_untouched(dev, orc, mode, aer):
    mode(1)
    c = S.nn_case(orc, 19)
    assert (c["masks"][0] != c["masks"][1]).any()
    a, b, n = (dual(c, dev, True, aer=aer, mask=m) for m in (0, 1, None))
    same(a[3:], b[3:], "clear set under two masks")
    same(a[3:], n[3:], "clear set with and without a mask")
    assert (a[1] != b[1]).any() and (a[1] != n[1]).any(), "the masks do not show in the all-sky set"


# ---- band layouts -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["plain", "gas_g_mask_aer"])
@pytest.mark.parametrize("ngpt", sorted(S.LAYOUTS))
def test_dual_band_layouts(dev, orc, mode, ngpt, variant):
    mode(1)
    c = S.seeded_case(orc, ngpt, S.LAYOUTS[ngpt])
    kw = VARIANTS[variant]
    m = None if kw.get("mask") is None else c["masks"][kw["mask"]]
    for top_at_1 in (True, False):
        got = dual(c, dev, top_at_1, guards=True, **kw)
        same(got, S.expect(orc, c, top_at_1, kw.get("with_g", False), kw.get("aer", False), m), "ngpt %d" % ngpt)


# ---- modes --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["plain", "mask_aer"])
def test_modes_agree(dev, orc, mode, variant):
    c = S.nn_case(orc, 19)
    kw = VARIANTS[variant]
    res = {}
    for m in (1, 2, 0):
        mode(m)
        res[m] = dual(c, dev, True, guards=True, **kw) + dual(c, dev, False, rfmip=True, **kw)
    same(res[2], res[1], "mode 2 against mode 1")
    same(res[0], res[1], "the default mode against mode 1")
    # ... and mode 2 when the checkpointed kernel is not the context's SW kernel (unmasked: the other kernels take no mask)
    if variant == "plain":
        from rrtmgpnn import api
        mode(1)
        api.set_sw_kernel_default(2)
        try:
            other = dual(c, dev, True, **kw) + dual(c, dev, False, rfmip=True, **kw)
        finally:
            api.set_sw_kernel_default(0)
        same(other, res[1], "SW kernel mode 2")


def test_rfmip_form_is_boundary_plus_the_plain_entry(dev, orc, mode):
    """_rfmip_clr_all == sw_boundary_rfmip + the dual entry, with columns at and past the usecol bound (mu0 = 1)."""
    mode(1)
    c = S.nn_case(orc, 10)
    d = _dev(c, dev)
    assert (c["sza"] >= 90).sum() >= 2
    toa, alb = torch.empty((c["ncol"], c["ng"]), device=dev), torch.empty((c["ncol"], c["ng"]), device=dev)
    mu0 = torch.empty(c["ncol"], device=dev)
    assert _L().rrtmgpnn_sw_boundary_rfmip(_ctx(), c["ng"], c["ncol"], P(d["solar"]), P(d["tsi"]), P(d["sfc_alb"]),
                                           P(d["sza"]), P(toa), P(alb), P(mu0)) == 0, _err()
    assert (mu0.cpu().numpy()[c["sza"] >= 90] == 1).all()
    for kw in ({}, {"mask": 1, "aer": True}):
        for top_at_1 in (True, False):
            got = dual(c, dev, top_at_1, rfmip=True, guards=True, **kw)
            same(got, _existing(c, dev, top_at_1, bc=(mu0, toa, alb), **kw), "rfmip form")
            m = None if kw.get("mask") is None else c["masks"][kw["mask"]]
            bc = (mu0.cpu().numpy(), toa.cpu().numpy(), alb.cpu().numpy())
            same(got, S.expect(orc, c, top_at_1, aer=kw.get("aer", False), mask=m, bc=bc), "rfmip form (oracle)")


def test_workspace_is_shared_with_the_single_entries(dev, orc, mode):
    """One context: the single entry, then the dual at a larger shape (its checkpoints are twice as wide), then the
    single again."""
    mode(1)
    small, big = S.nn_case(orc, 7), S.nn_case(orc, 28)
    want_s, want_b = S.expect(orc, small, True), S.expect(orc, big, True)
    same(single(small, dev, True, inc="cloud"), want_s[:3], "single, before")
    same(dual(big, dev, True), want_b, "dual at the larger shape")
    same(single(small, dev, True, inc="cloud"), want_s[:3], "single, after")
    same(single(big, dev, True), want_b[3:], "single clear at the larger shape")
    same(dual(small, dev, True), want_s, "dual at the smaller shape")


CHILD = r"""
import sys, numpy as np, torch
sys.path.insert(0, %(tests)r); sys.path.insert(0, %(pkg)r); sys.path.insert(0, %(oracle)r)
import oracle, test_gpu_sw_clr_all as G, sw_clr_all_cases as S
from rrtmgpnn import api
api.set_sw_clr_all_default(1)
dev = torch.device("cuda", 0)
c = S.nn_case(oracle.Oracle(), 19)
out = {}
for name, kw in sorted(G.VARIANTS.items()):
    for i, a in enumerate(G.dual(c, dev, True, guards=True, **kw)):
        out["%%s_%%d" %% (name, i)] = a
np.savez(%(out)r, **out)
"""


def test_dual_without_the_plane_workspace(dev, orc, mode, tmp_path):
    """With the planes' workspace denied (RRTMGPNN_SW_NO_PLANES=1, read once per process: a child), the plane-free dual
    instances give the same bits as the ones with planes."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / "noplanes.npz")
    code = CHILD % {"tests": os.path.join(root, "tests"), "pkg": os.path.join(root, "rte-rrtmgp-nn_amd"),
                    "oracle": os.path.join(root, "oracle"), "out": out}
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, RRTMGPNN_SW_NO_PLANES="1"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = dict(np.load(out))
    assert len(got) == 6 * len(VARIANTS)
    mode(1)
    c = S.nn_case(orc, 19)
    for name, kw in sorted(VARIANTS.items()):
        for i, w in enumerate(dual(c, dev, True, **kw)):
            np.testing.assert_array_equal(got["%s_%d" % (name, i)], w, err_msg="%s [%d]" % (name, i))


# ---- refusals -------------------------------------------------------------------------------------------------------------
def test_refusals_clear_the_requests(dev, orc, mode):
    from rrtmgpnn._lib import int_array
    mode(1)
    c = S.nn_case(orc, 7)
    L, d = _L(), _dev(c, dev)
    ng, nlay, ncol, nb = c["ng"], c["nlay"], c["ncol"], c["nb"]
    want = S.expect(orc, c, True)
    bnd = [torch.full((ncol, nlay + 1, nb), NAN, device=dev) for _ in range(3)]
    jac_in, jac_out = torch.zeros((ncol, ng), device=dev), torch.zeros((ncol, nlay + 1), device=dev)

    def byband():
        assert L.rrtmgpnn_solver_request_byband(_ctx(), nb, int_array(c["lims"].ravel()), *[P(b) for b in bnd]) == 0

    def byband_mcica():
        assert L.rrtmgpnn_solver_request_byband_mcica(_ctx(), nb, int_array(c["lims"].ravel()), *[P(b) for b in bnd], ng,
                                                      nlay, ncol, P(d["bits"][0])) == 0, _err()

    def jacobian():
        assert L.rrtmgpnn_solver_request_jacobian(_ctx(), ng, nlay, ncol, P(jac_in), P(jac_out)) == 0, _err()

    def aer_1scl():
        assert L.rrtmgpnn_solver_request_aerosol(_ctx(), nb, nlay, ncol, P(d["at"]), None, None) == 0, _err()

    def aer_extents():
        assert L.rrtmgpnn_solver_request_aerosol(_ctx(), nb, nlay + 1, ncol, P(d["at"]), P(d["aw"]), P(d["ag"])) == 0

    def mask_extents():
        assert L.rrtmgpnn_solver_request_cloud_mask(_ctx(), ng, nlay, ncol + 1, P(d["bits"][0])) == 0, _err()

    armed = [(byband, ERR_ARGUMENT, "by-band outputs are not available from this entry"),
             (byband_mcica, ERR_ARGUMENT, "by-band outputs are not available from this entry"),
             (jacobian, ERR_ARGUMENT, "no flux Jacobian from this entry"),
             (aer_1scl, ERR_ARGUMENT, "a shortwave entry takes a 2str aerosol"),
             (aer_extents, ERR_ARGUMENT, "the requested aerosol's extents"),
             (mask_extents, ERR_ARGUMENT, "the requested cloud mask's extents")]
    for rfmip in (False, True):
        for arm, status, text in armed:
            arm()
            rc, res = dual(c, dev, True, rfmip=rfmip, check=False)
            assert rc == status and text in _err(), (arm.__name__, rc, _err())
            assert all(np.isnan(r).all() for r in res), "a refused call wrote fluxes"
            # the request is gone: the plain entry and the dual run as if nothing had been armed
            same(single(c, dev, True), want[3:], "plain entry after a refused %s" % arm.__name__)
            if not rfmip:
                same(dual(c, dev, True), want, "dual after a refused %s" % arm.__name__)
    assert np.isnan(jac_out.cpu().numpy()).sum() == 0 and all(torch.isnan(b).all() for b in bnd)


def _shape_call(dev, ng, nb, lims, rfmip):
    from rrtmgpnn._lib import int_array
    L = _L()
    nlay, ncol = 3, 2
    z = lambda *s: torch.full(s, 0.5, device=dev)  # noqa: E731
    outs = [torch.full((ncol, nlay + 1), NAN, device=dev) for _ in range(6)]
    li = int_array(np.asarray(lims, np.int32).ravel()) if nb else None
    b = [P(z(ncol, nlay, max(nb, 1))) for _ in range(3)]
    if rfmip:
        rc = L.rrtmgpnn_sw_solver_2stream_rfmip_clr_all(
            _ctx(), ng, nlay, ncol, 1, P(z(ng)), P(z(ncol)), P(z(ncol)), P(z(ncol)), P(z(ncol, nlay, ng)),
            P(z(ncol, nlay, ng)), None, nb, li, *b, P(z(ncol, ng)), P(z(ncol, ng)), P(z(ncol)), *[P(o) for o in outs])
    else:
        rc = L.rrtmgpnn_sw_solver_2stream_clr_all(
            _ctx(), ng, nlay, ncol, 1, P(z(ncol, ng)), None, P(z(ncol, nlay, ng)), P(z(ncol, nlay, ng)), None, nb, li, *b,
            P(z(ncol)), P(z(ncol, ng)), P(z(ncol, ng)), *[P(o) for o in outs])
    torch.cuda.synchronize()
    assert all(torch.isnan(o).all() for o in outs)
    return rc


@pytest.mark.parametrize("rfmip", [False, True], ids=["plain", "rfmip"])
@pytest.mark.parametrize("m", [1, 2])
def test_shape_refusals(dev, orc, mode, m, rfmip):
    """nbnd == 0, odd ngpt and ngpt > 256, each with a cloud-mask and an aerosol request armed: the refusal is the
    shape's, and the requests are gone afterwards -- the plain entry, which refuses either request, then gives the
    oracle's clear set on a real case."""
    mode(m)
    c = S.nn_case(orc, 7)
    d = _dev(c, dev)
    want = S.expect(orc, c, True)[3:]
    for ng, nb, lims, status, text in ((16, 0, None, ERR_ARGUMENT, "needs the band increment (nbnd > 0)"),
                                       (15, 1, [(1, 15)], ERR_UNSUPPORTED, "ngpt must be even and at most 256"),
                                       (258, 1, [(1, 258)], ERR_UNSUPPORTED, "ngpt must be even and at most 256")):
        _arm(c, d, True, 0)
        assert _shape_call(dev, ng, nb, lims, rfmip) == status and text in _err(), (ng, nb, _err())
        same(single(c, dev, True), want, "plain entry after the refusal of ngpt %d, nbnd %d" % (ng, nb))
    assert _shape_call(dev, 16, 1, [(1, 15)], rfmip) == ERR_ARGUMENT and "outside every band" in _err()
    # what an armed request does to the plain entry, i.e. what the calls above would have met had one been left
    _arm(c, d, False, 0)
    _, outs = _outs(c, dev, 3)
    assert _L().rrtmgpnn_sw_solver_2stream(_ctx(), c["ng"], c["nlay"], c["ncol"], 1, P(d["inc"]), None, P(d["tau"]),
                                           P(d["ssa"]), None, P(d["mu0"]), P(d["alb"]), P(d["alb"]),
                                           *[P(o) for o in outs]) == ERR_ARGUMENT and "takes no cloud mask" in _err()


def test_two_launches_with_an_aerosol_need_the_band_pair_layout(dev, orc, mode):
    """Mode 2 runs the single-sky aerosol instances, which need every band to start at an odd 1-based g-point: on the
    18-g-point layout (starts 1, 6, 12) an aerosol request is refused there (and the request cleared), where the dual
    kernel takes it; without an aerosol both modes take the layout and agree."""
    c = S.seeded_case(orc, 18, S.LAYOUTS[18])
    mode(2)
    rc, res = dual(c, dev, True, aer=True, check=False)
    assert rc == ERR_UNSUPPORTED and "band-pair layout" in _err(), (rc, _err())
    assert all(np.isnan(r).all() for r in res)
    same(dual(c, dev, True, mask=0), S.expect(orc, c, True, mask=c["masks"][0]), "mode 2, no aerosol")
    mode(1)
    same(dual(c, dev, True, aer=True), S.expect(orc, c, True, aer=True), "mode 1 with the aerosol")


def test_dual_lane_flush_with_short_rows(dev, orc, mode):
    """20 g-points in a block of 64 lanes: with two layers every flush (one level, then two) fits the one-lane-per-partial
    flush, which then walks rows of five partial terms for two skies."""
    mode(1)
    c = S.seeded_case(orc, 20, S.LAYOUTS[20], nlay=2)
    for kw in ({}, {"with_g": True, "mask": 0, "aer": True}):
        m = None if kw.get("mask") is None else c["masks"][kw["mask"]]
        for top_at_1 in (True, False):
            got = dual(c, dev, top_at_1, guards=True, **kw)
            same(got, S.expect(orc, c, top_at_1, kw.get("with_g", False), kw.get("aer", False), m), "nlay 2")


def test_mode_argument(dev):
    L = _L()
    assert L.rrtmgpnn_context_set_sw_clr_all(_ctx(), 3) == ERR_ARGUMENT and "sw clr_all mode must be 0, 1 or 2" in _err()
    assert L.rrtmgpnn_context_set_sw_clr_all(None, -1) == ERR_ARGUMENT
