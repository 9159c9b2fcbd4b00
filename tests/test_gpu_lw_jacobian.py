"""GPU: flux_up_Jac, the Jacobian of the upward LW flux with respect to the surface temperature, carried through the
solvers' up pass (rrtmgpnn_solver_request_jacobian; kJac instances of lw_noscat_kernel and lw_rescl_kernel), bit for bit:

* every entry that honours the request -- lw_solver_noscat, _noscat_gpt with lw_Ds and null g-point arrays, _noscat_planck,
  _noscat_planck_inc overcast and under a McICA mask, lw_solver_1rescl -- against the oracle's flux_up on zero sources
  with sfc_source_Jac as the surface source (tests/lw_jacobian_ref.py), with flux_up / flux_dn those of the same call
  without the request and guard floats either side of flux_up_Jac intact;
* the request's lifecycle: cleared by the call it serves, every refusal with its message, extents, the NULL / non-NULL rule
  of sfc_source_Jac, ncol = 0.
"""
import numpy as np
import pytest

import lw_jacobian_ref as J

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GUARD = 64  # floats either side of flux_up_Jac
SENTINEL = -12345.5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a device"
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def T(a, dev):
    a = np.array(a, order="C", copy=True)
    return torch.as_tensor(a.view(np.int32) if a.dtype == np.uint32 else a, device=dev)


def P(t):
    return None if t is None else t.data_ptr()


def _lib_ctx():
    from rrtmgpnn import _lib
    from rrtmgpnn.api import context
    return _lib.lib(), context(0).h


def last_error():
    from rrtmgpnn import _lib
    return _lib.lib().rrtmgpnn_last_error().decode()


class Call:
    """One solver entry on device copies of a case's arrays: run(request) -> (rc, flux_up, flux_dn, flux_up_Jac with its
    guards); request: None, or "sources" / "null" for what is passed as sfc_source_Jac."""

    def __init__(self, entry, a, dev, top_at_1, nmus, gpt=False, ncol=None):
        from rrtmgpnn._lib import float_array, int_array
        from rrtmgpnn.api import GAUSS_DS, GAUSS_WTS
        self.entry, self.dev, self.gpt = entry, dev, gpt
        self.ncol, self.nlay, self.ngpt = a["tau"].shape
        if ncol is not None:
            self.ncol = ncol  # the arrays' leading columns
        self.d = {k: T(v, dev) for k, v in a.items() if isinstance(v, np.ndarray)}
        L, ctx = _lib_ctx()
        self.L, self.ctx = L, ctx
        d = self.d
        head = (ctx, self.ngpt, self.nlay, self.ncol, int(top_at_1), nmus, float_array(GAUSS_DS[nmus]),
                float_array(GAUSS_WTS[nmus]))
        if entry in ("planck", "planck_inc", "planck_inc_mask"):
            kd = a["kd"]
            tail = (kd["nband"], kd["nPlanckTemp"], P(d["tlay"]), P(d["tlev"]), P(d["tsfc"]), a["sfc_lay"],
                    int_array(np.asarray(a["lims"]).ravel()), float(kd["temp_ref_min"][0]), float(kd["totplnk_delta"]),
                    P(d["totplnk"]), 0, P(d["emis"]))
            if entry == "planck":
                self.fn = lambda o: L.rrtmgpnn_lw_solver_noscat_planck(*head, None, P(d["tau"]), P(d["pfrac"]), *tail, *o)
            else:
                self.fn = lambda o: L.rrtmgpnn_lw_solver_noscat_planck_inc(*head, None, P(d["tau"]), P(d["cld"]),
                                                                          P(d["pfrac"]), *tail, *o)
        elif entry == "noscat":
            self.fn = lambda o: L.rrtmgpnn_lw_solver_noscat(*head, None, P(d["tau"]), P(d["lay"]), P(d["lev"]),
                                                            P(d["emis"]), P(d["sfc"]), *o)
        elif entry == "noscat_gpt_Ds":
            self.fn = lambda o: L.rrtmgpnn_lw_solver_noscat_gpt(*head, P(d["lw_Ds"]), None, P(d["tau"]), P(d["lay"]),
                                                                P(d["lev"]), P(d["emis"]), P(d["sfc"]), *o,
                                                                *(self._gpt_out() if gpt else (None, None)))
        elif entry == "rescl":
            self.fn = lambda o: L.rrtmgpnn_lw_solver_1rescl(*head, None, P(d["tau"]), P(d["ssa"]), P(d["g"]), P(d["lay"]),
                                                            P(d["lev"]), P(d["emis"]), P(d["sfc"]), *o)
        else:
            raise KeyError(entry)

    def _gpt_out(self):
        self.g = [torch.zeros(self.ncol, self.nlay + 1, self.ngpt, device=self.dev) for _ in range(2)]
        return [P(t) for t in self.g]

    def jac_buffer(self):
        return torch.full((2 * GUARD + self.ncol * (self.nlay + 1),), SENTINEL, device=self.dev)

    def arm(self, buf, request, ext=None):
        sj = P(self.d["sjac"]) if request == "sources" else None
        ext = ext or (self.ngpt, self.nlay, self.ncol)
        return self.L.rrtmgpnn_solver_request_jacobian(self.ctx, *ext, sj, buf.data_ptr() + 4 * GUARD)

    def arm_mask(self):
        from rrtmgpnn._lib import check
        check(self.L.rrtmgpnn_solver_request_cloud_mask(self.ctx, self.ngpt, self.nlay, self.ncol, P(self.d["bits"])))

    def run(self, request=None, buf=None):
        from rrtmgpnn._lib import check
        buf = self.jac_buffer() if buf is None else buf
        if self.entry == "planck_inc_mask":
            self.arm_mask()
        if request is not None:
            check(self.arm(buf, request), "solver_request_jacobian")
        rows = max(self.ncol, 1)  # ncol = 0: the outputs are still arrays
        up, dn = (torch.full((rows, self.nlay + 1), float("nan"), device=self.dev) for _ in range(2))
        rc = self.fn((P(up), P(dn)))
        torch.cuda.synchronize()
        return rc, up[:self.ncol].cpu().numpy(), dn[:self.ncol].cpu().numpy(), buf.cpu().numpy()


def check_jacobian(call, request, want_up, want_dn, want_jac):
    rc0, up0, dn0, untouched = call.run(None)
    assert rc0 == 0, last_error()
    assert (untouched == SENTINEL).all()
    rc, up, dn, buf = call.run(request)
    assert rc == 0, last_error()
    n = call.ncol * (call.nlay + 1)
    assert (buf[:GUARD] == SENTINEL).all() and (buf[GUARD + n:] == SENTINEL).all(), "guard floats overwritten"
    np.testing.assert_array_equal(buf[GUARD:GUARD + n].reshape(call.ncol, call.nlay + 1), want_jac)
    np.testing.assert_array_equal(up, up0)
    np.testing.assert_array_equal(dn, dn0)
    np.testing.assert_array_equal(up, want_up)
    np.testing.assert_array_equal(dn, want_dn)
    assert (want_jac > 0).all()


def fused_arrays(case, route):
    return dict(tau=case["tau"], pfrac=case["pfrac"], cld=case["cld"], emis=case["emis"], bits=case["bits"],
                tlay=np.asarray(case["prob"]["tlay"], np.float32), tlev=np.asarray(case["tlev"], np.float32),
                tsfc=np.asarray(case["prob"]["tsfc"], np.float32), totplnk=np.asarray(case["kd"]["totplnk"], np.float32),
                kd=case["kd"], lims=case["lims"], sfc_lay=case["sfc_lay"])


def extras(shape, seed):
    """Scattering properties and per-(g-point, column) secants for a case of this shape."""
    ncol, nlay, ngpt = shape
    rng = np.random.default_rng(seed)
    u = lambda lo, hi, *s: rng.uniform(lo, hi, s).astype(np.float32)  # noqa: E731
    return dict(ssa=u(0.0, 0.9, ncol, nlay, ngpt), g=u(0.0, 0.9, ncol, nlay, ngpt), lw_Ds=u(1.2, 2.2, ncol, ngpt))


@pytest.mark.parametrize("ngpt", [256, 254])
@pytest.mark.parametrize("top_at_1", [True, False])
@pytest.mark.parametrize("nlay", J.NLAYS)
def test_fused_entries(dev, orc, nlay, top_at_1, ngpt):
    """_planck, _planck_inc overcast and _planck_inc under a mask request (the oracle's tau incremented on the host where
    the mask bit is set), 1 and 3 angles: sfc_source_Jac is formed in-kernel from B_b(tsfc + 1)."""
    case = J.solver_case(orc, nlay, top_at_1, None if ngpt == 256 else ngpt)
    assert (case["taus"]["masked"] != case["taus"]["clear"]).any() and (case["taus"]["masked"] != case["taus"]["overcast"]).any()
    for nmus in (1, 3):
        for entry, route in (("planck", "clear"), ("planck_inc", "overcast"), ("planck_inc_mask", "masked")):
            call = Call(entry, fused_arrays(case, route), dev, top_at_1, nmus)
            check_jacobian(call, "null", *J.expect(orc, case, route, top_at_1, nmus))


@pytest.mark.parametrize("ngpt", [256, 254])
@pytest.mark.parametrize("top_at_1", [True, False])
@pytest.mark.parametrize("nlay", J.NLAYS)
def test_source_array_entries(dev, orc, nlay, top_at_1, ngpt):
    """lw_solver_noscat (1 and 3 angles), _noscat_gpt with lw_Ds and null g-point arrays (one angle), lw_solver_1rescl
    (1 and 3 angles) on the NN gas optics' sources."""
    case = J.solver_case(orc, nlay, top_at_1, None if ngpt == 256 else ngpt)
    a = dict(tau=case["tau"], lay=case["lay"], lev=case["lev"], sfc=case["sfc"], sjac=case["sjac"], emis=case["emis"],
             **extras(case["tau"].shape, 900 + nlay))
    _source_entries(dev, orc, a, top_at_1)


@pytest.mark.parametrize("top_at_1", [True, False])
@pytest.mark.parametrize("nlay", J.NLAYS)
def test_source_array_entries_one_wave(dev, orc, nlay, top_at_1):
    """62 g-points on random arrays: one wave, not a multiple of 4 (the bare J summed sequentially at one angle)."""
    _source_entries(dev, orc, J.random_case(62, nlay, seed=40 + nlay, scat=True), top_at_1)


def _source_entries(dev, orc, a, top_at_1):
    src = (a["tau"], a["lay"], a["lev"], a["emis"], a["sfc"], top_at_1)
    jin = (a["tau"], a["emis"], a["sjac"], top_at_1)
    for nmus in (1, 3):
        up, dn = orc.lw_solver(*src, nmus)
        check_jacobian(Call("noscat", a, dev, top_at_1, nmus), "sources", up, dn, J.zero_source_flux_up(orc, *jin, nmus))
        up, dn = orc.lw_solver(*src, nmus, ssa=a["ssa"], g=a["g"])
        check_jacobian(Call("rescl", a, dev, top_at_1, nmus), "sources", up, dn,
                       J.zero_source_flux_up(orc, *jin, nmus, ssa=a["ssa"], g=a["g"]))
    up, dn = orc.lw_solver(*src, 1, lw_Ds=a["lw_Ds"])
    check_jacobian(Call("noscat_gpt_Ds", a, dev, top_at_1, 1), "sources", up, dn,
                   J.zero_source_flux_up(orc, *jin, 1, lw_Ds=a["lw_Ds"]))


# ---- lifecycle -----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def small(orc):
    case = J.solver_case(orc, 5, True)
    a = dict(tau=case["tau"], lay=case["lay"], lev=case["lev"], sfc=case["sfc"], sjac=case["sjac"], emis=case["emis"],
             **extras(case["tau"].shape, 77))
    return case, a


def test_request_is_cleared_by_the_call_it_serves(dev, orc, small):
    case, a = small
    call = Call("noscat", a, dev, True, 1)
    rc, _, _, buf = call.run("sources")
    assert rc == 0 and (buf[GUARD:-GUARD] != SENTINEL).all()
    rc, _, _, buf = call.run(None)  # a fresh sentinel-filled array that was never armed ...
    assert rc == 0 and (buf == SENTINEL).all()
    again = call.jac_buffer()
    assert call.arm(again, "sources") == 0
    assert call.L.rrtmgpnn_solver_request_jacobian(call.ctx, 0, 0, 0, None, None) == 0  # disarms
    rc, _, _, _ = call.run(None)
    assert rc == 0 and (again.cpu().numpy() == SENTINEL).all()


def _refused(call, request, text, buf=None, ext=None):
    """Arm, run: refused with `text` in the message and nothing written; then the same call runs unarmed."""
    buf = call.jac_buffer() if buf is None else buf
    assert call.arm(buf, request, ext) == 0
    up, dn = (torch.full((call.ncol, call.nlay + 1), float("nan"), device=call.dev) for _ in range(2))
    rc = call.fn((P(up), P(dn)))
    torch.cuda.synchronize()
    assert rc != 0 and text in last_error(), (rc, last_error())
    assert (buf.cpu().numpy() == SENTINEL).all() and torch.isnan(up).all()
    rc = call.fn((P(up), P(dn)))  # cleared: runs, and writes no Jacobian
    torch.cuda.synchronize()
    assert rc == 0, last_error()
    assert (buf.cpu().numpy() == SENTINEL).all() and not torch.isnan(up).any()


def test_null_rule_and_extents(dev, orc, small):
    case, a = small
    for entry in ("noscat", "noscat_gpt_Ds", "rescl"):
        _refused(Call(entry, a, dev, True, 1), "null", "lw_solver_" + ("1rescl" if entry == "rescl" else "noscat"))
    fa = fused_arrays(case, "clear") | {"sjac": case["sjac"]}
    for entry in ("planck", "planck_inc"):
        _refused(Call(entry, fa, dev, True, 1), "sources", "lw_solver_noscat_" + entry)
    ncol, nlay, ngpt = a["tau"].shape
    for ext in ((ngpt - 1, nlay, ncol), (ngpt, nlay + 1, ncol), (ngpt, nlay, ncol - 1)):
        _refused(Call("noscat", a, dev, True, 1), "sources", "extents", ext=ext)
        _refused(Call("planck", fa, dev, True, 3), "null", "extents", ext=ext)
    L, ctx = _lib_ctx()
    buf = torch.zeros(8, device=dev)
    assert L.rrtmgpnn_solver_request_jacobian(ctx, 0, nlay, ncol, None, P(buf)) != 0
    assert L.rrtmgpnn_solver_request_jacobian(ctx, ngpt, 0, ncol, None, P(buf)) != 0
    assert L.rrtmgpnn_solver_request_jacobian(ctx, ngpt, nlay, -1, None, P(buf)) != 0


def test_gpoint_outputs_and_byband_are_refused(dev, orc, small):
    from rrtmgpnn._lib import check, int_array
    case, a = small
    _refused_gpt = Call("noscat_gpt_Ds", a, dev, True, 1, gpt=True)
    buf = _refused_gpt.jac_buffer()
    assert _refused_gpt.arm(buf, "sources") == 0
    up, dn = (torch.zeros(_refused_gpt.ncol, _refused_gpt.nlay + 1, device=dev) for _ in range(2))
    assert _refused_gpt.fn((P(up), P(dn))) != 0 and "g-point outputs" in last_error()
    assert (buf.cpu().numpy() == SENTINEL).all()
    # by-band, plain or paired with a mask
    L, ctx = _lib_ctx()
    lims = int_array(np.asarray(case["lims"]).ravel())
    nb = len(case["lims"])
    ncol, nlay, ngpt = a["tau"].shape
    bnd = [torch.zeros(ncol, nlay + 1, nb, device=dev) for _ in range(2)]
    fa = fused_arrays(case, "clear")
    for entry, request, paired in (("noscat", "sources", False), ("planck", "null", False), ("planck_inc", "null", True)):
        call = Call(entry, a if entry == "noscat" else fa, dev, True, 1)
        buf = call.jac_buffer()
        if paired:
            check(L.rrtmgpnn_solver_request_byband_mcica(ctx, nb, lims, P(bnd[0]), P(bnd[1]), None, ngpt, nlay, ncol,
                                                         P(call.d["bits"])))
        else:
            check(L.rrtmgpnn_solver_request_byband(ctx, nb, lims, P(bnd[0]), P(bnd[1]), None))
        assert call.arm(buf, request) == 0
        assert call.fn((P(up), P(dn))) != 0 and "by-band" in last_error(), last_error()
        rc, _, _, b2 = call.run(None)  # both cleared
        assert rc == 0 and (b2 == SENTINEL).all() and (buf.cpu().numpy() == SENTINEL).all()
        assert not any(t.any() for t in bnd)


def test_other_entries_refuse(dev, orc, small):
    """lw_solver_2stream (the reference's text), the _clr_all entries and the SW entries: refused, naming the entry, and
    cleared."""
    from rrtmgpnn._lib import float_array, int_array
    from rrtmgpnn.api import GAUSS_DS, GAUSS_WTS
    case, a = small
    L, ctx = _lib_ctx()
    ncol, nlay, ngpt = a["tau"].shape
    d = {k: T(v, dev) for k, v in (a | fused_arrays(case, "clear")).items() if isinstance(v, np.ndarray)}
    d["mu0"] = torch.full((ncol,), 0.5, device=dev)
    d["zb"] = torch.zeros_like(d["cld"])  # band ssa and g of the SW increment
    out = [torch.full((ncol, nlay + 1), float("nan"), device=dev) for _ in range(4)]
    kd = case["kd"]
    head = (ctx, ngpt, nlay, ncol, 1)
    quad = (1, float_array(GAUSS_DS[1]), float_array(GAUSS_WTS[1]))
    lims = int_array(np.asarray(case["lims"]).ravel())
    tail = (kd["nband"], kd["nPlanckTemp"], P(d["tlay"]), P(d["tlev"]), P(d["tsfc"]), case["sfc_lay"], lims,
            float(kd["temp_ref_min"][0]), float(kd["totplnk_delta"]), P(d["totplnk"]), 0, P(d["emis"]))
    o = [P(t) for t in out]
    calls = {
        "rte_lw: can't provide Jacobian of fluxes w.r.t surface temperature with 2-stream":
            lambda: L.rrtmgpnn_lw_solver_2stream(*head, None, P(d["tau"]), P(d["ssa"]), P(d["g"]), P(d["lev"]),
                                                 P(d["emis"]), P(d["sfc"]), o[0], o[1]),
        "lw_solver_noscat_planck_clr_all:":
            lambda: L.rrtmgpnn_lw_solver_noscat_planck_clr_all(*head, *quad, None, P(d["tau"]), P(d["cld"]), P(d["pfrac"]),
                                                               *tail, *o),
        "lw_solver_noscat_planck_clr_all_mcica:":
            lambda: L.rrtmgpnn_lw_solver_noscat_planck_clr_all_mcica(*head, *quad, None, P(d["tau"]), P(d["cld"]),
                                                                     P(d["pfrac"]), *tail, *o, P(d["bits"])),
        "sw_solver_2stream:":
            lambda: L.rrtmgpnn_sw_solver_2stream(*head, P(d["sfc"]), None, P(d["tau"]), P(d["ssa"]), P(d["g"]), P(d["mu0"]),
                                                 P(d["emis"]), P(d["emis"]), o[0], o[1], o[2]),
        "sw_solver_noscat:":
            lambda: L.rrtmgpnn_sw_solver_noscat(*head, P(d["sfc"]), P(d["tau"]), P(d["mu0"]), o[2]),
        "sw_solver_2stream_inc:":
            lambda: L.rrtmgpnn_sw_solver_2stream_inc(*head, P(d["sfc"]), None, P(d["tau"]), P(d["ssa"]), P(d["g"]),
                                                     kd["nband"], lims, P(d["cld"]), P(d["zb"]), P(d["zb"]), P(d["mu0"]),
                                                     P(d["emis"]), P(d["emis"]), o[0], o[1], o[2]),
    }
    buf = torch.full((ncol * (nlay + 1),), SENTINEL, device=dev)
    for text, fn in calls.items():
        for sj in (P(d["sjac"]), None):
            assert L.rrtmgpnn_solver_request_jacobian(ctx, ngpt, nlay, ncol, sj, P(buf)) == 0
            assert fn() != 0 and text in last_error(), (text, last_error())
            for t in out:
                t.fill_(float("nan"))
            assert fn() == 0, (text, last_error())  # cleared: the entry runs
            torch.cuda.synchronize()
            assert not torch.isnan(out[2] if text.startswith("sw_solver_noscat") else out[0]).any()
    assert (buf.cpu().numpy() == SENTINEL).all()


def test_no_columns(dev, orc, small):
    case, a = small
    fa = fused_arrays(case, "clear")
    for entry, request in (("noscat", "sources"), ("rescl", "sources"), ("planck", "null"), ("planck_inc", "null")):
        for nmus in (1, 3):
            call = Call(entry, a if request == "sources" else fa, dev, True, nmus, ncol=0)
            rc, _, _, buf = call.run(request)
            assert rc == 0 and (buf == SENTINEL).all(), (entry, last_error())
            rc, _, _, buf = call.run(None)  # and the request is gone
            assert rc == 0 and (buf == SENTINEL).all()
