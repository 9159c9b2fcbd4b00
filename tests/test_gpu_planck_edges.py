"""GPU: every copy of interp1d (csrc/rte_device.hpp) at temperature and table edges, bit for bit against the oracle as
uint32 views (inputs and references: tests/planck_edges.py; the oracle's own pin: tests/test_planck_edges_host.py).

The copies: planck_source_kernel (rrtmgpnn_compute_planck_source_nn: four layers per block, pfrac overwritten in place);
the band-table loop in the prologue of lw_noscat_kernel's fused instances (the rrtmgpnn_lw_solver_noscat_planck* entries;
the Jacobian instances add a B_b(tsfc + 1) row); its second copy in lw_rescl_planck_inc_kernel (the
rrtmgpnn_lw_solver_1rescl_planck_* entries); bc_flux_kernel (rrtmgpnn_compute_bc_lw).  Each runs on four Planck tables
-- the shipped one, whose step is exactly 1, and three synthetic ones whose steps are 0.7, 50 and 3, so that a
reciprocal in place of the division shows -- with every temperature of planck_edges.edge_temps in every role, and the
fused kernels also on layer counts that take the table loop into its second and third round (it had never left the
first at 256 g-points).  Every call asserts the instance rrtmgpnn_context_get_solver_path reports.

Band limits: every Planck entry refuses limits that overlap or leave a g-point out (the reference leaves lev_source
undefined there and multiplies pfrac once per band here; the kernels' band lookup would have answered band 0 and the
first band), with the outputs left as they were.

What an MI355X gave: all 439 tests pass on the kernels as they were (3.4 s for the file), so no kernel changed; the one
change is the band-limit rule in csrc/api.cpp.  Six value-only breaks, each built once as a library of its own, run
against this file and against the GPU suite as it was before (without the Fortran programs, which link the unbroken
library), then dropped -- failures here / failures there:
  fmaf(frac, hi - lo, lo) in interp1d                          410 / 248 (24 earlier files)
  (val - offset) * (1.0f / delta)                              344 / 0; none of the 344 on the shipped table
  floorf(val0) for the truncation                              434 / 0
  frac clamped to [0, 1]                                       434 / 0
  lw_noscat_kernel's table loop stopped after its first round  162 (every loop shape past one round) / 35: the earlier
    suite does reach a second round -- at 128 g-points and in test_fused_lw_any_nlay and four others at 64 to 137 layers
  the same in lw_rescl_planck_inc_kernel's copy                24 (test_rescl_planck_edges, every such shape) / 0
"""
import ctypes

import numpy as np
import pytest

import planck_edges as PE
from test_gpu_solver_dispatch import BAND, DUAL, FUSED, INC, JAC, LW_NOSCAT, LW_RESCL_INC, MASK, MASKS, MULTI, SC_DUAL

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

OK, ERR_ARGUMENT, ERR_UNSUPPORTED = 0, 1, 4
GUARD = -777.25
F = np.float32
ORIENT = pytest.mark.parametrize("top_at_1", [True, False], ids=["top", "bot"])
NMUS = pytest.mark.parametrize("nmus", [1, 3], ids=["nmus1", "nmus3"])
# the four tables' nlay-5 problems and the table-loop shapes
PROBLEMS = [pytest.param(("table", n), id=n) for n in PE.TABLES] + \
    [pytest.param(("loop",) + s, id=PE.loop_id(s)) for s in PE.LOOP_SHAPES]
PROBLEM = pytest.mark.parametrize("which", PROBLEMS)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a device"
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def problem(which):
    return PE.build(which[1]) if which[0] == "table" else PE.build_loop(*which[1:])


def T(a, dev):
    return torch.as_tensor(np.array(a, dtype=np.float32, order="C"), device=dev)  # a copy: the problems are read-only


def P(t):
    return t.data_ptr() if t is not None else None


def nan(dev, *shape):
    return torch.full(shape, float("nan"), device=dev)


def last_error():
    from rrtmgpnn import _lib
    return _lib.lib().rrtmgpnn_last_error().decode()


def _solver_path(ctx):
    from rrtmgpnn import _lib
    out = (ctypes.c_int * 4)()
    _lib.check(_lib.lib().rrtmgpnn_context_get_solver_path(ctx, out), "context_get_solver_path")
    return list(out)[:3]


_dev = {}


def on_device(p, dev):
    """The problem's arrays on the device, copied once; the solver entries only read them."""
    import mcica_ref as M
    key = id(p)
    if key not in _dev:
        d = {k: T(p[k], dev) for k in ("tlay", "tlev", "tsfc", "pfrac", "tau", "emis", "emis_bnd", "inc", "tau_bnd",
                                       "ssa_bnd", "g_bnd", "tau_aer")}
        d["totplnk"] = T(p["kd"]["totplnk"], dev)
        d["bits"] = torch.as_tensor(M.pack_bits(p["mask"]).view(np.int32), device=dev)
        _dev[key] = d
    return _dev[key]


def head(p, top_at_1, nmus):
    from rrtmgpnn._lib import float_array
    from rrtmgpnn.api import GAUSS_DS, GAUSS_WTS, context
    return [context(0).h, p["ngpt"], p["nlay"], p["ncol"], int(top_at_1), nmus, float_array(GAUSS_DS[nmus]),
            float_array(GAUSS_WTS[nmus])]


def planck_tail(p, d, top_at_1, emis_by_band=False, lims=None):
    from rrtmgpnn._lib import int_array
    kd = p["kd"]
    lims = p["lims"] if lims is None else np.asarray(lims, np.int32)
    return [P(d["pfrac"]), len(lims), kd["nPlanckTemp"], P(d["tlay"]), P(d["tlev"]), P(d["tsfc"]),
            PE.sfc_lay_of(p, top_at_1), int_array(lims.ravel()), float(kd["temp_ref_min"][0]), float(kd["totplnk_delta"]),
            P(d["totplnk"]), int(emis_by_band), P(d["emis_bnd"] if emis_by_band else d["emis"])]


def unchanged(p, d):
    for k in ("pfrac", "tau", "tlay", "tlev", "tsfc"):
        assert np.array_equal(d[k].cpu().numpy().view(np.uint32), p[k].view(np.uint32)), "the call changed its input " + k


# ---- rrtmgpnn_compute_planck_source_nn ---------------------------------------------------------------------------------
def guarded(dev, values=None, n=None):
    """A device array of n floats one float off the allocation's alignment, between guard floats -> (buffer, pointer)."""
    n = values.size if values is not None else n
    buf = torch.full((n + 8,), GUARD, device=dev)
    if values is not None:
        buf[1:1 + n] = T(values, dev).ravel()
    assert buf.data_ptr() % 16 == 0
    return buf, buf.data_ptr() + 4


def payload(buf, shape):
    a = buf.cpu().numpy()
    n = int(np.prod(shape))
    assert a[0] == GUARD and (a[1 + n:] == GUARD).all(), "a guard float was overwritten"
    return a[1:1 + n].reshape(shape)


def run_sources(dev, p, sfc_lay, lims=None, ncol=None):
    """-> (rc, [lay_source, lev_source, sfc_source, sfc_source_Jac]), the guards checked"""
    from rrtmgpnn import _lib
    from rrtmgpnn._lib import int_array
    from rrtmgpnn.api import context
    kd = p["kd"]
    lims = p["lims"] if lims is None else np.asarray(lims, np.int32)
    nc, nlay, ngpt = p["ncol"], p["nlay"], p["ngpt"]
    tl, tv, ts, tab = (T(a, dev) for a in (p["tlay"], p["tlev"], p["tsfc"], kd["totplnk"]))
    shapes = [(nc, nlay, ngpt), (nc, nlay + 1, ngpt), (nc, ngpt), (nc, ngpt)]
    bufs = [guarded(dev, values=p["pfrac"])] + [guarded(dev, n=int(np.prod(s))) for s in shapes[1:]]
    rc = _lib.lib().rrtmgpnn_compute_planck_source_nn(
        context(0).h, nc if ncol is None else ncol, nlay, len(lims), ngpt, kd["nPlanckTemp"], P(tl), P(tv), P(ts), sfc_lay,
        int_array(lims.ravel()), float(kd["temp_ref_min"][0]), float(kd["totplnk_delta"]), P(tab), bufs[2][1], bufs[3][1],
        bufs[0][1], bufs[1][1])
    torch.cuda.synchronize()
    return rc, [payload(b[0], s) for b, s in zip(bufs, shapes)]


def check_sources(dev, orc, p, sfc_lay, what):
    rc, got = run_sources(dev, p, sfc_lay)
    assert rc == OK, last_error()
    for x, y, k in zip(got, PE.sources(orc, p, sfc_lay), ("lay_source", "lev_source", "sfc_source", "sfc_source_Jac")):
        PE.assert_bits(x, y, p, "%s %s" % (what, k))


@ORIENT
@pytest.mark.parametrize("name", PE.TABLES)
def test_planck_source_edges(dev, orc, name, top_at_1):
    p = PE.build(name)
    check_sources(dev, orc, p, PE.sfc_lay_of(p, top_at_1), name)


@pytest.mark.parametrize("shape", PE.kernel_shapes(), ids=lambda s: "nlay%d-ngpt%d-sfc%d" % s)
def test_planck_source_shapes(dev, orc, shape):
    """Layer counts below, at and above the kernel's 4-layer blocks with the surface layer in the first, the last and a
    middle position; g-point counts around the wave and up to the block's 1024 threads."""
    nlay, ngpt, sfc_lay = shape
    check_sources(dev, orc, PE.build_kernel(nlay, ngpt), sfc_lay, str(shape))


def test_planck_source_limits(dev):
    """1025 g-points are RRTMGPNN_ERR_UNSUPPORTED and no column is OK; neither touches an output."""
    base = PE.build_kernel(1, 1024)
    big = dict(base, ngpt=1025, pfrac=np.ones((3, 1, 1025), np.float32), lims=np.array([[1, 1025]], np.int32))
    rc, got = run_sources(dev, big, 1)
    assert rc == ERR_UNSUPPORTED and "1024" in last_error()
    assert all((a == GUARD).all() for a in got[1:]) and (got[0] == 1).all()
    p = PE.build_kernel(3, 65)
    rc, got = run_sources(dev, p, 1, ncol=0)
    assert rc == OK
    assert all((a == GUARD).all() for a in got[1:])
    assert np.array_equal(got[0].view(np.uint32), p["pfrac"].view(np.uint32))


# ---- the fused entries ---------------------------------------------------------------------------------------------------
def run_noscat(dev, p, top_at_1, nmus, entry="plain", request=None, mode=None, emis_by_band=False, lims=None):
    """entry "plain" / "gpt" / "inc" / "clr_all" / "clr_all_mcica"; request None / "byband" / "jac"; mode: of
    rrtmgpnn_context_set_lw_clr_all.  -> {"rc", "out": [up, dn(, up_clr, dn_clr)], "gpt", "bnd", "jac", "path"}"""
    from rrtmgpnn import _lib
    from rrtmgpnn._lib import check, int_array
    d = on_device(p, dev)
    ncol, nlay, ngpt, nb = p["ncol"], p["nlay"], p["ngpt"], p["nb"]
    h, tail = head(p, top_at_1, nmus), planck_tail(p, d, top_at_1, emis_by_band, lims)
    L, ctx = _lib.lib(), h[0]
    outs = [nan(dev, ncol, nlay + 1) for _ in range(4 if entry.startswith("clr_all") else 2)]
    gpt = [nan(dev, ncol, nlay + 1, ngpt) for _ in range(2)] if entry == "gpt" else []
    bnd = [nan(dev, ncol, nlay + 1, nb) for _ in range(2)] if request == "byband" else []
    jac = nan(dev, ncol, nlay + 1) if request == "jac" else None
    try:
        if mode is not None:
            check(L.rrtmgpnn_context_set_lw_clr_all(ctx, mode), "context_set_lw_clr_all")
        if request == "byband":
            check(L.rrtmgpnn_solver_request_byband(ctx, nb, int_array(p["lims"].ravel()), P(bnd[0]), P(bnd[1]), None),
                  "solver_request_byband")
        if request == "jac":
            check(L.rrtmgpnn_solver_request_jacobian(ctx, ngpt, nlay, ncol, None, P(jac)), "solver_request_jacobian")
        o = [P(t) for t in outs]
        if entry == "plain":
            rc = L.rrtmgpnn_lw_solver_noscat_planck(*h, P(d["inc"]), P(d["tau"]), *tail, *o)
        elif entry == "gpt":
            rc = L.rrtmgpnn_lw_solver_noscat_planck_gpt(*h, None, P(d["inc"]), P(d["tau"]), *tail, *o, *[P(t) for t in gpt])
        elif entry == "inc":
            rc = L.rrtmgpnn_lw_solver_noscat_planck_inc(*h, P(d["inc"]), P(d["tau"]), P(d["tau_bnd"]), *tail, *o)
        elif entry == "clr_all":
            rc = L.rrtmgpnn_lw_solver_noscat_planck_clr_all(*h, P(d["inc"]), P(d["tau"]), P(d["tau_bnd"]), *tail, *o)
        else:
            rc = L.rrtmgpnn_lw_solver_noscat_planck_clr_all_mcica(*h, P(d["inc"]), P(d["tau"]), P(d["tau_bnd"]), *tail, *o,
                                                                  P(d["bits"]))
        torch.cuda.synchronize()
    finally:
        if mode is not None:
            check(L.rrtmgpnn_context_set_lw_clr_all(ctx, 0), "context_set_lw_clr_all")
    unchanged(p, d)
    return {"rc": rc, "out": [t.cpu().numpy() for t in outs], "gpt": [t.cpu().numpy() for t in gpt],
            "bnd": [t.cpu().numpy() for t in bnd], "jac": None if jac is None else jac.cpu().numpy(),
            "path": _solver_path(ctx) if rc == OK else None}


def _multi(nmus):
    return MULTI if nmus > 1 else 0


def _compare(p, got, want, names, what):
    for x, y, k in zip(got, want, names):
        PE.assert_bits(x, y, p, "%s %s" % (what, k))


@pytest.mark.parametrize("request_", [None, "byband", "jac"], ids=["plain", "byband", "jac"])
@NMUS
@ORIENT
@PROBLEM
def test_noscat_planck_edges(dev, orc, which, top_at_1, nmus, request_):
    """rrtmgpnn_lw_solver_noscat_planck: the band table (with the Jacobian request its B_b(tsfc + 1) row, with the
    by-band request the emissivity by band as well) against planck_source + lw_solver; by band: sum_byband of the
    oracle's g-point terms; flux_up_Jac: the oracle's flux_up on zero sources with its sfc_source_Jac."""
    import byband_ref as BR
    import oracle as O
    p = problem(which)
    by_band = request_ == "byband"
    r = run_noscat(dev, p, top_at_1, nmus, "plain", request_, emis_by_band=by_band)
    assert r["rc"] == OK, last_error()
    opt = FUSED | _multi(nmus) | (BAND if by_band else 0) | (JAC if request_ == "jac" else 0)
    assert r["path"] == [LW_NOSCAT, opt, 1], r["path"]
    want = PE.ref_noscat(orc, p, top_at_1, nmus, "clear", emis_by_band=by_band, gpt=by_band, jac=request_ == "jac")
    _compare(p, r["out"], want[:2], ("up", "dn"), "noscat_planck")
    if by_band:
        gu, gd = want[2], want[3]
        if nmus == 1:
            w = O.gauss(1)[1][0]
            gu, gd = BR.lw_one_angle_terms(gu, w, p["ngpt"]), BR.lw_one_angle_terms(gd, w, p["ngpt"])
        _compare(p, r["bnd"], (BR.sum_byband(gu, p["lims"]), BR.sum_byband(gd, p["lims"])), ("bnd_up", "bnd_dn"),
                 "noscat_planck")
    if request_ == "jac":
        PE.assert_bits(r["jac"], want[-1], p, "noscat_planck flux_up_Jac")


@NMUS
@ORIENT
@PROBLEM
def test_noscat_planck_gpt_edges(dev, orc, which, top_at_1, nmus):
    """rrtmgpnn_lw_solver_noscat_planck_gpt: the g-point arrays themselves, where a one-ulp error in one band cannot hide
    in the sum over the spectrum."""
    p = problem(which)
    r = run_noscat(dev, p, top_at_1, nmus, "gpt")
    assert r["rc"] == OK, last_error()
    assert r["path"] == [LW_NOSCAT, FUSED | MULTI, 1], r["path"]
    want = PE.ref_noscat(orc, p, top_at_1, nmus, "clear", gpt=True)
    _compare(p, r["out"] + r["gpt"], want, ("up", "dn", "gpt_up", "gpt_dn"), "noscat_planck_gpt")


@pytest.mark.parametrize("request_", [None, "jac"], ids=["plain", "jac"])
@ORIENT
@PROBLEM
def test_noscat_planck_inc_edges(dev, orc, which, top_at_1, request_):
    p = problem(which)
    r = run_noscat(dev, p, top_at_1, 1, "inc", request_)
    assert r["rc"] == OK, last_error()
    assert r["path"] == [LW_NOSCAT, FUSED | INC | (JAC if request_ else 0), 1], r["path"]
    want = PE.ref_noscat(orc, p, top_at_1, 1, "inc", jac=request_ == "jac")
    _compare(p, r["out"], want[:2], ("up", "dn"), "noscat_planck_inc")
    if request_:
        PE.assert_bits(r["jac"], want[-1], p, "noscat_planck_inc flux_up_Jac")


@pytest.mark.parametrize("mode", [1, 2], ids=["dual", "two"])
@ORIENT
@PROBLEM
def test_noscat_planck_clr_all_edges(dev, orc, which, top_at_1, mode):
    """The dual kernel (one band table for both skies) and the two launches."""
    p = problem(which)
    r = run_noscat(dev, p, top_at_1, 1, "clr_all", mode=mode)
    assert r["rc"] == OK, last_error()
    assert r["path"] == ([LW_NOSCAT, FUSED | INC | DUAL, 1] if mode == 1 else [LW_NOSCAT, FUSED | INC, 2]), r["path"]
    want = PE.ref_noscat(orc, p, top_at_1, 1, "inc")[:2] + PE.ref_noscat(orc, p, top_at_1, 1, "clear")[:2]
    _compare(p, r["out"], want, ("up", "dn", "up_clr", "dn_clr"), "noscat_planck_clr_all")


@ORIENT
@PROBLEM
def test_noscat_planck_clr_all_mcica_edges(dev, orc, which, top_at_1):
    p = problem(which)
    r = run_noscat(dev, p, top_at_1, 1, "clr_all_mcica")
    assert r["rc"] == OK, last_error()
    pair = MASKS if p["ngpt"] % 64 == 0 else 0  # torch's allocations are 8-byte aligned
    assert r["path"] == [LW_NOSCAT, FUSED | INC | DUAL | MASK | pair, 1], r["path"]
    want = PE.ref_noscat(orc, p, top_at_1, 1, "masked")[:2] + PE.ref_noscat(orc, p, top_at_1, 1, "clear")[:2]
    _compare(p, r["out"], want, ("up", "dn", "up_clr", "dn_clr"), "noscat_planck_clr_all_mcica")


def run_rescl(dev, p, top_at_1, dual):
    """rrtmgpnn_lw_solver_1rescl_planck_inc, or _planck_clr_all in mode 1 (the dual instance)"""
    from rrtmgpnn import _lib
    from rrtmgpnn._lib import check
    d = on_device(p, dev)
    ncol, nlay = p["ncol"], p["nlay"]
    h = head(p, top_at_1, 1)
    outs = [nan(dev, ncol, nlay + 1) for _ in range(4 if dual else 2)]
    args = h + [P(d[k]) for k in ("inc", "tau", "tau_bnd", "ssa_bnd", "g_bnd")] + planck_tail(p, d, top_at_1) + \
        [P(t) for t in outs]
    L, ctx = _lib.lib(), h[0]
    try:
        if dual:
            check(L.rrtmgpnn_context_set_lw_scat_clr_all(ctx, 1), "context_set_lw_scat_clr_all")
            rc = L.rrtmgpnn_lw_solver_1rescl_planck_clr_all(*args)
        else:
            rc = L.rrtmgpnn_lw_solver_1rescl_planck_inc(*args)
        torch.cuda.synchronize()
    finally:
        if dual:
            check(L.rrtmgpnn_context_set_lw_scat_clr_all(ctx, 0), "context_set_lw_scat_clr_all")
    unchanged(p, d)
    return rc, [t.cpu().numpy() for t in outs], _solver_path(ctx) if rc == OK else None


@pytest.mark.parametrize("dual", [False, True], ids=["inc", "clr_all-dual"])
@ORIENT
@PROBLEM
def test_rescl_planck_edges(dev, orc, which, top_at_1, dual):
    """lw_rescl_planck_inc_kernel's copy of the table loop: the single and the dual instance."""
    p = problem(which)
    rc, got, path = run_rescl(dev, p, top_at_1, dual)
    assert rc == OK, last_error()
    assert path == [LW_RESCL_INC, SC_DUAL if dual else 0, 1], path
    want = PE.ref_rescl(orc, p, top_at_1, 1)
    _compare(p, got, want[:len(got)], ("up", "dn", "up_clr", "dn_clr"), "1rescl_planck")


# ---- rrtmgpnn_compute_bc_lw ----------------------------------------------------------------------------------------------
_bc = {}


def bc_kit(name, dev):
    """(kd, model dicts, device networks) of a table: the shipped pair where the table has its 256 g-points, else a seeded
    pair of small networks on the shipped inputs with the table's g-point count as outputs."""
    from rrtmgpnn import api, data
    import mlp_cases as MC
    if name not in _bc:
        kd = PE.tables()[name]
        if kd["ngpt"] == 256:
            models = [data.load_model("lw_abs"), data.load_model("lw_pfrac")]
            nets = [api.RrtmgpNetwork(0).load(data.path(n)) for n in ("lw_abs", "lw_pfrac")]
        else:
            shipped = data.load_model("lw_abs")
            nx = int(shipped["dims"][0])
            models = []
            for k, (hidden, scaling) in enumerate(((58, True), (16, False))):  # the shipped pair's hidden widths
                m = MC.make_model([nx, hidden, hidden, kd["ngpt"]], [int(a) for a in shipped["activation"]], 77 + k,
                                  scaling)
                m.update({key: shipped[key] for key in ("input_names", "input_min", "input_max")})
                if scaling:  # tau = (std y + mean)^8 col_dry with col_dry of order 1e22: optical depths of order 1
                    m["output_mean"], m["output_std"] = m["output_mean"] * F(2e-3), m["output_std"] * F(2e-3)
                models.append(m)
            nets = [api.RrtmgpNetwork(0).from_arrays(m) for m in models]
        _bc[name] = (kd, models, nets)
    return _bc[name]


@ORIENT
@pytest.mark.parametrize("name", PE.TABLES)
def test_compute_bc_lw_edges(dev, orc, rfmip, name, top_at_1):
    """bc_flux_kernel's two interp1d calls: the top layer's temperature over the table's whole edge set, one and three
    angles, radiance and flux units, against compute_bc_ref's composition (the one-layer problem, the oracle's gas optics
    and sources, its g-point solver)."""
    import compute_bc_ref as B
    from rrtmgpnn import _lib, data
    from rrtmgpnn._lib import check, float_array, int_array, ptr_array
    from rrtmgpnn.api import GAUSS_DS, GAUSS_WTS, context
    from rrtmgpnn.compute_bc import gas_arguments
    from test_gpu_compute_bc import gas_concs
    kd, models, nets = bc_kit(name, dev)
    temps = PE.edge_temps(name)
    n = len(temps)
    prob = dict(B.truncated(rfmip, (np.arange(n) * 7) % rfmip["ncol"], 1, 2, top_at_1))
    tlay = prob["tlay"].copy()
    tlay[:, 0 if top_at_1 else -1] = temps
    prob["tlay"] = tlay
    press_min = float(data.load_kdist("lw")["press_ref_min"][0])
    go = orc.lw_gas_optics(B.one_layer(prob, press_min), models, kd)
    ones = np.ones(go["sfc_source"].shape, np.float32)
    ncol, nlay, ngpt = n, 2, kd["ngpt"]
    play, plev, tl = (T(prob[k], dev) for k in ("play", "plev", "tlay"))
    gc = gas_concs(prob["gases"], dev)
    ptrs, nds, e = gas_arguments(nets[0], gc)
    assert e == ""
    tab = T(kd["totplnk"], dev)
    desc = {"describe": lambda cols: "temperatures %s" % temps[list(cols)[:8]].tolist()}
    for nmus in (1, 3):
        radn = orc.lw_solver(go["tau"], go["lay_source"], go["lev_source"], ones, go["sfc_source"], top_at_1, nmus,
                             gpt=True)[3][:, 1 if top_at_1 else 0]
        for as_flux in (0, 1):
            out = nan(dev, ncol, ngpt)
            check(_lib.lib().rrtmgpnn_compute_bc_lw(
                context(0).h, ncol, nlay, ngpt, nets[0].dims[0], int(top_at_1), press_min, P(play), P(plev), P(tl),
                gc.concs["h2o"].data_ptr(), ptr_array(ptrs), int_array(nds), ptr_array([x.h.value for x in nets]), 2,
                kd["nband"], kd["nPlanckTemp"], int_array(np.asarray(kd["band_lims_gpt"], np.int32).ravel()),
                float(kd["temp_ref_min"][0]), float(kd["totplnk_delta"]), P(tab), nmus, float_array(GAUSS_DS[nmus]),
                float_array(GAUSS_WTS[nmus]), as_flux, P(out)), "compute_bc_lw")
            torch.cuda.synchronize()
            want = B.in_flux_units(radn, nmus) if as_flux else radn
            PE.assert_bits(out.cpu().numpy(), np.ascontiguousarray(want), desc, "%s nmus %d as_flux %d" % (name, nmus,
                                                                                                          as_flux))


# ---- band limits -----------------------------------------------------------------------------------------------------------
def _bad_limits(p):
    """(overlapping, leaving a g-point out) on the problem's band count."""
    lims = np.array(p["lims"], np.int32)
    over, out = lims.copy(), lims.copy()
    over[1, 0] -= 1   # band 2 starts on band 1's last g-point
    out[0, 1] -= 1    # band 1's last g-point is in no band
    return [("overlap", over, "overlap"), ("uncovered", out, "outside every band")]


@pytest.mark.parametrize("entry", ["sources", "plain", "gpt"])
def test_planck_entries_refuse_band_limits_that_do_not_partition(dev, entry):
    """rrtmgpnn_compute_planck_source_nn, _lw_solver_noscat_planck and _planck_gpt take no increment and no by-band
    emissivity, and still look every g-point's band up: overlapping limits and limits that leave a g-point out are
    RRTMGPNN_ERR_ARGUMENT with bands_cover's messages, and no output is written."""
    p = PE.build("d07")
    for kind, lims, msg in _bad_limits(p):
        if entry == "sources":
            rc, got = run_sources(dev, p, 1, lims=lims)
            assert rc == ERR_ARGUMENT and msg in last_error(), (kind, rc, last_error())
            assert all((a == GUARD).all() for a in got[1:])
            assert np.array_equal(got[0].view(np.uint32), p["pfrac"].view(np.uint32))
        else:
            r = run_noscat(dev, p, True, 1, entry, lims=lims)
            assert r["rc"] == ERR_ARGUMENT and msg in last_error(), (kind, r["rc"], last_error())
            assert all(np.isnan(a).all() for a in r["out"] + r["gpt"])
    # the context serves the next call
    assert run_noscat(dev, p, True, 1, "plain")["rc"] == OK


def test_compute_bc_lw_refuses_band_limits_that_do_not_partition(dev, rfmip):
    import compute_bc_ref as B
    from rrtmgpnn import _lib, data
    from rrtmgpnn._lib import float_array, int_array, ptr_array
    from rrtmgpnn.api import GAUSS_DS, GAUSS_WTS, context
    from rrtmgpnn.compute_bc import gas_arguments
    from test_gpu_compute_bc import gas_concs
    kd, _, nets = bc_kit("shipped", dev)
    prob = B.truncated(rfmip, B.COLS["c7"], 1, 2, True)
    play, plev, tl = (T(prob[k], dev) for k in ("play", "plev", "tlay"))
    gc = gas_concs(prob["gases"], dev)
    ptrs, nds, e = gas_arguments(nets[0], gc)
    assert e == ""
    tab = T(kd["totplnk"], dev)
    for kind, lims, msg in _bad_limits({"lims": np.asarray(kd["band_lims_gpt"]).reshape(-1, 2)}):
        out = nan(dev, 7, 256)
        rc = _lib.lib().rrtmgpnn_compute_bc_lw(
            context(0).h, 7, 2, 256, nets[0].dims[0], 1, float(data.load_kdist("lw")["press_ref_min"][0]), P(play),
            P(plev), P(tl), gc.concs["h2o"].data_ptr(), ptr_array(ptrs), int_array(nds),
            ptr_array([x.h.value for x in nets]), 2, kd["nband"], kd["nPlanckTemp"], int_array(lims.ravel()),
            float(kd["temp_ref_min"][0]), float(kd["totplnk_delta"]), P(tab), 1, float_array(GAUSS_DS[1]),
            float_array(GAUSS_WTS[1]), 0, P(out))
        torch.cuda.synchronize()
        assert rc == ERR_ARGUMENT and msg in last_error(), (kind, rc, last_error())
        assert torch.isnan(out).all()
