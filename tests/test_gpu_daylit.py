"""GPU: the daylit-column entries of the C ABI, bit for bit.

  * rrtmgpnn_daylit_plan against rrtmgpnn.daylit.plan_host (tests/test_daylit_host.py holds that to the plan's
    properties) over sizes around the wave, the block and the chunk, every pattern, both kinds;
  * rrtmgpnn_gather_columns / _scatter_columns against numpy indexing, rows of 1, 3, 61 and 138 floats one float off
    alignment, guards and the rows past the count untouched;
  * rrtmgpnn_gas_optics_sw_nn_active (g224 and g112 pairs) against rrtmgpnn_gas_optics_sw_nn at ncol = nact, which in
    turn equals the oracle; samples past the count keep their prefill;
  * the three SW entries that honour rrtmgpnn_solver_request_active_columns against the oracle's sw_solver on the active
    columns, rows past the count untouched, with the instance each call must report (family 7): SOLVER_ROWS holds every
    instance of the family's list to a row; the plane-free ones run in a child process with RRTMGPNN_SW_NO_PLANES=1, as
    tests/test_gpu_solver_dispatch.py runs its own;
  * the refusals, each of which clears the request."""
import ctypes
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import subset
from test_daylit_host import PATTERNS, values

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
FILES = os.path.join(ROOT, "tests", "golden", "reference_files")
G112 = (os.path.join(FILES, "sw-g112-210809_absorption_BEST.nc"), os.path.join(FILES, "sw-g112-210809_rayleigh_BEST.nc"))
OK, ERR_ARGUMENT, ERR_UNSUPPORTED = 0, 1, 4
MFMA32, F_XIN, F_ACTIVE = 2, 4, 16
# rrtmgpnn_context_get_solver_path: family 7, family 2's option bits and 2048
SW_CK_ACTIVE, CK_INC, CK_TN, CK_EMK, CK_PAIR, CK_SMALL, CK_ACTIVE = 7, 2, 8, 16, 32, 1024, 2048
N_ACTIVE_INSTANCES = 7


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a device"
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def T(a, dev, dtype=np.float32):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device=dev)


def bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else a
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def P(t):
    return None if t is None else t.data_ptr()


def lib():
    from rrtmgpnn import _lib
    return _lib.lib()


@functools.lru_cache(maxsize=None)
def own_ctx():
    """A context of this file's own: the requests and kernel modes set here stay off the default one."""
    from rrtmgpnn import api
    return api.Context(0)


def last_error():
    return lib().rrtmgpnn_last_error().decode()


# ---- plan ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("ncol", [1, 2, 63, 64, 65, 1025, 4099, 1000003])
def test_plan_equals_plan_host(dev, ncol, pattern, kind):
    from rrtmgpnn import daylit
    v = values(ncol, pattern, kind, daylit.SZA_BOUND, seed=ncol)
    want = daylit.plan_host(v, kind, daylit.SZA_BOUND)
    pl = daylit.Plan(torch.full((ncol,), -7, dtype=torch.int32, device=dev),
                     torch.full((ncol,), -7, dtype=torch.int32, device=dev),
                     torch.full((1,), -7, dtype=torch.int32, device=dev))
    daylit.plan(T(v, dev), kind, daylit.SZA_BOUND, out=pl)
    torch.cuda.synchronize()
    assert int(pl.nday.item()) == want[2]
    np.testing.assert_array_equal(pl.idx.cpu().numpy(), want[0])
    np.testing.assert_array_equal(pl.slot.cpu().numpy(), want[1])


def test_plan_arguments(dev):
    L, c = lib(), own_ctx().h
    v, i = torch.zeros(4, device=dev), torch.zeros(4, dtype=torch.int32, device=dev)
    n = torch.full((1,), 5, dtype=torch.int32, device=dev)
    assert L.rrtmgpnn_daylit_plan(c, 4, P(v), 2, 1.0, P(i), P(i), P(n)) == ERR_ARGUMENT and "kind" in last_error()
    assert L.rrtmgpnn_daylit_plan(c, -1, P(v), 0, 1.0, P(i), P(i), P(n)) == ERR_ARGUMENT
    assert L.rrtmgpnn_daylit_plan(c, 4, None, 0, 1.0, P(i), P(i), P(n)) == ERR_ARGUMENT
    assert L.rrtmgpnn_daylit_plan(c, 4, P(v), 0, 1.0, P(i), P(i), None) == ERR_ARGUMENT
    assert L.rrtmgpnn_daylit_plan(c, 0, None, 0, 1.0, None, None, P(n)) == OK   # launches nothing
    torch.cuda.synchronize()
    assert int(n.item()) == 5


# ---- gather / scatter ---------------------------------------------------------------------------------------------
ROWS = (1, 3, 61, 138)
GUARD, SENTINEL = 32, -777.0


def offset_buffer(dev, n, fill):
    """n floats one float off the allocation's alignment, guard floats on both sides: (buffer, view)"""
    buf = torch.full((1 + n + GUARD,), SENTINEL, device=dev)
    view = buf[1:1 + n]
    view.fill_(fill)
    assert view.data_ptr() % 16 == 4
    return buf, view


def guards_intact(buf, n):
    return bool((buf[:1] == SENTINEL).all()) and bool((buf[1 + n:] == SENTINEL).all())


@pytest.mark.parametrize("pattern", ["random", "day", "night", "last"])
@pytest.mark.parametrize("ncol", [1, 65, 200])
def test_gather_and_scatter_equal_numpy_indexing(dev, ncol, pattern):
    from rrtmgpnn import daylit
    rng = np.random.default_rng(ncol)
    v = values(ncol, pattern, 0, daylit.SZA_BOUND, seed=ncol)
    idx, slot, nday = daylit.plan_host(v, 0, daylit.SZA_BOUND)
    pl = daylit.plan(T(v, dev))
    src = [rng.standard_normal((ncol, r)).astype(F32) for r in ROWS]
    dsrc = [T(a, dev) for a in src]
    dst = [offset_buffer(dev, ncol * r, float("nan")) for r in ROWS]
    daylit.gather(pl, [(s, d[1].view(ncol, r)) for s, d, r in zip(dsrc, dst, ROWS)])
    torch.cuda.synchronize()
    for a, (buf, view), r in zip(src, dst, ROWS):
        got = view.cpu().numpy().reshape(ncol, r)
        np.testing.assert_array_equal(bits(got[:nday]), bits(a[idx[:nday]]), err_msg="gather, rows of %d" % r)
        assert np.isnan(got[nday:]).all(), "gather wrote rows at or past nday (rows of %d)" % r
        assert guards_intact(buf, ncol * r)
    # scatter (at most 6 arrays): the dense rows past nday are NaN and not needed; night columns become zeros
    out = [offset_buffer(dev, ncol * r, float("nan")) for r in ROWS]
    daylit.scatter(pl, [(d[1].view(ncol, r), o[1].view(ncol, r)) for d, o, r in zip(dst, out, ROWS)])
    torch.cuda.synchronize()
    for a, (buf, view), r in zip(src, out, ROWS):
        got = view.cpu().numpy().reshape(ncol, r)
        want = np.where((slot >= 0)[:, None], a, F32(0))
        np.testing.assert_array_equal(bits(got), bits(want), err_msg="scatter, rows of %d" % r)
        assert guards_intact(buf, ncol * r)


def test_gather_scatter_arguments(dev):
    from rrtmgpnn._lib import int_array, ptr_array
    L, c = lib(), own_ctx().h
    a, b = torch.zeros(8, device=dev), torch.zeros(8, device=dev)
    i, n = torch.zeros(8, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    one = (ptr_array([P(a)]), ptr_array([P(b)]), int_array([1]))
    many = (ptr_array([P(a)] * 17), ptr_array([P(b)] * 17), int_array([1] * 17))
    assert L.rrtmgpnn_gather_columns(c, 8, 0, *one, P(i), P(n)) == ERR_ARGUMENT and "narrays" in last_error()
    assert L.rrtmgpnn_gather_columns(c, 8, 17, *many, P(i), P(n)) == ERR_ARGUMENT
    assert L.rrtmgpnn_gather_columns(c, 8, 16, *many, P(i), P(n)) == OK
    assert L.rrtmgpnn_gather_columns(c, -1, 1, *one, P(i), P(n)) == ERR_ARGUMENT
    assert L.rrtmgpnn_gather_columns(c, 8, 1, *one, None, P(n)) == ERR_ARGUMENT
    assert L.rrtmgpnn_gather_columns(c, 8, 1, ptr_array([None]), one[1], one[2], P(i), P(n)) == ERR_ARGUMENT
    assert L.rrtmgpnn_gather_columns(c, 0, 1, *one, P(i), P(n)) == OK
    assert L.rrtmgpnn_scatter_columns(c, 8, 7, *many, P(i)) == ERR_ARGUMENT and "narrays" in last_error()
    assert L.rrtmgpnn_scatter_columns(c, 8, 6, *many, P(i)) == OK
    assert L.rrtmgpnn_scatter_columns(c, 8, 1, *one, None) == ERR_ARGUMENT
    assert L.rrtmgpnn_scatter_columns(c, 0, 1, *one, P(i)) == OK
    torch.cuda.synchronize()


# ---- network ------------------------------------------------------------------------------------------------------
NCOL, NLAY = 5, 7   # 35 samples: a second, partial tile


@functools.lru_cache(maxsize=None)
def sw_models(ngpt):
    from rrtmgpnn import api, data
    paths = (data.path("sw_abs"), data.path("sw_ray")) if ngpt == 224 else G112
    return [data.load_model(p) for p in paths], [api.RrtmgpNetwork(0).load_netcdf(p) for p in paths]


@functools.lru_cache(maxsize=None)
def net_state(ngpt):
    """5 RFMIP columns x the 7 lowest layers, and the oracle's tau / ssa of them"""
    import oracle as O
    from rrtmgpnn import data, rbin
    orc = O.Oracle()
    p = subset(data.rfmip_problem(), (np.arange(NCOL) * 97 + 5) % 1800)
    lay0 = 60 - NLAY
    ms, _ = sw_models(ngpt)
    names = rbin.unchars(ms[0]["input_names"])
    s = {"play": np.ascontiguousarray(p["play"][:, lay0:]), "plev": np.ascontiguousarray(p["plev"][:, lay0:]),
         "tlay": np.ascontiguousarray(p["tlay"][:, lay0:]), "names": names,
         "gases": {n: np.ascontiguousarray(p["gases"][n][:, lay0:]) for n in names[2:]}}
    x = orc.nn_inputs(s["play"], s["tlay"], s["gases"], ms[0])
    cd = orc.col_dry(s["gases"]["h2o"], s["plev"])
    xf = x.reshape(-1, x.shape[-1])
    tau = orc.tau_post(ms[0], orc.mlp(ms[0], xf), cd)
    ssa = orc.tau_post(ms[1], orc.mlp(ms[1], xf), cd, tau_abs_to_tot=tau)
    assert np.isfinite(tau).all() and np.isfinite(ssa).all() and (tau > 0).any()
    return s, tau.reshape(NCOL * NLAY, ngpt), ssa.reshape(NCOL * NLAY, ngpt)


def gas_optics(dev, ngpt, ncol, entry, nact=None):
    """entry on the first `ncol` columns of the state; tau, ssa prefilled with NaN -> (rc, tau, ssa, mlp path)"""
    from rrtmgpnn._lib import int_array, ptr_array
    s, _, _ = net_state(ngpt)
    _, nn = sw_models(ngpt)
    L, c = lib(), own_ctx().h
    keep = [T(s[k][:ncol], dev) for k in ("play", "tlay", "plev")] + [T(s["gases"]["h2o"][:ncol], dev)]
    gases = [None if k < 2 else T(s["gases"][n][:ncol], dev) for k, n in enumerate(s["names"])]
    tau, ssa = (torch.full((ncol * NLAY, ngpt), float("nan"), device=dev) for _ in range(2))
    args = [c, ncol, NLAY, ngpt, len(s["names"])] + [P(t) for t in keep] + [
        ptr_array([P(t) for t in gases]), int_array([2] * len(gases)), ptr_array([n.h.value for n in nn]), P(tau), P(ssa),
        None]
    rc = getattr(L, entry)(*args, *([P(nact)] if entry.endswith("_active") else []))
    torch.cuda.synchronize()
    p = (ctypes.c_int * 8)()
    assert L.rrtmgpnn_context_get_mlp_path(c, p) == OK
    return rc, tau.cpu().numpy(), ssa.cpu().numpy(), list(p)


@pytest.mark.parametrize("nact", [0, 1, 3, 5])
@pytest.mark.parametrize("ngpt", [224, 112])
def test_network_on_the_active_columns(dev, ngpt, nact):
    _, tau_o, ssa_o = net_state(ngpt)
    word = torch.full((1,), nact, dtype=torch.int32, device=dev)
    rc, tau, ssa, path = gas_optics(dev, ngpt, NCOL, "rrtmgpnn_gas_optics_sw_nn_active", word)
    assert rc == OK, last_error()
    assert path[0] == MFMA32 and path[7] & F_XIN and path[7] & F_ACTIVE, path
    n = NLAY * nact
    assert np.isnan(tau[n:]).all() and np.isnan(ssa[n:]).all(), "samples at or past nlay * nact were written"
    if nact:
        rc, tau_p, ssa_p, path = gas_optics(dev, ngpt, nact, "rrtmgpnn_gas_optics_sw_nn")
        assert rc == OK and path[0] == MFMA32 and not path[7] & F_ACTIVE, (last_error(), path)
        for got, plain, want, k in ((tau, tau_p, tau_o, "tau"), (ssa, ssa_p, ssa_o, "ssa")):
            np.testing.assert_array_equal(bits(got[:n]), bits(plain), err_msg=k + " against gas_optics_sw_nn")
            np.testing.assert_array_equal(bits(plain), bits(want[:n]), err_msg=k + " against the oracle")


def test_network_refuses_the_16x16x4_route(dev):
    c = own_ctx()
    word = torch.full((1,), 3, dtype=torch.int32, device=dev)
    c.set_mlp_kernel(1)
    try:
        rc, tau, _, _ = gas_optics(dev, 224, NCOL, "rrtmgpnn_gas_optics_sw_nn_active", word)
    finally:
        c.set_mlp_kernel(0)
    assert rc == ERR_UNSUPPORTED and "32x32x2" in last_error()
    assert np.isnan(tau).all()
    rc, _, _, _ = gas_optics(dev, 224, NCOL, "rrtmgpnn_gas_optics_sw_nn_active", None)   # nact == NULL
    assert rc == ERR_ARGUMENT


# ---- solver -------------------------------------------------------------------------------------------------------
GENERAL_LIMS = ((1, 15), (16, 224))   # band 2 starts at an even 1-based g-point: not the band-pair layout
PL_SMALL, PL_NN, PL_INC = CK_TN | CK_EMK, CK_TN | CK_EMK, CK_TN
NACTS = (0, 1, 2, 3, 5)   # odd: a block's second column is inactive; 0: every block exits


def row(name, form, options, ngpt=224, nlay=4, top=1, lims=None, large=False, child=False):
    return dict(name=name, form=form, options=options | CK_ACTIVE, ngpt=ngpt, nlay=nlay, top=top, lims=lims, large=large,
                child=child)


def _rows():
    rows = []
    for ngpt in (224, 112):
        for nlay in (4, 7):   # neither a multiple of the chunk length 3
            for top in (1, 0):
                t = "g%d-l%d-top%d" % (ngpt, nlay, top)
                rows += [row("rfmip-" + t, "rfmip", CK_SMALL | PL_SMALL, ngpt, nlay, top),
                         row("plain-" + t, "plain", CK_SMALL | PL_SMALL, ngpt, nlay, top),
                         row("inc-" + t, "inc", CK_INC | CK_PAIR | PL_INC, ngpt, nlay, top),
                         row("rfmip-inc-" + t, "rfmip_inc", CK_INC | CK_PAIR | PL_INC, ngpt, nlay, top)]
    rows += [row("inc-general", "inc", CK_INC | PL_INC, lims=GENERAL_LIMS),
             row("nn-large", "plain", PL_NN, large=True, nlay=3)]
    # RRTMGPNN_SW_NO_PLANES=1 (a fresh process): the small-grid instance keeps its planes, the others run plane-free
    rows += [row("rfmip-noplanes", "rfmip", CK_SMALL | PL_SMALL, child=True),
             row("inc-noplanes", "inc", CK_INC | CK_PAIR, child=True),
             row("inc-general-noplanes", "inc", CK_INC, lims=GENERAL_LIMS, child=True),
             row("nn-large-noplanes", "plain", 0, large=True, nlay=3, child=True)]
    return rows


SOLVER_ROWS = _rows()
HERE_ROWS = [r for r in SOLVER_ROWS if not r["child"]]
CHILD_ROWS = [r for r in SOLVER_ROWS if r["child"]]


def test_solver_rows_hold_every_listed_instance():
    assert len({r["name"] for r in SOLVER_ROWS}) == len(SOLVER_ROWS)
    assert len({r["options"] for r in SOLVER_ROWS}) == N_ACTIVE_INSTANCES


def large_ncol(ngpt):
    """past the small-grid bound ncol * ngpt / 2 <= 64 * 16 * CUs of this device"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return 64 * 16 * cus // (ngpt // 2) + 52


@functools.lru_cache(maxsize=None)
def solver_problem(name):
    """The row's inputs and the oracle's fluxes of every column (the columns are independent)"""
    import oracle as O
    from rrtmgpnn import data
    r = next(r for r in SOLVER_ROWS if r["name"] == name)
    ngpt, nlay = r["ngpt"], r["nlay"]
    ncol = large_ncol(ngpt) if r["large"] else 5
    kd = data.load_kdist("sw", None if ngpt == 224 else ngpt)
    lims = np.asarray(r["lims"] or kd["band_lims_gpt"], np.int32)
    nb = len(lims)
    rng = np.random.default_rng(1000 * ngpt + 10 * nlay + r["top"] + 7 * len(r["form"]))
    u = lambda lo, hi, *s: rng.uniform(lo, hi, s).astype(F32)  # noqa: E731
    p = dict(tau=rng.lognormal(-2, 1.5, (ncol, nlay, ngpt)).astype(F32), ssa=u(0.1, 0.95, ncol, nlay, ngpt),
             tb=rng.lognormal(-1, 1, (ncol, nlay, nb)).astype(F32), wb=u(0.3, 0.95, ncol, nlay, nb),
             gb=u(0.3, 0.9, ncol, nlay, nb), tsi=u(1300, 1400, ncol), sfc_alb=u(0.05, 0.6, ncol),
             sza=np.where(rng.random(ncol) < 0.7, u(0, 85, ncol), u(91, 119, ncol)).astype(F32))
    p["solar_source"] = data.set_tsi(kd["solar_source"], 1361.0)
    if r["form"].startswith("rfmip"):
        use = p["sza"] < F32(90.0) - F32(2.0) * data.spacing(90.0)
        deg = F32(np.arccos(F32(-1.0)) / F32(180.0))
        p["mu0"] = np.where(use, data.ref_cosf(p["sza"] * deg), F32(1.0)).astype(F32)
        p["toa"] = data.toa_flux({"ncol": ncol, "tsi": p["tsi"]}, kd)
        p["alb"] = np.repeat(p["sfc_alb"][:, None], ngpt, axis=1)
    else:
        p["mu0"], p["toa"], p["alb"] = u(0.1, 1, ncol), u(0.1, 10, ncol, ngpt), u(0, 0.9, ncol, ngpt)
    orc = O.Oracle()
    io = (p["tau"], p["ssa"], np.zeros_like(p["tau"]))
    if "inc" in r["form"]:
        io = orc.increment_bybnd(lims, io, (p["tb"], p["wb"], p["gb"]))
    want = orc.sw_solver(*io, p["mu0"], p["toa"], p["alb"], p["alb"], bool(r["top"]))
    assert all(np.isfinite(w).all() for w in want)
    return r, ncol, lims, p, want


def run_solver(dev, name, nact, arm=True):
    """The row's call with the request armed on `nact` columns -> (rc, path, [up, dn, dir] prefilled with NaN)"""
    from rrtmgpnn._lib import int_array
    r, ncol, lims, p, _ = solver_problem(name)
    L, c = lib(), own_ctx().h
    d = {k: T(v, dev) for k, v in p.items()}
    ngpt, nlay = r["ngpt"], r["nlay"]
    fl = [torch.full((ncol, nlay + 1), float("nan"), device=dev) for _ in range(3)]
    word = torch.full((1,), nact, dtype=torch.int32, device=dev)
    if arm:
        assert L.rrtmgpnn_solver_request_active_columns(c, ncol, P(word)) == OK
    bands = [len(lims), int_array(lims.ravel()), P(d["tb"]), P(d["wb"]), P(d["gb"])]
    head = [c, ngpt, nlay, ncol, r["top"]]
    outs = [P(t) for t in fl]
    if r["form"].startswith("rfmip"):
        scratch = [torch.zeros(ncol, ngpt, device=dev), torch.zeros(ncol, ngpt, device=dev), torch.zeros(ncol, device=dev)]
        rc = L.rrtmgpnn_sw_solver_2stream_rfmip(*head, P(d["solar_source"]), P(d["tsi"]), P(d["sfc_alb"]), P(d["sza"]),
                                                P(d["tau"]), P(d["ssa"]), None,
                                                *(bands if "inc" in r["form"] else [0, None, None, None, None]),
                                                *[P(t) for t in scratch], *outs)
    elif r["form"] == "inc":
        rc = L.rrtmgpnn_sw_solver_2stream_inc(*head, P(d["toa"]), None, P(d["tau"]), P(d["ssa"]), None, *bands,
                                              P(d["mu0"]), P(d["alb"]), P(d["alb"]), *outs)
    else:
        rc = L.rrtmgpnn_sw_solver_2stream(*head, P(d["toa"]), None, P(d["tau"]), P(d["ssa"]), None, P(d["mu0"]),
                                          P(d["alb"]), P(d["alb"]), *outs)
    torch.cuda.synchronize()
    path = (ctypes.c_int * 4)()
    assert L.rrtmgpnn_context_get_solver_path(c, path) == OK
    return rc, list(path), [t.cpu().numpy() for t in fl]


def nacts_of(name):
    r, ncol, _, _, _ = solver_problem(name)
    return (0, 3, ncol - 1, ncol) if r["large"] else NACTS


def check_row(name, nact, rc, path, got):
    r, ncol, _, _, want = solver_problem(name)
    assert rc == OK, "%s nact %d: %s" % (name, nact, last_error())
    for g, w, k in zip(got, want, ("up", "dn", "dir")):
        np.testing.assert_array_equal(bits(g[:nact]), bits(w[:nact]), err_msg="%s nact %d: flux_%s" % (name, nact, k))
        assert np.isnan(g[nact:]).all(), "%s nact %d: flux_%s rows at or past nact were written" % (name, nact, k)
    assert path == [SW_CK_ACTIVE, r["options"], 1, N_ACTIVE_INSTANCES], (name, nact, path)


@pytest.mark.parametrize("name", [r["name"] for r in HERE_ROWS])
def test_solver_on_the_active_columns(dev, name):
    assert "RRTMGPNN_SW_NO_PLANES" not in os.environ
    for nact in nacts_of(name):
        check_row(name, nact, *run_solver(dev, name, nact))


def child_main(out_json, out_npz):
    """The plane-free rows (the parent process set RRTMGPNN_SW_NO_PLANES=1): codes and paths to JSON, fluxes to npz"""
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    meta, flux = {}, {}
    for r in CHILD_ROWS:
        for nact in nacts_of(r["name"]):
            rc, path, got = run_solver(dev, r["name"], nact)
            meta["%s/%d" % (r["name"], nact)] = [rc, path, last_error() if rc else ""]
            for k, a in zip(("up", "dn", "dir"), got):
                flux["%s/%d/%s" % (r["name"], nact, k)] = a
    json.dump(meta, open(out_json, "w"))
    np.savez(out_npz, **flux)


def test_solver_plane_free_instances_in_a_child_process(dev, tmp_path):
    oj, on = str(tmp_path / "meta.json"), str(tmp_path / "flux.npz")
    code = ("import sys; sys.path[:0] = [%r, %r, %r]; import test_gpu_daylit as D; D.child_main(%r, %r)"
            % (os.path.join(ROOT, "tests"), os.path.join(ROOT, "rte-rrtmgp-nn_amd"), os.path.join(ROOT, "oracle"), oj, on))
    env = dict(os.environ, RRTMGPNN_SW_NO_PLANES="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    meta, flux = json.load(open(oj)), np.load(on)
    for r in CHILD_ROWS:
        for nact in nacts_of(r["name"]):
            rc, path, msg = meta["%s/%d" % (r["name"], nact)]
            assert rc == OK, msg
            check_row(r["name"], nact, rc, path, [flux["%s/%d/%s" % (r["name"], nact, k)] for k in ("up", "dn", "dir")])


# ---- refusals -----------------------------------------------------------------------------------------------------
def plain_result_follows(dev, name="plain-g224-l4-top1"):
    """A plain call after a refusal: the request is gone, every column is solved"""
    _, ncol, _, _, want = solver_problem(name)
    rc, path, got = run_solver(dev, name, 0, arm=False)
    assert rc == OK, last_error()
    assert path[0] == 2 and not path[1] & CK_ACTIVE, path
    for g, w in zip(got, want):
        np.testing.assert_array_equal(bits(g), bits(w))


@pytest.mark.parametrize("entry", ["lw_solver_noscat", "sw_solver_noscat", "sw_solver_2stream_clr_all", "byband"])
def test_refusals_clear_the_request(dev, entry):
    from rrtmgpnn._lib import float_array, int_array
    from rrtmgpnn.api import GAUSS_DS, GAUSS_WTS
    name = "inc-g224-l4-top1"
    r, ncol, lims, p, _ = solver_problem(name)
    L, c = lib(), own_ctx().h
    ngpt, nlay = r["ngpt"], r["nlay"]
    d = {k: T(v, dev) for k, v in p.items()}
    word = torch.full((1,), 2, dtype=torch.int32, device=dev)
    fl = [torch.full((ncol, nlay + 1), float("nan"), device=dev) for _ in range(6)]
    lev = torch.ones(ncol, nlay + 1, ngpt, device=dev)
    bands = [len(lims), int_array(lims.ravel()), P(d["tb"]), P(d["wb"]), P(d["gb"])]
    assert L.rrtmgpnn_solver_request_active_columns(c, ncol, P(word)) == OK
    if entry == "lw_solver_noscat":
        rc = L.rrtmgpnn_lw_solver_noscat(c, ngpt, nlay, ncol, 1, 1, float_array(GAUSS_DS[1]), float_array(GAUSS_WTS[1]),
                                         None, P(d["tau"]), P(d["ssa"]), P(lev), P(d["alb"]), P(d["toa"]), P(fl[0]), P(fl[1]))
    elif entry == "sw_solver_noscat":
        rc = L.rrtmgpnn_sw_solver_noscat(c, ngpt, nlay, ncol, 1, P(d["toa"]), P(d["tau"]), P(d["mu0"]), P(fl[2]))
    elif entry == "sw_solver_2stream_clr_all":
        rc = L.rrtmgpnn_sw_solver_2stream_clr_all(c, ngpt, nlay, ncol, 1, P(d["toa"]), None, P(d["tau"]), P(d["ssa"]), None,
                                                  *bands, P(d["mu0"]), P(d["alb"]), P(d["alb"]), *[P(t) for t in fl])
    else:   # the request together with a by-band request, ahead of an entry that honours either alone
        bnd = [torch.full((ncol, nlay + 1, len(lims)), float("nan"), device=dev) for _ in range(3)]
        assert L.rrtmgpnn_solver_request_byband(c, len(lims), int_array(lims.ravel()), *[P(t) for t in bnd]) == OK
        rc = L.rrtmgpnn_sw_solver_2stream_inc(c, ngpt, nlay, ncol, 1, P(d["toa"]), None, P(d["tau"]), P(d["ssa"]), None,
                                              *bands, P(d["mu0"]), P(d["alb"]), P(d["alb"]), *[P(t) for t in fl[:3]])
        assert rc == ERR_UNSUPPORTED and "by-band" in last_error(), last_error()
        assert all(torch.isnan(t).all() for t in bnd)
    if entry != "byband":
        assert rc == ERR_ARGUMENT, (rc, last_error())
        msg = last_error()
        assert all(w in msg for w in ("sw_solver_2stream,", "sw_solver_2stream_inc", "sw_solver_2stream_rfmip")), msg
    torch.cuda.synchronize()
    assert all(torch.isnan(t).all() for t in fl), "a refused call wrote fluxes"
    plain_result_follows(dev)


def test_request_arguments(dev):
    L, c = lib(), own_ctx().h
    word = torch.full((1,), 2, dtype=torch.int32, device=dev)
    assert L.rrtmgpnn_solver_request_active_columns(c, -1, P(word)) == ERR_ARGUMENT
    assert L.rrtmgpnn_solver_request_active_columns(None, 5, P(word)) == ERR_ARGUMENT
    # ncol other than the call's
    assert L.rrtmgpnn_solver_request_active_columns(c, 4, P(word)) == OK
    rc, _, got = run_solver(dev, "plain-g224-l4-top1", 2, arm=False)
    assert rc == ERR_ARGUMENT and "ncol" in last_error() and all(np.isnan(g).all() for g in got)
    # a null word disarms
    assert L.rrtmgpnn_solver_request_active_columns(c, 5, P(word)) == OK
    assert L.rrtmgpnn_solver_request_active_columns(c, 5, None) == OK
    plain_result_follows(dev)


# ---- the Python class layer: plan, gather, rte_sw(active=), scatter ---------------------------------------------------
def test_class_layer_plan_gather_rte_sw_scatter(dev):
    """A caller that holds mu0 (kind 1): the dense arrays' rows past the count are NaN and never read; the scattered
    fluxes are the oracle's on the daylit columns and 0 elsewhere."""
    from rrtmgpnn import api, daylit, data
    _, ncol, _, p, want = solver_problem("plain-g224-l4-top1")
    kd = data.load_kdist("sw")
    bound = float(np.sort(p["mu0"])[ncol // 2 - 1])   # the columns with mu0 above it are "daylit"
    idx, slot, nday = daylit.plan_host(p["mu0"], daylit.KIND_GT, bound)
    assert 0 < nday < ncol
    src = {k: T(p[k], dev) for k in ("tau", "ssa", "mu0", "toa", "alb")}
    pl = daylit.plan(src["mu0"], daylit.KIND_GT, bound)
    dense = {k: torch.full_like(v, float("nan")) for k, v in src.items()}
    daylit.gather(pl, [(src[k], dense[k]) for k in src])
    op = api.OpticalProps2str()
    assert op.init(kd["band_lims_wvn"], kd["band_lims_gpt"]) == ""
    op.tau, op.ssa, op.g = dense["tau"], dense["ssa"], None
    nlev = p["tau"].shape[1] + 1
    d_fl = [torch.full((ncol, nlev), float("nan"), device=dev) for _ in range(3)]
    fl = api.FluxesBroadband(flux_up=d_fl[0], flux_dn=d_fl[1], flux_dn_dir=d_fl[2])
    assert api.rte_sw(op, True, dense["mu0"], dense["toa"], dense["alb"], dense["alb"], fl, active=pl) == ""
    out = [torch.full((ncol, nlev), float("nan"), device=dev) for _ in range(3)]
    daylit.scatter(pl, list(zip(d_fl, out)))
    torch.cuda.synchronize()
    assert int(pl.nday.item()) == nday
    day = slot >= 0
    for d, o, w, k in zip(d_fl, out, want, ("up", "dn", "dir")):
        assert torch.isnan(d[nday:]).all(), "flux_%s rows at or past the count were written" % k
        np.testing.assert_array_equal(bits(o.cpu().numpy()), bits(np.where(day[:, None], w, F32(0))), err_msg=k)
    gp = torch.zeros((ncol, nlev, p["tau"].shape[2]), device=dev)
    flex = api.FluxesFlexible(flux_up=d_fl[0], flux_dn=d_fl[1], flux_dn_dir=d_fl[2], gpt_flux_up=gp)
    assert "active columns" in api.rte_sw(op, True, dense["mu0"], dense["toa"], dense["alb"], dense["alb"], flex, active=pl)
