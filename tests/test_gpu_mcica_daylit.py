"""GPU: McICA clouds and aerosols on compacted daylit columns, bit for bit.

  * the four rrtmgpnn_sampled_mask_*_active entries against the rows idx[j] of their full-extent twins' packed masks
    (tests/test_mcica_daylit_host.py restates the compact mask on the CPU and holds the cases, tests/mcica_daylit_cases.py,
    to their non-vacuity): every pattern's count, rows at or past the count keeping a prefill, a count word outside
    [0, ncol] clamped, col0 != 0;
  * solver family 8 (the active-column count beside a cloud mask and / or an aerosol) on rrtmgpnn_sw_solver_2stream_inc
    and _rfmip: SOLVER_ROWS holds every instance of the family's list to a row; rows below the count against the oracle
    (mask bits -> draw_samples in numpy -> increment_bybnd by the aerosol, then by the sampled cloud -> sw_solver) and
    against the same call at full extent without the count; rows at or past it keep their NaN prefill; the plane-free
    twins run in a child process started fresh with RRTMGPNN_SW_NO_PLANES=1;
  * the refusals that remain: their codes, nothing written, every request cleared (a plain call afterwards solves every
    column on family 2); mask or aerosol extents other than the call's;
  * the class layer: plan, gather, compact mask, arm_cloud_mask (and arm_aerosol), rte_sw(active=, band_inc=), scatter."""
import ctypes
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import mcica_daylit_cases as C
import mcica_ref as M

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
OK, ERR_ARGUMENT, ERR_UNSUPPORTED = 0, 1, 4
# rrtmgpnn_context_get_solver_path: family 8, family 2's option bits and 2048
SW_CK, SW_CK_ACTIVE_SKY = 2, 8
CK_INC, CK_TN, CK_PAIR, CK_MASK, CK_AER, CK_ACTIVE = 2, 8, 32, 128, 256, 2048
N_SKY_INSTANCES = 8


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a device"
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def T(a, dev, dtype=np.float32):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device=dev)


def words_t(bits, dev):
    """packed uint32 words as the int32 device tensor torch holds them in"""
    return torch.as_tensor(np.ascontiguousarray(bits, np.uint32).view(np.int32), device=dev)


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


# ---- the compact mask entries ----------------------------------------------------------------------------------------
def rng_words(dev, col0):
    L, c = lib(), own_ctx().h
    rng = torch.zeros(4, dtype=torch.int32, device=dev)
    assert L.rrtmgpnn_mcica_rng_set(c, C.SEED, C.STREAM, col0, P(rng)) == OK, last_error()
    return rng


def mask_call(dev, route, exp_ran, ngpt, d, rng, plan=None, out=None):
    """The route's full-extent entry (plan None: packed words only) or its _active twin on (idx, count word) -> rc"""
    L, c = lib(), own_ctx().h
    ncol, nlay = d["cf"].shape
    name = "rrtmgpnn_sampled_mask_%s%s%s" % ("exp_ran" if exp_ran else "max_ran", "_seeded" if route == "seeded" else "",
                                              "_active" if plan else "")
    args = [c, ngpt, nlay, ncol, P(rng if route == "seeded" else d["r"]), P(d["cf"])]
    if exp_ran:
        args.append(P(d["ov"]) if nlay > 1 else None)
    args += [P(plan[0]), P(plan[1]), P(out)] if plan else [None, P(out)]
    return getattr(L, name)(*args)


@pytest.mark.parametrize("route", ["array", "seeded"])
@pytest.mark.parametrize("overlap", ["max_ran", "exp_ran"])
@pytest.mark.parametrize("shape", C.CASES, ids=lambda s: "g%d-l%d-c%d" % s)
def test_compact_masks_are_the_full_masks_rows(dev, shape, overlap, route):
    from rrtmgpnn import daylit
    ngpt, nlay, ncol = shape
    nw = (ngpt + 31) // 32
    exp_ran = overlap == "exp_ran"
    r, cf, ov = C.inputs(ngpt, nlay, ncol)
    d = {"r": T(r, dev), "cf": T(cf, dev), "ov": T(ov, dev)}
    prefill = np.uint32(C.PREFILL).view(np.int32).item()
    counts = set()
    for col0 in C.COL0 if route == "seeded" else (0,):
        rng = rng_words(dev, col0) if route == "seeded" else None
        full = torch.full((ncol, nlay, nw), prefill, dtype=torch.int32, device=dev)
        assert mask_call(dev, route, exp_ran, ngpt, d, rng, out=full) == OK, last_error()
        torch.cuda.synchronize()
        want = full.cpu().numpy().view(np.uint32)
        m = M.unpack_bits(want, ngpt)
        assert m.any() and not m.all(), "the full mask is all set or all clear"
        np.testing.assert_array_equal(m, C.full_mask(route, col0, ngpt, r, cf, ov if exp_ran else None))

        def compact(idx, word):
            out = torch.full((ncol, nlay, nw), prefill, dtype=torch.int32, device=dev)
            assert mask_call(dev, route, exp_ran, ngpt, d, rng, plan=(idx, word), out=out) == OK, last_error()
            torch.cuda.synchronize()
            return out.cpu().numpy().view(np.uint32)

        for pattern in C.PATTERNS:
            pl = daylit.plan(T(C.sun(ncol, pattern), dev))
            idx = pl.idx.cpu().numpy()
            nday = int(pl.nday.item())
            counts.add(nday)
            got = compact(pl.idx, pl.nday)
            np.testing.assert_array_equal(got[:nday], want[idx[:nday]], err_msg="%s col0 %d" % (pattern, col0))
            assert (got[nday:] == np.uint32(C.PREFILL)).all(), "%s: rows at or past the count were written" % pattern
        # a count word outside [0, ncol] is clamped: idx is a permutation, so every row is some column's mask
        perm = torch.as_tensor(np.arange(ncol - 1, -1, -1, dtype=np.int32), device=dev)
        for word, n in ((-3, 0), (ncol + 7, ncol)):
            got = compact(perm, torch.full((1,), word, dtype=torch.int32, device=dev))
            np.testing.assert_array_equal(got[:n], want[::-1][:n], err_msg="count word %d" % word)
            assert (got[n:] == np.uint32(C.PREFILL)).all(), "count word %d: rows past the clamped count" % word
    assert {0, 1, ncol - 1, ncol} <= counts


def test_compact_mask_arguments(dev):
    ngpt, nlay, ncol = 33, 5, 5
    r, cf, ov = C.inputs(ngpt, nlay, ncol)
    d = {"r": T(r, dev), "cf": T(cf, dev), "ov": T(ov, dev)}
    rng = rng_words(dev, 0)
    idx = torch.arange(ncol, dtype=torch.int32, device=dev)
    word = torch.full((1,), ncol, dtype=torch.int32, device=dev)
    out = torch.full((ncol, nlay, 2), 7, dtype=torch.int32, device=dev)
    L, c = lib(), own_ctx().h
    for route in ("array", "seeded"):
        for exp_ran in (False, True):
            for plan, o in (((None, word), out), ((idx, None), out), ((idx, word), None)):
                name = "rrtmgpnn_sampled_mask_%s%s_active" % ("exp_ran" if exp_ran else "max_ran",
                                                              "_seeded" if route == "seeded" else "")
                args = [c, ngpt, nlay, ncol, P(rng if route == "seeded" else d["r"]), P(d["cf"])]
                args += ([P(d["ov"])] if exp_ran else []) + [P(plan[0]), P(plan[1]), P(o)]
                assert getattr(L, name)(*args) == ERR_ARGUMENT and "NULL" in last_error(), name
    # the full-extent twins' checks and messages
    assert L.rrtmgpnn_sampled_mask_max_ran_seeded_active(c, ngpt, nlay, ncol, None, P(d["cf"]), P(idx), P(word), P(out)) \
        == ERR_ARGUMENT and "rng is NULL" in last_error()
    assert L.rrtmgpnn_sampled_mask_exp_ran_active(c, ngpt, nlay, ncol, P(d["r"]), P(d["cf"]), None, P(idx), P(word),
                                                  P(out)) == ERR_ARGUMENT and "bad argument" in last_error()
    assert L.rrtmgpnn_sampled_mask_max_ran_active(c, ngpt, 0, ncol, P(d["r"]), P(d["cf"]), P(idx), P(word), P(out)) \
        == ERR_ARGUMENT
    assert L.rrtmgpnn_sampled_mask_max_ran_active(None, ngpt, nlay, ncol, P(d["r"]), P(d["cf"]), P(idx), P(word), P(out)) \
        == ERR_ARGUMENT
    assert L.rrtmgpnn_sampled_mask_max_ran_active(c, ngpt, nlay, 0, P(d["r"]), P(d["cf"]), P(idx), P(word), P(out)) == OK
    torch.cuda.synchronize()
    assert bool((out == 7).all()), "a refused or empty call wrote the mask"


# ---- the gather of long rows (an aerosol's band arrays) -----------------------------------------------------------------
LONG_ROWS = (256, 840, 1001)   # the threshold of the long-row kernel, 14 bands x 60 layers, an odd length
GUARD, SENTINEL = 32, -777.0


@pytest.mark.parametrize("pattern", ["random", "day", "night", "last"])
@pytest.mark.parametrize("ncol", [1, 65, 200])
def test_gather_of_long_rows_equals_numpy_indexing(dev, ncol, pattern):
    """Tables whose rows are all long take a kernel of their own (a block per column and array): rows one float off the
    allocation's alignment, guard floats on both sides, the rows at or past the count untouched."""
    from rrtmgpnn import daylit
    rng = np.random.default_rng(ncol)
    idx, _, nday = daylit.plan_host(C.sun(ncol, pattern), daylit.KIND_LT, daylit.SZA_BOUND)
    pl = daylit.plan(T(C.sun(ncol, pattern), dev))
    src = [rng.standard_normal((ncol, r)).astype(F32) for r in LONG_ROWS]
    dsrc = [T(a, dev) for a in src]
    bufs = [torch.full((1 + ncol * r + GUARD,), SENTINEL, device=dev) for r in LONG_ROWS]
    views = [b[1:1 + ncol * r].view(ncol, r) for b, r in zip(bufs, LONG_ROWS)]
    for v in views:
        v.fill_(float("nan"))
        assert v.data_ptr() % 16 == 4
    daylit.gather(pl, list(zip(dsrc, views)))
    torch.cuda.synchronize()
    for a, b, v, r in zip(src, bufs, views, LONG_ROWS):
        got = v.cpu().numpy()
        np.testing.assert_array_equal(bits(got[:nday]), bits(a[idx[:nday]]), err_msg="rows of %d" % r)
        assert np.isnan(got[nday:]).all(), "gather wrote rows at or past nday (rows of %d)" % r
        assert bool((b[:1] == SENTINEL).all()) and bool((b[1 + ncol * r:] == SENTINEL).all())


# ---- solver family 8 ------------------------------------------------------------------------------------------------
GENERAL_LIMS = ((1, 15), (16, 224))   # band 2 starts at an even 1-based g-point: not the band-pair layout
NACTS = (0, 1, 2, 3, 5)   # odd: a block's second column is inactive; 0: every block exits
KINDS = {"mask": CK_MASK, "mask-aer": CK_MASK | CK_AER, "aer": CK_AER}


def row(name, form, kind, options, ngpt=224, nlay=4, top=1, lims=None, child=False):
    return dict(name=name, form=form, kind=kind, options=options | KINDS[kind] | CK_INC | CK_ACTIVE, ngpt=ngpt, nlay=nlay,
                top=top, lims=lims, child=child)


def _rows():
    rows = []
    for ngpt in (224, 112):
        for nlay in (4, 7):   # neither a multiple of the chunk length 3
            for top in (1, 0):
                t = "g%d-l%d-top%d" % (ngpt, nlay, top)
                for kind in KINDS:
                    rows += [row("inc-%s-%s" % (kind, t), "inc", kind, CK_PAIR | CK_TN, ngpt, nlay, top),
                             row("rfmip-%s-%s" % (kind, t), "rfmip", kind, CK_PAIR | CK_TN, ngpt, nlay, top)]
    rows += [row("inc-mask-general", "inc", "mask", CK_TN, lims=GENERAL_LIMS),
             row("rfmip-mask-general", "rfmip", "mask", CK_TN, lims=GENERAL_LIMS, nlay=7, top=0)]
    # RRTMGPNN_SW_NO_PLANES=1 (a fresh process): the plane-free twins
    rows += [row("inc-%s-noplanes" % kind, "inc", kind, CK_PAIR, child=True) for kind in KINDS]
    rows += [row("rfmip-mask-aer-noplanes", "rfmip", "mask-aer", CK_PAIR, nlay=7, top=0, child=True),
             row("inc-mask-general-noplanes", "inc", "mask", 0, lims=GENERAL_LIMS, child=True)]
    return rows


SOLVER_ROWS = _rows()
HERE_ROWS = [r for r in SOLVER_ROWS if not r["child"]]
CHILD_ROWS = [r for r in SOLVER_ROWS if r["child"]]


def test_solver_rows_hold_every_listed_instance():
    assert len({r["name"] for r in SOLVER_ROWS}) == len(SOLVER_ROWS)
    assert len({r["options"] for r in SOLVER_ROWS}) == N_SKY_INSTANCES
    pl = CK_TN
    assert {r["options"] for r in SOLVER_ROWS} == {
        CK_ACTIVE | CK_INC | o for o in (CK_MASK | CK_PAIR | pl, CK_MASK | CK_PAIR, CK_MASK | pl, CK_MASK,
                                         CK_MASK | CK_AER | CK_PAIR | pl, CK_MASK | CK_AER | CK_PAIR,
                                         CK_AER | CK_PAIR | pl, CK_AER | CK_PAIR)}


def make_mask(rng, ncol, nlay, ngpt):
    """A mask with set and clear bits in every word of most layers, a layer all clear and a layer all set"""
    m = rng.random((ncol, nlay, ngpt)) < 0.5
    m[:, 1 % nlay] &= rng.random((ncol, ngpt)) < 0.1
    m[ncol // 2, 0] = False
    m[ncol - 1, nlay - 1] = True
    return m


@functools.lru_cache(maxsize=None)
def solver_problem(name):
    """The row's inputs and the oracle's fluxes of every column (the columns are independent)"""
    import oracle as O
    from rrtmgpnn import data
    r = next(r for r in SOLVER_ROWS if r["name"] == name)
    ngpt, nlay, ncol = r["ngpt"], r["nlay"], 5
    kd = data.load_kdist("sw", None if ngpt == 224 else ngpt)
    lims = np.asarray(r["lims"] or kd["band_lims_gpt"], np.int32)
    nb = len(lims)
    rng = np.random.default_rng(2000 * ngpt + 10 * nlay + r["top"] + 7 * len(r["form"]) + 13 * len(r["kind"]))
    u = lambda lo, hi, *s: rng.uniform(lo, hi, s).astype(F32)  # noqa: E731
    p = dict(tau=rng.lognormal(-2, 1.5, (ncol, nlay, ngpt)).astype(F32), ssa=u(0.1, 0.95, ncol, nlay, ngpt),
             tb=rng.lognormal(-1, 1, (ncol, nlay, nb)).astype(F32), wb=u(0.3, 0.95, ncol, nlay, nb),
             gb=u(0.3, 0.9, ncol, nlay, nb), ta=rng.lognormal(-2, 1, (ncol, nlay, nb)).astype(F32),
             wa=u(0.6, 1, ncol, nlay, nb), ga=u(0.3, 0.8, ncol, nlay, nb), tsi=u(1300, 1400, ncol),
             sfc_alb=u(0.05, 0.6, ncol), sza=np.where(rng.random(ncol) < 0.7, u(0, 85, ncol), u(91, 119, ncol)).astype(F32))
    p["solar_source"] = data.set_tsi(kd["solar_source"], 1361.0)
    mask = make_mask(rng, ncol, nlay, ngpt)
    p["bits"] = M.pack_bits(mask)
    if r["form"] == "rfmip":
        use = p["sza"] < F32(90.0) - F32(2.0) * data.spacing(90.0)
        deg = F32(np.arccos(F32(-1.0)) / F32(180.0))
        p["mu0"] = np.where(use, data.ref_cosf(p["sza"] * deg), F32(1.0)).astype(F32)
        p["toa"] = data.toa_flux({"ncol": ncol, "tsi": p["tsi"]}, kd)
        p["alb"] = np.repeat(p["sfc_alb"][:, None], ngpt, axis=1)
    else:
        p["mu0"], p["toa"], p["alb"] = u(0.1, 1, ncol), u(0.1, 10, ncol, ngpt), u(0, 0.9, ncol, ngpt)
    orc = O.Oracle()
    io = (p["tau"], p["ssa"], np.zeros_like(p["tau"]))
    if "aer" in r["kind"]:
        io = orc.increment_bybnd(lims, io, (p["ta"], p["wa"], p["ga"]))
    if "mask" in r["kind"]:   # the mask's bits -> draw_samples -> an increment at g-point resolution
        m = M.unpack_bits(p["bits"], ngpt)
        assert m.any() and not m.all()
        ident = np.stack([np.arange(1, ngpt + 1)] * 2, axis=1).astype(np.int32)
        io = orc.increment_bybnd(ident, io, [M.draw(m, p[k], lims) for k in ("tb", "wb", "gb")])
    else:
        io = orc.increment_bybnd(lims, io, (p["tb"], p["wb"], p["gb"]))
    want = orc.sw_solver(*io, p["mu0"], p["toa"], p["alb"], p["alb"], bool(r["top"]))
    assert all(np.isfinite(w).all() for w in want)
    return r, ncol, lims, p, want


def run_solver(dev, name, nact, mask=None, aer=None, ext=None, g=False, ctx=None):
    """The row's call with its requests armed (nact None: no active-column request; mask / aer: override the row's kind;
    ext: {"mask": ncol, "aer": ncol}, the extents the requests state) -> (rc, path, [up, dn, dir] prefilled with NaN)"""
    from rrtmgpnn._lib import int_array
    r, ncol, lims, p, _ = solver_problem(name)
    L, c = lib(), (ctx or own_ctx()).h
    d = {k: (words_t(v, dev) if k == "bits" else T(v, dev)) for k, v in p.items()}
    ngpt, nlay, nb = r["ngpt"], r["nlay"], len(lims)
    ext = ext or {}
    fl = [torch.full((ncol, nlay + 1), float("nan"), device=dev) for _ in range(3)]
    if ("mask" in r["kind"]) if mask is None else mask:
        assert L.rrtmgpnn_solver_request_cloud_mask(c, ngpt, nlay, ext.get("mask", ncol), P(d["bits"])) == OK
    if ("aer" in r["kind"]) if aer is None else aer:
        assert L.rrtmgpnn_solver_request_aerosol(c, nb, nlay, ext.get("aer", ncol), P(d["ta"]), P(d["wa"]), P(d["ga"])) == OK
    if nact is not None:
        word = torch.full((1,), nact, dtype=torch.int32, device=dev)
        assert L.rrtmgpnn_solver_request_active_columns(c, ncol, P(word)) == OK
    gas_g = P(torch.zeros_like(d["tau"])) if g else None
    bands = [nb, int_array(lims.ravel()), P(d["tb"]), P(d["wb"]), P(d["gb"])]
    head = [c, ngpt, nlay, ncol, r["top"]]
    outs = [P(t) for t in fl]
    if r["form"] == "rfmip":
        scratch = [torch.zeros(ncol, ngpt, device=dev), torch.zeros(ncol, ngpt, device=dev), torch.zeros(ncol, device=dev)]
        rc = L.rrtmgpnn_sw_solver_2stream_rfmip(*head, P(d["solar_source"]), P(d["tsi"]), P(d["sfc_alb"]), P(d["sza"]),
                                                P(d["tau"]), P(d["ssa"]), gas_g, *bands, *[P(t) for t in scratch], *outs)
    else:
        rc = L.rrtmgpnn_sw_solver_2stream_inc(*head, P(d["toa"]), None, P(d["tau"]), P(d["ssa"]), gas_g, *bands,
                                              P(d["mu0"]), P(d["alb"]), P(d["alb"]), *outs)
    torch.cuda.synchronize()
    path = (ctypes.c_int * 4)()
    assert L.rrtmgpnn_context_get_solver_path(c, path) == OK
    return rc, list(path), [t.cpu().numpy() for t in fl]


def check_row(name, nact, rc, path, got, full):
    r, ncol, _, _, want = solver_problem(name)
    assert rc == OK, "%s nact %d: %s" % (name, nact, last_error())
    for g, w, f, k in zip(got, want, full, ("up", "dn", "dir")):
        np.testing.assert_array_equal(bits(g[:nact]), bits(w[:nact]), err_msg="%s nact %d: flux_%s, oracle" % (name, nact, k))
        np.testing.assert_array_equal(bits(g[:nact]), bits(f[:nact]),
                                      err_msg="%s nact %d: flux_%s, the call at full extent" % (name, nact, k))
        assert np.isnan(g[nact:]).all(), "%s nact %d: flux_%s rows at or past nact were written" % (name, nact, k)
    assert path == [SW_CK_ACTIVE_SKY, r["options"], 1, N_SKY_INSTANCES], (name, nact, path)


def full_extent(dev, name):
    """The row's call without the count: every column, on family 2 with the row's options less the active bit"""
    r, _, _, _, want = solver_problem(name)
    rc, path, full = run_solver(dev, name, None)
    assert rc == OK, last_error()
    assert path[:2] == [SW_CK, r["options"] & ~CK_ACTIVE], (name, path)
    for f, w in zip(full, want):
        np.testing.assert_array_equal(bits(f), bits(w), err_msg=name + ": the call at full extent against the oracle")
    return full


@pytest.mark.parametrize("name", [r["name"] for r in HERE_ROWS])
def test_solver_on_the_active_columns(dev, name):
    assert "RRTMGPNN_SW_NO_PLANES" not in os.environ
    full = full_extent(dev, name)
    for nact in NACTS:
        check_row(name, nact, *run_solver(dev, name, nact), full)


def child_main(out_json, out_npz):
    """The plane-free rows (the parent process set RRTMGPNN_SW_NO_PLANES=1): codes and paths to JSON, fluxes to npz"""
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    meta, flux = {}, {}
    for r in CHILD_ROWS:
        for nact in (None,) + NACTS:
            rc, path, got = run_solver(dev, r["name"], nact)
            meta["%s/%s" % (r["name"], nact)] = [rc, path, last_error() if rc else ""]
            for k, a in zip(("up", "dn", "dir"), got):
                flux["%s/%s/%s" % (r["name"], nact, k)] = a
    json.dump(meta, open(out_json, "w"))
    np.savez(out_npz, **flux)


def test_solver_plane_free_instances_in_a_child_process(dev, tmp_path):
    oj, on = str(tmp_path / "meta.json"), str(tmp_path / "flux.npz")
    code = ("import sys; sys.path[:0] = [%r, %r, %r]; import test_gpu_mcica_daylit as D; D.child_main(%r, %r)"
            % (os.path.join(ROOT, "tests"), os.path.join(ROOT, "rte-rrtmgp-nn_amd"), os.path.join(ROOT, "oracle"), oj, on))
    env = dict(os.environ, RRTMGPNN_SW_NO_PLANES="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    meta, flux = json.load(open(oj)), np.load(on)
    for r in CHILD_ROWS:
        fl = lambda nact: [flux["%s/%s/%s" % (r["name"], nact, k)] for k in ("up", "dn", "dir")]  # noqa: E731
        rc, path, msg = meta["%s/None" % r["name"]]
        assert rc == OK and path[:2] == [SW_CK, r["options"] & ~CK_ACTIVE], (msg, path)
        for nact in NACTS:
            rc, path, msg = meta["%s/%d" % (r["name"], nact)]
            assert rc == OK, msg
            check_row(r["name"], nact, rc, path, fl(nact), fl(None))


# ---- the refusals that remain -----------------------------------------------------------------------------------------
ROW = "inc-mask-aer-g224-l4-top1"


def plain_result_follows(dev, ctx=None):
    """A call with nothing armed after a refusal: every request is gone, every column is solved on family 2 with the
    plain band increment (no mask, no aerosol)"""
    import oracle as O
    r, ncol, lims, p, _ = solver_problem(ROW)
    rc, path, got = run_solver(dev, ROW, None, mask=False, aer=False, ctx=ctx)
    assert rc == OK, last_error()
    assert path[:2] == [SW_CK, CK_INC | CK_PAIR | CK_TN], path
    orc = O.Oracle()
    io = orc.increment_bybnd(lims, (p["tau"], p["ssa"], np.zeros_like(p["tau"])), (p["tb"], p["wb"], p["gb"]))
    for g, w in zip(got, orc.sw_solver(*io, p["mu0"], p["toa"], p["alb"], p["alb"], bool(r["top"]))):
        np.testing.assert_array_equal(bits(g), bits(w))


def arm_all(dev, d, ncol, nlay, ngpt, nb, paired_bnd=None):
    L, c = lib(), own_ctx().h
    word = torch.full((1,), 2, dtype=torch.int32, device=dev)
    if paired_bnd is None:
        assert L.rrtmgpnn_solver_request_cloud_mask(c, ngpt, nlay, ncol, P(d["bits"])) == OK
    assert L.rrtmgpnn_solver_request_aerosol(c, nb, nlay, ncol, P(d["ta"]), P(d["wa"]), P(d["ga"])) == OK
    assert L.rrtmgpnn_solver_request_active_columns(c, ncol, P(word)) == OK
    return word


@pytest.mark.parametrize("what", ["paired-byband", "byband", "plain-entry", "gpt-entry", "clr_all-entry",
                                  "rfmip_clr_all-entry", "gas-g", "sw-kernel-1", "sw-kernel-2", "odd-ngpt",
                                  "aerosol-general-limits", "rfmip-no-increment"])
def test_remaining_refusals_clear_every_request(dev, what):
    from rrtmgpnn._lib import int_array
    r, ncol, lims, p, _ = solver_problem(ROW)
    L, ctx = lib(), own_ctx()
    c = ctx.h
    ngpt, nlay, nb = r["ngpt"], r["nlay"], len(lims)
    d = {k: (words_t(v, dev) if k == "bits" else T(v, dev)) for k, v in p.items()}
    fl = [torch.full((ncol, nlay + 1), float("nan"), device=dev) for _ in range(6)]
    extra = [torch.full((ncol, nlay + 1, max(nb, ngpt)), float("nan"), device=dev) for _ in range(3)]
    bands = [nb, int_array(lims.ravel()), P(d["tb"]), P(d["wb"]), P(d["gb"])]
    head = [c, ngpt, nlay, ncol, 1]
    tail = [P(d["mu0"]), P(d["alb"]), P(d["alb"])]
    inc = lambda gas_g=None, b=bands, h=head, o=fl[:3]: L.rrtmgpnn_sw_solver_2stream_inc(  # noqa: E731
        *h, P(d["toa"]), None, P(d["tau"]), P(d["ssa"]), gas_g, *b, *tail, *[P(t) for t in o])
    scratch = [torch.zeros(ncol, ngpt, device=dev), torch.zeros(ncol, ngpt, device=dev), torch.zeros(ncol, device=dev)]
    rf = [P(d["solar_source"]), P(d["tsi"]), P(d["sfc_alb"]), P(d["sza"]), P(d["tau"]), P(d["ssa"]), None]
    code, word = ERR_UNSUPPORTED, None
    if what == "paired-byband":
        bnd = [t[:, :, :nb].contiguous() for t in extra]
        assert L.rrtmgpnn_solver_request_byband_mcica(c, nb, int_array(lims.ravel()), *[P(t) for t in bnd], ngpt, nlay,
                                                      ncol, P(d["bits"])) == OK
        keep = arm_all(dev, d, ncol, nlay, ngpt, nb, paired_bnd=bnd)
        rc = inc()
        word = "by-band"
        assert all(torch.isnan(t).all() for t in bnd)
    elif what == "byband":
        keep = arm_all(dev, d, ncol, nlay, ngpt, nb)
        bnd = [t[:, :, :nb].contiguous() for t in extra]
        assert L.rrtmgpnn_solver_request_byband(c, nb, int_array(lims.ravel()), *[P(t) for t in bnd]) == OK
        rc = inc()
        word = "by-band"
        assert all(torch.isnan(t).all() for t in bnd)
    elif what in ("plain-entry", "gpt-entry"):
        keep = arm_all(dev, d, ncol, nlay, ngpt, nb)
        if what == "plain-entry":
            rc = L.rrtmgpnn_sw_solver_2stream(*head, P(d["toa"]), None, P(d["tau"]), P(d["ssa"]), None, *tail,
                                              *[P(t) for t in fl[:3]])
        else:
            rc = L.rrtmgpnn_sw_solver_2stream_gpt(*head, P(d["toa"]), None, P(d["tau"]), P(d["ssa"]), None, *tail,
                                                  *[P(t) for t in fl[:3]], *[P(t) for t in extra])
            assert all(torch.isnan(t).all() for t in extra)
    elif what == "clr_all-entry":
        keep = arm_all(dev, d, ncol, nlay, ngpt, nb)
        rc = L.rrtmgpnn_sw_solver_2stream_clr_all(*head, P(d["toa"]), None, P(d["tau"]), P(d["ssa"]), None, *bands, *tail,
                                                  *[P(t) for t in fl])
        code, word = ERR_ARGUMENT, "sw_solver_2stream_rfmip"
    elif what == "rfmip_clr_all-entry":
        keep = arm_all(dev, d, ncol, nlay, ngpt, nb)
        rc = L.rrtmgpnn_sw_solver_2stream_rfmip_clr_all(*head, *rf, *bands, *[P(t) for t in scratch], *[P(t) for t in fl])
        code, word = ERR_ARGUMENT, "sw_solver_2stream_rfmip"
    elif what == "gas-g":
        keep = arm_all(dev, d, ncol, nlay, ngpt, nb)
        rc = inc(gas_g=P(torch.zeros_like(d["tau"])))
        word = "gas g"
    elif what.startswith("sw-kernel"):
        keep = arm_all(dev, d, ncol, nlay, ngpt, nb)
        ctx.set_sw_kernel(int(what[-1]))
        try:
            rc = inc()
        finally:
            ctx.set_sw_kernel(0)
        word = "checkpointed"
    elif what == "odd-ngpt":
        # 223 g-points: the last band one short; the mask keeps its seven words
        lims_odd = lims.copy()
        lims_odd[-1, 1] = ngpt - 1
        odd = {k: d[k][..., :ngpt - 1].contiguous() for k in ("tau", "ssa", "toa", "alb")}
        keep = torch.full((1,), 2, dtype=torch.int32, device=dev)
        assert L.rrtmgpnn_solver_request_cloud_mask(c, ngpt - 1, nlay, ncol, P(d["bits"])) == OK
        assert L.rrtmgpnn_solver_request_aerosol(c, nb, nlay, ncol, P(d["ta"]), P(d["wa"]), P(d["ga"])) == OK
        assert L.rrtmgpnn_solver_request_active_columns(c, ncol, P(keep)) == OK
        rc = L.rrtmgpnn_sw_solver_2stream_inc(c, ngpt - 1, nlay, ncol, 1, P(odd["toa"]), None, P(odd["tau"]), P(odd["ssa"]),
                                              None, nb, int_array(lims_odd.ravel()), P(d["tb"]), P(d["wb"]), P(d["gb"]),
                                              P(d["mu0"]), P(odd["alb"]), P(odd["alb"]), *[P(t) for t in fl[:3]])
        word = "checkpointed"
    elif what == "aerosol-general-limits":
        gl = np.asarray(GENERAL_LIMS, np.int32)
        keep = torch.full((1,), 2, dtype=torch.int32, device=dev)
        two = {k: d[k][..., :2].contiguous() for k in ("tb", "wb", "gb", "ta", "wa", "ga")}
        assert L.rrtmgpnn_solver_request_aerosol(c, 2, nlay, ncol, P(two["ta"]), P(two["wa"]), P(two["ga"])) == OK
        assert L.rrtmgpnn_solver_request_active_columns(c, ncol, P(keep)) == OK
        rc = inc(b=[2, int_array(gl.ravel()), P(two["tb"]), P(two["wb"]), P(two["gb"])])
        word = "band-pair"
    else:   # rfmip-no-increment: nbnd == 0 beside a mask
        keep = torch.full((1,), 2, dtype=torch.int32, device=dev)
        assert L.rrtmgpnn_solver_request_cloud_mask(c, ngpt, nlay, ncol, P(d["bits"])) == OK
        assert L.rrtmgpnn_solver_request_active_columns(c, ncol, P(keep)) == OK
        rc = L.rrtmgpnn_sw_solver_2stream_rfmip(*head, *rf, 0, None, None, None, None, *[P(t) for t in scratch],
                                                *[P(t) for t in fl[:3]])
        code, word = ERR_ARGUMENT, "nbnd > 0"
    msg = last_error()
    assert rc == code, (what, rc, msg)
    assert word is None or word in msg, (what, msg)
    torch.cuda.synchronize()
    assert all(torch.isnan(t).all() for t in fl), what + ": a refused call wrote fluxes"
    del keep
    plain_result_follows(dev)


@pytest.mark.parametrize("which", ["mask", "aer"])
def test_request_extents_other_than_the_calls(dev, which):
    rc, _, got = run_solver(dev, ROW, 2, ext={which: 4})
    assert rc == ERR_ARGUMENT and "extents" in last_error(), last_error()
    assert all(np.isnan(g).all() for g in got)
    plain_result_follows(dev)


# ---- the Python class layer: plan, gather, compact mask, arm_cloud_mask, rte_sw(active=), scatter ----------------------
@pytest.mark.parametrize("aerosol", [False, True], ids=["mask", "mask-aer"])
def test_class_layer_plan_gather_mask_rte_sw_scatter(dev, aerosol):
    """A caller that holds mu0 (kind 1).  The dense arrays' rows past the count are NaN and never read; the mask is
    sampled for the compacted columns from the full-extent cloud fraction and random numbers; the scattered fluxes are
    the oracle's on the daylit columns and 0 elsewhere."""
    import oracle as O
    from rrtmgpnn import api, cloud_sampling as cs, daylit, data
    name = "inc-mask-aer-g224-l7-top0" if aerosol else "inc-mask-g224-l7-top0"
    r, ncol, lims, p, _ = solver_problem(name)
    ngpt, nlay = r["ngpt"], r["nlay"]
    kd = data.load_kdist("sw")
    rng = np.random.default_rng(5)
    rnd = rng.random((ncol, nlay, ngpt), dtype=F32)
    cf = np.where(rng.random((ncol, nlay)) < 0.7, rng.uniform(0.3, 0.9, (ncol, nlay)), 0).astype(F32)
    mask = M.sampled_mask(rnd, cf, None)
    assert mask.any() and not mask[cf > 0].all()
    orc = O.Oracle()
    io = (p["tau"], p["ssa"], np.zeros_like(p["tau"]))
    if aerosol:
        io = orc.increment_bybnd(lims, io, (p["ta"], p["wa"], p["ga"]))
    ident = np.stack([np.arange(1, ngpt + 1)] * 2, axis=1).astype(np.int32)
    io = orc.increment_bybnd(ident, io, [M.draw(mask, p[k], lims) for k in ("tb", "wb", "gb")])
    want = orc.sw_solver(*io, p["mu0"], p["toa"], p["alb"], p["alb"], bool(r["top"]))
    bound = float(np.sort(p["mu0"])[ncol // 2 - 1])   # the columns with mu0 above it are "daylit"
    idx, slot, nday = daylit.plan_host(p["mu0"], daylit.KIND_GT, bound)
    assert 0 < nday < ncol
    keys = ("tau", "ssa", "mu0", "toa", "alb", "tb", "wb", "gb") + (("ta", "wa", "ga") if aerosol else ())
    src = {k: T(p[k], dev) for k in keys}
    pl = daylit.plan(src["mu0"], daylit.KIND_GT, bound)
    dense = {k: torch.full_like(v, float("nan")) for k, v in src.items()}
    daylit.gather(pl, [(src[k], dense[k]) for k in src])
    mask_bits = torch.full((ncol, nlay, (ngpt + 31) // 32), -1, dtype=torch.int32, device=dev)
    daylit.sampled_mask_active(pl, T(rnd, dev), T(cf, dev), mask_bits)   # neither randoms nor cloud_frac is gathered

    def props(t, w, g):
        op = api.OpticalProps2str()
        assert op.init(kd["band_lims_wvn"], kd["band_lims_gpt"]) == ""
        op.tau, op.ssa, op.g = t, w, g
        return op

    op = props(dense["tau"], dense["ssa"], None)
    cld = api.OpticalProps2str()
    assert cld.init(kd["band_lims_wvn"]) == ""
    cld.tau, cld.ssa, cld.g = dense["tb"], dense["wb"], dense["gb"]
    nlev = nlay + 1
    d_fl = [torch.full((ncol, nlev), float("nan"), device=dev) for _ in range(3)]
    fl = api.FluxesBroadband(flux_up=d_fl[0], flux_dn=d_fl[1], flux_dn_dir=d_fl[2])
    ctx = api.context(0)
    if aerosol:
        aer = api.OpticalProps2str()
        assert aer.init(kd["band_lims_wvn"]) == ""
        aer.tau, aer.ssa, aer.g = dense["ta"], dense["wa"], dense["ga"]
        cs.arm_aerosol(ctx, aer)
    cs.arm_cloud_mask(ctx, ngpt, mask_bits)
    assert api.rte_sw(op, bool(r["top"]), dense["mu0"], dense["toa"], dense["alb"], dense["alb"], fl, active=pl,
                      band_inc=cld) == ""
    out = [torch.full((ncol, nlev), float("nan"), device=dev) for _ in range(3)]
    daylit.scatter(pl, list(zip(d_fl, out)))
    torch.cuda.synchronize()
    path = (ctypes.c_int * 4)()
    assert lib().rrtmgpnn_context_get_solver_path(ctx.h, path) == OK
    assert list(path) == [SW_CK_ACTIVE_SKY, r["options"], 1, N_SKY_INSTANCES], list(path)
    got_bits = mask_bits.cpu().numpy().view(np.uint32)
    np.testing.assert_array_equal(got_bits[:nday], M.pack_bits(mask)[idx[:nday]])
    assert (got_bits[nday:] == np.uint32(0xFFFFFFFF)).all()
    day = slot >= 0
    for d, o, w, k in zip(d_fl, out, want, ("up", "dn", "dir")):
        assert torch.isnan(d[nday:]).all(), "flux_%s rows at or past the count were written" % k
        np.testing.assert_array_equal(bits(o.cpu().numpy()), bits(np.where(day[:, None], w, F32(0))), err_msg=k)
    # the seeded helper: the same bits as the seeded full-extent mask's rows
    rng_buf = cs._rng(ctx, C.SEED, C.STREAM, 11)
    sb = torch.zeros_like(mask_bits)
    daylit.sampled_mask_seeded_active(pl, rng_buf, T(cf, dev), sb, ngpt)
    fb = torch.zeros_like(mask_bits)
    assert cs.sampled_mask_max_ran_seeded(C.SEED, C.STREAM, 11, T(cf, dev), mask_bits=fb, ngpt=ngpt) == ""
    torch.cuda.synchronize()
    np.testing.assert_array_equal(sb.cpu().numpy()[:nday], fb.cpu().numpy()[idx[:nday]])
