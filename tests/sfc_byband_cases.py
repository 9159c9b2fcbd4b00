"""Surface by-band SW fluxes from the fused solvers (rrtmgpnn_solver_request_sfc_byband): the rows, their inputs and the
oracle's expectations, shared by tests/test_sfc_byband_host.py (CPU: the cases are not vacuous) and
tests/test_gpu_sfc_byband.py (GPU: the kernel family against them).

A row is one call: ngpt 224 or 112 with the shipped band limits (both in the band-pair layout), a depth that puts the
surface at each place of the kernel's flux ring (nine levels in chunks of three behind a one-level first flush: nlay 1
the first slot of a partial chunk, 4 and 7 a partial chunk, 9 the end of a ring exactly full, 10 one layer past a full
flush), both orientations, five columns (odd: a block's second column is idle), the three kinds of sky the request goes
with and the two entries that take it.  Expected: the oracle's g-point fluxes of the materialised problem -- aerosol
increment, then the sampled cloud's -- and sum_byband of their surface level."""
import functools

import numpy as np

import byband_ref as B
import mcica_ref as M

F32 = np.float32
NCOL = 5
NGPTS = (224, 112)
NLAYS = (1, 4, 7, 9, 10)
KINDS = ("mask", "mask-aer", "aer")
FORMS = ("inc", "rfmip")
NACTS = (None, 0, 1, 2, 3, 5)
# rrtmgpnn_context_get_solver_path: the family and the option bits of sw_2stream_ck_kernel
SW_CK, SW_CK_ACTIVE_SKY, SW_CK_SFC_BAND = 2, 8, 9
CK_INC, CK_TN, CK_PAIR, CK_MASK, CK_AER, CK_ACTIVE, CK_SFC = 2, 8, 32, 128, 256, 2048, 4096
KIND_BITS = {"mask": CK_MASK, "mask-aer": CK_MASK | CK_AER, "aer": CK_AER}
N_SFC_INSTANCES = 12


def row(form, kind, ngpt, nlay, top, child=False):
    name = "%s-%s-g%d-l%d-top%d%s" % (form, kind, ngpt, nlay, top, "-noplanes" if child else "")
    options = CK_SFC | CK_INC | CK_PAIR | KIND_BITS[kind] | (0 if child else CK_TN)
    return dict(name=name, form=form, kind=kind, ngpt=ngpt, nlay=nlay, top=top, child=child, options=options)


def _rows():
    rows = [row(form, kind, ngpt, nlay, top)
            for ngpt in NGPTS for nlay in NLAYS for top in (1, 0) for kind in KINDS for form in FORMS]
    # RRTMGPNN_SW_NO_PLANES=1 (a fresh process): the plane-free twins, one per kind
    rows += [row("inc", "mask", 224, 4, 1, child=True), row("rfmip", "mask-aer", 224, 10, 0, child=True),
             row("inc", "aer", 112, 7, 0, child=True)]
    return rows


ROWS = _rows()
HERE_ROWS = [r for r in ROWS if not r["child"]]
CHILD_ROWS = [r for r in ROWS if r["child"]]
BY_NAME = {r["name"]: r for r in ROWS}


def sfc_level(r):
    """array index of the surface level"""
    return r["nlay"] if r["top"] else 0


def make_mask(rng, ncol, nlay, ngpt):
    """A mask with set and clear bits in every word of most layers, a layer all clear and a layer all set"""
    m = rng.random((ncol, nlay, ngpt)) < 0.5
    m[:, 1 % nlay] &= rng.random((ncol, ngpt)) < 0.1
    m[ncol // 2, 0] = False
    m[ncol - 1, nlay - 1] = True
    return m


@functools.lru_cache(maxsize=None)
def inputs(name):
    """The row, its band limits (nbnd, 2) and its input arrays"""
    from rrtmgpnn import data
    r = BY_NAME[name]
    ngpt, nlay, ncol = r["ngpt"], r["nlay"], NCOL
    kd = data.load_kdist("sw", None if ngpt == 224 else ngpt)
    lims = np.asarray(kd["band_lims_gpt"], np.int32)
    nb = len(lims)
    rng = np.random.default_rng(3000 * ngpt + 10 * nlay + r["top"] + 7 * len(r["form"]) + 13 * len(r["kind"]) + r["child"])
    u = lambda lo, hi, *s: rng.uniform(lo, hi, s).astype(F32)  # noqa: E731
    p = dict(tau=rng.lognormal(-2, 1.5, (ncol, nlay, ngpt)).astype(F32), ssa=u(0.1, 0.95, ncol, nlay, ngpt),
             tb=rng.lognormal(-1, 1, (ncol, nlay, nb)).astype(F32), wb=u(0.3, 0.95, ncol, nlay, nb),
             gb=u(0.3, 0.9, ncol, nlay, nb), ta=rng.lognormal(-2, 1, (ncol, nlay, nb)).astype(F32),
             wa=u(0.6, 1, ncol, nlay, nb), ga=u(0.3, 0.8, ncol, nlay, nb), tsi=u(1300, 1400, ncol),
             sfc_alb=u(0.05, 0.6, ncol), sza=np.where(rng.random(ncol) < 0.7, u(0, 85, ncol), u(91, 119, ncol)).astype(F32))
    p["solar_source"] = data.set_tsi(kd["solar_source"], 1361.0)
    p["mask"] = make_mask(rng, ncol, nlay, ngpt)
    p["bits"] = M.pack_bits(p["mask"])
    if r["form"] == "rfmip":
        use = p["sza"] < F32(90.0) - F32(2.0) * data.spacing(90.0)
        deg = F32(np.arccos(F32(-1.0)) / F32(180.0))
        p["mu0"] = np.where(use, data.ref_cosf(p["sza"] * deg), F32(1.0)).astype(F32)
        p["toa"] = data.toa_flux({"ncol": ncol, "tsi": p["tsi"]}, kd)
        p["alb"] = np.repeat(p["sfc_alb"][:, None], ngpt, axis=1)
        p["daylit"] = use
    else:
        p["mu0"], p["toa"], p["alb"] = u(0.1, 1, ncol), u(0.1, 10, ncol, ngpt), u(0, 0.9, ncol, ngpt)
        p["daylit"] = np.ones(ncol, bool)
    return r, lims, p


def gpt_fluxes(name, aerosol, cloud):
    """The oracle's surface-level g-point (up, total dn, dir) fluxes, (ncol, ngpt) each, of the row's gases behind its
    aerosol (or none) and its cloud: "masked" (sampled by the row's mask), "whole" (every g-point cloudy) or None"""
    import oracle as O
    r, lims, p = inputs(name)
    orc = O.Oracle()
    io = (p["tau"], p["ssa"], np.zeros_like(p["tau"]))
    if aerosol:
        io = orc.increment_bybnd(lims, io, (p["ta"], p["wa"], p["ga"]))
    if cloud == "masked":   # the mask's bits -> draw_samples -> an increment at g-point resolution
        m = M.unpack_bits(p["bits"], r["ngpt"])
        assert m.any() and not m.all()
        ident = np.stack([np.arange(1, r["ngpt"] + 1)] * 2, axis=1).astype(np.int32)
        io = orc.increment_bybnd(ident, io, [M.draw(m, p[k], lims) for k in ("tb", "wb", "gb")])
    elif cloud == "whole":
        io = orc.increment_bybnd(lims, io, (p["tb"], p["wb"], p["gb"]))
    out = orc.sw_solver(*io, p["mu0"], p["toa"], p["alb"], p["alb"], bool(r["top"]), gpt=True)
    assert all(np.isfinite(w).all() for w in out)
    return tuple(np.ascontiguousarray(g[:, sfc_level(r)]) for g in out[3:])


@functools.lru_cache(maxsize=None)
def expected(name):
    """-> the row's surface g-point fluxes (up, total dn, dir) and their band sums (ncol, nbnd) in the reference's order"""
    r, lims, _ = inputs(name)
    gpt = gpt_fluxes(name, "aer" in r["kind"], "masked" if "mask" in r["kind"] else "whole")
    return gpt, tuple(B.sum_byband(g, lims) for g in gpt)
