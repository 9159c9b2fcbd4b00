"""GPU: the solvers at operand edges, one lit g-point per column, bit for bit against the oracle on every level of every
column (inputs: tests/solver_edges.py; the conditions that keep these comparisons meaningful: tests/
test_solver_edges_host.py).

Each entry point is compared on the columns whose edge operands lie inside the domain that the shortened division
sequences state (tau <= 1e4, ssa == 0 or ssa >= 2^-99, every mu0) and, separately, on the others (tau of 1e30 and 2e38,
0 < ssa < 2^-100), so that a failure names the side it is on.

What an MI355X gave: every SW entry point, kernel and orientation is bitwise on BOTH sides (the quotient of
solver_div(w0 * RT, dd) stays exact for the tiny numerators too, and so do tau = 1e30 and 2e38).  The LW solvers are
bitwise for every tau up to 1e30; at tau = 2e38, where tau * D exceeds 2^126 or overflows to inf, (1 - T) / t leaves
div_rn_normal's domain: v_rcp_f32 returns 0 where 1/t is subnormal (the quotient becomes 0 instead of ~3e-39) and the
Newton step forms inf * 0 = nan at t = inf.  Two closing forms were measured on the standalone LW solver at C3,
alternating with two builds of the parent on one device: v_div_fixup_f32 after the sequence (removes the nan, not the
flushed quotients) 0.0936 ms against 0.0924 / 0.0925 ms (+1.2 %), and a branch into the IEEE division for t > 2^126
(every case below bitwise) 0.0965 ms against 0.0945 / 0.0941 ms (+2.3 %).  Both are outside the parent's own spread
(0.1 % / 0.4 %), so the fast sequence stays, the bound is stated in include/rrtmgpnn.h, and exactly those cases are
strict xfails below.

The scattering and fused LW solvers (solver_edges.build_lw_scat: 1224 columns, an edge (ssa, g) pair beside the edge
tau; classes by the operand the layer's division sees -- tau * D * scaleTau for the rescaled radiance, tau * D for a
clear radiance, the incremented tau for the fused entries).  What an MI355X gave, columns differing per class
(in_domain / large_tau / beyond_2p126), both orientations alike:
  lw_solver_1rescl, _1rescl_gpt, flux_up_Jac, one and three angles      0 of 1080 / 0 of 72-82 / 0 of 62-72
  lw_solver_2stream, _2stream_gpt, with and without incident flux       0 of 1080 / 0 of 144 (no secant, no third class)
  lw_solver_1rescl_planck_inc, plain / masked, 1 and 3 angles, emissivity by band: 0 in every class
  lw_solver_1rescl_planck_clr_all, modes 1 and 2, mask and aerosol off / on: all-sky set 0 in every class; clear set
    0 / 0 / 8 of 24: the columns with tau = 3e38, whose tau * 1.66 overflows to inf, are nan (tau = 1e38 and 2e38, beyond
    2^126 but finite, are bitwise: the Planck level sources absorb the flushed quotient) -- ns_layer is the no-scattering
    step expression for expression, solver_div included, and carries its bound
  lw_solver_noscat_planck_inc, _planck_clr_all and _planck_clr_all_mcica (modes 1 and 2): 0 in every class (tau = 2e38
    with D = 1.66 stays finite); lw_solver_noscat_planck_gpt with lw_Ds: 0 / 0 / 8 of 24 (tau = 2e38 with lw_Ds = 2.5)
The rescaled layer divides plainly and the two-stream layer has no shortened division: neither has a bound on tau.  The
two classes that differ are the stated bound of the no-scattering step (include/rrtmgpnn.h) and strict xfails below; no
kernel was changed.
"""
import functools

import numpy as np
import pytest

import solver_edges as E

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DOMAINS = ["in_domain", "out_of_domain"]
LW_XFAIL = pytest.mark.xfail(strict=True, reason=(
    "tau * D > 2^126 is outside div_rn_normal's domain (include/rrtmgpnn.h states the bound); the closing form, a "
    "branch into the IEEE division, cost 2.3 % of the C3 LW solver (0.0965 vs 0.0945 / 0.0941 ms for two builds of the "
    "parent, spread 0.4 %), and v_div_fixup_f32 alone, which leaves the flushed quotients, 1.2 % (0.0936 vs 0.0924)"))
# LW: tau <= 1e4 / tau = 1e30 (tau * D still below 2^126: inside solver_div's own bound) / tau = 2e38 (beyond it).  The
# fused-Planck entry passes there too: its level sources are never zero next to a lit layer, and the flushed quotient
# (an error of ~3e-39 in fact) is absorbed.
LW_CASES = [pytest.param(mode, dom, id="%s-%s" % (name, dom),
                         marks=[LW_XFAIL] if dom == "beyond_2p126" and mode != "planck" else [])
            for mode, name in ((1, "nmus1"), (3, "nmus3"), ("lw_ds", "lw_ds"), ("planck", "planck"))
            for dom in ("in_domain", "large_tau", "beyond_2p126")]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a device"
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def T(a, dev):
    return torch.as_tensor(np.array(a, dtype=np.float32, order="C"), device=dev)  # a copy: the problems are read-only


def P(t):
    return t.data_ptr() if t is not None else None


def nan(dev, *shape):
    return torch.full(shape, float("nan"), device=dev)


def _cols(p, domain, subset=None):
    """Columns of one side of the operand domain (within `subset`, if given)."""
    m = {"in_domain": lambda: p["in_domain"], "out_of_domain": lambda: ~p["in_domain"],
         "large_tau": lambda: ~p["in_domain"] & ~p["beyond_2p126"], "beyond_2p126": lambda: p["beyond_2p126"]}[domain]()
    if subset is not None:
        keep = np.zeros(p["ncol"], bool)
        keep[subset] = True
        m = m & keep
    cols = np.nonzero(m)[0]
    assert cols.size >= 20
    return cols


def _orc():
    import oracle as O
    return O.Oracle()


# ---- references: computed once per configuration on all columns (the oracle treats columns independently) ----------
@functools.lru_cache(maxsize=None)
def sw_reference(top_at_1, with_dif, gpt=False):
    p = E.build_sw()
    return _orc().sw_solver(p["tau"], p["ssa"], p["g"], p["mu0"], p["inc"], p["alb_dir"], p["alb_dif"], top_at_1,
                            inc_flux_dif=p["inc_dif"] if with_dif else None, gpt=gpt)


@functools.lru_cache(maxsize=None)
def sw_inc_reference(top_at_1):
    p = E.build_sw()
    orc = _orc()
    io = orc.increment_bybnd(p["band_lims_gpt"], (p["tau"], p["ssa"], p["g"]), (p["tau_bnd"], p["ssa_bnd"], p["g_bnd"]))
    return orc.sw_solver(*io, p["mu0"], p["inc"], p["alb_dir"], p["alb_dif"], top_at_1, inc_flux_dif=p["inc_dif"])


@functools.lru_cache(maxsize=None)
def sw_noscat_reference(top_at_1):
    p = E.build_sw()
    return _orc().sw_solver_noscat(p["tau"], p["mu0"], p["inc"], top_at_1)


@functools.lru_cache(maxsize=None)
def lw_reference(top_at_1, mode):
    """mode: 1 / 3 Gauss angles, "lw_ds" the per-(g-point, column) secants, "planck" sources from the Planck fraction"""
    p = E.build_lw()
    orc = _orc()
    if mode == "planck":
        from rrtmgpnn import data
        lay, lev, sfc, _ = orc.planck_source(data.load_kdist("lw"), p["tlay"], p["tlev"], E.lw_tsfc(p, top_at_1),
                                             p["pfrac"], p["nlay"] if top_at_1 else 1)
        return orc.lw_solver(p["tau"], lay, lev, p["emis"], sfc, top_at_1, 1, inc_flux=p["inc"])
    return orc.lw_solver(p["tau"], p["lay"], p["lev"], p["emis"], p["sfc"], top_at_1, 1 if mode == "lw_ds" else mode,
                         inc_flux=p["inc"], lw_Ds=p["lw_ds"] if mode == "lw_ds" else None)


# ---- kernel runs --------------------------------------------------------------------------------------------------
def run_sw(dev, top_at_1, with_dif, with_g=True, cols=None, entry="plain"):
    """rrtmgpnn_sw_solver_2stream / _gpt / _inc on the columns `cols` of the SW edge problem -> list of numpy outputs"""
    from rrtmgpnn import _lib
    from rrtmgpnn._lib import check, int_array
    from rrtmgpnn.api import context
    p = E.build_sw()
    s = slice(None) if cols is None else cols
    a = {k: T(p[k][s], dev) for k in ("inc", "inc_dif", "tau", "ssa", "g", "mu0", "alb_dir", "alb_dif")}
    ncol, nlay, ngpt = a["tau"].shape
    outs = [nan(dev, ncol, nlay + 1) for _ in range(3)]
    head = [context(0).h, ngpt, nlay, ncol, int(top_at_1), P(a["inc"]), P(a["inc_dif"]) if with_dif else None,
            P(a["tau"]), P(a["ssa"]), P(a["g"]) if with_g else None]
    tail = [P(a["mu0"]), P(a["alb_dir"]), P(a["alb_dif"])] + [P(t) for t in outs]
    L = _lib.lib()
    if entry == "plain":
        check(L.rrtmgpnn_sw_solver_2stream(*head, *tail), "sw_solver_2stream")
    elif entry == "gpt":
        outs += [nan(dev, ncol, nlay + 1, ngpt) for _ in range(3)]
        check(L.rrtmgpnn_sw_solver_2stream_gpt(*head, *tail, *[P(t) for t in outs[3:]]), "sw_solver_2stream_gpt")
    else:
        b = [T(p[k][s], dev) for k in ("tau_bnd", "ssa_bnd", "g_bnd")]
        check(L.rrtmgpnn_sw_solver_2stream_inc(*head, E.INC_NBND, int_array(p["band_lims_gpt"].ravel()),
                                               *[P(t) for t in b], *tail), "sw_solver_2stream_inc")
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in outs]


def run_sw_noscat(dev, top_at_1):
    from rrtmgpnn import _lib
    from rrtmgpnn.api import context
    p = E.build_sw()
    a = [T(p[k], dev) for k in ("inc", "tau", "mu0")]
    out = nan(dev, p["ncol"], p["nlay"] + 1)
    _lib.check(_lib.lib().rrtmgpnn_sw_solver_noscat(context(0).h, p["ngpt"], p["nlay"], p["ncol"], int(top_at_1),
                                                    *[P(t) for t in a], P(out)), "sw_solver_noscat")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def run_lw(dev, top_at_1, mode):
    from rrtmgpnn import _lib, data
    from rrtmgpnn._lib import check, float_array, int_array
    from rrtmgpnn.api import GAUSS_DS, GAUSS_WTS, context
    p = E.build_lw()
    ncol, nlay, ngpt = p["tau"].shape
    nmus = mode if mode in (1, 3) else 1
    up, dn = nan(dev, ncol, nlay + 1), nan(dev, ncol, nlay + 1)
    head = [context(0).h, ngpt, nlay, ncol, int(top_at_1), nmus, float_array(GAUSS_DS[nmus]), float_array(GAUSS_WTS[nmus])]
    inc, tau, emis = T(p["inc"], dev), T(p["tau"], dev), T(p["emis"], dev)
    L = _lib.lib()
    if mode == "planck":
        kd = data.load_kdist("lw")
        assert kd["ngpt"] == ngpt
        a = [T(x, dev) for x in (p["pfrac"], p["tlay"], p["tlev"], E.lw_tsfc(p, top_at_1), kd["totplnk"])]
        check(L.rrtmgpnn_lw_solver_noscat_planck(
            *head, P(inc), P(tau), P(a[0]), kd["nband"], kd["nPlanckTemp"], P(a[1]), P(a[2]), P(a[3]),
            nlay if top_at_1 else 1, int_array(kd["band_lims_gpt"].ravel()), float(kd["temp_ref_min"][0]),
            float(kd["totplnk_delta"]), P(a[4]), 0, P(emis), P(up), P(dn)), "lw_solver_noscat_planck")
    else:
        a = [T(p[k], dev) for k in ("lay", "lev", "sfc")]
        if mode == "lw_ds":
            ds = T(p["lw_ds"], dev)
            check(L.rrtmgpnn_lw_solver_noscat_gpt(*head, P(ds), P(inc), P(tau), P(a[0]), P(a[1]), P(emis), P(a[2]),
                                                  P(up), P(dn), None, None), "lw_solver_noscat_gpt")
        else:
            check(L.rrtmgpnn_lw_solver_noscat(*head, P(inc), P(tau), P(a[0]), P(a[1]), P(emis), P(a[2]), P(up), P(dn)),
                  "lw_solver_noscat")
    torch.cuda.synchronize()
    return [up.cpu().numpy(), dn.cpu().numpy()]


# ---- tests --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("domain", DOMAINS)
@pytest.mark.parametrize("with_dif", [True, False], ids=["dif", "nodif"])
@pytest.mark.parametrize("top_at_1", [True, False], ids=["top", "bot"])
def test_sw_2stream_edges(dev, sw_kernel, top_at_1, with_dif, domain):
    p = E.build_sw()
    got = run_sw(dev, top_at_1, with_dif)
    cols = _cols(p, domain)
    for x, y, what in zip(got, sw_reference(top_at_1, with_dif), ("up", "dn", "dir")):
        E.assert_bitwise(x, y, p, what, cols)


@pytest.mark.parametrize("domain", DOMAINS)
@pytest.mark.parametrize("with_dif", [True, False], ids=["dif", "nodif"])
@pytest.mark.parametrize("top_at_1", [True, False], ids=["top", "bot"])
def test_sw_2stream_edges_without_g(dev, sw_kernel, top_at_1, with_dif, domain):
    """g = NULL (the literal-0 instances) on the columns whose edge layer has g == 0 (every other g is 0 already)."""
    p = E.build_sw()
    sub = p["g0"]
    got = run_sw(dev, top_at_1, with_dif, with_g=False, cols=sub)
    pick = np.nonzero(np.isin(sub, _cols(p, domain, sub)))[0]
    for x, y, what in zip(got, sw_reference(top_at_1, with_dif), ("up", "dn", "dir")):
        full = np.full_like(y, np.nan)
        full[sub] = x
        E.assert_bitwise(full, y, p, what, sub[pick])


@pytest.mark.parametrize("domain", DOMAINS)
@pytest.mark.parametrize("top_at_1", [True, False], ids=["top", "bot"])
def test_sw_2stream_gpt_edges(dev, sw_kernel, top_at_1, domain):
    """The g-point instances on the same inputs: the broadband fluxes and the g-point arrays themselves."""
    p = E.build_sw()
    got = run_sw(dev, top_at_1, True, entry="gpt")
    cols = _cols(p, domain)
    for x, y, what in zip(got, sw_reference(top_at_1, True, gpt=True), ("up", "dn", "dir", "gpt_up", "gpt_dn", "gpt_dir")):
        E.assert_bitwise(x, y, p, what, cols)


@pytest.mark.parametrize("domain", DOMAINS)
@pytest.mark.parametrize("with_g", [True, False], ids=["g", "nog"])
@pytest.mark.parametrize("top_at_1", [True, False], ids=["top", "bot"])
def test_sw_2stream_inc_edges(dev, sw_kernel, top_at_1, with_g, domain):
    """The fused band increment at its max(eps, .) clamps (both taus 0, tau*ssa sums that underflow) against the oracle's
    increment_bybnd followed by its sw_solver; g = NULL on the g == 0 columns."""
    p = E.build_sw()
    sub = np.arange(p["ncol"]) if with_g else p["g0"]
    got = run_sw(dev, top_at_1, True, with_g=with_g, cols=sub, entry="inc")
    pick = _cols(p, domain, sub)
    for x, y, what in zip(got, sw_inc_reference(top_at_1), ("up", "dn", "dir")):
        full = np.full_like(y, np.nan)
        full[sub] = x
        E.assert_bitwise(full, y, p, what, pick)


@pytest.mark.parametrize("top_at_1", [True, False], ids=["top", "bot"])
def test_sw_noscat_edges(dev, top_at_1):
    """The direct beam alone (no division: every tau and mu0 of the lists is in its domain)."""
    p = E.build_sw()
    E.assert_bitwise(run_sw_noscat(dev, top_at_1), sw_noscat_reference(top_at_1), p, "dir")


@pytest.mark.parametrize("mode,domain", LW_CASES)
@pytest.mark.parametrize("top_at_1", [True, False], ids=["top", "bot"])
def test_lw_noscat_edges(dev, top_at_1, mode, domain):
    """rrtmgpnn_lw_solver_noscat with one and three angles, with rte_lw's lw_Ds secants (tau*D on both sides of the
    threshold for every secant), and rrtmgpnn_lw_solver_noscat_planck with the sources formed from a lit Planck
    fraction (reference: the oracle's planck_source followed by its lw_solver)."""
    p = E.build_lw()
    got = run_lw(dev, top_at_1, mode)
    cols = _cols(p, domain)
    for x, y, what in zip(got, lw_reference(top_at_1, mode), ("up", "dn")):
        E.assert_bitwise(x, y, p, what, cols)


# ---- the scattering and fused LW solvers (inputs: solver_edges.build_lw_scat) --------------------------------------------
LW3 = ("in_domain", "large_tau", "beyond_2p126")
LW_NAN_XFAIL = pytest.mark.xfail(strict=True, reason=(
    "tau * D > 2^126 is outside div_rn_normal's domain (include/rrtmgpnn.h states the bound at the entry): where tau * D "
    "overflows to inf (tau = 3e38 with D = 1.66, tau = 2e38 with lw_Ds = 2.5) the Newton step of solver_div(1 - T, t) "
    "forms inf * 0 and the column's fluxes are nan where the oracle's are finite; 8 of the 24 columns beyond the bound.  "
    "The finite products beyond 2^126 pass here: the Planck level sources beside a lit layer are never zero and absorb "
    "the flushed quotient (~3e-39).  The closing forms and their cost: LW_XFAIL above"))
ORIENT = pytest.mark.parametrize("top_at_1", [True, False], ids=["top", "bot"])
NMUS = pytest.mark.parametrize("nmus", [1, 3], ids=["nmus1", "nmus3"])
_dev_arrays, _runs = {}, {}


def _lw_head(nmus, p, top_at_1):
    from rrtmgpnn._lib import float_array
    from rrtmgpnn.api import GAUSS_DS, GAUSS_WTS, context
    return [context(0).h, p["ngpt"], p["nlay"], p["ncol"], int(top_at_1), nmus, float_array(GAUSS_DS[nmus]),
            float_array(GAUSS_WTS[nmus])]


def _dev_of(name, p, keys, dev):
    """The problem's arrays on the device, copied once and only read by the entries."""
    d = _dev_arrays.setdefault(name, {})
    for k in keys:
        if k not in d:
            d[k] = T(p[k], dev)
    return d


def _bits(mask, dev):
    import mcica_ref as M
    return torch.as_tensor(M.pack_bits(mask).view(np.int32), device=dev)


def _once(key, fn):
    """One launch per configuration: the domain classes of a parametrised test compare the same outputs."""
    if key not in _runs:
        _runs[key] = fn()
    return _runs[key]


def _compare(q, domain, triples):
    cols = _cols(q, domain)
    for got, want, what in triples:
        E.assert_bitwise(got, want, q, what, cols)


def _rescl_classes(p, nmus):
    e = p["edge"]
    return E.classes(p, e["tau"], E.scale_tau(e["ssa"], e["g"])[1], E.gauss_ds(nmus))


def run_rescl(dev, top_at_1, nmus, gpt=False, jac=False):
    """rrtmgpnn_lw_solver_1rescl / _gpt on the scattering edge problem; jac: under rrtmgpnn_solver_request_jacobian ->
    [up, dn(, gpt_up, gpt_dn)(, flux_up_Jac)]"""
    from rrtmgpnn import _lib
    from rrtmgpnn._lib import check
    p = E.build_lw_scat()
    d = _dev_of("scat", p, ("inc", "tau", "ssa", "g", "lay", "lev", "emis", "sfc", "sjac"), dev)
    ncol, nlay, ngpt = p["ncol"], p["nlay"], p["ngpt"]
    outs = [nan(dev, ncol, nlay + 1) for _ in range(2)]
    args = _lw_head(nmus, p, top_at_1) + [P(d[k]) for k in ("inc", "tau", "ssa", "g", "lay", "lev", "emis", "sfc")]
    L = _lib.lib()
    if jac:
        outs.append(nan(dev, ncol, nlay + 1))
        check(L.rrtmgpnn_solver_request_jacobian(args[0], ngpt, nlay, ncol, P(d["sjac"]), P(outs[2])),
              "solver_request_jacobian")
        check(L.rrtmgpnn_lw_solver_1rescl(*args, P(outs[0]), P(outs[1])), "lw_solver_1rescl")
    elif gpt:
        outs += [nan(dev, ncol, nlay + 1, ngpt) for _ in range(2)]
        check(L.rrtmgpnn_lw_solver_1rescl_gpt(*args, *[P(t) for t in outs]), "lw_solver_1rescl_gpt")
    else:
        check(L.rrtmgpnn_lw_solver_1rescl(*args, *[P(t) for t in outs]), "lw_solver_1rescl")
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in outs]


def run_lw_2stream(dev, top_at_1, with_inc, gpt):
    from rrtmgpnn import _lib
    from rrtmgpnn.api import context
    p = E.build_lw_scat()
    d = _dev_of("scat", p, ("inc", "tau", "ssa", "g", "lev", "emis", "sfc"), dev)
    ncol, nlay, ngpt = p["ncol"], p["nlay"], p["ngpt"]
    outs = [nan(dev, ncol, nlay + 1) for _ in range(2)] + ([nan(dev, ncol, nlay + 1, ngpt) for _ in range(2)] if gpt else [])
    args = [context(0).h, ngpt, nlay, ncol, int(top_at_1), P(d["inc"]) if with_inc else None] + \
        [P(d[k]) for k in ("tau", "ssa", "g", "lev", "emis", "sfc")] + [P(t) for t in outs]
    L = _lib.lib()
    _lib.check((L.rrtmgpnn_lw_solver_2stream_gpt if gpt else L.rrtmgpnn_lw_solver_2stream)(*args), "lw_solver_2stream")
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in outs]


def _planck_tail(p, d, kd, lims, top_at_1, dev, emis_by_band=False):
    from rrtmgpnn._lib import int_array
    key = "tsfc%d" % top_at_1
    if key not in d:
        d[key], d["totplnk"] = T(E.lw_tsfc(p, top_at_1), dev), T(kd["totplnk"], dev)
    return [P(d["pfrac"]), kd["nband"], kd["nPlanckTemp"], P(d["tlay"]), P(d["tlev"]), P(d[key]),
            p["nlay"] if top_at_1 else 1, int_array(np.asarray(lims).ravel()), float(kd["temp_ref_min"][0]),
            float(kd["totplnk_delta"]), P(d["totplnk"]), int(emis_by_band), P(d["emis_bnd"] if emis_by_band else d["emis"])]


def run_fused_scat(dev, top_at_1, nmus, masked, aer=False, dual=None, emis_by_band=False):
    """rrtmgpnn_lw_solver_1rescl_planck_inc (dual None) or _planck_clr_all under rrtmgpnn_context_set_lw_scat_clr_all
    mode `dual`, with the mask and the 1scl aerosol armed as asked -> [up, dn(, up_clr, dn_clr)]"""
    from rrtmgpnn import _lib
    from rrtmgpnn._lib import check
    p = E.build_lw_scat()
    d = _dev_of("scat", p, ("inc", "tau_gas", "tau_bnd", "ssa_bnd", "g_bnd", "tau_aer", "pfrac", "tlay", "tlev", "emis",
                            "emis_bnd"), dev)
    if "bits" not in d:
        d["bits"] = _bits(p["mask"], dev)
    ncol, nlay, ngpt = p["ncol"], p["nlay"], p["ngpt"]
    outs = [nan(dev, ncol, nlay + 1) for _ in range(2 if dual is None else 4)]
    args = _lw_head(nmus, p, top_at_1) + [P(d[k]) for k in ("inc", "tau_gas", "tau_bnd", "ssa_bnd", "g_bnd")] + \
        _planck_tail(p, d, p["kd"], p["lims"], top_at_1, dev, emis_by_band) + [P(t) for t in outs]
    L, ctx = _lib.lib(), args[0]
    try:
        if dual is not None:
            check(L.rrtmgpnn_context_set_lw_scat_clr_all(ctx, dual), "context_set_lw_scat_clr_all")
        if masked:
            check(L.rrtmgpnn_solver_request_cloud_mask(ctx, ngpt, nlay, ncol, P(d["bits"])), "solver_request_cloud_mask")
        if aer:
            check(L.rrtmgpnn_solver_request_aerosol(ctx, p["nb"], nlay, ncol, P(d["tau_aer"]), None, None),
                  "solver_request_aerosol")
        if dual is None:
            check(L.rrtmgpnn_lw_solver_1rescl_planck_inc(*args), "lw_solver_1rescl_planck_inc")
        else:
            check(L.rrtmgpnn_lw_solver_1rescl_planck_clr_all(*args), "lw_solver_1rescl_planck_clr_all")
        torch.cuda.synchronize()
    finally:
        if dual is not None:
            check(L.rrtmgpnn_context_set_lw_scat_clr_all(ctx, 0), "context_set_lw_scat_clr_all")
    return [t.cpu().numpy() for t in outs]


def _fused_classes(orc, p, top_at_1, nmus, masked, aer, which):
    """The classes of the all-sky set (the rescaled division sees tau_incremented * D * scaleTau) or of the clear set (the
    no-scattering step sees (tau [+ tau_aer]) * D)."""
    ref = E.ref_fused(orc, top_at_1, nmus, masked, aer)
    if which == "clr":
        return E.classes(p, E.edge_values(p, ref[5]), None, E.gauss_ds(nmus))
    io = ref[4]
    scale = E.scale_tau(E.edge_values(p, io[1]), E.edge_values(p, io[2]))[1]
    return E.classes(p, E.edge_values(p, io[0]), scale, E.gauss_ds(nmus))


def run_noscat_fused(dev, top_at_1, entry, mode=0):
    """The no-scattering fused entries on build_lw()'s problem with lw_band_inc()'s band tau: "inc", "clr_all",
    "clr_all_mcica" (under rrtmgpnn_context_set_lw_clr_all mode `mode`), "gpt" (with lw_Ds)."""
    from rrtmgpnn import _lib
    from rrtmgpnn._lib import check
    p, b = E.build_lw(), E.lw_band_inc()
    d = _dev_of("lw", p, ("inc", "tau", "pfrac", "tlay", "tlev", "emis", "lw_ds"), dev)
    if "tau_bnd" not in d:
        d["tau_bnd"], d["bits"] = T(b["tau_bnd"], dev), _bits(b["mask"], dev)
    ncol, nlay, ngpt = p["ncol"], p["nlay"], p["ngpt"]
    head, tail = _lw_head(1, p, top_at_1), _planck_tail(p, d, b["kd"], b["lims"], top_at_1, dev)
    L, ctx = _lib.lib(), head[0]
    n_out = {"inc": 2, "clr_all": 4, "clr_all_mcica": 4, "gpt": 2}[entry]
    outs = [nan(dev, ncol, nlay + 1) for _ in range(n_out)]
    try:
        if entry == "gpt":
            outs += [nan(dev, ncol, nlay + 1, ngpt) for _ in range(2)]
            check(L.rrtmgpnn_lw_solver_noscat_planck_gpt(*head, P(d["lw_ds"]), P(d["inc"]), P(d["tau"]), *tail,
                                                         *[P(t) for t in outs]), "lw_solver_noscat_planck_gpt")
        elif entry == "inc":
            check(L.rrtmgpnn_lw_solver_noscat_planck_inc(*head, P(d["inc"]), P(d["tau"]), P(d["tau_bnd"]), *tail,
                                                         *[P(t) for t in outs]), "lw_solver_noscat_planck_inc")
        else:
            check(L.rrtmgpnn_context_set_lw_clr_all(ctx, mode), "context_set_lw_clr_all")
            a = head + [P(d["inc"]), P(d["tau"]), P(d["tau_bnd"])] + tail + [P(t) for t in outs]
            if entry == "clr_all":
                check(L.rrtmgpnn_lw_solver_noscat_planck_clr_all(*a), "lw_solver_noscat_planck_clr_all")
            else:
                check(L.rrtmgpnn_lw_solver_noscat_planck_clr_all_mcica(*a, P(d["bits"])),
                      "lw_solver_noscat_planck_clr_all_mcica")
        torch.cuda.synchronize()
    finally:
        if entry.startswith("clr_all"):
            check(L.rrtmgpnn_context_set_lw_clr_all(ctx, 0), "context_set_lw_clr_all")
    return [t.cpu().numpy() for t in outs]


@pytest.mark.parametrize("domain", LW3)
@NMUS
@ORIENT
def test_lw_1rescl_edges(dev, orc, top_at_1, nmus, domain):
    """rrtmgpnn_lw_solver_1rescl with incident flux: rs_layer's scaleTau, Cn, An, the threshold on tau * D * scaleTau and
    its plain division, against the oracle's rescaled solver."""
    p = E.build_lw_scat()
    got = _once(("rescl", top_at_1, nmus), lambda: run_rescl(dev, top_at_1, nmus))
    _compare(_rescl_classes(p, nmus), domain, zip(got, E.ref_rescl(orc, top_at_1, nmus), ("up", "dn")))


@pytest.mark.parametrize("domain", LW3)
@NMUS
@ORIENT
def test_lw_1rescl_gpt_edges(dev, orc, top_at_1, nmus, domain):
    """rrtmgpnn_lw_solver_1rescl_gpt: with one angle the g-point radiances (quirk B-5), with three the fluxes."""
    p = E.build_lw_scat()
    got = _once(("rescl_gpt", top_at_1, nmus), lambda: run_rescl(dev, top_at_1, nmus, gpt=True))
    _compare(_rescl_classes(p, nmus), domain,
             zip(got, E.ref_rescl(orc, top_at_1, nmus, gpt=True), ("up", "dn", "gpt_up", "gpt_dn")))


@pytest.mark.parametrize("domain", LW3)
@NMUS
@ORIENT
def test_lw_1rescl_jacobian_edges(dev, orc, top_at_1, nmus, domain):
    """The Jacobian recurrence J = trans * J on the rescaled transmittance: flux_up_Jac against the oracle's flux_up on
    zero sources; the fluxes of the armed call are the unarmed call's on every column."""
    p = E.build_lw_scat()
    got = _once(("rescl_jac", top_at_1, nmus), lambda: run_rescl(dev, top_at_1, nmus, jac=True))
    plain = _once(("rescl", top_at_1, nmus), lambda: run_rescl(dev, top_at_1, nmus))
    q = _rescl_classes(p, nmus)
    E.assert_bitwise(got[0], plain[0], p, "up against the unarmed call")
    E.assert_bitwise(got[1], plain[1], p, "dn against the unarmed call")
    _compare(q, domain, [(got[2], E.ref_rescl_jac(orc, top_at_1, nmus), "flux_up_Jac")])


@pytest.mark.parametrize("domain", DOMAINS)
@pytest.mark.parametrize("gpt", [False, True], ids=["bb", "gpt"])
@pytest.mark.parametrize("with_inc", [True, False], ids=["inc", "noinc"])
@ORIENT
def test_lw_2stream_edges(dev, orc, top_at_1, with_inc, gpt, domain):
    """rrtmgpnn_lw_solver_2stream / _2stream_gpt: l2_layer's k_min clamp, exp(-tau k) and its square underflowing, the
    tau > 1e-8 branch with Z just above it, and the adding step, against the oracle's lw_solver_2stream."""
    p = E.build_lw_scat()
    got = _once(("2str", top_at_1, with_inc, gpt), lambda: run_lw_2stream(dev, top_at_1, with_inc, gpt))
    _compare(E.classes(p, p["edge"]["tau"]), domain,
             zip(got, E.ref_2stream(orc, top_at_1, with_inc, gpt), ("up", "dn", "gpt_up", "gpt_dn")))


FUSED_RUNS = [pytest.param(nmus, masked, by_band, id="nmus%d-%s%s" % (nmus, "masked" if masked else "plain",
                                                                      "-emisbnd" if by_band else ""))
              for nmus, masked, by_band in ((1, False, False), (1, True, False), (3, False, False), (3, True, False),
                                            (1, True, True))]


@pytest.mark.parametrize("domain", LW3)
@pytest.mark.parametrize("nmus,masked,by_band", FUSED_RUNS)
@ORIENT
def test_lw_1rescl_planck_inc_edges(dev, orc, top_at_1, nmus, masked, by_band, domain):
    """rrtmgpnn_lw_solver_1rescl_planck_inc: the edge reaches rs_layer through inc_2str on literal-zero gas ssa / g (both
    max(3 FLT_MIN, .) clamps) and, masked, through the mask word switching the band operands to 0; against the composed
    oracle (planck_source, increment_bybnd, mcica_ref.draw at identity limits, lw_solver(ssa=, g=))."""
    p = E.build_lw_scat()
    got = _once(("fused", top_at_1, nmus, masked, by_band),
                lambda: run_fused_scat(dev, top_at_1, nmus, masked, emis_by_band=by_band))
    want = E.ref_fused(orc, top_at_1, nmus, masked, False, by_band)
    _compare(_fused_classes(orc, p, top_at_1, nmus, masked, False, "all"), domain, zip(got, want[:2], ("up", "dn")))


DUAL_RUNS = [pytest.param(masked, aer, by_band, id="%s-%s%s" % ("masked" if masked else "plain", "aer" if aer else "noaer",
                                                                "-emisbnd" if by_band else ""))
             for masked, aer, by_band in ((False, False, False), (True, False, False), (False, True, False),
                                          (True, True, False), (True, True, True))]


# the dual's clear set is the no-scattering step (ns_layer in mode 1, lw_noscat_kernel in mode 2; both divide with
# solver_div) and carries its bound; the all-sky set divides plainly and has none
DUAL_SETS = [pytest.param(which, dom, id="%s-%s" % (which, dom),
                          marks=[LW_NAN_XFAIL] if (which, dom) == ("clr", "beyond_2p126") else [])
             for which in ("all", "clr") for dom in LW3]


@pytest.mark.parametrize("which,domain", DUAL_SETS)
@pytest.mark.parametrize("masked,aer,by_band", DUAL_RUNS)
@pytest.mark.parametrize("mode", [1, 2], ids=["dual", "two"])
@ORIENT
def test_lw_1rescl_planck_clr_all_edges(dev, orc, top_at_1, mode, masked, aer, by_band, which, domain):
    """rrtmgpnn_lw_solver_1rescl_planck_clr_all in both modes: the all-sky set as the single entry's, with the 1scl
    aerosol added in front of the cloud (two separately rounded adds); the clear set -- in mode 1 ns_layer, the dual
    instance's copy of the no-scattering step -- against the oracle's no-scattering solve of tau [+ tau_aer]."""
    p = E.build_lw_scat()
    got = _once(("dual", top_at_1, mode, masked, aer, by_band),
                lambda: run_fused_scat(dev, top_at_1, 1, masked, aer, dual=mode, emis_by_band=by_band))
    want = E.ref_fused(orc, top_at_1, 1, masked, aer, by_band)
    s = slice(0, 2) if which == "all" else slice(2, 4)
    _compare(_fused_classes(orc, p, top_at_1, 1, masked, aer, which), domain,
             zip(got[s], want[s], ("up", "dn") if which == "all" else ("up_clr", "dn_clr")))


NOSCAT_FUSED = [("inc", 0), ("clr_all", 1), ("clr_all", 2), ("clr_all_mcica", 1), ("clr_all_mcica", 2), ("gpt", 0)]


NOSCAT_FUSED_CASES = [pytest.param(e, m, dom, id="%s%s-%s" % (e, m or "", dom),
                                   marks=[LW_NAN_XFAIL] if (e, dom) == ("gpt", "beyond_2p126") else [])
                      for e, m in NOSCAT_FUSED for dom in LW3]


@pytest.mark.parametrize("entry,mode,domain", NOSCAT_FUSED_CASES)
@ORIENT
def test_lw_noscat_fused_edges(dev, orc, top_at_1, entry, mode, domain):
    """The no-scattering fused entries whose tau * D <= 2^126 bound include/rrtmgpnn.h states: _planck_inc,
    _planck_clr_all and _planck_clr_all_mcica in both modes of rrtmgpnn_context_set_lw_clr_all, _planck_gpt with lw_Ds;
    against planck_source, increment_bybnd (masked where applicable) and lw_solver.  Each flux set is classed by the
    optical depth its own division sees."""
    p = E.build_lw()
    got = _once(("noscat_fused", top_at_1, entry, mode), lambda: run_noscat_fused(dev, top_at_1, entry, mode))
    if entry == "gpt":
        with np.errstate(over="ignore"):
            q = dict(p, beyond_2p126=p["edge"]["tau"] * p["edge"]["lw_d"] > np.float32(2.0 ** 126))
        _compare(q, domain, zip(got, E.ref_noscat_fused(orc, top_at_1, 1, "gpt"), ("up", "dn", "gpt_up", "gpt_dn")))
        return
    sets = [("inc" if entry != "clr_all_mcica" else "masked", got[:2], ("up", "dn"))]
    if entry != "inc":
        sets.append(("clear", got[2:], ("up_clr", "dn_clr")))
    for kind, arrs, names in sets:
        up, dn, tau = E.ref_noscat_fused(orc, top_at_1, 1, kind)
        _compare(E.classes(p, E.edge_values(p, tau), None, E.gauss_ds(1)), domain, zip(arrs, (up, dn), names))
