"""GPU: the elementwise kernels and the gas-optics glue at operand edges and shape edges, through the C ABI, bit for bit
against the oracle (compared as uint32 views; tests/test_elementwise_edges_host.py pins the oracle to the reference on
the same cases and checks that the cases reach the edges).

* The operand cases of tests/elementwise_edges.py through rrtmgpnn_delta_scale_2str, rrtmgpnn_increment_bybnd and
  rrtmgpnn_increment, rrtmgpnn_cloud_optics_compute (tables from _load and from _create_lut / _create_pade), both
  heating-rate entries, rrtmgpnn_expand_band_to_gpt, rrtmgpnn_compute_nn_inputs, rrtmgpnn_get_col_dry,
  rrtmgpnn_interpolate_tlev, and the fused rrtmgpnn_gas_optics_lw_nn / _sw_nn under both MFMA tilings (the full models,
  the reduced g128 / g112 models, the LW "both" model), against the oracle and against the three separate GPU calls.
  Where the host file allows nan (the SW ssa under a layer of zero thickness) the nan masks must be equal.
* The shape edges on benign values: the second, partial trip of every capped grid-stride loop (the caps formed from the
  device's CU count as the launchers form them), blocks of every rows-per-block of the cloud-optics kernel, the
  g-point counts around a wave and at the block limit, the refusals at the limits.

Measured on an MI355X: the whole file (125 tests) takes 3 s of wall time, its slowest test 0.25 s.
"""
import ctypes

import numpy as np
import pytest

import elementwise_edges as E

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F = np.float32
OK, ERR_ARGUMENT, ERR_UNSUPPORTED = 0, 1, 4
MFMA32, MFMA16, F_XIN = 2, 3, 4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a device"
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def T(a, dev):
    return torch.as_tensor(np.array(a, dtype=np.float32, order="C"), device=dev)  # a copy: the cases are read-only


def N(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def lib():
    from rrtmgpnn import _lib
    return _lib.lib()


def ctx():
    from rrtmgpnn.api import context
    return context(0).h


def check(rc, what):
    from rrtmgpnn import _lib
    _lib.check(rc, what)


def last_error():
    return lib().rrtmgpnn_last_error().decode(errors="replace")


def cus():
    """The CU count the launchers cap their grids with (hipDeviceProp_t::multiProcessorCount)."""
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def p_(t):
    return None if t is None else t.data_ptr()


def fp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def assert_bits_nan(got, want, what, describe=None):
    """Equal nan masks, equal bits elsewhere (a nan's sign and payload are the machine's, not the operation's)."""
    got, want = np.asarray(got, F), np.asarray(want, F)
    gn, wn = np.isnan(got), np.isnan(want)
    bad = np.unique(np.nonzero((gn != wn).reshape(gn.shape[0], -1))[0])
    assert not bad.size, "%s: nan masks differ; %s" % (what, describe(bad) if describe else bad[:6])
    E.assert_bits(np.where(gn, F(0), got), np.where(wn, F(0), want), what, describe)


def ramp(n, lo, hi, period):
    """n benign float32 values walking [lo, hi) with the given period."""
    return (F(lo) + F(hi - lo) * ((np.arange(n) % period).astype(F) / F(period))).astype(F)


# ---- delta scaling ------------------------------------------------------------------------------------------------------
def run_delta_scale(dev, tau, ssa, g, fwd):
    t, w, q = T(tau, dev), T(ssa, dev), T(g, dev)
    f = None if fwd is None else T(fwd, dev)
    check(lib().rrtmgpnn_delta_scale_2str(ctx(), t.numel(), p_(t), p_(w), p_(q), p_(f)), "delta_scale_2str")
    return N(t), N(w), N(q)


@pytest.mark.parametrize("form", E.DS_FORMS, ids=str)
def test_delta_scale_operand_edges(dev, orc, form):
    p = E.build_delta_scale()
    fwd = p["fwd"][form]
    got = run_delta_scale(dev, p["tau"], p["ssa"], p["g"], fwd)
    for x, y, name in zip(got, orc.delta_scale(p["tau"], p["ssa"], p["g"], fwd), ("tau", "ssa", "g")):
        E.assert_bits(x, y, "delta_scale %s (%s)" % (name, form), p["describe"])


@pytest.mark.parametrize("n", [1, 255, 257, "cap"])
@pytest.mark.parametrize("with_fwd", [False, True])
def test_delta_scale_shapes(dev, orc, n, with_fwd):
    """256 threads a block, at most 8 * CUs blocks: cap * 256 + 3 elements take a second trip of three elements."""
    n = 8 * cus() * 256 + 3 if n == "cap" else n
    tau, ssa, g = ramp(n, 0.01, 30, 97), ramp(n, 0, 1, 89), ramp(n, -0.5, 0.95, 53)
    fwd = ramp(n, 0, 1, 61) if with_fwd else None
    got = run_delta_scale(dev, tau, ssa, g, fwd)
    for x, y, name in zip(got, orc.delta_scale(tau, ssa, g, fwd), ("tau", "ssa", "g")):
        E.assert_bits(x, y, "delta_scale %s, n = %d" % (name, n))


# ---- increment -------------------------------------------------------------------------------------------------------------
def run_increment(dev, ncol, nlay, ngpt, lims, io, inc, same=False):
    """rrtmgpnn_increment_bybnd (or, same: rrtmgpnn_increment) -> the io arrays afterwards, the inputs' too."""
    from rrtmgpnn._lib import int_array
    a, b = [T(x, dev) for x in io], [T(x, dev) for x in inc]
    pa, pb = [p_(t) for t in a] + [None] * (3 - len(a)), [p_(t) for t in b] + [None] * (3 - len(b))
    if same:
        rc = lib().rrtmgpnn_increment(ctx(), ncol, nlay, ngpt, *pa, *pb)
    else:
        rc = lib().rrtmgpnn_increment_bybnd(ctx(), ncol, nlay, ngpt, len(lims), int_array(np.asarray(lims).ravel()),
                                            *pa, *pb)
    check(rc, "increment")
    out = [N(t) for t in a]
    for t, x in zip(b, inc):
        E.assert_bits(N(t), x, "the increment itself was written")
    return out


@pytest.mark.parametrize("nstr_io,nstr_in", E.PAIRINGS)
@pytest.mark.parametrize("layout", E.INC_LAYOUTS)
def test_increment_operand_edges(dev, orc, layout, nstr_io, nstr_in):
    """Whole arrays are compared: in the layout with a gap the g-points in no band must come back untouched."""
    p = E.build_increment(layout)
    io, inc = p["io"][:1 if nstr_io == 1 else 3], p["inc"][:1 if nstr_in == 1 else 3]
    got = run_increment(dev, p["ncol"], p["nlay"], p["ngpt"], p["lims"], io, inc, same=layout == "same")
    want = E.increment_ref(orc, p, nstr_io, nstr_in)
    for x, y, name in zip(got, want, ("tau", "ssa", "g")):
        E.assert_bits(x.reshape(-1, p["ngpt"]), y.reshape(-1, p["ngpt"]), "increment %d by %d, %s, layout %s"
                      % (nstr_io, nstr_in, name, layout), p["describe"])


def _three_bands(ngpt):
    """Up to three bands of unequal widths covering 1..ngpt."""
    cuts = sorted({1, ngpt // 3 + 1, (3 * ngpt) // 4 + 1, ngpt + 1})
    return np.array([[lo, hi - 1] for lo, hi in zip(cuts[:-1], cuts[1:])], np.int32)


@pytest.mark.parametrize("ngpt", [1, 63, 64, 65, 224, 1024])
def test_increment_shapes(dev, orc, ngpt):
    """A block of ngpt rounded up to a wave, at most CUs * (2048 / threads) blocks striding over the rows: one row past
    that cap at 64 and at 256 threads (ngpt 64 and 224), so that block 0 takes a second trip; a few rows elsewhere."""
    threads = (ngpt + 63) // 64 * 64
    nrow = cus() * (2048 // threads) + 1 if ngpt in (64, 224) else 7
    ncol, nlay = nrow, 1
    lims = _three_bands(ngpt)
    n = nrow * ngpt
    mk = lambda k, last, s: tuple(a.reshape(ncol, nlay, last) for a in (  # noqa: E731
        ramp(k, 0.01, 8, 101 + s), ramp(k, 0, 1, 83 + s), ramp(k, 0, 0.9, 59 + s)))
    io, bnd, gpt = mk(n, ngpt, 0), mk(nrow * len(lims), len(lims), 2), mk(n, ngpt, 6)
    ident = np.stack([np.arange(1, ngpt + 1)] * 2, axis=1).astype(np.int32)
    for nstr_io, nstr_in in E.PAIRINGS:
        a = io[:1 if nstr_io == 1 else 3]
        for same, inc, lm in ((False, bnd, lims), (True, gpt, ident)):
            b = inc[:1 if nstr_in == 1 else 3]
            got = run_increment(dev, ncol, nlay, ngpt, lm, a, b, same=same)
            for x, y, name in zip(got, orc.increment_bybnd(lm, a, b), ("tau", "ssa", "g")):
                E.assert_bits(x.reshape(nrow, ngpt), y.reshape(nrow, ngpt), "increment %d by %d, %s, ngpt %d, same %s"
                              % (nstr_io, nstr_in, name, ngpt, same))


def test_increment_refusals(dev):
    """1025 g-points; overlapping band limits in rrtmgpnn_increment_bybnd and in a fused entry that takes a band
    increment (rrtmgpnn_sw_solver_2stream_inc): refused before anything is launched, the arrays untouched."""
    from rrtmgpnn._lib import int_array
    L = lib()
    a, b = torch.full((1025,), 0.5, device=dev), torch.full((1025,), 0.25, device=dev)
    rc = L.rrtmgpnn_increment(ctx(), 1, 1, 1025, p_(a), None, None, p_(b), None, None)
    assert rc == ERR_UNSUPPORTED and "1024" in last_error()
    rc = L.rrtmgpnn_increment_bybnd(ctx(), 1, 1, 1025, 1, int_array([1, 1025]), p_(a), None, None, p_(b), None, None)
    assert rc == ERR_UNSUPPORTED and "1024" in last_error()
    rc = L.rrtmgpnn_increment_bybnd(ctx(), 1, 1, 16, 2, int_array([1, 8, 8, 16]), p_(a), None, None, p_(b), None, None)
    assert rc == ERR_ARGUMENT and "overlap" in last_error()
    ng, nlay, ncol = 16, 2, 3
    f = lambda *s: torch.full(s, 0.5, device=dev)  # noqa: E731
    tau, ssa, inc, mu0, alb = f(ncol, nlay, ng), f(ncol, nlay, ng), f(ncol, ng), f(ncol), f(ncol, ng)
    bt, bw, bg = f(ncol, nlay, 2), f(ncol, nlay, 2), f(ncol, nlay, 2)
    outs = [torch.full((ncol, nlay + 1), -777.0, device=dev) for _ in range(3)]
    rc = L.rrtmgpnn_sw_solver_2stream_inc(ctx(), ng, nlay, ncol, 1, p_(inc), None, p_(tau), p_(ssa), None, 2,
                                          int_array([1, 9, 9, 16]), p_(bt), p_(bw), p_(bg), p_(mu0), p_(alb), p_(alb),
                                          *[p_(o) for o in outs])
    assert rc == ERR_ARGUMENT and "overlap" in last_error()
    assert (N(a) == 0.5).all() and all((N(o) == -777.0).all() for o in outs)


# ---- cloud optics ---------------------------------------------------------------------------------------------------------
CO_KEYS_LUT = ("lut_extliq", "lut_ssaliq", "lut_asyliq", "lut_extice", "lut_ssaice", "lut_asyice")
CO_KEYS_PADE = tuple("pade_" + k for k in ("extliq", "ssaliq", "asyliq", "extice", "ssaice", "asyice")) + \
    tuple("pade_sizreg_" + k for k in ("extliq", "ssaliq", "asyliq", "extice", "ssaice", "asyice"))


def cloud_handle(co, lut, path=None):
    """A rrtmgpnn_cloud_optics from the file (path) or from the host arrays of the dict (the file's layout)."""
    from rrtmgpnn import _lib
    h = _lib.c_vp()
    L = lib()
    if path is not None:
        check(L.rrtmgpnn_cloud_optics_load(ctx(), str(path).encode(), int(lut), h), "cloud_optics_load")
        return h
    nband = co["bnd_limits_wavenumber"].shape[0]
    wvn = np.ascontiguousarray(co["bnd_limits_wavenumber"], F)
    if lut:
        a = [np.ascontiguousarray(co[k], F) for k in CO_KEYS_LUT]
        check(L.rrtmgpnn_cloud_optics_create_lut(
            ctx(), nband, fp(wvn), a[0].shape[1], a[3].shape[2], a[3].shape[0], float(co["radliq_lwr"][0]),
            float(co["radliq_upr"][0]), float(co["radice_lwr"][0]), float(co["radice_upr"][0]), *[fp(x) for x in a], h),
            "cloud_optics_create_lut")
    else:
        a = [np.ascontiguousarray(co[k], F) for k in CO_KEYS_PADE]
        check(L.rrtmgpnn_cloud_optics_create_pade(ctx(), nband, fp(wvn), a[0].shape[1], a[0].shape[0], a[1].shape[0],
                                                  a[3].shape[0], *[fp(x) for x in a], h), "cloud_optics_create_pade")
    return h


def run_cloud_optics(dev, h, nband, args, nstr, icergh):
    L = lib()
    check(L.rrtmgpnn_cloud_optics_set_ice_roughness(h, icergh), "set_ice_roughness")
    ncol, nlay = args[0].shape
    ins = [T(a, dev) for a in args]
    outs = [torch.full((ncol, nlay, nband), -777.0, device=dev) for _ in range(1 if nstr == 1 else 3)]
    po = [p_(o) for o in outs] + [None] * (3 - len(outs))
    check(L.rrtmgpnn_cloud_optics_compute(ctx(), h, ncol, nlay, *[p_(t) for t in ins], *po), "cloud_optics_compute")
    return [N(o) for o in outs]


@pytest.mark.parametrize("lut", [True, False], ids=["lut", "pade"])
@pytest.mark.parametrize("source", ["load", "create"])
@pytest.mark.parametrize("which", ["lw", "sw"])
def test_cloud_optics_operand_edges(dev, orc, which, source, lut):
    """Every LUT knot and Pade size-regime bound with its float neighbours under every water path, liquid only, ice only
    and both; 1scl and 2str; each ice roughness.  The Pade runs hold -inf: bit patterns, never a tolerance."""
    from rrtmgpnn import data
    co = data.load_cloud_optics(which)
    p = E.build_cloud_optics(co, which)
    nband = co["bnd_limits_wavenumber"].shape[0]
    h = cloud_handle(co, lut, data.cloud_optics_path(which) if source == "load" else None)
    try:
        for nstr in (1, 2):
            for icergh in (1, 2, 3):
                got = run_cloud_optics(dev, h, nband, p["args"], nstr, icergh)
                want = orc.cloud_optics(co, *p["args"], nstr=nstr, lut=lut, icergh=icergh)
                for x, y, name in zip(got, want, ("tau", "ssa", "g")):
                    E.assert_bits(E.co_rows(x), E.co_rows(y), "cloud optics %s %s, nstr %d, roughness %d"
                                  % (which, name, nstr, icergh), p["describe"])
    finally:
        lib().rrtmgpnn_cloud_optics_destroy(h)


def synthetic_cloud_tables(nband):
    """Small tables of any band count in the coefficient file's layout (5 liquid and 4 ice sizes, 2 roughness types)."""
    nl, ni, nr = 5, 4, 2
    b, i = np.meshgrid(np.arange(nband), np.arange(nl), indexing="ij")
    r, bi, ii = np.meshgrid(np.arange(nr), np.arange(nband), np.arange(ni), indexing="ij")
    co = {"bnd_limits_wavenumber": np.stack([10.0 + 5 * np.arange(nband), 15.0 + 5 * np.arange(nband)], axis=1).astype(F),
          "radliq_lwr": np.array([2.5], F), "radliq_upr": np.array([21.5], F),
          "radice_lwr": np.array([10.0], F), "radice_upr": np.array([180.0], F),
          "lut_extliq": (0.1 + 0.01 * ((3 * b + i) % 17)).astype(F), "lut_ssaliq": (0.5 + 0.02 * ((b + 2 * i) % 13)).astype(F),
          "lut_asyliq": (0.7 + 0.01 * ((b + i) % 11)).astype(F),
          "lut_extice": (0.05 + 0.01 * ((bi + 2 * ii + r) % 19)).astype(F),
          "lut_ssaice": (0.4 + 0.03 * ((2 * bi + ii + r) % 7)).astype(F),
          "lut_asyice": (0.6 + 0.02 * ((bi + ii + 3 * r) % 5)).astype(F)}

    def pade(ncoef, rough):
        shp = ((nr,) if rough else ()) + (ncoef, 3, nband)
        idx = np.indices(shp).astype(np.float64)
        c, s, bb = idx[-3], idx[-2], idx[-1]
        rr = idx[0] if rough else 0.0
        return (0.05 * (1.0 + ((bb + 2 * s + rr) % 5)) * 10.0 ** (-3.0 * c)).astype(F)
    for k, n in (("ext", 6), ("ssa", 5), ("asy", 5)):
        co["pade_" + k + "liq"], co["pade_" + k + "ice"] = pade(n, False), pade(n, True)
        co["pade_sizreg_" + k + "liq"] = np.array([2, 10, 35, 60], F)
        co["pade_sizreg_" + k + "ice"] = np.array([10, 20, 30, 180], F)
    return co


def benign_clouds(nrow, co):
    """(nrow, 1) water paths and radii inside the tables: liquid only, ice only, both and neither by turns."""
    k = np.arange(nrow)
    lwp = np.where(k % 4 < 2, 10.0 + (k % 7), 0.0)
    iwp = np.where((k % 4) % 3 != 0, 5.0 + (k % 5), 0.0)
    rl = ramp(nrow, float(co["radliq_lwr"][0]), float(co["radliq_upr"][0]), 23)
    ri = ramp(nrow, float(co["radice_lwr"][0]), float(co["radice_upr"][0]), 29)
    return tuple(np.ascontiguousarray(a.astype(F).reshape(nrow, 1)) for a in (lwp, iwp, rl, ri))


@pytest.mark.parametrize("lut", [True, False], ids=["lut", "pade"])
@pytest.mark.parametrize("nband", [1, 3, 14, 16, 129, 256])
def test_cloud_optics_band_counts(dev, orc, nband, lut):
    """rows per block 256 // nband = 256, 85, 18, 16, 1, 1: a block of 255 threads (3 bands), lanes beyond rpb * nband
    that must leave (14, 129 bands); 2 * rpb + 3 rows: three blocks, the last one short."""
    co = synthetic_cloud_tables(nband)
    rpb = 256 // nband
    args = benign_clouds(2 * rpb + 3, co)
    h = cloud_handle(co, lut)
    try:
        for nstr, icergh in ((1, 1), (2, 2)):
            got = run_cloud_optics(dev, h, nband, args, nstr, icergh)
            want = orc.cloud_optics(co, *args, nstr=nstr, lut=lut, icergh=icergh)
            for x, y, name in zip(got, want, ("tau", "ssa", "g")):
                assert np.isfinite(y).all() and (y != 0).any()
                E.assert_bits(E.co_rows(x), E.co_rows(y), "cloud optics %s, %d bands, nstr %d" % (name, nband, nstr))
    finally:
        lib().rrtmgpnn_cloud_optics_destroy(h)


@pytest.mark.parametrize("delta", [-1, 1])
def test_cloud_optics_rows_around_the_grid_cap(dev, orc, delta):
    """At most 8 * CUs blocks of rpb rows: cap * rpb + 1 rows give block 0 a second trip of one row, cap * rpb - 1 rows
    leave the last block's last row out (the shipped LW tables, 16 bands, rpb 16)."""
    from rrtmgpnn import data
    co = data.load_cloud_optics("lw")
    nband = co["bnd_limits_wavenumber"].shape[0]
    nrow = 8 * cus() * (256 // nband) + delta
    args = benign_clouds(nrow, co)
    h = cloud_handle(co, True)
    try:
        got = run_cloud_optics(dev, h, nband, args, 2, 1)
    finally:
        lib().rrtmgpnn_cloud_optics_destroy(h)
    for x, y, name in zip(got, orc.cloud_optics(co, *args, nstr=2, lut=True, icergh=1), ("tau", "ssa", "g")):
        E.assert_bits(E.co_rows(x), E.co_rows(y), "cloud optics %s, %d rows" % (name, nrow))


def test_cloud_optics_host_side_returns(dev):
    """257 bands are refused where the tables are made; no rows is a return before any launch."""
    from rrtmgpnn import _lib
    co = synthetic_cloud_tables(257)
    h = _lib.c_vp()
    a = [np.ascontiguousarray(co[k], F) for k in CO_KEYS_LUT]
    rc = lib().rrtmgpnn_cloud_optics_create_lut(ctx(), 257, None, 5, 4, 2, 2.5, 21.5, 10.0, 180.0, *[fp(x) for x in a], h)
    assert rc == ERR_ARGUMENT and not h.value
    a = [np.ascontiguousarray(co[k], F) for k in CO_KEYS_PADE]
    rc = lib().rrtmgpnn_cloud_optics_create_pade(ctx(), 257, None, 3, 6, 5, 2, *[fp(x) for x in a], h)
    assert rc == ERR_ARGUMENT and not h.value
    co = synthetic_cloud_tables(3)
    h = cloud_handle(co, True)
    try:
        z = torch.full((4,), -777.0, device=dev)
        for ncol, nlay in ((0, 4), (4, 0)):
            rc = lib().rrtmgpnn_cloud_optics_compute(ctx(), h, ncol, nlay, p_(z), p_(z), p_(z), p_(z), p_(z), None, None)
            assert rc == OK
        assert (N(z) == -777.0).all()
    finally:
        lib().rrtmgpnn_cloud_optics_destroy(h)


# ---- heating rates --------------------------------------------------------------------------------------------------------
def run_heating(dev, up, dn, plev, k_day):
    ncol, nlev = up.shape
    u, d, pl = T(up, dev), T(dn, dev), T(plev, dev)
    out = torch.full((ncol, nlev - 1), -777.0, device=dev)
    f = lib().rrtmgpnn_calc_heating_rate_k_day if k_day else lib().rrtmgpnn_compute_heating_rate
    check(f(ctx(), ncol, nlev - 1, p_(u), p_(d), p_(pl), p_(out)), "heating rate")
    return N(out)


@pytest.mark.parametrize("k_day", [False, True], ids=["k_per_s", "k_per_day"])
def test_heating_rate_operand_edges(dev, orc, k_day):
    p = E.build_heating()
    got = run_heating(dev, p["up"], p["dn"], p["plev"], k_day)
    E.assert_bits(got, orc.heating_rate(p["up"], p["dn"], p["plev"], k_day=k_day), "heating rate", p["describe"])


@pytest.mark.parametrize("k_day", [False, True], ids=["k_per_s", "k_per_day"])
@pytest.mark.parametrize("ncol,nlay", [(1, 1), (3, 85), (257, 1)])
def test_heating_rate_shapes(dev, orc, ncol, nlay, k_day):
    n = ncol * (nlay + 1)
    plev = (100.0 + 1013.0 * np.arange(nlay + 1, dtype=F)[None, :] + 3.0 * np.arange(ncol, dtype=F)[:, None]).astype(F)
    if ncol > 1:
        plev[1::2] = plev[1::2, ::-1].copy()  # every other column bottom first
    up, dn = ramp(n, 50, 450, 71).reshape(ncol, nlay + 1), ramp(n, 0, 400, 43).reshape(ncol, nlay + 1)
    got = run_heating(dev, up, dn, np.ascontiguousarray(plev), k_day)
    E.assert_bits(got, orc.heating_rate(up, dn, plev, k_day=k_day), "heating rate (%d, %d)" % (ncol, nlay))


# ---- expand ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["sw", "lw", "one", "odd", "gap"])
def test_expand_band_to_gpt(dev, orc, layout):
    """Every kind of value, signed zeros, denormals and infinities among them, copied bit for bit; a g-point in no band
    keeps what the output held."""
    from rrtmgpnn._lib import int_array
    p = E.build_expand(layout)
    arr = T(p["arr"], dev)
    out = torch.full((p["ncol"], p["ngpt"]), float(E.SENTINEL), device=dev)
    check(lib().rrtmgpnn_expand_band_to_gpt(ctx(), p["nb"], p["ngpt"], p["ncol"], int_array(p["lims"].ravel()), p_(arr),
                                            p_(out)), "expand_band_to_gpt")
    want = E.expand_ref(orc, p)
    assert (want[:, ~p["covered"]] == E.SENTINEL).all() and (want[:, p["covered"]] != E.SENTINEL).all()
    E.assert_bits(N(out), want, "expand, layout %s" % layout, p["describe"])


# ---- the glue kernels -----------------------------------------------------------------------------------------------------
_NETS = {}


def nets(kind):
    """The kind's networks through the class layer (the shipped RBIN models, the reduced-resolution netCDF fixtures)."""
    from rrtmgpnn import api
    if kind not in _NETS:
        _NETS[kind] = [api.RrtmgpNetwork(0).load_netcdf(E.model_path(n)) for n in E.NET_KINDS[kind]]
    return _NETS[kind]


def gas_args(p, dev, keep):
    from rrtmgpnn._lib import int_array, ptr_array
    ptrs, nds = [], []
    for k, n in enumerate(p["names"]):
        form = p["forms"].get(n, "absent")
        if k < 2 or form == "absent":
            ptrs.append(None)
            nds.append(2)
            continue
        t = T(np.atleast_1d(p["gases"][n]), dev)
        keep.append(t)
        ptrs.append(t.data_ptr())
        nds.append({"scalar": 0, "1d": 1, "2d": 2}[form])
    return ptr_array(ptrs), int_array(nds)


def run_nn_inputs(dev, p, net):
    keep = []
    gp, nd = gas_args(p, dev, keep)
    nx = len(p["names"])
    play, tlay = T(p["play"], dev), T(p["tlay"], dev)
    out = torch.full((p["ncol"] * p["nlay"] + 1, nx), -777.0, device=dev)  # a guard row behind the samples
    check(lib().rrtmgpnn_compute_nn_inputs(ctx(), p["ncol"], p["nlay"], nx, p_(play), p_(tlay), gp, nd, net.h, p_(out)),
          "compute_nn_inputs")
    got = N(out)
    assert (got[-1] == -777.0).all(), "wrote past the last sample"
    return got[:-1]


@pytest.mark.parametrize("variant", E.GL_VARIANTS)
@pytest.mark.parametrize("kind", ["lw_pair", "sw_pair"])
def test_nn_inputs_operand_edges(dev, orc, kind, variant):
    m = E.models(kind)[0]
    p = E.build_glue(m, kind, variant)
    got = run_nn_inputs(dev, p, nets(kind)[0])
    want = orc.nn_inputs(p["play"], p["tlay"], p["gases"], m)
    E.assert_bits(got, E.glue_rows(want, p), "compute_nn_inputs (%s, variant %d)" % (kind, variant), p["describe"])


def synthetic_input_model(nx):
    """A network of nx inputs whose only purpose is its input scaling (compute_nn_inputs reads nothing else)."""
    from rrtmgpnn import rbin
    dims = [nx, 4, 4, 4]
    m = {"dims": np.array(dims, np.int32), "activation": np.array([1, 1, 0], np.int32),
         "input_min": (0.01 * np.arange(nx)).astype(F), "input_max": (1.5 + 0.25 * np.arange(nx)).astype(F),
         "input_names": rbin.chars(["tlay", "play", "h2o", "o3"] + ["gas%d" % k for k in range(4, nx)])}
    for n in range(1, 4):
        w = ((np.arange(dims[n - 1] * dims[n]) % 7) - 3.0) / 8.0
        m["w%d" % n], m["b%d" % n] = w.reshape(dims[n - 1], dims[n]).astype(F), np.zeros(dims[n], F)
    return m


@pytest.mark.parametrize("nsamp", [1, 255, 256, 257])
@pytest.mark.parametrize("nx", [4, 7, 18, 32])
def test_nn_inputs_shapes(dev, orc, nx, nsamp):
    """256 samples a block, staged in LDS as (nx, 256): the input counts at both ends of the unrolled gas loop, the
    sample counts around one block; the gases behind o3 scalar, 1-D, 2-D and absent by turns."""
    from rrtmgpnn import api, rbin
    m = synthetic_input_model(nx)
    net = api.RrtmgpNetwork(0).from_arrays(m)
    ncol, nlay = (nsamp, 1) if nsamp < 255 else ((85, 3) if nsamp == 255 else ((64, 4) if nsamp == 256 else (257, 1)))
    n = ncol * nlay
    names = rbin.unchars(m["input_names"])
    gases = {"h2o": ramp(n, 1e-6, 0.04, 37).reshape(ncol, nlay), "o3": ramp(n, 1e-8, 1e-5, 31).reshape(ncol, nlay)}
    forms = {"h2o": "2d", "o3": "2d"}
    for i, g in enumerate(names[4:]):
        forms[g] = E.GL_FORMS[i % 4]
        if forms[g] == "2d":
            gases[g] = ramp(n, 0, 1, 17 + i).reshape(ncol, nlay)
        elif forms[g] == "1d":
            gases[g] = ramp(nlay, 0, 1, 5 + i)
        elif forms[g] == "scalar":
            gases[g] = F(0.1 * (i + 1))
    p = {"ncol": ncol, "nlay": nlay, "names": names, "forms": forms, "gases": gases,
         "play": ramp(n, 100, 101325, 53).reshape(ncol, nlay), "tlay": ramp(n, 180, 320, 47).reshape(ncol, nlay)}
    got = run_nn_inputs(dev, p, net)
    want = orc.nn_inputs(p["play"], p["tlay"], gases, m)
    E.assert_bits(got, want.reshape(n, nx), "compute_nn_inputs, %d inputs, %d samples" % (nx, nsamp))


def run_col_dry(dev, h2o, plev):
    ncol, nlay = h2o.shape
    v, pl = T(h2o, dev), T(plev, dev)
    out = torch.full((ncol, nlay), -777.0, device=dev)
    check(lib().rrtmgpnn_get_col_dry(ctx(), ncol, nlay, p_(v), p_(pl), p_(out)), "get_col_dry")
    return N(out)


def test_col_dry_operand_edges(dev, orc):
    """Every h2o beside every level pair, the zero-thickness layer and (1e-45, 0) among them."""
    m = E.models("sw_pair")[0]
    p = E.build_glue(m, "sw_pair", 0)
    h2o = p["gases"][p["names"][2]]
    E.assert_bits(run_col_dry(dev, h2o, p["plev"]), orc.col_dry(h2o, p["plev"]), "get_col_dry", p["describe"])


@pytest.mark.parametrize("nlay", [2, 5])
def test_interpolate_tlev_operand_edges(dev, orc, nlay):
    p = E.build_tlev(nlay)
    pa, pv, ta = T(p["play"], dev), T(p["plev"], dev), T(p["tlay"], dev)
    out = torch.full((p["ncol"], nlay + 1), -777.0, device=dev)
    check(lib().rrtmgpnn_interpolate_tlev(ctx(), p["ncol"], nlay, p_(pa), p_(pv), p_(ta), p_(out)), "interpolate_tlev")
    E.assert_bits(N(out), orc.interpolate_tlev(p["play"], p["plev"], p["tlay"]), "interpolate_tlev", p["describe"])
    rc = lib().rrtmgpnn_interpolate_tlev(ctx(), p["ncol"], 1, p_(pa), p_(pv), p_(ta), p_(out))
    assert rc == ERR_ARGUMENT and "nlay >= 2" in last_error()


# ---- the fused entries: the inputs formed inside both MFMA tilings ---------------------------------------------------------
def mlp_path():
    path = (ctypes.c_int * 8)()
    check(lib().rrtmgpnn_context_get_mlp_path(ctx(), path), "context_get_mlp_path")
    return list(path)


def run_networks(dev, kind, p, fused, x=None, cd=None):
    """rrtmgpnn_gas_optics_*_nn (fused), or rrtmgpnn_compute_nn_inputs + rrtmgpnn_get_col_dry + rrtmgpnn_predict_nn_*
    -> (first output, second output, mlp path), the outputs (ncol * nlay, ngpt)."""
    from rrtmgpnn._lib import ptr_array
    L, c = lib(), ctx()
    nn = nets(kind)
    hs = ptr_array([n.h.value for n in nn])
    ncol, nlay, ngpt, nx = p["ncol"], p["nlay"], E.NET_NGPT[kind], len(p["names"])
    keep = []
    gp, nd = gas_args(p, dev, keep)
    ins = [T(p[k], dev) for k in ("play", "tlay", "plev")] + [T(p["gases"][p["names"][2]], dev)]
    o0, o1 = (torch.full((ncol * nlay, ngpt), -777.0, device=dev) for _ in range(2))
    sw = kind.startswith("sw")
    if fused:
        head = (c, ncol, nlay, ngpt, nx) + tuple(p_(t) for t in ins) + (gp, nd, hs)
        if sw:
            check(L.rrtmgpnn_gas_optics_sw_nn(*head, p_(o0), p_(o1), None), "gas_optics_sw_nn")
        else:
            check(L.rrtmgpnn_gas_optics_lw_nn(*head, len(nn), p_(o0), p_(o1)), "gas_optics_lw_nn")
    else:
        xd, cdd = torch.empty((ncol * nlay, nx), device=dev), torch.empty((ncol, nlay), device=dev)
        check(L.rrtmgpnn_compute_nn_inputs(c, ncol, nlay, nx, p_(ins[0]), p_(ins[1]), gp, nd, nn[0].h, p_(xd)),
              "compute_nn_inputs")
        check(L.rrtmgpnn_get_col_dry(c, ncol, nlay, p_(ins[3]), p_(ins[2]), p_(cdd)), "get_col_dry")
        head = (c, ncol, nlay, ngpt, nx, p_(xd), p_(cdd), hs)
        if sw:
            check(L.rrtmgpnn_predict_nn_sw(*head, p_(o0), p_(o1), None), "predict_nn_sw")
        else:
            check(L.rrtmgpnn_predict_nn_lw(*head, len(nn), p_(o0), p_(o1)), "predict_nn_lw")
    got = N(o0), N(o1)
    return got[0], got[1], mlp_path()


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("kind", sorted(E.NET_KINDS))
def test_fused_gas_optics_operand_edges(dev, orc, kind, variant, mlp_kernel):
    """The one-layer glue columns through the fused entries under both tilings: the oracle's nn_inputs -> mlp ->
    tau_post / both_post bit for bit, and the three separate GPU calls bit for bit (include/rrtmgpnn.h promises it).
    The SW ssa is nan exactly where the oracle's is (tau == 0: the layer of zero thickness)."""
    p, x, cd, w0, w1 = E.network_ref(orc, kind, variant)
    f0, f1, path = run_networks(dev, kind, p, True)
    if mlp_kernel == 0:
        assert path[0] == MFMA32 and path[7] & F_XIN, path  # form_x of kernels_nn32.hip
    else:
        assert path[0] == MFMA16, path
        if kind in ("lw_pair", "sw_pair"):
            assert path[7] & F_XIN, path  # the XIN path of kernels_nn.hip
    s0, s1, _ = run_networks(dev, kind, p, False)
    what = "%s, variant %d, mlp kernel %d" % (kind, variant, mlp_kernel)
    E.assert_bits(f0, w0, "fused first output against the oracle: " + what, p["describe"])
    assert_bits_nan(f1, w1, "fused second output against the oracle: " + what, p["describe"])
    E.assert_bits(f0, s0, "fused first output against the three calls: " + what, p["describe"])
    assert_bits_nan(f1, s1, "fused second output against the three calls: " + what, p["describe"])
    if kind.startswith("sw"):
        assert np.array_equal(np.isnan(f1), f0 == 0)
    else:
        assert not np.isnan(f1).any()
