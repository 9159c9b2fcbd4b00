"""GPU: the reduced-resolution spectral configuration (the 2021 networks: LW g128 pair 18-72-72-128 + 18-24-24-128, SW
g112 pair 7-32-32-112 twice, and the LW g128 single model 18-64-64-256), every comparison bit for bit.

  * the network kernels against the oracle (pinned to the reference on these models by
    tests/test_reduced_spectral_host.py), through rrtmgpnn_predict_nn_* and the fused rrtmgpnn_gas_optics_*_nn, on the
    32x32x2 instances (asserted: rrtmgpnn_context_get_mlp_path) and, forced, on the 16x16x4 route;
  * the SW pair's partial last g-tile (112 = 3 x 32 + 16): guard floats behind every output, ssa == NULL, g != NULL,
    an output base off 16-byte alignment;
  * ClearSkyStep(spectral=...) on 36 RFMIP columns: clear sky at one and three angles, McICA (seeded) with clear-sky
    fluxes and aerosols, by band, the upper boundary condition -- with the solver instance each runs
    (rrtmgpnn_context_get_solver_path; the table in DESIGN.md);
  * the Fortran host program with its model and k-distribution path arguments;
  * ClearSkyStep(spectral=None): the committed step plans, unchanged."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import byband_ref as R
import mcica_ref as MC
import philox_ref as PH
import step_plan as P
from conftest import ROOT, subset

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FILES = os.path.join(ROOT, "tests", "golden", "reference_files")
PATHS = {"lw_abs": os.path.join(FILES, "lw-g128-210809_absorption_BEST.nc"),
         "lw_pfrac": os.path.join(FILES, "lw-g128-210809_planck_frac_BEST.nc"),
         "sw_abs": os.path.join(FILES, "sw-g112-210809_absorption_BEST.nc"),
         "sw_ray": os.path.join(FILES, "sw-g112-210809_rayleigh_BEST.nc")}
SPECTRAL = {"lw_models": (PATHS["lw_abs"], PATHS["lw_pfrac"]), "sw_models": (PATHS["sw_abs"], PATHS["sw_ray"]),
            "ngpt_lw": 128, "ngpt_sw": 112}
KINDS = {"lw_pair": ("lw_abs", "lw_pfrac"), "sw_pair": ("sw_abs", "sw_ray"), "lw_both": ("lw_g128_both",)}
NGPT = {"lw_pair": 128, "sw_pair": 112, "lw_both": 128}
# nbatch = ncol * nlay: a wave owns 32 samples
SHAPES = {1: (1, 1), 31: (1, 31), 32: (2, 16), 33: (3, 11), 1100: (20, 55)}
MFMA32, MFMA16 = 2, 3
F_SSL, F_NGTC, F_XIN, F_VEC4 = 1, 2, 4, 8
SENTINEL, GUARD = -777.0, 64
FLUX = ("lw_up", "lw_dn", "sw_up", "sw_dn", "sw_dir")
SEED = 20261020


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a device"
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def T(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=dev)


def bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else a
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(got, want, msg):
    np.testing.assert_array_equal(bits(got).reshape(-1), bits(want).reshape(-1), err_msg=msg)


def lib():
    from rrtmgpnn import _lib
    return _lib.lib()


def ctx():
    from rrtmgpnn.api import context
    return context(0)


def mlp_path():
    from rrtmgpnn._lib import check
    p = (ctypes.c_int * 8)()
    check(lib().rrtmgpnn_context_get_mlp_path(ctx().h, p), "context_get_mlp_path")
    return list(p)


def solver_path(c):
    from rrtmgpnn._lib import check
    p = (ctypes.c_int * 4)()
    check(lib().rrtmgpnn_context_get_solver_path(c.h, p), "context_get_solver_path")
    return list(p)[:3]


_MODELS, _NETS, _WANT = {}, {}, {}


def model(key):
    from rrtmgpnn import data
    if key not in _MODELS:
        _MODELS[key] = data.load_model(PATHS.get(key, key))
    return _MODELS[key]


def nets(kind):
    """The kind's networks through the class layer (load_netcdf: the netCDF fixtures, or the shipped RBIN model)."""
    from rrtmgpnn import api, data
    if kind not in _NETS:
        _NETS[kind] = [api.RrtmgpNetwork(0).load_netcdf(PATHS.get(k) or data.path(k)) for k in KINDS[kind]]
    return _NETS[kind]


def state(rfmip, kind, nbatch):
    """ncol x nlay = nbatch samples of RFMIP columns; the gases behind h2o and o3 in every gas_ndims form, by turns with
    the batch and the gas: 2-D, a 1-D profile, a scalar, absent."""
    from rrtmgpnn import rbin
    ncol, nlay = SHAPES[nbatch]
    p = subset(rfmip, (np.arange(ncol) * 97 + 5) % 1800)
    lay0 = 60 - nlay  # the lowest layers: the widest range of water vapour
    out = {"ncol": ncol, "nlay": nlay, "play": np.ascontiguousarray(p["play"][:, lay0:]),
           "plev": np.ascontiguousarray(p["plev"][:, lay0:]), "tlay": np.ascontiguousarray(p["tlay"][:, lay0:])}
    names = rbin.unchars(model(KINDS[kind][0])["input_names"])
    gases, forms = {}, {}
    for i, n in enumerate(names[2:]):
        v = np.ascontiguousarray(p["gases"][n][:, lay0:])
        form = 2 if i < 2 else (3, 1, 0, 2)[(i + nbatch) % 4]  # 3: absent
        forms[n] = form
        if form == 2:
            gases[n] = v
        elif form == 1:
            gases[n] = np.ascontiguousarray(v[0])
        elif form == 0:
            gases[n] = np.float32(v[0, 0])
    assert set(forms.values()) >= ({0, 1, 2, 3} if len(names) > 7 else {2}) and len(set(forms.values())) >= 3
    out["gases"], out["names"], out["forms"] = gases, names, forms
    return out


def want(orc, rfmip, kind, nbatch):
    """(state, x, col_dry, out0, out1): the oracle's network inputs and outputs, computed once per case."""
    key = (kind, nbatch)
    if key not in _WANT:
        s = state(rfmip, kind, nbatch)
        ms = [model(k) for k in KINDS[kind]]
        x = orc.nn_inputs(s["play"], s["tlay"], s["gases"], ms[0])
        cd = orc.col_dry(s["gases"]["h2o"], s["plev"])
        xf = x.reshape(-1, x.shape[-1])
        if kind == "lw_pair":
            y = orc.mlp(ms[1], xf)
            o0, o1 = orc.tau_post(ms[0], orc.mlp(ms[0], xf), cd), (y * y).astype(np.float32)
        elif kind == "lw_both":
            o0, o1 = orc.both_post(ms[0], orc.mlp(ms[0], xf), cd)
        else:
            o0 = orc.tau_post(ms[0], orc.mlp(ms[0], xf), cd)
            o1 = orc.tau_post(ms[1], orc.mlp(ms[1], xf), cd, tau_abs_to_tot=o0)
        assert np.isfinite(o0).all() and np.isfinite(o1).all() and (o0 > 0).any()
        _WANT[key] = (s, x, cd, o0, o1)
    return _WANT[key]


def guarded(dev, n, offset=0):
    """n output floats with GUARD sentinel floats behind them (and `offset` in front): (buffer, view)."""
    buf = torch.full((offset + n + GUARD,), SENTINEL, device=dev)
    return buf, buf[offset:offset + n]


def guards_intact(buf, n, offset=0):
    torch.cuda.synchronize()
    return bool((buf[offset + n:] == SENTINEL).all()) and bool((buf[:offset] == SENTINEL).all())


def gas_args(s, dev, keep):
    from rrtmgpnn._lib import int_array, ptr_array
    ptrs, nds = [], []
    for k, n in enumerate(s["names"]):
        form = s["forms"].get(n, 2) if k >= 2 else 2
        if k < 2 or form == 3:
            ptrs.append(None)
            nds.append(2)
            continue
        t = T(np.atleast_1d(s["gases"][n]), dev)
        keep.append(t)
        ptrs.append(t.data_ptr())
        nds.append(form)
    return ptr_array(ptrs), int_array(nds)


def run(kind, fused, s, x, cd, dev, outs, g=None, ssa=True):
    """One call of rrtmgpnn_predict_nn_* (fused False) or rrtmgpnn_gas_optics_*_nn (True) into the views `outs`."""
    from rrtmgpnn._lib import check, ptr_array
    L, c = lib(), ctx().h
    nn = nets(kind)
    hs = ptr_array([n.h.value for n in nn])
    ncol, nlay, ngpt, nx = s["ncol"], s["nlay"], NGPT[kind], len(s["names"])
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    keep = []
    o1 = outs[1] if ssa else None
    if fused:
        ins = [T(s[k], dev) for k in ("play", "tlay", "plev")] + [T(s["gases"]["h2o"], dev)]
        gp, nd = gas_args(s, dev, keep)
        head = (c, ncol, nlay, ngpt, nx) + tuple(p(t) for t in ins) + (gp, nd)
        if kind == "sw_pair":
            check(L.rrtmgpnn_gas_optics_sw_nn(*head, hs, p(outs[0]), p(o1), p(g)), "gas_optics_sw_nn")
        else:
            check(L.rrtmgpnn_gas_optics_lw_nn(*head, hs, len(nn), p(outs[0]), p(o1)), "gas_optics_lw_nn")
    else:
        xd, cdd = T(x, dev), T(cd, dev)
        head = (c, ncol, nlay, ngpt, nx, p(xd), p(cdd), hs)
        if kind == "sw_pair":
            check(L.rrtmgpnn_predict_nn_sw(*head, p(outs[0]), p(o1), p(g)), "predict_nn_sw")
        else:
            check(L.rrtmgpnn_predict_nn_lw(*head, len(nn), p(outs[0]), p(o1)), "predict_nn_lw")
    torch.cuda.synchronize()
    return mlp_path()


@pytest.mark.parametrize("nbatch", sorted(SHAPES))
@pytest.mark.parametrize("fused", [False, True], ids=["predict", "fused"])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_network_kernels_match_the_oracle(dev, orc, rfmip, kind, fused, nbatch):
    """The 32x32x2 instance of each reduced model set, then the same call forced onto the 16x16x4 route: both the
    oracle's bits, each on the kernel meant.  1100 samples on one CU's worth of blocks: the waves stride several tiles
    and a second block round runs."""
    s, x, cd, w0, w1 = want(orc, rfmip, kind, nbatch)
    n = nbatch * NGPT[kind]
    c = ctx()
    cap = c.mlp_max_cus()
    if nbatch == 1100:
        c.set_mlp_max_cus(1)
    try:
        got = {}
        for mode in (0, 1):
            c.set_mlp_kernel(mode)
            b0, o0 = guarded(dev, n)
            b1, o1 = guarded(dev, n)
            path = run(kind, fused, s, x, cd, dev, (o0, o1))
            assert guards_intact(b0, n) and guards_intact(b1, n), "wrote past the outputs"
            if mode == 0:
                assert path[0] == MFMA32 and path[7] == F_SSL | F_NGTC | F_VEC4 | (F_XIN if fused else 0), path
            else:
                assert path[0] == MFMA16, path
            same(o0, w0, "%s first output, mlp kernel %d" % (kind, mode))
            same(o1, w1, "%s second output, mlp kernel %d" % (kind, mode))
            got[mode] = (o0.clone(), o1.clone())
        same(got[0][0], got[1][0], "32x32x2 against 16x16x4")
        same(got[0][1], got[1][1], "32x32x2 against 16x16x4")
    finally:
        c.set_mlp_kernel(0)
        c.set_mlp_max_cus(cap)


@pytest.mark.parametrize("fused", [False, True], ids=["predict", "fused"])
@pytest.mark.parametrize("nbatch", [33, 1100])
def test_sw_partial_last_tile(dev, orc, rfmip, fused, nbatch):
    """SW g112: the last g-tile holds 16 g-points.  GUARD sentinel floats behind tau, ssa and g stay as they were; g
    (non-NULL) is zero; ssa == NULL gives the absorption optical depth alone (1scl); an output base one float off
    16-byte alignment runs the 16x16x4 kernel and gives the same bits."""
    s, x, cd, w0, w1 = want(orc, rfmip, "sw_pair", nbatch)
    n = nbatch * 112
    bufs = [guarded(dev, n) for _ in range(3)]
    path = run("sw_pair", fused, s, x, cd, dev, (bufs[0][1], bufs[1][1]), g=bufs[2][1])
    assert path[0] == MFMA32, path
    assert all(guards_intact(b, n) for b, _ in bufs), "wrote past the outputs"
    same(bufs[0][1], w0, "tau")
    same(bufs[1][1], w1, "ssa")
    assert bool((bufs[2][1] == 0).all()), "g"
    # 1scl: absorption alone
    b0, o0 = guarded(dev, n)
    run("sw_pair", fused, s, x, cd, dev, (o0, None), ssa=False)
    assert guards_intact(b0, n)
    m = model("sw_abs")
    same(o0, orc.tau_post(m, orc.mlp(m, x.reshape(-1, 7)), cd), "tau (ssa == NULL)")
    # one float off 16-byte alignment
    off = [guarded(dev, n, offset=1) for _ in range(2)]
    assert off[0][1].data_ptr() % 16 == 4
    path = run("sw_pair", fused, s, x, cd, dev, (off[0][1], off[1][1]))
    assert path[0] == MFMA16, path
    assert all(guards_intact(b, n, 1) for b, _ in off)
    same(off[0][1], w0, "tau, unaligned")
    same(off[1][1], w1, "ssa, unaligned")


# ---- the step --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case(rfmip):
    """36 RFMIP columns x 60 layers (every 50th: sunlit and dark columns), the all-sky example's clouds, a cloud fraction
    and overlap parameter, aerosols by band."""
    from rrtmgpnn import data
    prob = subset(rfmip, np.arange(0, 1800, 50))
    ncol, nlay = prob["ncol"], prob["nlay"]
    use = prob["usecol"]
    assert ncol == 36 and use.any() and (~use).any()
    clouds = data.allsky_clouds(prob, data.load_cloud_optics("lw"))
    cloudy = (clouds[0] > 0) | (clouds[1] > 0)
    assert cloudy.any()
    rng = np.random.default_rng(64)
    cf = np.where(cloudy, rng.uniform(0.2, 0.9, cloudy.shape), 0).astype(np.float32)
    ov = rng.uniform(-1, 1, (ncol, nlay - 1)).astype(np.float32)
    kl, ks = data.load_kdist("lw", 128), data.load_kdist("sw", 112)
    aer = {"lw_tau": rng.lognormal(-2, 1, (ncol, nlay, kl["nband"])).astype(np.float32),
           "sw_tau": rng.lognormal(-2, 1, (ncol, nlay, ks["nband"])).astype(np.float32),
           "sw_ssa": rng.uniform(0.6, 1, (ncol, nlay, ks["nband"])).astype(np.float32),
           "sw_g": rng.uniform(0.3, 0.8, (ncol, nlay, ks["nband"])).astype(np.float32)}
    return dict(prob=prob, use=use, clouds=clouds, cf=cf, ov=ov, aer=aer, kl=kl, ks=ks,
                lw=[model("lw_abs"), model("lw_pfrac")], sw=[model("sw_abs"), model("sw_ray")])


def run_step(step):
    for k in FLUX:
        getattr(step, k).fill_(float("nan"))
    step.step()
    torch.cuda.synchronize()
    assert step.ng_lw == 128 and step.ng_sw == 112 and tuple(step.tau_sw.shape)[-1] == 112
    out = dict(step.fluxes())
    if step.clrsky:
        out.update(step.clrsky_fluxes())
    paths = (solver_path(step.ctx), solver_path(step.ctx2 if step.ctx2 is not None else step.ctx))
    return out, paths


def equal(got, want_, use, keys=None):
    """Bitwise; the SW arrays on the sunlit columns (the oracle solves the others with the driver's mu0 = 1)."""
    for k in (keys or want_):
        g, w = got[k], want_[k]
        if k.startswith("sw"):
            g, w = g[use], w[use]
        np.testing.assert_array_equal(bits(g), bits(w), err_msg=k)


# The solver instance each step runs, (family, options) of the LW and of the SW context's last launch, as the launchers
# select at ngpt 128 / 112 on 36 columns (select_lw_noscat, select_sw_ck; the same as at 256 / 224: no rule of theirs
# turns on ngpt below 256 but "ngpt % 64 == 0" for the wave-uniform mask pair, which 128 meets).
#   LW lw_noscat_kernel (1): 1 fused sources, +4 several angles, +8 by band, 3|16|32|64|256 = 371 dual + mask pair +
#   aerosol; SW sw_2stream_ck_kernel (2): 1024|8|16 = 1048 the small-grid instance with its planes, +64 by band; the
#   McICA step's last SW launch is its clear solve (sw_solver_clr follows sw_solver in the fused chain), the aerosol as
#   that call's band increment on the band-pair layout with the transmittance plane, 2|8|32 = 42 (the all-sky launch
#   before it: 2|8|32|128|256 = 426, aerosol + masked cloud).
SOLVER_PATHS = {"clear": ((1, 1), (2, 1048)), "nmus3": ((1, 5), (2, 1048)), "mcica": ((1, 371), (2, 42)),
                "byband": ((1, 9), (2, 1112)), "upper_bc": ((1, 1), (2, 1048))}


def assert_paths(paths, mode):
    (lw, sw), w = paths, SOLVER_PATHS[mode]
    assert (lw[0], lw[1]) == w[0] and (sw[0], sw[1]) == w[1], (mode, paths)


@pytest.mark.parametrize("nmus", [1, 3])
def test_step_clear_sky(dev, orc, case, nmus):
    from rrtmgpnn.pipeline import ClearSkyStep
    c = case
    step = ClearSkyStep(c["prob"], device=0, nmus=nmus, spectral=SPECTRAL)
    got, paths = run_step(step)
    p = mlp_path_of(step)
    step.close()
    assert p[0][0] == MFMA32 and p[0][7] & F_XIN and p[1][0] == MFMA32 and p[1][7] & F_XIN, p
    lu, ld, _ = orc.clear_sky_lw(c["prob"], c["lw"], c["kl"], nmus)
    su, sd, sr, _ = orc.clear_sky_sw(c["prob"], c["sw"], c["ks"], zero_unused=False)
    equal(got, dict(lw_up=lu, lw_dn=ld, sw_up=su, sw_dn=sd, sw_dir=sr), c["use"])
    assert_paths(paths, "clear" if nmus == 1 else "nmus3")


def mlp_path_of(step):
    from rrtmgpnn._lib import check
    out = []
    for c in (step.ctx, step.ctx2 if step.ctx2 is not None else step.ctx):
        p = (ctypes.c_int * 8)()
        check(lib().rrtmgpnn_context_get_mlp_path(c.h, p), "context_get_mlp_path")
        out.append(list(p))
    return out


def test_step_mcica_clrsky_aerosols(dev, orc, case):
    """McICA (seeded) with clear-sky fluxes and aerosols: gas optics, + aerosol, the clear solve, + the sampled cloud,
    the all-sky solve (the composition of tests/test_gpu_aerosol_step.py, on the reduced grids)."""
    from rrtmgpnn import data
    from rrtmgpnn.pipeline import ClearSkyStep
    c = case
    prob, clouds, aer, kl, ks = c["prob"], c["clouds"], c["aer"], c["kl"], c["ks"]
    ncol, nlay = prob["ncol"], prob["nlay"]
    step = ClearSkyStep(prob, device=0, clouds=clouds, aerosols=aer, spectral=SPECTRAL,
                        mcica={"cloud_frac": c["cf"], "overlap_param": c["ov"], "seed": SEED, "clrsky": True})
    assert tuple(step.mask_bits_lw.shape) == (ncol, nlay, 4) and tuple(step.mask_bits_sw.shape) == (ncol, nlay, 4)
    got, paths = run_step(step)
    step.close()
    ident = lambda ng: np.stack([np.arange(1, ng + 1)] * 2, axis=1).astype(np.int32)  # noqa: E731
    out = {}
    go = orc.lw_gas_optics(prob, c["lw"], kl)
    (tau_a,) = orc.increment_bybnd(kl["band_lims_gpt"], (go["tau"],), (aer["lw_tau"],))
    emis = np.repeat(np.asarray(prob["sfc_emis"], np.float32)[:, None], 128, axis=1)
    solve = lambda t: orc.lw_solver(t, go["lay_source"], go["lev_source"], emis, go["sfc_source"], prob["top_at_1"], 1)  # noqa: E731
    out["lw_up_clr"], out["lw_dn_clr"] = solve(tau_a)
    (ct,) = orc.cloud_optics(data.load_cloud_optics("lw"), *clouds, nstr=1, lut=True, icergh=2)
    mask = MC.sampled_mask(PH.randoms(SEED, 0, 0, 128, nlay, ncol), c["cf"], c["ov"])
    (tau,) = orc.increment_bybnd(ident(128), (tau_a,), (MC.draw(mask, ct, kl["band_lims_gpt"]),))
    out["lw_up"], out["lw_dn"] = solve(tau)
    go = orc.sw_gas_optics(prob, c["sw"])
    io_a = orc.increment_bybnd(ks["band_lims_gpt"], (go["tau"], go["ssa"], go["g"]),
                               (aer["sw_tau"], aer["sw_ssa"], aer["sw_g"]))
    alb = np.repeat(np.asarray(prob["sfc_alb"], np.float32)[:, None], 112, axis=1)
    solve = lambda io: orc.sw_solver(*io, prob["mu0"], data.toa_flux(prob, ks), alb, alb, prob["top_at_1"])  # noqa: E731
    out["sw_up_clr"], out["sw_dn_clr"], out["sw_dir_clr"] = solve(io_a)
    cld = orc.delta_scale(*orc.cloud_optics(data.load_cloud_optics("sw"), *clouds, nstr=2, lut=True, icergh=2))
    mask = MC.sampled_mask(PH.randoms(SEED, 1, 0, 112, nlay, ncol), c["cf"], c["ov"])
    io = orc.increment_bybnd(ident(112), io_a, [MC.draw(mask, a, ks["band_lims_gpt"]) for a in cld])
    out["sw_up"], out["sw_dn"], out["sw_dir"] = solve(io)
    assert set(got) == set(out)
    equal(got, out, c["use"])
    assert (got["lw_dn"] != got["lw_dn_clr"]).any()
    assert_paths(paths, "mcica")


def test_step_byband(dev, orc, case):
    from oracle import gauss
    from rrtmgpnn import data
    from rrtmgpnn.pipeline import ClearSkyStep
    c = case
    prob, kl, ks = c["prob"], c["kl"], c["ks"]
    step = ClearSkyStep(prob, device=0, byband=True, spectral=SPECTRAL)
    for k in ("lw_bnd_up", "lw_bnd_dn", "sw_bnd_up", "sw_bnd_dn", "sw_bnd_dir"):
        getattr(step, k).fill_(float("nan"))
    got, paths = run_step(step)
    bnd = step.byband_fluxes()
    step.close()
    assert bnd["lw_bnd_up"].shape == (36, 61, 16) and bnd["sw_bnd_dir"].shape == (36, 61, 14)
    go = orc.lw_gas_optics(prob, c["lw"], kl)
    emis = np.repeat(np.asarray(prob["sfc_emis"], np.float32)[:, None], 128, axis=1)
    up, dn, gu, gd = orc.lw_solver(go["tau"], go["lay_source"], go["lev_source"], emis, go["sfc_source"],
                                   prob["top_at_1"], 1, gpt=True)
    w = gauss(1)[1][0]
    ll, sl = kl["band_lims_gpt"].reshape(-1, 2), ks["band_lims_gpt"].reshape(-1, 2)
    same(got["lw_up"], up, "lw_up")
    same(got["lw_dn"], dn, "lw_dn")
    same(bnd["lw_bnd_up"], R.sum_byband(R.lw_one_angle_terms(gu, w, 128), ll), "lw_bnd_up")
    same(bnd["lw_bnd_dn"], R.sum_byband(R.lw_one_angle_terms(gd, w, 128), ll), "lw_bnd_dn")
    gs = orc.sw_gas_optics(prob, c["sw"])
    alb = np.repeat(np.asarray(prob["sfc_alb"], np.float32)[:, None], 112, axis=1)
    sw = orc.sw_solver(gs["tau"], gs["ssa"], gs["g"], prob["mu0"], data.toa_flux(prob, ks), alb, alb, prob["top_at_1"],
                       gpt=True)
    use = c["use"]
    for k, y in zip(("sw_bnd_up", "sw_bnd_dn", "sw_bnd_dir"), sw[3:]):
        same(bnd[k][use], R.sum_byband(y, sl)[use], k)
    assert_paths(paths, "byband")


def test_step_upper_bc(dev, orc, case, rfmip):
    """upper_bc=True on the columns without their topmost layer: rte_lw with the one-layer boundary flux (radiance in
    flux units) as inc_flux, both from the reduced models."""
    import compute_bc_ref as B
    import step_plan_upper_bc as PU
    from rrtmgpnn.pipeline import ClearSkyStep
    c = case
    kl = c["kl"]
    prob = subset(PU.without_top(rfmip), np.arange(3, 1800, 50))
    step = ClearSkyStep(prob, device=0, upper_bc=True, spectral=SPECTRAL)
    got, paths = run_step(step)
    inc_got = step.lw_inc_flux.cpu().numpy()
    step.close()
    p1 = B.one_layer(prob, kl["press_ref_min"][0])
    g1 = orc.lw_gas_optics(p1, c["lw"], kl)
    ones = np.ones(g1["sfc_source"].shape, np.float32)
    radn = orc.lw_solver(g1["tau"], g1["lay_source"], g1["lev_source"], ones, g1["sfc_source"], True, 1, gpt=True)[3]
    inc = B.in_flux_units(np.ascontiguousarray(radn[:, 1]), 1)
    assert inc.shape == (36, 128)
    same(inc_got, inc, "lw_inc_flux")
    go = orc.lw_gas_optics(prob, c["lw"], kl)
    emis = np.repeat(np.asarray(prob["sfc_emis"], np.float32)[:, None], 128, axis=1)
    up, dn = orc.lw_solver(go["tau"], go["lay_source"], go["lev_source"], emis, go["sfc_source"], True, 1, inc_flux=inc)
    same(got["lw_up"], up, "lw_up")
    same(got["lw_dn"], dn, "lw_dn")
    assert (dn[:, 0] > 0).all()
    su, sd, sr, _ = orc.clear_sky_sw(prob, c["sw"], c["ks"], zero_unused=False)
    equal(got, dict(sw_up=su, sw_dn=sd, sw_dir=sr), prob["usecol"])
    assert_paths(paths, "upper_bc")


def test_step_single_lw_model_and_refusals(dev, orc, case):
    """lw_models of one entry: the g128 single model beside the g112 SW pair; a model that does not fit the grid and an
    unknown key are refused before anything is allocated."""
    from rrtmgpnn import data
    from rrtmgpnn.pipeline import ClearSkyStep
    c = case
    both = data.path("lw_g128_both")
    step = ClearSkyStep(c["prob"], device=0, spectral=dict(SPECTRAL, lw_models=(both,)))
    got, _ = run_step(step)
    p = mlp_path_of(step)
    step.close()
    assert p[0][0] == MFMA32 and p[0][7] & F_XIN, p
    lu, ld, _ = orc.clear_sky_lw(c["prob"], [data.load_model("lw_g128_both")], c["kl"])
    same(got["lw_up"], lu, "lw_up")
    same(got["lw_dn"], ld, "lw_dn")
    with pytest.raises(ValueError, match="outputs"):
        ClearSkyStep(c["prob"], device=0, spectral=dict(SPECTRAL, ngpt_lw=None))
    with pytest.raises(ValueError, match="unknown keys"):
        ClearSkyStep(c["prob"], device=0, spectral=dict(SPECTRAL, ngpt=128))
    with pytest.raises(ValueError, match="load_kdist"):
        ClearSkyStep(c["prob"], device=0, spectral=dict(SPECTRAL, ngpt_sw=128))


@pytest.mark.parametrize("cid", ["clear-fused", "clear-unfused", "allsky-clrsky-fused", "mcica-seeded-expran-fused",
                                 "knob-ctx"])
def test_spectral_none_plans_equal_the_goldens(dev, rfmip, cid):
    """spectral=None is today's step: the committed plans of tests/golden/step_plan.json, call for call."""
    with open(os.path.join(ROOT, "tests", "golden", "step_plan.json")) as f:
        golden = json.load(f)
    env = P.environment(rfmip)
    build = dict(P.CASES)[cid]
    got = json.loads(json.dumps(P.run_case(lambda e: dict(build(e), spectral=None), env)))
    assert got == golden[cid]


# ---- the Fortran host program ----------------------------------------------------------------------------------------
FC = os.environ.get("FC_RRTMGPNN", "/opt/rocm/lib/llvm/bin/amdflang")


@pytest.mark.skipif(not os.path.exists(FC), reason="amdflang not available")
def test_fortran_driver_with_path_overrides(tmp_path, orc, case):
    """rrtmgpnn_rfmip_clear_sky with the four netCDF models and the two reduced tables as arguments 6-11, blocked (16
    columns, ragged last block), against the oracle; "-" keeps a default (here: all six, the full-resolution run)."""
    from rrtmgpnn import data, rbin
    exe = os.path.join(ROOT, "rte-rrtmgp-nn_amd", "fortran", "build", "rrtmgpnn_rfmip_clear_sky")
    assert os.path.exists(exe), "build() makes the Fortran host programs"
    c = case
    prob, use = c["prob"], c["use"]
    fin, fout = str(tmp_path / "prob.rbin"), str(tmp_path / "flux.rbin")
    data.write_problem(prob, fin)
    over = [PATHS["lw_abs"], PATHS["lw_pfrac"], PATHS["sw_abs"], PATHS["sw_ray"],
            os.path.join(ROOT, "tests", "golden", "kdist_lw_g128.rbin"),
            os.path.join(ROOT, "tests", "golden", "kdist_sw_g112.rbin")]
    want_ = {}
    want_["lw_flux_up"], want_["lw_flux_dn"], _ = orc.clear_sky_lw(prob, c["lw"], c["kl"])
    want_["sw_flux_up"], want_["sw_flux_dn"], want_["sw_flux_dir"], _ = orc.clear_sky_sw(prob, c["sw"], c["ks"])
    full = {}
    full["lw_flux_up"], full["lw_flux_dn"], _ = orc.clear_sky_lw(
        prob, [data.load_model("lw_abs"), data.load_model("lw_pfrac")], data.load_kdist("lw"))
    for args, ref in ((over, want_), (["-"] * 6, full)):
        r = subprocess.run(["timeout", "-k", "10", "120", exe, fin, fout, data.DATA_DIR, "16", "1"] + args,
                           capture_output=True, text=True, env=dict(os.environ, OMP_NUM_THREADS="2"))
        assert r.returncode == 0, r.stdout + r.stderr
        got = rbin.read(fout)
        for k, w in ref.items():
            g = got[k]
            if k == "sw_flux_dir":
                g, w = g[use], w[use]
            np.testing.assert_array_equal(bits(g), bits(w), err_msg=k)
