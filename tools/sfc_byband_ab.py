"""Surface by-band SW fluxes from the fused solver call (rrtmgpnn_solver_request_sfc_byband) against the only other route
to the same numbers, and the cost of the request in the call and in the step.

    python tools/sfc_byband_ab.py [--rounds 7] [--iters 20] [--ncols 1800,10000] [--what solver,step]

solver: at ncol x 60 layers, g224, random gas, cloud and aerosol properties and a packed McICA mask, alternating in one
process on one device for --rounds rounds of --iters calls each (HIP events around each batch):
  (a)  rrtmgpnn_sw_solver_2stream_inc with the cloud-mask, aerosol and surface by-band requests (solver family 9),
  (a') the same again (two samples of one thing: their difference is the yardstick),
  (b)  the same call without the surface by-band request (family 2): (a) - (b) is the cost of the band walk,
  (c)  the materialised route: rrtmgpnn_increment_bybnd by the aerosol, rrtmgpnn_draw_samples, rrtmgpnn_increment,
       rrtmgpnn_solver_request_byband and rrtmgpnn_sw_solver_2stream into (nbnd, nlay+1, ncol) outputs.  Its increments
       work in place, so the properties are restored before every batch, outside the timing.
Before any timing the bits are checked: (a)'s surface arrays equal the surface level of (c)'s by-band outputs, (a')
equals (a), and (a)'s broadband fluxes equal (b)'s.
step: ClearSkyStep in the host configuration -- seeded McICA, aerosols, mcica["daylit"], mcica["clrsky"] -- on a
half-night block (1800: the RFMIP columns; else synthetic), captured, with sfc_byband, a second such step, and without.
One line per variant: median, min, max and spread in ms.
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rte-rrtmgp-nn_amd"))
from rrtmgpnn import _lib, api, data  # noqa: E402
from rrtmgpnn._lib import check, int_array  # noqa: E402
from rrtmgpnn.pipeline import ClearSkyStep  # noqa: E402

SFC = ("sw_sfc_bnd_up", "sw_sfc_bnd_dn", "sw_sfc_bnd_dir")


def timed(fn, iters, before=None):
    if before:
        before()
    fn()
    torch.cuda.synchronize()
    if before:
        before()
        torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def report(label, what, times):
    print("%-44s %-28s median %.4f ms  min %.4f  max %.4f  spread %.4f  (%d samples)"
          % (label, what, statistics.median(times), min(times), max(times), max(times) - min(times), len(times)),
          flush=True)
    return statistics.median(times)


def P(t):
    return None if t is None else t.data_ptr()


def solver(ncol, rounds, iters):
    L, ctx = _lib.lib(), api.context(0)  # torch's current (default) stream: the events are recorded on it
    c, dev = ctx.h, torch.device("cuda", 0)
    kd = data.load_kdist("sw")
    ngpt, nlay, nb = kd["ngpt"], 60, kd["nband"]
    lims = int_array(np.asarray(kd["band_lims_gpt"], np.int32).ravel())
    g = torch.Generator(device=dev).manual_seed(7)
    u = lambda lo, hi, *s: torch.rand(*s, generator=g, device=dev) * (hi - lo) + lo  # noqa: E731
    tau0 = torch.exp(torch.randn(ncol, nlay, ngpt, generator=g, device=dev) * 1.5 - 2)
    ssa0 = u(0.1, 0.95, ncol, nlay, ngpt)
    tb, wb, gb = torch.exp(torch.randn(ncol, nlay, nb, generator=g, device=dev) - 1), u(0.3, 0.95, ncol, nlay, nb), \
        u(0.3, 0.9, ncol, nlay, nb)
    ta, wa, ga = torch.exp(torch.randn(ncol, nlay, nb, generator=g, device=dev) - 2), u(0.6, 1, ncol, nlay, nb), \
        u(0.3, 0.8, ncol, nlay, nb)
    mu0, toa, alb = u(0.1, 1, ncol), u(0.1, 10, ncol, ngpt), u(0, 0.9, ncol, ngpt)
    mask = torch.rand(ncol, nlay, ngpt, generator=g, device=dev) < 0.5
    nw = (ngpt + 31) // 32
    pad = torch.zeros(ncol, nlay, nw * 32, dtype=torch.int64, device=dev)
    pad[..., :ngpt] = mask
    words = (pad.view(ncol, nlay, nw, 32) << torch.arange(32, device=dev)).sum(-1)
    bits = torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32).contiguous()
    mask8 = mask.to(torch.uint8).contiguous()
    fl = [torch.zeros(ncol, nlay + 1, device=dev) for _ in range(3)]
    flb = [torch.zeros(ncol, nlay + 1, device=dev) for _ in range(3)]
    so = [torch.zeros(ncol, nb, device=dev) for _ in range(3)]
    io = [tau0.clone(), ssa0.clone(), torch.zeros_like(tau0)]
    smp = [torch.zeros_like(tau0) for _ in range(3)]
    bnd = [torch.zeros(ncol, nlay + 1, nb, device=dev) for _ in range(3)]
    bands = (nb, lims, P(tb), P(wb), P(gb))

    def fused(out, sfc):
        check(L.rrtmgpnn_solver_request_cloud_mask(c, ngpt, nlay, ncol, P(bits)), "cloud_mask")
        check(L.rrtmgpnn_solver_request_aerosol(c, nb, nlay, ncol, P(ta), P(wa), P(ga)), "aerosol")
        if sfc:
            check(L.rrtmgpnn_solver_request_sfc_byband(c, nb, lims, ncol, *[P(t) for t in so]), "sfc_byband")
        check(L.rrtmgpnn_sw_solver_2stream_inc(c, ngpt, nlay, ncol, 1, P(toa), None, P(tau0), P(ssa0), None, *bands, P(mu0),
                                               P(alb), P(alb), *[P(t) for t in out]), "sw_solver_2stream_inc")

    def restore():
        io[0].copy_(tau0)
        io[1].copy_(ssa0)
        io[2].zero_()

    def materialised():
        check(L.rrtmgpnn_increment_bybnd(c, ncol, nlay, ngpt, nb, lims, *[P(t) for t in io], P(ta), P(wa), P(ga)), "increment_bybnd")
        check(L.rrtmgpnn_draw_samples(c, ngpt, nlay, ncol, nb, lims, P(mask8), P(tb), P(wb), P(gb), *[P(t) for t in smp]),
              "draw_samples")
        check(L.rrtmgpnn_increment(c, ncol, nlay, ngpt, *[P(t) for t in io], *[P(t) for t in smp]), "increment")
        check(L.rrtmgpnn_solver_request_byband(c, nb, lims, *[P(t) for t in bnd]), "byband")
        check(L.rrtmgpnn_sw_solver_2stream(c, ngpt, nlay, ncol, 1, P(toa), None, *[P(t) for t in io], P(mu0), P(alb), P(alb),
                                           *[P(t) for t in flb]), "sw_solver_2stream")

    what = "mask + aerosol, %d x %d, g%d" % (ncol, nlay, ngpt)
    torch.cuda.synchronize()
    fused(fl, True)
    torch.cuda.synchronize()
    first = [t.clone() for t in so + fl]
    for t in so:
        t.fill_(float("nan"))
    fused(fl, True)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, so + fl)), "(a') differs from (a)"
    fused(flb, False)
    restore()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first[3:], flb)), "(a)'s broadband fluxes differ from (b)'s"
    materialised()
    torch.cuda.synchronize()
    for a, b, k in zip(so, bnd, ("up", "dn", "dir")):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b[:, nlay]), "sfc_bnd_%s differs from the by-band route" % k
    print("%s: bits: (a) == the surface level of (c)'s by-band fluxes, (a') == (a), (a) == (b) broadband" % what, flush=True)
    variants = {"(a) fused call, surface by-band request": (lambda: fused(fl, True), None),
                "(a') the same again": (lambda: fused(fl, True), None),
                "(b) fused call without the request": (lambda: fused(fl, False), None),
                "(c) materialised route, by-band solver": (materialised, restore)}
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, (fn, before) in variants.items():
            times[k].append(timed(fn, iters, before))
    ma, ma2, mb, mc = (report(k, what, times[k]) for k in variants)
    spread = max(max(t) - min(t) for t in times.values())
    print("%s  (c) / (a) = %.2f  ((c) - (a) = %.4f ms); (a) - (b) = %+.4f ms (%+.1f %%); |(a) - (a')| = %.4f ms; the "
          "largest spread of a variant's samples %.4f ms" % (what, mc / ma, mc - ma, ma - mb, 100 * (ma / mb - 1),
                                                          abs(ma - ma2), spread), flush=True)


def step(ncol, rounds, iters):
    kl, ks = data.load_kdist("lw"), data.load_kdist("sw")
    prob = data.rfmip_columns(0, 1800) if ncol == 1800 else data.synthetic_problem(ncol, 60, seed=20251015, col0=0)
    nlay = prob["nlay"]
    use = torch.as_tensor(np.asarray(prob["usecol"]), device="cuda")
    night = 1.0 - float(prob["usecol"].mean())
    clouds = data.allsky_clouds(prob, data.load_cloud_optics("lw"))
    cloudy = (clouds[0] > 0) | (clouds[1] > 0)
    rng = np.random.default_rng(51)
    cf = np.where(cloudy, rng.uniform(0.2, 0.9, cloudy.shape), 0).astype(np.float32)
    ov = rng.uniform(-1, 1, (ncol, nlay - 1)).astype(np.float32)
    rng = np.random.default_rng(98)
    aer = {"lw_tau": rng.lognormal(-2, 1, (ncol, nlay, kl["nband"])).astype(np.float32),
           "sw_tau": rng.lognormal(-2, 1, (ncol, nlay, ks["nband"])).astype(np.float32),
           "sw_ssa": rng.uniform(0.6, 1, (ncol, nlay, ks["nband"])).astype(np.float32),
           "sw_g": rng.uniform(0.3, 0.8, (ncol, nlay, ks["nband"])).astype(np.float32)}

    def build(sfc):
        mc = {"cloud_frac": cf, "overlap_param": ov, "seed": 2026, "clrsky": True, "daylit": True}
        kw = {"sfc_byband": True} if sfc else {}
        return ClearSkyStep(prob, device=0, clouds=clouds, mcica=mc, aerosols=aer, **kw)

    what = "host configuration, %d" % ncol
    steps = {"(a) sfc_byband=True": build(True), "(a') a second such step": build(True), "(b) without sfc_byband": build(False)}
    sa, sa2, sb = steps.values()
    for st in steps.values():
        st.capture()
        st.replay()
    torch.cuda.synchronize()
    for k in ("sw_up", "sw_dn", "sw_dir", "lw_up", "lw_dn", "sw_up_clr", "sw_dn_clr", "sw_dir_clr"):
        assert torch.equal(getattr(sa, k), getattr(sb, k)) and torch.equal(getattr(sa, k), getattr(sa2, k)), k
    for k in SFC:
        t = getattr(sa, k)
        assert torch.equal(t, getattr(sa2, k)) and not bool(t[~use].any()) and bool((t[use] > 0).any()), k
    print("%s: %.1f %% of the columns at night; bits: the broadband fluxes of (a), (a') and (b) are equal, the surface "
          "arrays of (a) and (a') equal and 0 at night" % (what, 100 * night), flush=True)
    times = {label: [] for label in steps}
    for _ in range(rounds):
        for label, st in steps.items():
            times[label].append(timed(st.replay, iters))
    ma, ma2, mb = (report(label, what, times[label]) for label in steps)
    spread = max(max(t) - min(t) for t in times.values())
    print("%s  (a) - (b) = %+.4f ms (%+.1f %% of the step); |(a) - (a')| = %.4f ms; the largest spread of a variant's "
          "samples %.4f ms" % (what, ma - mb, 100 * (ma / mb - 1), abs(ma - ma2), spread), flush=True)
    for st in steps.values():
        st.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--ncols", default="1800,10000")
    ap.add_argument("--what", default="solver,step")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    for ncol in [int(n) for n in a.ncols.split(",") if n]:
        for w in a.what.split(","):
            {"solver": solver, "step": step}[w](ncol, a.rounds, a.iters)


if __name__ == "__main__":
    main()
