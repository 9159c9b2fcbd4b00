"""LW scattering clouds under McICA: the composed route of the existing entries against the fused rescaled solve
(rrtmgpnn_lw_solver_1rescl_planck_inc).

    python tools/lw_scat_allsky_ab.py --config c4 [--rounds 9] [--iters 20] [--variant pf1=/path/lib.so ...]

The McICA step of the config with lw_scattering=True (c4: 10 000 x 60 synthetic columns; c3: the 1800 RFMIP columns,
both with the all-sky example's clouds, a cloud fraction per cloudy layer and uniform random numbers) runs once, which
leaves the gas optical depth, the Planck fraction, the two-stream band cloud properties and the packed mask in HBM.
Then, alternating in one process on one device for --rounds rounds of --iters calls each (HIP events around each batch):
  (a) the composed route: scratch copies of tau and of the Planck fraction (the increment and compute_planck_source_nn
      overwrite them), zero-filled ssa and g, rrtmgpnn_compute_planck_source_nn, rrtmgpnn_draw_samples (three g-point
      arrays from the byte mask), rrtmgpnn_increment, rrtmgpnn_expand_band_to_gpt and rrtmgpnn_lw_solver_1rescl;
  (e) the two scratch copies of (a) alone: a step's gas optics rewrites tau and the Planck fraction anyway, so a step
      would not make them and (a) - (e) is the route's own cost (the zero fills stay in: no 2str gas optics exists that
      would write ssa and g for free; the mask kernel is left out of both, (a) would have it write bytes and (b) bits);
  (b) the mask request and the new entry;
  (c) the mask request and rrtmgpnn_lw_solver_noscat_planck_inc on the same mask and the cloud's tau alone:
      (b) - (c) is what scattering costs over absorption-only clouds;
  (v) --variant name=path: (b) through another build of the library (the prefetch depths, -DRRTMGPNN_LW_SCAT_PF=n),
      loaded beside the shipped one with a context of its own on the same stream.
One line per variant: median, min and max ms; (a)'s spread (max - min) is the yardstick for (a) - (e) - (b).  The fluxes
of (a), (b) and every (v) are compared bit for bit first.  The byte-count estimate: (a) makes about 36 passes over a
(ngpt, nlay, ncol) array under a mask, (b) about 10.1 (tau and pfrac in three passes, four workspace passes, 3/32 for the
mask bits); were both bound by HBM alone, (b) would take 10.1 / 36 of (a) - (e); the tool prints the fraction of that
saving that was realised.  Last, the whole McICA step's ms per graph replay with and without lw_scattering=True.
"""
import argparse
import ctypes
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rte-rrtmgp-nn_amd"))
from rrtmgpnn import _lib, api, data  # noqa: E402
from rrtmgpnn.pipeline import ClearSkyStep  # noqa: E402

PASSES_COMPOSED, PASSES_FUSED = 36.0, 6.0 + 4.0 + 3.0 / 32.0


def problem(config):
    p = data.rfmip_columns(0, 1800) if config == "c3" else data.synthetic_problem(10000, 60, seed=20251015, col0=0)
    return p, data.allsky_clouds(p, data.load_cloud_optics("lw"))


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def report(label, config, times):
    med = statistics.median(times)
    print("%-58s %s  median %.4f ms  min %.4f  max %.4f  spread %.4f  (%d samples)"
          % (label, config, med, min(times), max(times), max(times) - min(times), len(times)), flush=True)


def unpack_bits(bits, ngpt):
    b = np.asarray(bits).view(np.uint32)
    u = (b[..., :, None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)
    return u.reshape(b.shape[:-1] + (-1,))[..., :ngpt].astype(np.uint8)


def variant_library(path):
    """Another build of the library with the signatures of the three calls (v) makes, and a context on the current
    stream."""
    h = ctypes.CDLL(path)
    for name in ("rrtmgpnn_context_create", "rrtmgpnn_solver_request_cloud_mask", "rrtmgpnn_lw_solver_1rescl_planck_inc",
                 "rrtmgpnn_last_error"):
        f = getattr(h, name)
        f.restype, f.argtypes = _lib.SIGNATURES[name]
    c = _lib.c_vp()
    assert h.rrtmgpnn_context_create(0, torch.cuda.current_stream(0).cuda_stream, c) == 0, h.rrtmgpnn_last_error()
    return h, c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c4", choices=["c3", "c4"])
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--variant", action="append", default=[], help="name=path of another build of librrtmgpnn.so")
    ap.add_argument("--no-step", action="store_true", help="skip the whole-step timings")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    L = _lib.lib()
    prob, clouds = problem(a.config)
    ncol, nlay = prob["ncol"], prob["nlay"]
    rng = np.random.default_rng(7)
    cloudy = (clouds[0] > 0) | (clouds[1] > 0)
    kl, ks = data.load_kdist("lw"), data.load_kdist("sw")
    ng, nb = kl["ngpt"], kl["nband"]
    mc = {"cloud_frac": np.where(cloudy, rng.uniform(0.1, 1.0, cloudy.shape), 0).astype(np.float32),
          "randoms_lw": rng.random((ncol, nlay, ng), dtype=np.float32),
          "randoms_sw": rng.random((ncol, nlay, ks["ngpt"]), dtype=np.float32), "overlap_param": None}
    ctx = api.context(0)  # torch's current (default) stream: the events are recorded on it
    f32 = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)  # noqa: E731
    p = lambda t: t.data_ptr()  # noqa: E731

    def chain(*steps, lib=L):
        def run():
            for fn, args in steps:
                rc = fn(*args)
                assert rc == 0, lib.rrtmgpnn_last_error()
        return run

    step = ClearSkyStep(prob, device=0, clouds=clouds, mcica=mc, lw_scattering=True, overlap=False)
    step.step()
    torch.cuda.synchronize()
    call = {n: (f, (ctx.h,) + tuple(x[1:])) for n, f, x in step.calls}
    sfn, sargs = call["lw_solver"]  # ctx, ngpt, nlay, ncol, top, nmus, Ds, W, inc, tau, tb, wb, gb, pfrac, ...
    mask_bytes = torch.as_tensor(unpack_bits(step.mask_bits_lw.cpu().numpy(), ng), device=dev)
    n = ncol * nlay * ng
    stau, slay, sssa, sg = (f32(ncol, nlay, ng) for _ in range(4))
    smp = [f32(ncol, nlay, ng) for _ in range(3)]
    lev, sfc, jac, emis = f32(ncol, nlay + 1, ng), f32(ncol, ng), f32(ncol, ng), f32(ncol, ng)
    copies = [(L.rrtmgpnn_copy_d2d, (ctx.h, p(stau), p(step.tau_lw), 4 * n)),
              (L.rrtmgpnn_copy_d2d, (ctx.h, p(slay), p(step.lay_src), 4 * n))]
    zeros = [(L.rrtmgpnn_memset_async, (ctx.h, p(sssa), 0, 4 * n)), (L.rrtmgpnn_memset_async, (ctx.h, p(sg), 0, 4 * n))]
    planck = (L.rrtmgpnn_compute_planck_source_nn,
              (ctx.h, ncol, nlay, nb, ng, kl["nPlanckTemp"], p(step.tlay), p(step.tlev), p(step.tsfc), step.sfc_lay,
               step._lims_lw, float(kl["temp_ref_min"][0]), float(kl["totplnk_delta"]), p(step.totplnk), p(sfc), p(jac),
               p(slay), p(lev)))
    draw = (L.rrtmgpnn_draw_samples, (ctx.h, ng, nlay, ncol, nb, step._lims_lw, p(mask_bytes), p(step.cld_tau_lw),
                                      p(step.cld_ssa_lw), p(step.cld_g_lw), *[p(s) for s in smp]))
    inc = (L.rrtmgpnn_increment, (ctx.h, ncol, nlay, ng, p(stau), p(sssa), p(sg), *[p(s) for s in smp]))
    expand = (L.rrtmgpnn_expand_band_to_gpt, (ctx.h, nb, ng, ncol, step._lims_lw, p(step.sfc_emis), p(emis)))
    up_a, dn_a = f32(ncol, nlay + 1), f32(ncol, nlay + 1)
    solver = (L.rrtmgpnn_lw_solver_1rescl, sargs[:9] + (p(stau), p(sssa), p(sg), p(slay), p(lev), p(emis), p(sfc), p(up_a),
                                                        p(dn_a)))
    run_a = chain(*copies, *zeros, planck, draw, inc, expand, solver)
    run_e = chain(*copies)
    run_b = chain(call["lw_mask"], (sfn, sargs))
    up_c, dn_c = f32(ncol, nlay + 1), f32(ncol, nlay + 1)
    run_c = chain(call["lw_mask"], (L.rrtmgpnn_lw_solver_noscat_planck_inc,
                                    sargs[:11] + sargs[13:-2] + (p(up_c), p(dn_c))))
    variants = []
    for spec in a.variant:
        name, path = spec.split("=", 1)
        h, c = variant_library(path)
        margs = call["lw_mask"][1]
        variants.append(("(v) %s: mask request + lw_solver_1rescl_planck_inc" % name,
                         chain((h.rrtmgpnn_solver_request_cloud_mask, (c,) + margs[1:]),
                               (h.rrtmgpnn_lw_solver_1rescl_planck_inc, (c,) + sargs[1:]), lib=h)))

    # the bits first
    def fluxes(run, outs):
        for o in outs:
            o.fill_(float("nan"))
        run()
        torch.cuda.synchronize()
        got = [o.cpu().numpy() for o in outs]
        assert not any(np.isnan(x).any() for x in got), "an output was not written"
        return [x.view(np.uint32).copy() for x in got]

    ref = fluxes(run_a, [up_a, dn_a])
    for label, run in [("(b)", run_b)] + variants:
        got = fluxes(run, [step.lw_up, step.lw_dn])
        assert all(np.array_equal(x, y) for x, y in zip(got, ref)), label + ": fluxes differ from the composed route's"
    print("bits: (a), (b)%s give the same flux_up and flux_dn" % "".join(", " + v[0].split(":")[0] for v in variants),
          flush=True)

    names = ["(a) copies + zero ssa, g + planck + draw + increment + 1rescl", "(e) the two scratch copies alone",
             "(b) mask request + lw_solver_1rescl_planck_inc", "(c) mask request + lw_solver_noscat_planck_inc"]
    todo = list(zip(names, (run_a, run_e, run_b, run_c))) + variants
    times = {label: [] for label, _ in todo}
    for _ in range(a.rounds):
        for label, run in todo:
            times[label].append(timed(run, a.iters))
    for label, _ in todo:
        report(label, a.config, times[label])
    med = {k: statistics.median(v) for k, v in times.items()}
    ta = times[names[0]]
    own = med[names[0]] - med[names[1]]
    saved = own - med[names[2]]
    print("(a) - (e) - (b) = %.4f ms against (a)'s spread %.4f ms; (a) - (e) = %.4f ms, (b) / ((a) - (e)) = %.3f; "
          "byte-count estimate %.3f (%.1f / %.0f passes): %.0f %% of the estimated saving realised; (b) - (c) = %.4f ms"
          % (saved, max(ta) - min(ta), own, med[names[2]] / own, PASSES_FUSED / PASSES_COMPOSED, PASSES_FUSED,
             PASSES_COMPOSED, 100.0 * (1.0 - med[names[2]] / own) / (1.0 - PASSES_FUSED / PASSES_COMPOSED),
             med[names[2]] - med[names[3]]), flush=True)
    step.close()
    del stau, slay, sssa, sg, smp, lev
    torch.cuda.empty_cache()
    if a.no_step:
        return

    # ---- (d) the whole step, per graph replay ----
    steps = {"with lw_scattering=True": ClearSkyStep(prob, device=0, clouds=clouds, mcica=mc, lw_scattering=True),
             "without": ClearSkyStep(prob, device=0, clouds=clouds, mcica=mc)}
    for s in steps.values():
        s.step()
        torch.cuda.synchronize()
        s.capture()
    times = {k: [] for k in steps}
    for _ in range(a.rounds):
        for k, s in steps.items():
            times[k].append(timed(s.replay, a.iters))
    for k in steps:
        report("(d) McICA step per replay, " + k, a.config, times[k])
    for s in steps.values():
        s.close()


if __name__ == "__main__":
    main()
