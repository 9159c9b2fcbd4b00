"""Aerosols: the materialising increment ahead of the fused all-sky solvers against the aerosol request fused into them.

    python tools/aerosol_ab.py --config c4 [--rounds 9] [--iters 35]

The McICA step of the config with aerosols (c4: 10 000 x 60 synthetic columns; c3: the 1800 RFMIP columns, both with
the all-sky example's clouds, a cloud fraction per cloudy layer, uniform random numbers and synthetic aerosol band
properties) runs once, which leaves the gas optical properties, the Planck fraction, the band cloud properties and the
packed masks in HBM.  Then, LW and SW separately, alternating in one process on one device for --rounds rounds of --iters
calls each (HIP events around each batch):
  (a) the route without the request: a scratch copy of the gas arrays (increment overwrites them; SW: also a zeroed g,
      which gas optics would otherwise have to write), rrtmgpnn_increment_bybnd by the aerosol, the mask request and the
      fused solver (SW: reading g);
  (b) rrtmgpnn_solver_request_aerosol, the mask request and the fused solver (SW: g NULL);
  (c) the mask request and the fused solver with no aerosol at all: (b) - (c) is what the aerosol costs;
  (d) LW: (a) and (b) of the clear + all-sky entry (rrtmgpnn_lw_solver_noscat_planck_clr_all_mcica);
  (e) the scratch copies of (a) alone: a step's gas optics rewrites the arrays anyway, so (a) - (e) is the route's own cost.
One line per variant: median, min and max ms; (a)'s spread (max - min) is the yardstick for (a) - (e) - (b).  The fluxes
of (a) and (b) are compared bit for bit first.  Last, the whole McICA step's ms per graph replay with and without
aerosols=.
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
from rrtmgpnn.pipeline import ClearSkyStep  # noqa: E402


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
    print("%-52s %s  median %.4f ms  min %.4f  max %.4f  spread %.4f  (%d samples)"
          % (label, config, med, min(times), max(times), max(times) - min(times), len(times)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c4", choices=["c3", "c4"])
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=35)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    L = _lib.lib()
    prob, clouds = problem(a.config)
    ncol, nlay = prob["ncol"], prob["nlay"]
    rng = np.random.default_rng(7)
    cloudy = (clouds[0] > 0) | (clouds[1] > 0)
    kl, ks = data.load_kdist("lw"), data.load_kdist("sw")
    ng_lw, ng_sw, nb_lw, nb_sw = kl["ngpt"], ks["ngpt"], kl["nband"], ks["nband"]
    mc = {"cloud_frac": np.where(cloudy, rng.uniform(0.1, 1.0, cloudy.shape), 0).astype(np.float32),
          "randoms_lw": rng.random((ncol, nlay, ng_lw), dtype=np.float32),
          "randoms_sw": rng.random((ncol, nlay, ng_sw), dtype=np.float32), "overlap_param": None}
    aer = {"lw_tau": rng.lognormal(-3, 1, (ncol, nlay, nb_lw)).astype(np.float32),
           "sw_tau": rng.lognormal(-3, 1, (ncol, nlay, nb_sw)).astype(np.float32),
           "sw_ssa": rng.uniform(0.6, 1, (ncol, nlay, nb_sw)).astype(np.float32),
           "sw_g": rng.uniform(0.3, 0.8, (ncol, nlay, nb_sw)).astype(np.float32)}
    ctx = api.context(0)  # torch's current (default) stream: the events are recorded on it
    f32 = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)  # noqa: E731
    p = lambda t: t.data_ptr()  # noqa: E731

    def chain(*steps):
        def run():
            for fn, args in steps:
                rc = fn(*args)
                assert rc == 0, L.rrtmgpnn_last_error()
        return run

    def calls_of(step):
        return {n: (f, (ctx.h,) + tuple(x[1:])) for n, f, x in step.calls}

    def compare(which, outs, runs):
        ref = None
        for run in runs:
            for o in outs:
                o.fill_(float("nan"))
            run()
            torch.cuda.synchronize()
            got = [o.cpu().numpy().view(np.uint32).copy() for o in outs]
            assert not any(np.isnan(o.cpu().numpy()).any() for o in outs), which + ": an output was not written"
            if ref is None:
                ref = got
            else:
                assert all(np.array_equal(x, y) for x, y in zip(got, ref)), which + ": the two routes' fluxes differ"

    def measure(which, variants):
        times = {label: [] for label, _ in variants}
        for _ in range(a.rounds):
            for label, run in variants:
                times[label].append(timed(run, a.iters))
        for label, _ in variants:
            report(label, a.config, times[label])
        return {label: statistics.median(t) for label, t in times.items()}, times

    step = ClearSkyStep(prob, device=0, clouds=clouds, mcica=mc, aerosols=aer, overlap=False)
    step.step()
    torch.cuda.synchronize()
    call = calls_of(step)
    dual = ClearSkyStep(prob, device=0, clouds=clouds, mcica=dict(mc, clrsky=True), aerosols=aer, overlap=False)
    dual.step()
    torch.cuda.synchronize()
    dcall = calls_of(dual)

    # ---- LW ----
    n = ncol * nlay * ng_lw
    stau = f32(ncol, nlay, ng_lw)
    copy = (L.rrtmgpnn_copy_d2d, (ctx.h, p(stau), p(step.tau_lw), 4 * n))
    inc = (L.rrtmgpnn_increment_bybnd, (ctx.h, ncol, nlay, ng_lw, nb_lw, step._lims_lw, p(stau), None, None,
                                        p(step.aer_tau_lw), None, None))
    sfn, sargs = call["lw_solver"]
    on_copy = (sfn, sargs[:9] + (p(stau),) + sargs[10:])
    lw_a = chain(copy, inc, call["lw_mask"], on_copy)
    lw_b = chain(call["lw_aerosol"], call["lw_mask"], (sfn, sargs))
    lw_c = chain(call["lw_mask"], (sfn, sargs))
    compare("lw", [step.lw_up, step.lw_dn], (lw_a, lw_b))
    dfn, dargs = dcall["lw_solver"]
    dcopy = (L.rrtmgpnn_copy_d2d, (ctx.h, p(stau), p(dual.tau_lw), 4 * n))
    dinc = (L.rrtmgpnn_increment_bybnd, (ctx.h, ncol, nlay, ng_lw, nb_lw, dual._lims_lw, p(stau), None, None,
                                         p(dual.aer_tau_lw), None, None))
    lw_da = chain(dcopy, dinc, (dfn, dargs[:9] + (p(stau),) + dargs[10:]))
    lw_db = chain(dcall["lw_aerosol"], (dfn, dargs))
    compare("lw dual", [dual.lw_up, dual.lw_dn, dual.lw_up_clr, dual.lw_dn_clr], (lw_da, lw_db))
    names = ["(a) lw copy + increment_bybnd + masked _planck_inc", "(b) lw aerosol request + masked _planck_inc",
             "(c) lw masked _planck_inc, no aerosol", "(d) lw dual: copy + increment_bybnd + _clr_all_mcica",
             "(d) lw dual: aerosol request + _clr_all_mcica", "(e) lw scratch copy alone"]
    med, times = measure("lw", list(zip(names, (lw_a, lw_b, lw_c, lw_da, lw_db, chain(copy)))))
    ta = times[names[0]]
    print("lw: (a) - (e) - (b) = %.4f ms against (a)'s spread %.4f ms; (b) - (c) = %.4f ms; dual (a) - (e) - (b) = %.4f ms"
          % (med[names[0]] - med[names[5]] - med[names[1]], max(ta) - min(ta), med[names[1]] - med[names[2]],
             med[names[3]] - med[names[5]] - med[names[4]]), flush=True)
    del stau
    torch.cuda.empty_cache()

    # ---- SW ----
    n = ncol * nlay * ng_sw
    st, sw_, sg = f32(ncol, nlay, ng_sw), f32(ncol, nlay, ng_sw), f32(ncol, nlay, ng_sw)
    copies = [(L.rrtmgpnn_copy_d2d, (ctx.h, p(st), p(step.tau_sw), 4 * n)),
              (L.rrtmgpnn_copy_d2d, (ctx.h, p(sw_), p(step.ssa_sw), 4 * n))]
    zero_g = (L.rrtmgpnn_memset_async, (ctx.h, p(sg), 0, 4 * n))
    inc = (L.rrtmgpnn_increment_bybnd, (ctx.h, ncol, nlay, ng_sw, nb_sw, step._lims_sw, p(st), p(sw_), p(sg),
                                        p(step.aer_tau_sw), p(step.aer_ssa_sw), p(step.aer_g_sw)))
    sfn, sargs = call["sw_solver"]
    on_copy = (sfn, sargs[:9] + (p(st), p(sw_), p(sg)) + sargs[12:])
    sw_a = chain(*copies, zero_g, inc, call["sw_mask"], on_copy)
    sw_b = chain(call["sw_aerosol"], call["sw_mask"], (sfn, sargs))
    sw_c = chain(call["sw_mask"], (sfn, sargs))
    compare("sw", [step.sw_up, step.sw_dn, step.sw_dir], (sw_a, sw_b))
    names = ["(a) sw copies + zero g + increment_bybnd + masked solver", "(b) sw aerosol request + masked solver, g NULL",
             "(c) sw masked solver, no aerosol", "(e) sw scratch copies alone"]
    med, times = measure("sw", list(zip(names, (sw_a, sw_b, sw_c, chain(*copies)))))
    ta = times[names[0]]
    print("sw: (a) - (e) - (b) = %.4f ms against (a)'s spread %.4f ms; (b) - (c) = %.4f ms"
          % (med[names[0]] - med[names[3]] - med[names[1]], max(ta) - min(ta), med[names[1]] - med[names[2]]), flush=True)
    step.close()
    dual.close()
    del st, sw_, sg
    torch.cuda.empty_cache()

    # ---- the whole step, per graph replay ----
    steps = {"with aerosols": ClearSkyStep(prob, device=0, clouds=clouds, mcica=mc, aerosols=aer),
             "with aerosols, fused=False": ClearSkyStep(prob, device=0, clouds=clouds, mcica=mc, aerosols=aer, fused=False),
             "without aerosols": ClearSkyStep(prob, device=0, clouds=clouds, mcica=mc)}
    for s in steps.values():
        s.step()
        torch.cuda.synchronize()
        s.capture()
    times = {k: [] for k in steps}
    for _ in range(a.rounds):
        for k, s in steps.items():
            times[k].append(timed(s.replay, a.iters))
    for k in steps:
        report("McICA step per replay, " + k, a.config, times[k])
    for s in steps.values():
        s.close()


if __name__ == "__main__":
    main()
