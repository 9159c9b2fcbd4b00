"""By-band fluxes under McICA-sampled clouds: the class layer's route through g-point cloud arrays against the paired
request of the fused solvers (rrtmgpnn_solver_request_byband_mcica).

    python tools/mcica_byband_ab.py --config c4 [--rounds 9] [--iters 35] [--overlap max_ran|exp_ran]

The McICA by-band step of the config (c4: 10 000 x 60 synthetic columns; c3: the 1800 RFMIP columns, both with the
all-sky example's clouds, a cloud fraction per cloudy layer and uniform random numbers) runs once, which leaves the gas
optical properties, the Planck fraction, the band cloud properties and both forms of the masks in HBM.  Then, LW and SW
separately, each solver alone, alternating in one process on one device for --rounds rounds of --iters calls each (HIP
events around each batch):
  (a)  the unfused route with by-band outputs: a scratch copy of the gas arrays (increment overwrites them; SW: also a
       zeroed g), rrtmgpnn_draw_samples, rrtmgpnn_increment at g-point resolution, rrtmgpnn_solver_request_byband and
       the plain solver;
  (a0) (a)'s scratch copies alone, which a host that may overwrite its gas arrays does not pay;
  (b)  the paired request and the fused solver;
  (c)  rrtmgpnn_solver_request_cloud_mask and the fused solver, without by-band outputs: (b) - (c) is what the by-band
       outputs cost under a mask;
  (d)  rrtmgpnn_solver_request_byband and the unmasked fused solver: (b) - (d) is what the mask costs beside them.
The mask kernels are not timed (tools/mcica_ab.py measures them).  One line per variant: median, min and max ms; (a)'s
spread (max - min) is the yardstick for (a) - (b).  The broadband and by-band fluxes of (a) and (b) are compared bit for
bit first.
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
    ap.add_argument("--overlap", default="max_ran", choices=["max_ran", "exp_ran"])
    a = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    L = _lib.lib()
    prob, clouds = problem(a.config)
    ncol, nlay = prob["ncol"], prob["nlay"]
    rng = np.random.default_rng(7)
    cloudy = (clouds[0] > 0) | (clouds[1] > 0)
    ng_lw, ng_sw = data.load_kdist("lw")["ngpt"], data.load_kdist("sw")["ngpt"]
    mc = {"cloud_frac": np.where(cloudy, rng.uniform(0.1, 1.0, cloudy.shape), 0).astype(np.float32),
          "randoms_lw": rng.random((ncol, nlay, ng_lw), dtype=np.float32),
          "randoms_sw": rng.random((ncol, nlay, ng_sw), dtype=np.float32),
          "overlap_param": rng.uniform(-1, 1, (ncol, nlay - 1)).astype(np.float32) if a.overlap == "exp_ran" else None,
          "byband": True}
    step = ClearSkyStep(prob, device=0, clouds=clouds, mcica=mc, overlap=False)
    step.step()
    torch.cuda.synchronize()
    ctx = api.context(0)  # torch's current (default) stream: the events are recorded on it
    call = {n: (f, (ctx.h,) + tuple(x[1:])) for n, f, x in step.calls}
    f32 = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)  # noqa: E731
    p = lambda t: t.data_ptr()  # noqa: E731

    def chain(*steps):
        def run():
            for fn, args in steps:
                rc = fn(*args)
                assert rc == 0, L.rrtmgpnn_last_error()
        return run

    for which, ng in (("lw", ng_lw), ("sw", ng_sw)):
        mask_fn, mask_args = call["mcica_mask_" + which]  # (..., cloud_mask = None, mask_bits)
        solver_fn, solver_args = call[which + "_solver"]
        pair_fn, pair_args = call[which + "_mask_byband"]
        byband = (L.rrtmgpnn_solver_request_byband, pair_args[:6])
        mask_rq = (L.rrtmgpnn_solver_request_cloud_mask, (ctx.h,) + pair_args[6:])
        outs = [step.lw_up, step.lw_dn, step.lw_bnd_up, step.lw_bnd_dn] if which == "lw" else \
            [step.sw_up, step.sw_dn, step.sw_dir, step.sw_bnd_up, step.sw_bnd_dn, step.sw_bnd_dir]
        n = ncol * nlay * ng
        mbytes = torch.empty((ncol, nlay, ng), dtype=torch.uint8, device=dev)
        chain((mask_fn, mask_args[:-2] + (p(mbytes), None)))()  # the same mask as bytes, for draw_samples
        if which == "lw":
            stau, smp = f32(ncol, nlay, ng), f32(ncol, nlay, ng)
            copies = [(L.rrtmgpnn_copy_d2d, (ctx.h, p(stau), p(step.tau_lw), 4 * n))]
            unfused = chain(
                *copies,
                (L.rrtmgpnn_draw_samples, (ctx.h, ng, nlay, ncol, step.nb_lw, step._lims_lw, p(mbytes),
                                           p(step.cld_tau_lw), None, None, p(smp), None, None)),
                (L.rrtmgpnn_increment, (ctx.h, ncol, nlay, ng, p(stau), None, None, p(smp), None, None)),
                byband,
                (L.rrtmgpnn_lw_solver_noscat_planck, solver_args[:9] + (p(stau),) + solver_args[11:]))
        else:
            st, sw_, sg = f32(ncol, nlay, ng), f32(ncol, nlay, ng), f32(ncol, nlay, ng)
            smp = [f32(ncol, nlay, ng) for _ in range(3)]
            copies = [(L.rrtmgpnn_copy_d2d, (ctx.h, p(st), p(step.tau_sw), 4 * n)),
                      (L.rrtmgpnn_copy_d2d, (ctx.h, p(sw_), p(step.ssa_sw), 4 * n)),
                      (L.rrtmgpnn_memset_async, (ctx.h, p(sg), 0, 4 * n))]
            unfused = chain(
                *copies,
                (L.rrtmgpnn_draw_samples, (ctx.h, ng, nlay, ncol, step.nb_sw, step._lims_sw, p(mbytes),
                                           p(step.cld_tau_sw), p(step.cld_ssa_sw), p(step.cld_g_sw),
                                           *[p(x) for x in smp])),
                (L.rrtmgpnn_increment, (ctx.h, ncol, nlay, ng, p(st), p(sw_), p(sg), *[p(x) for x in smp])),
                byband,
                (L.rrtmgpnn_sw_solver_2stream_rfmip, solver_args[:9] + (p(st), p(sw_), p(sg), 0, None, None, None, None)
                 + solver_args[17:]))
        paired = chain((pair_fn, pair_args), (solver_fn, solver_args))
        masked = chain(mask_rq, (solver_fn, solver_args))
        unmasked = chain(byband, (solver_fn, solver_args))
        ref = None
        for label, run in (("(a)", unfused), ("(b)", paired)):
            for o in outs:
                o.fill_(float("nan"))
            run()
            torch.cuda.synchronize()
            got = [o.cpu().numpy().view(np.uint32).copy() for o in outs]
            if ref is None:
                ref = got
            else:
                assert all(np.array_equal(x, y) for x, y in zip(got, ref)), which + ": fused and unfused fluxes differ"
        print("%s: broadband and by-band fluxes of (a) and (b) are bitwise equal" % which, flush=True)
        variants = [("(a) %s unfused: copy+draw+inc+byband request+solver" % which, unfused),
                    ("(a0) %s the scratch copies of (a) alone" % which, chain(*copies)),
                    ("(b) %s paired request + fused solver" % which, paired),
                    ("(c) %s mask request + fused solver, no by-band" % which, masked),
                    ("(d) %s by-band request + unmasked fused solver" % which, unmasked)]
        times = {label: [] for label, _ in variants}
        for _ in range(a.rounds):
            for label, run in variants:
                times[label].append(timed(run, a.iters))
        for label, _ in variants:
            report(label, a.config + " " + a.overlap, times[label])
        med = {label[:4].strip(): statistics.median(times[label]) for label, _ in variants}
        ta = times[variants[0][0]]
        print("%s: (a) - (b) = %.4f ms ((a) - (a0) - (b) = %.4f) against (a)'s spread %.4f ms; (b) - (c) = %.4f ms; "
              "(b) - (d) = %.4f ms; (a) / (b) = %.2f"
              % (which, med["(a)"] - med["(b)"], med["(a)"] - med["(a0)"] - med["(b)"], max(ta) - min(ta),
                 med["(b)"] - med["(c)"], med["(b)"] - med["(d)"], med["(a)"] / med["(b)"]), flush=True)
        del unfused, paired, smp
        torch.cuda.empty_cache()
    step.close()


if __name__ == "__main__":
    main()
