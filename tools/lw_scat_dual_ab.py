"""Clear-sky beside all-sky LW fluxes for scattering clouds under McICA, with and without aerosols: the dual kernel
against the two launches of rrtmgpnn_lw_solver_1rescl_planck_clr_all, and the entry against the materialising sequence.

    python tools/lw_scat_dual_ab.py --config c4 [--rounds 9] [--iters 20]

As tools/lw_scat_allsky_ab.py: the McICA step of the config with lw_scattering=True (c4: 10 000 x 60 synthetic columns;
c3: the 1800 RFMIP columns) runs once, which leaves the gas optical depth, the Planck fraction, the two-stream band cloud
properties and the packed mask in HBM; the aerosol is a 1scl band set, lognormal(-1, 1).  Then, alternating in one
process on one device for --rounds rounds of --iters calls each (HIP events around each batch):
  (1) / (2)   the mask request and the entry in mode 1 (the dual kernel) / mode 2 (the two launches), no aerosol;
  (1a) / (2a) the same with the aerosol request armed;
  (a) the materialising sequence with the aerosol: scratch copies of tau and of the Planck fraction, zero-filled ssa and
      g, rrtmgpnn_compute_planck_source_nn, rrtmgpnn_increment_bybnd by the aerosol, rrtmgpnn_expand_band_to_gpt, the
      rescaled solve (clear), rrtmgpnn_draw_samples, rrtmgpnn_increment, the rescaled solve again (all-sky);
  (e) the two scratch copies of (a) alone: (a) - (e) is the sequence's own cost.
One line per variant: median, min and max ms.  The four flux arrays of (1), (2) and of (1a), (2a), (a) are compared bit
for bit first.  Mode 1 decides mode 0 where it beats mode 2 by more than the two samples' spreads; the entry is the class
layers' aerosol route where (a) - (e) - (2a or 1a) exceeds (a)'s spread.
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rte-rrtmgp-nn_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from rrtmgpnn import _lib, api, data  # noqa: E402
from rrtmgpnn.pipeline import ClearSkyStep  # noqa: E402
from lw_scat_allsky_ab import problem, report, timed, unpack_bits  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c4", choices=["c3", "c4"])
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
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
    ctx = api.context(0)
    f32 = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)  # noqa: E731
    p = lambda t: t.data_ptr()  # noqa: E731

    def chain(*steps):
        def run():
            for fn, args in steps:
                rc = fn(*args)
                assert rc == 0, L.rrtmgpnn_last_error()
        return run

    step = ClearSkyStep(prob, device=0, clouds=clouds, mcica=mc, lw_scattering=True, overlap=False)
    step.step()
    torch.cuda.synchronize()
    call = {n: (f, (ctx.h,) + tuple(x[1:])) for n, f, x in step.calls}
    _, sargs = call["lw_solver"]  # ctx, ngpt, nlay, ncol, top, nmus, Ds, W, inc, tau, tb, wb, gb, pfrac, ..., up, dn
    aer = torch.as_tensor(rng.lognormal(-1, 1, (ncol, nlay, nb)).astype(np.float32), device=dev)
    outs = [f32(ncol, nlay + 1) for _ in range(4)]
    entry = (L.rrtmgpnn_lw_solver_1rescl_planck_clr_all, sargs[:-2] + tuple(p(o) for o in outs))
    arm_aer = (L.rrtmgpnn_solver_request_aerosol, (ctx.h, nb, nlay, ncol, p(aer), None, None))

    def mode(m):
        return (L.rrtmgpnn_context_set_lw_scat_clr_all, (ctx.h, m))

    runs = {"(1) mask request + entry, mode 1 (dual kernel)": chain(mode(1), call["lw_mask"], entry),
            "(2) mask request + entry, mode 2 (two launches)": chain(mode(2), call["lw_mask"], entry),
            "(1a) mask + aerosol requests + entry, mode 1": chain(mode(1), call["lw_mask"], arm_aer, entry),
            "(2a) mask + aerosol requests + entry, mode 2": chain(mode(2), call["lw_mask"], arm_aer, entry)}

    # (a) the materialising sequence with the aerosol
    mask_bytes = torch.as_tensor(unpack_bits(step.mask_bits_lw.cpu().numpy(), ng), device=dev)
    n = ncol * nlay * ng
    stau, slay, sssa, sg = (f32(ncol, nlay, ng) for _ in range(4))
    smp = [f32(ncol, nlay, ng) for _ in range(3)]
    lev, sfc, jac, emis = f32(ncol, nlay + 1, ng), f32(ncol, ng), f32(ncol, ng), f32(ncol, ng)
    outs_a = [f32(ncol, nlay + 1) for _ in range(4)]
    copies = [(L.rrtmgpnn_copy_d2d, (ctx.h, p(stau), p(step.tau_lw), 4 * n)),
              (L.rrtmgpnn_copy_d2d, (ctx.h, p(slay), p(step.lay_src), 4 * n))]
    zeros = [(L.rrtmgpnn_memset_async, (ctx.h, p(sssa), 0, 4 * n)), (L.rrtmgpnn_memset_async, (ctx.h, p(sg), 0, 4 * n))]
    planck = (L.rrtmgpnn_compute_planck_source_nn,
              (ctx.h, ncol, nlay, nb, ng, kl["nPlanckTemp"], p(step.tlay), p(step.tlev), p(step.tsfc), step.sfc_lay,
               step._lims_lw, float(kl["temp_ref_min"][0]), float(kl["totplnk_delta"]), p(step.totplnk), p(sfc), p(jac),
               p(slay), p(lev)))
    inc_aer = (L.rrtmgpnn_increment_bybnd, (ctx.h, ncol, nlay, ng, nb, step._lims_lw, p(stau), p(sssa), p(sg), p(aer),
                                            None, None))
    draw = (L.rrtmgpnn_draw_samples, (ctx.h, ng, nlay, ncol, nb, step._lims_lw, p(mask_bytes), p(step.cld_tau_lw),
                                      p(step.cld_ssa_lw), p(step.cld_g_lw), *[p(s) for s in smp]))
    inc = (L.rrtmgpnn_increment, (ctx.h, ncol, nlay, ng, p(stau), p(sssa), p(sg), *[p(s) for s in smp]))
    expand = (L.rrtmgpnn_expand_band_to_gpt, (ctx.h, nb, ng, ncol, step._lims_lw, p(step.sfc_emis), p(emis)))

    def solve(up, dn):
        return (L.rrtmgpnn_lw_solver_1rescl, sargs[:9] + (p(stau), p(sssa), p(sg), p(slay), p(lev), p(emis), p(sfc), p(up),
                                                          p(dn)))

    run_a = chain(*copies, *zeros, planck, inc_aer, expand, solve(outs_a[2], outs_a[3]), draw, inc,
                  solve(outs_a[0], outs_a[1]))
    run_e = chain(*copies)

    def fluxes(run, o):
        for t in o:
            t.fill_(float("nan"))
        run()
        torch.cuda.synchronize()
        got = [t.cpu().numpy() for t in o]
        assert not any(np.isnan(x).any() for x in got), "an output was not written"
        return [x.view(np.uint32).copy() for x in got]

    names = list(runs)
    got = {k: fluxes(runs[k], outs) for k in names}
    ref = fluxes(run_a, outs_a)
    same = lambda x, y: all(np.array_equal(u, v) for u, v in zip(x, y))  # noqa: E731
    assert same(got[names[0]], got[names[1]]), "modes 1 and 2 differ without the aerosol"
    assert same(got[names[2]], got[names[3]]), "modes 1 and 2 differ with the aerosol"
    assert same(got[names[2]], ref), "the entry's fluxes differ from the materialising sequence's"
    assert not same(got[names[0]], got[names[2]]), "the aerosol does not show"
    print("bits: (1) = (2); (1a) = (2a) = (a), four flux arrays each", flush=True)

    na, ne = "(a) the materialising sequence with the aerosol", "(e) the two scratch copies alone"
    todo = [(k, runs[k]) for k in names] + [(na, run_a), (ne, run_e)]
    times = {label: [] for label, _ in todo}
    for _ in range(a.rounds):
        for label, run in todo:
            times[label].append(timed(run, a.iters))
    for label, _ in todo:
        report(label, a.config, times[label])
    med = {k: statistics.median(v) for k, v in times.items()}
    spread = {k: max(v) - min(v) for k, v in times.items()}
    for one, two in ((names[0], names[1]), (names[2], names[3])):
        print("%s - %s = %.4f ms (%.1f %% of mode 2) against the spreads %.4f and %.4f ms"
              % (two.split()[0], one.split()[0], med[two] - med[one], 100.0 * (med[two] - med[one]) / med[two],
                 spread[one], spread[two]), flush=True)
    own = med[na] - med[ne]
    best = min(med[names[2]], med[names[3]])
    print("(a) - (e) = %.4f ms; (a) - (e) - entry = %.4f ms against (a)'s spread %.4f ms; entry / ((a) - (e)) = %.3f"
          % (own, own - best, spread[na], best / own), flush=True)
    L.rrtmgpnn_context_set_lw_scat_clr_all(ctx.h, 0)
    step.close()


if __name__ == "__main__":
    main()
