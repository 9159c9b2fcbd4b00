"""The LW solver alone, with and without the flux Jacobian request, against the route available without it.

    python tools/lw_jacobian_ab.py --config c3 [--rounds 9] [--iters 35] [--parent-lib PATH]

The fused step of the config (c3: the 1800 RFMIP columns, clear sky, rrtmgpnn_lw_solver_noscat_planck; c4: 10 000 x 60
synthetic columns with the all-sky example's clouds, rrtmgpnn_lw_solver_noscat_planck_inc) runs once, which leaves the LW
optical depth, the Planck fraction and the band cloud optical depth in HBM.  Then, alternating in one process on one
device for --rounds rounds of --iters calls each (HIP events around each batch):
  (a) the step's LW solver call,
  (a') the same call again (two samples of one thing: their difference is the yardstick),
  (b) rrtmgpnn_solver_request_jacobian + that call,
  (c) the route without the request: that call, then the sources materialised (a copy of the Planck fraction, which
      rrtmgpnn_compute_planck_source_nn overwrites; c4: also a copy of tau and rrtmgpnn_increment_bybnd) and a second,
      unfused rrtmgpnn_lw_solver_noscat on zeroed layer and level sources with sfc_source_Jac as the surface source,
  (p) with --parent-lib: call (a) through another build of the library (the parent commit's), on a context of its own.
One line per variant: median, min and max ms.  First the outputs are compared bit for bit: flux_up / flux_dn of (a), (b),
(c) and (p), and flux_up_Jac of (b) against (c)'s second solve.
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


def problem(config):
    if config == "c3":
        return data.rfmip_columns(0, 1800), None
    p = data.synthetic_problem(10000, 60, seed=20251015, col0=0)
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
    print("%-46s %s  median %.4f ms  min %.4f  max %.4f  spread %.4f  (%d samples)"
          % (label, config, statistics.median(times), min(times), max(times), max(times) - min(times), len(times)),
          flush=True)


def other_library(path, name):
    """`name` of another build of the library, and a context of that build on torch's current stream."""
    h = ctypes.CDLL(path)
    for n in (name, "rrtmgpnn_context_create"):
        f = getattr(h, n)
        f.restype, f.argtypes = _lib.SIGNATURES[n]
    ctx = _lib.c_vp()
    assert h.rrtmgpnn_context_create(0, torch.cuda.current_stream(0).cuda_stream, ctx) == 0
    return getattr(h, name), ctx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3", choices=["c3", "c4"])
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=35)
    ap.add_argument("--parent-lib", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    L = _lib.lib()
    prob, clouds = problem(a.config)
    step = ClearSkyStep(prob, device=0, clouds=clouds, overlap=False)
    step.step()
    torch.cuda.synchronize()
    ctx = api.context(0)  # torch's current (default) stream: the events below are recorded on it
    name, entry, lw = next((n, f, args) for n, f, args in step.calls if n == "lw_solver")
    plain = (ctx.h,) + tuple(lw[1:])
    ncol, nlay, ng, nb = step.ncol, step.nlay, step.ng_lw, step.nb_lw
    f = lambda *s: torch.zeros(s, dtype=torch.float32, device=step.dev)  # noqa: E731
    jac_b, jac_c, up_c, dn_c = f(ncol, nlay + 1), f(ncol, nlay + 1), f(ncol, nlay + 1), f(ncol, nlay + 1)
    lay, lev, sfc, sjac, tau2 = f(ncol, nlay, ng), f(ncol, nlay + 1, ng), f(ncol, ng), f(ncol, ng), f(ncol, nlay, ng)
    zlay, zlev, emis_gpt = f(ncol, nlay, ng), f(ncol, nlay + 1, ng), f(ncol, ng)
    P = lambda t: t.data_ptr()  # noqa: E731
    kd = step.kd_lw
    assert L.rrtmgpnn_expand_band_to_gpt(ctx.h, nb, ng, ncol, step._lims_lw, P(step.sfc_emis), P(emis_gpt)) == 0
    outs = [step.lw_up, step.lw_dn]

    def call_a():
        assert entry(*plain) == 0, L.rrtmgpnn_last_error()

    def call_b():
        assert L.rrtmgpnn_solver_request_jacobian(ctx.h, ng, nlay, ncol, None, P(jac_b)) == 0
        assert entry(*plain) == 0, L.rrtmgpnn_last_error()

    def call_c():
        call_a()
        lay.copy_(step.lay_src)
        assert L.rrtmgpnn_compute_planck_source_nn(
            ctx.h, ncol, nlay, nb, ng, kd["nPlanckTemp"], P(step.tlay), P(step.tlev), P(step.tsfc), step.sfc_lay,
            step._lims_lw, float(kd["temp_ref_min"][0]), float(kd["totplnk_delta"]), P(step.totplnk), P(sfc), P(sjac),
            P(lay), P(lev)) == 0
        tau = step.tau_lw
        if clouds is not None:
            tau2.copy_(step.tau_lw)
            assert L.rrtmgpnn_increment_bybnd(ctx.h, ncol, nlay, ng, nb, step._lims_lw, P(tau2), None, None,
                                              P(step.cld_tau_lw), None, None) == 0
            tau = tau2
        assert L.rrtmgpnn_lw_solver_noscat(ctx.h, ng, nlay, ncol, step.top_at_1, step.nmus, step._Ds, step._W, None,
                                           P(tau), P(zlay), P(zlev), P(emis_gpt), P(sjac), P(jac_c), P(dn_c)) == 0

    variants = [("(a) " + entry.__name__, call_a), ("(a') the same again", call_a),
                ("(b) request_jacobian + (a)", call_b), ("(c) (a) + sources + zero-source solve", call_c)]
    if a.parent_lib:
        pentry, pctx = other_library(a.parent_lib, entry.__name__)
        pargs = (pctx,) + tuple(lw[1:])

        def call_p():
            assert pentry(*pargs) == 0

        variants.append(("(p) (a) with " + os.path.basename(a.parent_lib), call_p))
    ref = None
    for label, fn in variants:
        for o in outs:
            o.fill_(float("nan"))
        fn()
        torch.cuda.synchronize()
        got = [o.cpu().numpy().view(np.uint32).copy() for o in outs]
        if ref is None:
            ref = got
        assert all(np.array_equal(x, y) for x, y in zip(got, ref)), label + ": fluxes differ"
    assert torch.equal(jac_b, jac_c) and bool((jac_b > 0).all()), "flux_up_Jac differs from the zero-source solve"
    print("bitwise: flux_up, flux_dn of every variant equal; flux_up_Jac of (b) == (c)'s second solve", flush=True)
    times = {label: [] for label, _ in variants}
    for _ in range(a.rounds):
        for label, fn in variants:
            times[label].append(timed(fn, a.iters))
    for label, _ in variants:
        report(label, a.config, times[label])
    med = {k: statistics.median(v) for k, v in times.items()}
    la, lb, lc = variants[0][0], variants[2][0], variants[3][0]
    print("%s  request's added cost %+.4f ms (%+.1f %%); route (c) adds %+.4f ms; (b) / (c) = %.3f"
          % (a.config, med[lb] - med[la], 100 * (med[lb] / med[la] - 1), med[lc] - med[la], med[lb] / med[lc]), flush=True)
    step.close()


if __name__ == "__main__":
    main()
