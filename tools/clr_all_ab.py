"""Clear-sky + all-sky LW fluxes: two launches against the dual kernel, and the step with and without clrsky.

    python tools/clr_all_ab.py --config c4 [--rounds 9] [--iters 35] [--step]

The all-sky step of the config (c4: 10 000 x 60 synthetic columns; c3: the 1800 RFMIP columns, both with the all-sky
example's clouds) runs once, which leaves the LW optical depth, the Planck fraction and the band cloud optical depth
in HBM.  Then, alternating in one process on one device for --rounds rounds of --iters calls each (HIP events around
each batch):
  (a) rrtmgpnn_lw_solver_noscat_planck followed by rrtmgpnn_lw_solver_noscat_planck_inc,
  (b) rrtmgpnn_lw_solver_noscat_planck_clr_all in mode 1 (the dual kernel),
  (c) the same entry in mode 2 (the two kernels issued by the library).
One line per variant: median, min and max ms per pair of flux sets; (a)'s spread (max - min) is the yardstick for
(b)'s gain.  The four flux arrays are compared bit for bit first.
--step: also the captured step's ms per replay, all-sky alone and with clrsky=True, alternating, and the clear SW
solver launch timed alone.
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
    print("%-34s %s  median %.4f ms  min %.4f  max %.4f  spread %.4f  (%d samples)"
          % (label, config, statistics.median(times), min(times), max(times), max(times) - min(times), len(times)),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c4", choices=["c3", "c4"])
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=35)
    ap.add_argument("--step", action="store_true")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    L = _lib.lib()
    prob, clouds = problem(a.config)
    step = ClearSkyStep(prob, device=0, clouds=clouds, clrsky=True, overlap=False)
    step.step()
    torch.cuda.synchronize()
    ctx = api.context(0)  # torch's current (default) stream: the events below are recorded on it
    lw = next(args for n, _, args in step.calls if n == "lw_solver")
    both = (ctx.h,) + tuple(lw[1:])
    inc = both[:-2]                      # _planck_inc: without the clear outputs
    clr = inc[:10] + inc[11:-2] + both[-2:]  # _planck: without tau_bnd, into the clear outputs
    outs = [step.lw_up, step.lw_dn, step.lw_up_clr, step.lw_dn_clr]

    def sep():
        assert L.rrtmgpnn_lw_solver_noscat_planck(*clr) == 0 and L.rrtmgpnn_lw_solver_noscat_planck_inc(*inc) == 0

    def entry(mode):
        def run():
            assert L.rrtmgpnn_lw_solver_noscat_planck_clr_all(*both) == 0, L.rrtmgpnn_last_error()
        def go():
            ctx.set_lw_clr_all(mode)
            run()
        return go, run

    variants = [("(a) _planck + _planck_inc", sep, sep)] + [
        ("(%s) _planck_clr_all mode %d" % (t, m),) + entry(m) for t, m in (("b", 1), ("c", 2))]
    ref = None
    for label, first, _ in variants:
        for o in outs:
            o.fill_(float("nan"))
        first()
        torch.cuda.synchronize()
        got = [o.cpu().numpy().view(np.uint32).copy() for o in outs]
        if ref is None:
            ref = got
        else:
            assert all(np.array_equal(x, y) for x, y in zip(got, ref)), label + ": fluxes differ"
    times = {label: [] for label, _, _ in variants}
    for _ in range(a.rounds):
        for label, first, run in variants:
            first()
            times[label].append(timed(run, a.iters))
    for label, _, _ in variants:
        report(label, a.config, times[label])
    ctx.set_lw_clr_all(0)
    if not a.step:
        return
    plain = ClearSkyStep(prob, device=0, clouds=clouds)
    both_step = ClearSkyStep(prob, device=0, clouds=clouds, clrsky=True)
    for s in (plain, both_step):
        s.capture()
    st = {"step all-sky": [], "step all-sky + clrsky": []}
    for _ in range(a.rounds):
        for label, s in zip(st, (plain, both_step)):
            st[label].append(timed(s.replay, a.iters))
    for label in st:
        report(label, a.config, st[label])
    # the SW solver launches of the clrsky step alone, serialised on its SW stream
    for name in ("sw_solver", "sw_solver_clr", "lw_solver"):
        fn, args = next((f, x) for n, f, x in both_step.calls if n == name)
        s = both_step.stream_for(name)
        with torch.cuda.stream(s):
            ts = [timed(lambda: fn(*args), a.iters) for _ in range(5)]
        report("clrsky step's %s alone" % name, a.config, ts)
    fn, args = next((f, x) for n, f, x in plain.calls if n == "lw_solver")
    with torch.cuda.stream(plain.stream_for("lw_solver")):
        ts = [timed(lambda: fn(*args), a.iters) for _ in range(5)]
    report("all-sky step's lw_solver alone", a.config, ts)


if __name__ == "__main__":
    main()
