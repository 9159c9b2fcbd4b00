"""Clear-sky beside McICA all-sky LW fluxes: two launches against the masked dual kernel, and the step with and without
the "clrsky" key.

    python tools/mcica_clr_ab.py --config c4 [--rounds 9] [--iters 35] [--step]

The McICA step of the config with mcica={..., "clrsky": True} (c4: 10 000 x 60 synthetic columns; c3: the 1800 RFMIP
columns; the all-sky example's clouds, tools/mcica_ab.py's cloud fraction per cloudy layer, maximum-random overlap,
uniform random numbers) runs once, which leaves the LW optical depth, the Planck fraction, the band cloud optical depth
and the packed mask in HBM.  Then, alternating in one process on one device for --rounds rounds of --iters calls each
(HIP events around each batch):
  (a) rrtmgpnn_lw_solver_noscat_planck, then rrtmgpnn_solver_request_cloud_mask + rrtmgpnn_lw_solver_noscat_planck_inc,
  (b) rrtmgpnn_lw_solver_noscat_planck_clr_all_mcica in mode 1 (the masked dual kernel),
  (c) the same entry in mode 2 (the two kernels issued by the library),
  (d) rrtmgpnn_lw_solver_noscat_planck_clr_all in mode 1 (the unmasked dual kernel): (b) - (d) is what the mask costs.
One line per variant: median, min and max ms per pair of flux sets; (a)'s spread (max - min) is the yardstick for
(b)'s gain.  The four flux arrays of (a), (b) and (c) are compared bit for bit first.
--step: also the captured step's ms per replay, mcica alone and with "clrsky", alternating, and the added launches
(the clear SW solve, the LW entry) timed alone beside the McICA step's LW solve.
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
    print("%-44s %s  median %.4f ms  min %.4f  max %.4f  spread %.4f  (%d samples)"
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
    ncol, nlay = prob["ncol"], prob["nlay"]
    rng = np.random.default_rng(7)
    cloudy = (clouds[0] > 0) | (clouds[1] > 0)
    ng_lw, ng_sw = data.load_kdist("lw")["ngpt"], data.load_kdist("sw")["ngpt"]
    mc = {"cloud_frac": np.where(cloudy, rng.uniform(0.1, 1.0, cloudy.shape), 0).astype(np.float32),
          "randoms_lw": rng.random((ncol, nlay, ng_lw), dtype=np.float32),
          "randoms_sw": rng.random((ncol, nlay, ng_sw), dtype=np.float32), "overlap_param": None}
    step = ClearSkyStep(prob, device=0, clouds=clouds, mcica=dict(mc, clrsky=True), overlap=False)
    step.step()
    torch.cuda.synchronize()
    ctx = api.context(0)  # torch's current (default) stream: the events below are recorded on it
    lw = next(args for n, _, args in step.calls if n == "lw_solver")
    both = (ctx.h,) + tuple(lw[1:])
    dual = both[:-1]                             # _planck_clr_all: without the mask
    inc = both[:-3]                              # _planck_inc: without the clear outputs and the mask
    clr = inc[:10] + inc[11:-2] + both[-3:-1]    # _planck: without tau_bnd, into the clear outputs
    arm = (ctx.h, ng_lw, nlay, ncol, both[-1])
    outs = [step.lw_up, step.lw_dn, step.lw_up_clr, step.lw_dn_clr]

    def sep():
        assert L.rrtmgpnn_lw_solver_noscat_planck(*clr) == 0 and L.rrtmgpnn_solver_request_cloud_mask(*arm) == 0 \
            and L.rrtmgpnn_lw_solver_noscat_planck_inc(*inc) == 0, L.rrtmgpnn_last_error()

    def entry(fn, args, mode):
        def run():
            assert fn(*args) == 0, L.rrtmgpnn_last_error()

        def go():
            ctx.set_lw_clr_all(mode)
            run()
        return go, run

    mcica = L.rrtmgpnn_lw_solver_noscat_planck_clr_all_mcica
    variants = [("(a) _planck + armed _planck_inc", sep, sep),
                ("(b) _planck_clr_all_mcica mode 1",) + entry(mcica, both, 1),
                ("(c) _planck_clr_all_mcica mode 2",) + entry(mcica, both, 2),
                ("(d) _planck_clr_all mode 1 (no mask)",) + entry(L.rrtmgpnn_lw_solver_noscat_planck_clr_all, dual, 1)]
    ref = None
    for label, first, _ in variants[:3]:
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
    med = {k: statistics.median(v) for k, v in times.items()}
    ka, kb, kc, kd = [label for label, _, _ in variants]
    print("lw pair %s: (a) - (b) = %.4f ms (%.1f %% of (a)) against (a)'s spread %.4f ms; (c) - (a) = %.4f ms; "
          "(b) - (d) = %.4f ms" % (a.config, med[ka] - med[kb], 100 * (med[ka] - med[kb]) / med[ka],
                                   max(times[ka]) - min(times[ka]), med[kc] - med[ka], med[kb] - med[kd]), flush=True)
    ctx.set_lw_clr_all(0)
    step.close()
    if not a.step:
        return
    plain = ClearSkyStep(prob, device=0, clouds=clouds, mcica=mc)
    both_step = ClearSkyStep(prob, device=0, clouds=clouds, mcica=dict(mc, clrsky=True))
    for s in (plain, both_step):
        s.capture()
    st = {"step mcica": [], "step mcica + clrsky": []}
    for _ in range(a.rounds):
        for label, s in zip(st, (plain, both_step)):
            st[label].append(timed(s.replay, a.iters))
    for label in st:
        report(label, a.config, st[label])

    def alone(s, name, before=()):
        """One call of a step's list (after the host-only calls `before`), serialised on the stream it runs on."""
        calls = [(f, x) for n, f, x in s.calls if n in before + (name,)]

        def run():
            for f, x in calls:
                assert f(*x) == 0, L.rrtmgpnn_last_error()
        with torch.cuda.stream(s.stream_for(name)):
            return [timed(run, a.iters) for _ in range(5)]

    for name, before in (("sw_solver", ("sw_mask",)), ("sw_solver_clr", ()), ("lw_solver", ())):
        report("mcica + clrsky step's %s alone" % name, a.config, alone(both_step, name, before))
    report("mcica step's lw_solver alone", a.config, alone(plain, "lw_solver", ("lw_mask",)))
    for s in (plain, both_step):
        s.close()


if __name__ == "__main__":
    main()
