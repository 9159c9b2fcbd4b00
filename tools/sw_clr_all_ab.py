"""Clear-sky + all-sky SW fluxes: two launches against the dual kernel, and the step with and without sw_dual.

    python tools/sw_clr_all_ab.py --config c4 [--variant plain|mask|mask_aer] [--rounds 9] [--iters 35] [--step]

A step of the config with clear-sky outputs and sw_dual=True (c4: 10 000 x 60 synthetic columns; c3: the 1800 RFMIP
columns, both with the all-sky example's clouds; mask: seeded McICA; mask_aer: and seeded band aerosols) runs once,
which leaves the SW gas properties, the delta-scaled band clouds, the mask bits and the aerosol in HBM.  Then the SW
solver alone, alternating in one process on one device for --rounds rounds of --iters calls each (HIP events around each
batch), every variant arming the step's own mask and aerosol requests ahead of its all-sky call:
  (a) the two-launch route a step without sw_dual issues: rrtmgpnn_sw_solver_2stream_rfmip with the cloud increment,
      then without (with aerosols: the aerosol as its increment),
  (b) rrtmgpnn_sw_solver_2stream_rfmip_clr_all in mode 1 (the dual kernel),
  (c) the same entry in mode 2 (the two launches issued by the library).
One line per variant: median, min and max ms per pair of flux sets; (a)'s spread (max - min) is the yardstick for
(b)'s gain.  The six flux arrays are compared bit for bit first.
--step (plain only): also the captured step's ms per replay with clrsky=True, without and with sw_dual (the context in
mode 1), alternating.
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


def options(prob, clouds, variant):
    """ClearSkyStep keywords of the variant: clear-sky outputs beside overcast or McICA-sampled clouds, aerosols."""
    if variant == "plain":
        return {"clrsky": True}
    ncol, nlay = prob["ncol"], prob["nlay"]
    rng = np.random.default_rng(17)
    cloudy = (clouds[0] > 0) | (clouds[1] > 0)
    kw = {"mcica": {"cloud_frac": np.where(cloudy, rng.uniform(0.1, 1.0, cloudy.shape), 0).astype(np.float32),
                    "seed": 20261020, "clrsky": True}}
    if variant == "mask_aer":
        nb_lw, nb_sw = data.load_kdist("lw")["nband"], data.load_kdist("sw")["nband"]
        kw["aerosols"] = {"lw_tau": rng.lognormal(-2, 1, (ncol, nlay, nb_lw)).astype(np.float32),
                          "sw_tau": rng.lognormal(-2, 1, (ncol, nlay, nb_sw)).astype(np.float32),
                          "sw_ssa": rng.uniform(0.6, 1, (ncol, nlay, nb_sw)).astype(np.float32),
                          "sw_g": rng.uniform(0.3, 0.8, (ncol, nlay, nb_sw)).astype(np.float32)}
    return kw


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
    ap.add_argument("--variant", default="plain", choices=["plain", "mask", "mask_aer"])
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=35)
    ap.add_argument("--step", action="store_true")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    L = _lib.lib()
    prob, clouds = problem(a.config)
    kw = options(prob, clouds, a.variant)
    step = ClearSkyStep(prob, device=0, clouds=clouds, overlap=False, sw_dual=True, **kw)
    step.step()
    torch.cuda.synchronize()
    ctx = api.context(0)  # torch's current (default) stream: the events below are recorded on it
    calls = {n: (f, x) for n, f, x in step.calls}
    requests = [(f, (ctx.h,) + tuple(x[1:])) for n, (f, x) in calls.items() if n in ("sw_mask", "sw_aerosol")]
    both = (ctx.h,) + tuple(calls["sw_solver"][1][1:])
    allsky = both[:-3]
    # the clear launch: no increment, or the aerosol's band arrays as its increment; into the clear outputs
    aer = [x for n, (f, x) in calls.items() if n == "sw_aerosol"]
    inc = both[12:14] + tuple(aer[0][-3:]) if aer else (0, None, None, None, None)
    clear = both[:12] + inc + both[17:20] + both[-3:]
    outs = [step.sw_up, step.sw_dn, step.sw_dir, step.sw_up_clr, step.sw_dn_clr, step.sw_dir_clr]
    label_v = "" if a.variant == "plain" else " [%s]" % a.variant

    def arm():
        for f, x in requests:
            assert f(*x) == 0, L.rrtmgpnn_last_error()

    def sep():
        arm()
        assert L.rrtmgpnn_sw_solver_2stream_rfmip(*allsky) == 0, L.rrtmgpnn_last_error()
        assert L.rrtmgpnn_sw_solver_2stream_rfmip(*clear) == 0, L.rrtmgpnn_last_error()

    def entry(mode):
        def run():
            arm()
            assert L.rrtmgpnn_sw_solver_2stream_rfmip_clr_all(*both) == 0, L.rrtmgpnn_last_error()
        def go():
            ctx.set_sw_clr_all(mode)
            run()
        return go, run

    variants = [("(a) _rfmip + _rfmip" + label_v, sep, sep)] + [
        ("(%s) _rfmip_clr_all mode %d%s" % (t, m, label_v),) + entry(m) for t, m in (("b", 1), ("c", 2))]
    ref = None
    for label, first, _ in variants:
        for o in outs:
            o.fill_(float("nan"))
        first()
        torch.cuda.synchronize()
        got = [o.cpu().numpy().view(np.uint32).copy() for o in outs]
        assert not any(np.isnan(g.view(np.float32)).any() for g in got), label + ": an output was not written"
        if ref is None:
            ref = got
        else:
            assert all(np.array_equal(x, y) for x, y in zip(got, ref)), label + ": fluxes differ"
    print("six flux arrays bitwise equal across (a), (b), (c)%s %s" % (label_v, a.config), flush=True)
    times = {label: [] for label, _, _ in variants}
    for _ in range(a.rounds):
        for label, first, run in variants:
            first()
            times[label].append(timed(run, a.iters))
    for label, _, _ in variants:
        report(label, a.config, times[label])
    ctx.set_sw_clr_all(0)
    if not a.step or a.variant != "plain":
        return
    two = ClearSkyStep(prob, device=0, clouds=clouds, clrsky=True)
    one = ClearSkyStep(prob, device=0, clouds=clouds, clrsky=True, sw_dual=True)
    api.set_sw_clr_all_default(1)  # the steps' own contexts: the dual kernel behind sw_dual
    for s in (two, one):
        s.capture()
    st = {"step all-sky + clrsky": [], "step all-sky + clrsky, sw_dual (mode 1)": []}
    for _ in range(a.rounds):
        for label, s in zip(st, (two, one)):
            st[label].append(timed(s.replay, a.iters))
    for label in st:
        report(label, a.config, st[label])
    api.set_sw_clr_all_default(0)


if __name__ == "__main__":
    main()
