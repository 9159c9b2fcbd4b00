"""The upper boundary condition (rrtmgpnn_compute_bc_lw / _sw) against the route a host can compose from the other
entries, the step's added time with upper_bc=True, and the default step against the parent commit's library.

    python tools/compute_bc_ab.py [--rounds 9] [--iters 35] [--parent-lib PATH [--bench-rounds 3]] [--step-only]

At 1800 columns (the RFMIP columns without their topmost layer, whose upper edge is the gas optics' minimum pressure
itself) and 10 000 (synthetic columns, likewise), LW (one angle, flux units) and SW, alternating in one process on one
device for --rounds rounds of --iters calls each (HIP events around each batch):
  (a)  the entry,
  (a') the same call again (two samples of one thing: their difference is the yardstick),
  (b)  the composed route on device arrays: rrtmgpnn_gas_optics_*_nn at nlay = 1 on the one-layer problem (gathered on
       the host beforehand, not counted), the _gpt solver into (ngpt, 2, ncol) arrays, and the copy of one level.
First (a) and (b) are compared bit for bit (LW in radiance units, what the composed route gives at one angle).
Then the fused clear-sky step at 1800 columns with and without upper_bc=True, captured, alternating replays.
With --parent-lib: plain `bench.py --gpus 1 --steps 50 --warmup 5` (the default step), alternating that library
(RRTMGPNN_LIB) and this tree's for --bench-rounds rounds, each run a fresh process, the order alternating.
One line per variant: median, min, max and spread in ms.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rte-rrtmgp-nn_amd"))
from rrtmgpnn import _lib, api, data  # noqa: E402
from rrtmgpnn._lib import float_array, int_array, ptr_array  # noqa: E402
from rrtmgpnn.api import GAUSS_DS, GAUSS_WTS  # noqa: E402
from rrtmgpnn.pipeline import ClearSkyStep  # noqa: E402


def without_top(p):
    out = dict(p, nlay=p["nlay"] - 1)
    for k in ("play", "plev", "tlay", "tlev"):
        out[k] = np.ascontiguousarray(p[k][:, 1:])
    out["gases"] = {k: np.ascontiguousarray(v[:, 1:]) for k, v in p["gases"].items()}
    return out


def problem(ncol):
    return without_top(data.rfmip_columns(0, 1800) if ncol == 1800 else
                       data.synthetic_problem(ncol, 60, seed=20251015, col0=0))


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


def report(label, what, times):
    print("%-44s %-10s median %.4f ms  min %.4f  max %.4f  spread %.4f  (%d samples)"
          % (label, what, statistics.median(times), min(times), max(times), max(times) - min(times), len(times)),
          flush=True)


def entries(which, prob, kd, nets, dev):
    """(call_a, call_b, out_a, out_b) of one stream on one problem; as_flux: LW units of (a)."""
    L, ctx = _lib.lib(), api.context(0)
    T = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=dev)  # noqa: E731
    ncol, nlay, ngpt, top_at_1 = prob["ncol"], prob["nlay"], kd.get_ngpt(), int(prob["top_at_1"])
    top = 0 if top_at_1 else nlay - 1
    names = nets[0].input_names
    play, plev, tlay, mu0 = (T(prob[k]) for k in ("play", "plev", "tlay", "mu0"))
    gases = {k: T(v) for k, v in prob["gases"].items()}
    gp = lambda g: ptr_array([g[n].data_ptr() if (k >= 2 and n in g) else None for k, n in enumerate(names)])  # noqa: E731
    nd = int_array([2] * len(names))
    hnets = ptr_array([n.h.value for n in nets])
    out_a, out_b = (torch.empty((ncol, ngpt), device=dev) for _ in range(2))
    pmin = kd.get_press_min()
    head = (ctx.h, ncol, nlay, ngpt, len(names), top_at_1, pmin, play.data_ptr(), plev.data_ptr(), tlay.data_ptr(),
            gases["h2o"].data_ptr(), gp(gases), nd, hnets)
    # the one-layer problem, gathered on the host (mo_compute_bc.F90:108-140)
    tl1 = prob["tlay"][:, top:top + 1]
    pl1 = np.stack([np.full(ncol, pmin, np.float32), prob["plev"][:, top + 1]], axis=1)
    py1 = (np.float32(0.5) * (pl1[:, 0] + pl1[:, 1]))[:, None]
    play1, plev1, tlay1, tlev1 = T(py1), T(pl1), T(tl1), T(np.concatenate([tl1, tl1], axis=1))
    gases1 = {k: T(v[:, top:top + 1]) for k, v in prob["gases"].items()}
    tau, second = (torch.empty((ncol, 1, ngpt), device=dev) for _ in range(2))
    flux = [torch.empty((ncol, 2), device=dev) for _ in range(3)]
    gpt = [torch.empty((ncol, 2, ngpt), device=dev) for _ in range(3)]
    ones = torch.ones((ncol, ngpt), device=dev)
    head1 = (ctx.h, ncol, 1, ngpt, len(names), play1.data_ptr(), tlay1.data_ptr(), plev1.data_ptr(),
             gases1["h2o"].data_ptr(), gp(gases1), nd, hnets)
    bottom = 1 if top_at_1 else 0
    if which == "lw":
        lims = int_array(kd.band_lims_gpt.ravel())
        Ds, W = float_array(GAUSS_DS[1]), float_array(GAUSS_WTS[1])
        state = {"as_flux": 1}

        def call_a():
            assert L.rrtmgpnn_compute_bc_lw(*head, len(nets), kd.get_nband(), kd.get_nPlanckTemp(), lims,
                                            kd.temp_ref_min, kd.totplnk_delta, kd.totplnk.data_ptr(), 1, Ds, W,
                                            state["as_flux"], out_a.data_ptr()) == 0, L.rrtmgpnn_last_error()

        def call_b():
            assert L.rrtmgpnn_gas_optics_lw_nn(*head1, len(nets), tau.data_ptr(), second.data_ptr()) == 0
            assert L.rrtmgpnn_lw_solver_noscat_planck_gpt(
                ctx.h, ngpt, 1, ncol, top_at_1, 1, Ds, W, None, None, tau.data_ptr(), second.data_ptr(),
                kd.get_nband(), kd.get_nPlanckTemp(), tlay1.data_ptr(), tlev1.data_ptr(), tlay1.data_ptr(), 1, lims,
                kd.temp_ref_min, kd.totplnk_delta, kd.totplnk.data_ptr(), 0, ones.data_ptr(), flux[0].data_ptr(),
                flux[1].data_ptr(), gpt[0].data_ptr(), gpt[1].data_ptr()) == 0, L.rrtmgpnn_last_error()
            out_b.copy_(gpt[1][:, bottom])

        return call_a, call_b, out_a, out_b, state
    src = T(kd.solar_source)
    inc = T(np.broadcast_to(kd.solar_source, (ncol, ngpt)))

    def call_a():
        assert L.rrtmgpnn_compute_bc_sw(*head, src.data_ptr(), mu0.data_ptr(), out_a.data_ptr()) == 0, \
            L.rrtmgpnn_last_error()

    def call_b():
        assert L.rrtmgpnn_gas_optics_sw_nn(*head1, tau.data_ptr(), second.data_ptr(), None) == 0
        assert L.rrtmgpnn_sw_solver_2stream_gpt(
            ctx.h, ngpt, 1, ncol, top_at_1, inc.data_ptr(), None, tau.data_ptr(), second.data_ptr(), None,
            mu0.data_ptr(), ones.data_ptr(), ones.data_ptr(), *[t.data_ptr() for t in flux + gpt]) == 0, \
            L.rrtmgpnn_last_error()
        out_b.copy_(gpt[2][:, bottom])

    return call_a, call_b, out_a, out_b, {}


def bench_line(lib):
    env = dict(os.environ)
    env.pop("RRTMGPNN_LIB", None)
    if lib:
        env["RRTMGPNN_LIB"] = lib
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "50", "--warmup", "5"],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    return {k: d[k] for k in ("value", "unit", "n_gpus", "steps", "warmup", "ms_per_step") if k in d}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=35)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--bench-rounds", type=int, default=3)
    ap.add_argument("--step-only", action="store_true", help="only the step with and without upper_bc=True")
    a = ap.parse_args()
    if a.parent_lib:  # fresh processes first, before this one holds the device
        ms = {"parent": [], "this": []}
        for r in range(a.bench_rounds):
            for who in (("parent", "this") if r % 2 == 0 else ("this", "parent")):
                d = bench_line(a.parent_lib if who == "parent" else None)
                ms[who].append(d["ms_per_step"])
                print("== %s library, round %d\n%s" % (who, r + 1, json.dumps(d)), flush=True)
        print("# ms_per_step min / median / max over the rounds: parent library %s, this tree's %s"
              % tuple(" / ".join("%.4f" % f(ms[w]) for f in (min, statistics.median, max)) for w in ("parent", "this")),
              flush=True)
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    kds, nets = {}, {}
    for w, names in (("lw", ("lw_abs", "lw_pfrac")), ("sw", ("sw_abs", "sw_ray"))):
        kds[w] = api.GasOpticsRRTMGP()
        assert kds[w].load(w) == ""
        nets[w] = [api.RrtmgpNetwork(0).load(data.path(n)) for n in names]
    for ncol in (() if a.step_only else (1800, 10000)):
        prob = problem(ncol)
        for w in ("lw", "sw"):
            call_a, call_b, out_a, out_b, state = entries(w, prob, kds[w], nets[w], dev)
            state["as_flux"] = 0  # the composed route's units at one angle
            for o, fn in ((out_a, call_a), (out_b, call_b)):
                o.fill_(float("nan"))
                fn()
            torch.cuda.synchronize()
            assert torch.equal(out_a, out_b) and bool(torch.isfinite(out_a).all()), "%s %d: (a) != (b)" % (w, ncol)
            state["as_flux"] = 1
            variants = [("(a) rrtmgpnn_compute_bc_" + w, call_a), ("(a') the same again", call_a),
                        ("(b) gas optics at nlay = 1 + _gpt solver + copy", call_b)]
            times = {label: [] for label, _ in variants}
            for _ in range(a.rounds):
                for label, fn in variants:
                    times[label].append(timed(fn, a.iters))
            what = "%s %d" % (w, ncol)
            for label, _ in variants:
                report(label, what, times[label])
            med = [statistics.median(times[label]) for label, _ in variants]
            spread = max(max(times[variants[k][0]]) - min(times[variants[k][0]]) for k in (0, 1))
            print("%s  bitwise (a) == (b); (a) / (b) = %.3f; (b) - (a) = %+.4f ms; |(a) - (a')| = %.4f ms, their largest "
                  "spread %.4f ms" % (what, med[0] / med[2], med[2] - med[0], abs(med[0] - med[1]), spread), flush=True)
    # the step
    prob = problem(1800)
    steps = {k: ClearSkyStep(prob, device=0, upper_bc=k) for k in (False, True)}
    for st in steps.values():
        st.capture()
    times = {k: [] for k in steps}
    for _ in range(a.rounds):
        for k, st in steps.items():
            times[k].append(timed(st.replay, a.iters))
    report("(s) fused clear-sky step, captured", "1800", times[False])
    report("(t) the same with upper_bc=True", "1800", times[True])
    m0, m1 = statistics.median(times[False]), statistics.median(times[True])
    print("step 1800  upper_bc=True adds %+.4f ms (%+.1f %%)" % (m1 - m0, 100 * (m1 / m0 - 1)), flush=True)
    for st in steps.values():
        st.close()


if __name__ == "__main__":
    main()
