"""ClearSkyStep(clouds=, mcica={..., "daylit": True}) -- the McICA SW chain on the block's daylit columns -- against the
full-extent McICA step (the same arguments without the key), and the default step against the parent commit's library.

    python tools/mcica_daylit_ab.py [--rounds 7] [--iters 30] [--ncols 1800,10000] [--parent-lib PATH [--bench-rounds 3]]

At 1800 columns (RFMIP, 882 of them at night) and 10 000 (synthetic), seeded McICA clouds (exponential-random overlap)
-- alone, with aerosols=, and with aerosols= and "clrsky" -- captured steps alternating in one process on one device
for --rounds rounds of --iters replays each (HIP events around each batch):
  (a)  mcica["daylit"],
  (a') a second step of the same kind (two samples of one thing: their difference is the yardstick),
  (b)  the full-extent McICA step, the parent's route.
Before any timing the bits are checked: (a) equals (b) on the daylit columns (SW) and everywhere (LW) and is 0 at night,
the clear set included; (a') equals (a).  Then (a) and (b) after set_sza to all day (plan + gather + compact mask +
scatter with nothing saved: the overhead) and to all night.
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
from rrtmgpnn import data  # noqa: E402
from rrtmgpnn.pipeline import ClearSkyStep  # noqa: E402

SW = ("sw_up", "sw_dn", "sw_dir")
LW = ("lw_up", "lw_dn")


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
    print("%-44s %-28s median %.4f ms  min %.4f  max %.4f  spread %.4f  (%d samples)"
          % (label, what, statistics.median(times), min(times), max(times), max(times) - min(times), len(times)),
          flush=True)
    return statistics.median(times)


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


def names(step):
    return SW + LW + (tuple(k + "_clr" for k in SW + LW) if step.clrsky else ())


def fluxes(step):
    for k in names(step):
        getattr(step, k).fill_(float("nan"))
    torch.cuda.synchronize()
    step.replay()
    torch.cuda.synchronize()
    return {k: getattr(step, k).clone() for k in names(step)}


def aerosols(ncol, nlay, nb_lw, nb_sw):
    rng = np.random.default_rng(98)
    return {"lw_tau": rng.lognormal(-2, 1, (ncol, nlay, nb_lw)).astype(np.float32),
            "sw_tau": rng.lognormal(-2, 1, (ncol, nlay, nb_sw)).astype(np.float32),
            "sw_ssa": rng.uniform(0.6, 1, (ncol, nlay, nb_sw)).astype(np.float32),
            "sw_g": rng.uniform(0.3, 0.8, (ncol, nlay, nb_sw)).astype(np.float32)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--ncols", default="1800,10000")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--bench-rounds", type=int, default=3)
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
    kl, ks = data.load_kdist("lw"), data.load_kdist("sw")
    for ncol in [int(n) for n in a.ncols.split(",") if n]:
        prob = data.rfmip_columns(0, 1800) if ncol == 1800 else data.synthetic_problem(ncol, 60, seed=20251015, col0=0)
        nlay = prob["nlay"]
        use = torch.as_tensor(np.asarray(prob["usecol"]), device="cuda")
        night = 1.0 - float(prob["usecol"].mean())
        clouds = data.allsky_clouds(prob, data.load_cloud_optics("lw"))
        cloudy = (clouds[0] > 0) | (clouds[1] > 0)
        rng = np.random.default_rng(51)
        cf = np.where(cloudy, rng.uniform(0.2, 0.9, cloudy.shape), 0).astype(np.float32)
        ov = rng.uniform(-1, 1, (ncol, nlay - 1)).astype(np.float32)
        aer = aerosols(ncol, nlay, kl["nband"], ks["nband"])
        for sky in ("seeded", "seeded + aerosols", "seeded + aerosols + clrsky"):
            def build(daylit):
                mc = {"cloud_frac": cf, "overlap_param": ov, "seed": 2026}
                if "clrsky" in sky:
                    mc["clrsky"] = True
                if daylit:
                    mc["daylit"] = True
                return ClearSkyStep(prob, device=0, clouds=clouds, mcica=mc, aerosols=aer if "aerosols" in sky else None)
            what = "%s, %d" % (sky, ncol)
            steps = {"(a) mcica['daylit']": build(True), "(a') a second such step": build(True),
                     "(b) the full-extent McICA step": build(False)}
            sa, sa2, sb = steps.values()
            for st in steps.values():
                st.capture()
            fa, fa2, fb = (fluxes(st) for st in steps.values())
            for k in fa:
                assert torch.equal(fa[k], fa2[k]), k
                assert bool(torch.isfinite(fa[k]).all()), k
                if k.startswith("lw"):
                    assert torch.equal(fa[k], fb[k]), k
                else:
                    assert torch.equal(fa[k][use], fb[k][use]), k
                    assert not bool(fa[k][~use].any()), k + ": a night column is not 0"
            assert int(sa.nday.item()) == int(use.sum())
            print("%s: %.1f %% of the columns at night; bits: (a) == (b) on the daylit columns (LW everywhere), 0 at night, "
                  "(a') == (a)" % (what, 100 * night), flush=True)
            times = {label: [] for label in steps}
            for _ in range(a.rounds):
                for label, st in steps.items():
                    times[label].append(timed(st.replay, a.iters))
            med = {label: report(label, what, times[label]) for label in steps}
            ma, ma2, mb = med.values()
            spread = max(max(times[k]) - min(times[k]) for k in list(steps)[:2])
            print("%s  (a) - (b) = %+.4f ms (%+.1f %% of the step; %.1f %% of the columns are at night); |(a) - (a')| = "
                  "%.4f ms, their largest spread %.4f ms" % (what, ma - mb, 100 * (ma / mb - 1), 100 * night, abs(ma - ma2),
                                                          spread), flush=True)
            sza0 = sa.sza.clone()
            for name, sza in (("all day", torch.full_like(sza0, 30.0)), ("all night", torch.full_like(sza0, 120.0))):
                sa.set_sza(sza)
                sb.set_sza(sza)
                t, tb = [], []
                for _ in range(a.rounds):
                    t.append(timed(sa.replay, a.iters))
                    tb.append(timed(sb.replay, a.iters))
                m, m0 = report("(a) after set_sza, " + name, what, t), report("(b) beside it", what, tb)
                print("%s  %s: (a) - (b) = %+.4f ms (%+.1f %%)" % (what, name, m - m0, 100 * (m / m0 - 1)), flush=True)
            for st in steps.values():
                st.close()


if __name__ == "__main__":
    main()
