"""McICA mask kernels: the caller's random numbers read from an array against numbers drawn in the kernel (Philox4x32-10).

    python tools/mcica_seeded_ab.py --config c4 [--rounds 9] [--iters 35]

The config's columns (c4: 10 000 x 60 synthetic columns; c3: the 1800 RFMIP columns) with the all-sky example's clouds
and the cloud fraction per cloudy layer tools/mcica_ab.py uses.  LW (256 g-points) and SW (224), maximum-random and
exponential-random overlap, alternating in one process on one device for --rounds rounds of --iters calls each (HIP
events around each batch):
  (a) the array mask kernel (packed bits) on a randoms array;
  (b) the seeded mask kernel (packed bits);
  (c) rrtmgpnn_mcica_randoms followed by (a): what a caller pays today if it generates on the device;
  (d) (b) with every layer cloudy, so that no group of 4 layers is skipped: the generator's ceiling cost.
One line per variant: median, min and max ms; (a)'s spread (max - min) is the yardstick for (b) - (a).  The masks of (a)
(on rrtmgpnn_mcica_randoms' output) and (b) are compared bit for bit first.
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


def report(label, tag, times):
    med = statistics.median(times)
    print("%-52s %s  median %.4f ms  min %.4f  max %.4f  spread %.4f  (%d samples)"
          % (label, tag, med, min(times), max(times), max(times) - min(times), len(times)), flush=True)
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c4", choices=["c3", "c4"])
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=35)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    L = _lib.lib()
    prob = data.rfmip_columns(0, 1800) if a.config == "c3" else data.synthetic_problem(10000, 60, seed=20251015, col0=0)
    clouds = data.allsky_clouds(prob, data.load_cloud_optics("lw"))
    ncol, nlay = prob["ncol"], prob["nlay"]
    rs = np.random.default_rng(7)
    cloudy = (clouds[0] > 0) | (clouds[1] > 0)
    cf_np = np.where(cloudy, rs.uniform(0.1, 1.0, cloudy.shape), 0).astype(np.float32)
    pad = np.zeros((ncol, (nlay + 3) // 4 * 4), bool)
    pad[:, :nlay] = cf_np > 0
    drawn = pad.reshape(ncol, -1, 4).any(axis=2).mean()
    print("%s: %d x %d, %.1f %% of the layers cloudy, %.1f %% of the groups of 4 layers draw"
          % (a.config, ncol, nlay, 100 * (cf_np > 0).mean(), 100 * drawn), flush=True)
    T = lambda x: torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32), device=dev)  # noqa: E731
    cf, cf_all = T(cf_np), T(rs.uniform(0.1, 1.0, cf_np.shape))
    ov = T(rs.uniform(-1, 1, (ncol, nlay - 1)))
    ctx = api.context(0)  # torch's current (default) stream: the events are recorded on it
    rng = torch.zeros(4, dtype=torch.int32, device=dev)
    p = lambda t: t.data_ptr()  # noqa: E731

    def chain(*steps):
        def run():
            for fn, args in steps:
                rc = fn(*args)
                assert rc == 0, L.rrtmgpnn_last_error()
        return run

    for which, ng, stream in (("lw", data.load_kdist("lw")["ngpt"], 0), ("sw", data.load_kdist("sw")["ngpt"], 1)):
        _lib.check(L.rrtmgpnn_mcica_rng_set(ctx.h, 2026, stream, 0, p(rng)), "mcica_rng_set")
        randoms = torch.empty((ncol, nlay, ng), dtype=torch.float32, device=dev)
        bits_a, bits_b = (torch.empty((ncol, nlay, (ng + 31) // 32), dtype=torch.int32, device=dev) for _ in range(2))
        gen = (L.rrtmgpnn_mcica_randoms, (ctx.h, ng, nlay, ncol, p(rng), p(randoms)))
        for overlap in ("max_ran", "exp_ran"):
            head = (ctx.h, ng, nlay, ncol)
            if overlap == "max_ran":
                arr = (L.rrtmgpnn_sampled_mask_max_ran, head + (p(randoms), p(cf), None, p(bits_a)))
                sed = (L.rrtmgpnn_sampled_mask_max_ran_seeded, head + (p(rng), p(cf), None, p(bits_b)))
                top = (L.rrtmgpnn_sampled_mask_max_ran_seeded, head + (p(rng), p(cf_all), None, p(bits_b)))
            else:
                arr = (L.rrtmgpnn_sampled_mask_exp_ran, head + (p(randoms), p(cf), p(ov), None, p(bits_a)))
                sed = (L.rrtmgpnn_sampled_mask_exp_ran_seeded, head + (p(rng), p(cf), p(ov), None, p(bits_b)))
                top = (L.rrtmgpnn_sampled_mask_exp_ran_seeded, head + (p(rng), p(cf_all), p(ov), None, p(bits_b)))
            chain(gen, arr, sed)()
            torch.cuda.synchronize()
            assert torch.equal(bits_a, bits_b), "%s %s: the array and the seeded masks differ" % (which, overlap)
            assert bool((bits_a != 0).any())
            variants = [("(a) %s array mask kernel, packed bits" % which, chain(arr)),
                        ("(b) %s seeded mask kernel, packed bits" % which, chain(sed)),
                        ("(c) %s mcica_randoms + array mask kernel" % which, chain(gen, arr)),
                        ("(d) %s seeded mask kernel, every layer cloudy" % which, chain(top))]
            times = {label: [] for label, _ in variants}
            for _ in range(a.rounds):
                for label, run in variants:
                    times[label].append(timed(run, a.iters))
            tag = a.config + " " + overlap
            med = [report(label, tag, times[label]) for label, _ in variants]
            ta = times[variants[0][0]]
            print("%s %s: (b) - (a) = %+.4f ms against (a)'s spread %.4f ms; (b) - (c) = %+.4f ms; (d) - (a) = %+.4f ms"
                  % (which, overlap, med[1] - med[0], max(ta) - min(ta), med[1] - med[2], med[3] - med[0]), flush=True)
        del randoms, bits_a, bits_b
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
