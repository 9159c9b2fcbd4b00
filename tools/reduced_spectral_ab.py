"""The reduced-resolution networks (LW g128 pair, SW g112 pair, LW g128 single model) on their 32x32x2 instances against
the 16x16x4 route, and the whole clear-sky step at reduced against full resolution.

    python tools/reduced_spectral_ab.py [--rounds 9] [--iters 30] [--parent-lib PATH] [--only net|step]

Without --child the script touches no device: it starts every measurement as a child process of its own under
`timeout`, one after the other on one box, and stops at the first child that does not end with status 0.
  (a) each network alone through the fused entry (rrtmgpnn_gas_optics_*_nn, what the step calls) at 1800 x 60 (C3:
      the RFMIP columns) and 10 000 x 60 (C4: synthetic columns), alternating in one process for --rounds rounds of
      --iters calls (HIP events around each batch):
        (m32)  the 32x32x2 instance (rrtmgpnn_context_set_mlp_kernel 0),
        (m32') the same again -- two samples of one build: their difference is the yardstick,
        (m16)  rrtmgpnn_context_set_mlp_kernel 1: compute_nn_inputs + get_col_dry + the 16x16x4 kernel, the route
               these models took before they had 32x32x2 instances.
      The outputs of (m32) and (m16) are compared bit for bit first, and the kernel each ran is asserted.
      With --parent-lib (a build of the parent commit): the same call on that library (its only route) and (m16) on
      this tree's, in alternating fresh processes (RRTMGPNN_LIB), to confirm that (m16) stands for the parent.
  (b) the fused clear-sky step, captured, alternating replays: full resolution (g256 / g224), reduced resolution with
      the 32x32x2 instances, reduced resolution on the 16x16x4 route; at 1800 and 10 000 columns.
One line per variant: median, min, max and spread in ms.
"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rte-rrtmgp-nn_amd"))
FILES = os.path.join(ROOT, "tests", "golden", "reference_files")
MODELS = {"lw_pair": ("lw-g128-210809_absorption_BEST.nc", "lw-g128-210809_planck_frac_BEST.nc"),
          "sw_pair": ("sw-g112-210809_absorption_BEST.nc", "sw-g112-210809_rayleigh_BEST.nc"),
          "lw_both": ("nn_lw_g128_both.rbin",)}
NGPT = {"lw_pair": 128, "sw_pair": 112, "lw_both": 128}
SIZES = (1800, 10000)
MFMA32, MFMA16 = 2, 3


def model_paths(kind):
    from rrtmgpnn import data
    return [os.path.join(FILES, n) if n.endswith(".nc") else data.path(n) for n in MODELS[kind]]


def problem(ncol):
    from rrtmgpnn import data
    return data.rfmip_columns(0, 1800) if ncol == 1800 else data.synthetic_problem(ncol, 60, seed=20251015, col0=0)


def report(label, what, times):
    print("%-46s %-16s median %.4f ms  min %.4f  max %.4f  spread %.4f  (%d samples)"
          % (label, what, statistics.median(times), min(times), max(times), max(times) - min(times), len(times)),
          flush=True)


def timed(fn, iters):
    import torch
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def network_call(kind, ncol):
    """(call, outputs, ctx): the fused gas-optics entry of one model set on ncol x 60 samples, on the default context."""
    import ctypes
    import numpy as np
    import torch
    from rrtmgpnn import _lib, api
    from rrtmgpnn._lib import int_array, ptr_array
    dev = torch.device("cuda", 0)
    L, ctx = _lib.lib(), api.context(0)
    prob = problem(ncol)
    T = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=dev)  # noqa: E731
    nets = [api.RrtmgpNetwork(0).load(p) for p in model_paths(kind)]
    names = nets[0].input_names
    play, tlay, plev = (T(prob[k]) for k in ("play", "tlay", "plev"))
    gases = {k: T(v) for k, v in prob["gases"].items()}
    gp = ptr_array([gases[n].data_ptr() if (k >= 2 and n in gases) else None for k, n in enumerate(names)])
    nd = int_array([2] * len(names))
    hs = ptr_array([n.h.value for n in nets])
    nlay, ngpt = prob["nlay"], NGPT[kind]
    outs = [torch.empty((ncol, nlay, ngpt), device=dev) for _ in range(2)]
    head = (ctx.h, ncol, nlay, ngpt, len(names), play.data_ptr(), tlay.data_ptr(), plev.data_ptr(),
            gases["h2o"].data_ptr(), gp, nd, hs)
    keep = (nets, play, tlay, plev, gases, gp, nd, hs)

    def call():
        if kind == "sw_pair":
            rc = L.rrtmgpnn_gas_optics_sw_nn(*head, outs[0].data_ptr(), outs[1].data_ptr(), None)
        else:
            rc = L.rrtmgpnn_gas_optics_lw_nn(*head, len(nets), outs[0].data_ptr(), outs[1].data_ptr())
        assert rc == 0, L.rrtmgpnn_last_error()

    def path():
        p = (ctypes.c_int * 8)()
        assert L.rrtmgpnn_context_get_mlp_path(ctx.h, p) == 0
        return p[0]

    call.keep = keep
    return call, outs, ctx, path


def child_net(a):
    import torch
    torch.cuda.set_device(0)
    for kind in a.kinds.split(","):
        for ncol in SIZES:
            call, outs, ctx, path = network_call(kind, ncol)
            got = {}
            for mode, want in ((0, MFMA32), (1, MFMA16)):
                ctx.set_mlp_kernel(mode)
                for o in outs:
                    o.fill_(float("nan"))
                call()
                torch.cuda.synchronize()
                assert path() == want, (kind, mode, path())
                got[mode] = [o.clone() for o in outs]
            for x, y in zip(got[0], got[1]):
                assert torch.equal(x.view(torch.int32), y.view(torch.int32)) and bool(torch.isfinite(x).all())
            variants = [("(m32) 32x32x2 instance", 0), ("(m32') the same again", 0), ("(m16) 16x16x4 route", 1)]
            times = {label: [] for label, _ in variants}
            for _ in range(a.rounds):
                for label, mode in variants:
                    ctx.set_mlp_kernel(mode)
                    times[label].append(timed(call, a.iters))
            ctx.set_mlp_kernel(0)
            what = "%s %d" % (kind, ncol)
            for label, _ in variants:
                report(label, what, times[label])
            med = [statistics.median(times[label]) for label, _ in variants]
            spread = max(max(times[variants[k][0]]) - min(times[variants[k][0]]) for k in (0, 1))
            print("%s  bitwise (m32) == (m16); (m32) / (m16) = %.3f; (m16) - (m32) = %+.4f ms; |(m32) - (m32')| = %.4f ms, "
                  "their largest spread %.4f ms" % (what, med[0] / med[2], med[2] - med[0], abs(med[0] - med[1]), spread),
                  flush=True)


def child_route(a):
    """One library's own default-or-forced route of one model set, for the parent-library confirmation."""
    import torch
    torch.cuda.set_device(0)
    for ncol in SIZES:
        call, outs, ctx, path = network_call(a.kinds, ncol)
        if a.mode >= 0:
            ctx.set_mlp_kernel(a.mode)
        call()
        torch.cuda.synchronize()
        assert path() == MFMA16, path()
        times = [timed(call, a.iters) for _ in range(a.rounds)]
        report("(%s) %s" % (a.tag, "16x16x4 route"), "%s %d" % (a.kinds, ncol), times)


def child_step(a):
    import torch
    from rrtmgpnn import api
    from rrtmgpnn.pipeline import ClearSkyStep
    torch.cuda.set_device(0)
    lw, sw = model_paths("lw_pair"), model_paths("sw_pair")
    spectral = {"lw_models": tuple(lw), "sw_models": tuple(sw), "ngpt_lw": 128, "ngpt_sw": 112}
    for ncol in SIZES:
        prob = problem(ncol)
        variants = [("(full) g256 / g224", None, 0), ("(full') the same again", None, 0),
                    ("(red32) g128 / g112, 32x32x2 instances", spectral, 0), ("(red16) g128 / g112, 16x16x4 route", spectral, 1)]
        steps = {}
        for label, sp, mode in variants:
            api.set_mlp_kernel_default(mode)  # the captured launches keep the kernel chosen here
            st = ClearSkyStep(prob, device=0, spectral=sp)
            st.step()
            torch.cuda.synchronize()
            st.capture()
            steps[label] = st
        api.set_mlp_kernel_default(0)
        a32, a16 = steps[variants[2][0]].fluxes(), steps[variants[3][0]].fluxes()
        for k in a32:
            assert (a32[k].view("uint32") == a16[k].view("uint32")).all(), k
        times = {label: [] for label, _, _ in variants}
        for _ in range(a.rounds):
            for label, _, _ in variants:
                times[label].append(timed(steps[label].replay, a.iters))
        for label, _, _ in variants:
            report(label, "step %d" % ncol, times[label])
        med = {label: statistics.median(times[label]) for label, _, _ in variants}
        f, f2, r32, r16 = (med[v[0]] for v in variants)
        print("step %d  (red32) / (full) = %.3f; (red32) / (red16) = %.3f; |(full) - (full')| = %.4f ms; lw_net_cus %d "
              "(full) %d (reduced)" % (ncol, r32 / f, r32 / r16, abs(f - f2), steps[variants[0][0]].lw_net_cus,
                                       steps[variants[2][0]].lw_net_cus), flush=True)
        for st in steps.values():
            st.close()


def spawn(args, seconds, env=None):
    cmd = ["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(__file__)] + args
    r = subprocess.run(cmd, env=env)
    if r.returncode != 0:
        print("# child %s ended with status %d: stopping" % (" ".join(args), r.returncode), flush=True)
        sys.exit(r.returncode)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--only", choices=("net", "step"), default=None)
    ap.add_argument("--child", choices=("net", "route", "step"), default=None)
    ap.add_argument("--kinds", default="lw_pair,sw_pair,lw_both")
    ap.add_argument("--mode", type=int, default=-1)
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    if a.child:
        {"net": child_net, "route": child_route, "step": child_step}[a.child](a)
        return
    common = ["--rounds", str(a.rounds), "--iters", str(a.iters)]
    if a.only in (None, "net"):
        for kind in a.kinds.split(","):
            print("== (a) %s alone" % kind, flush=True)
            spawn(["--child", "net", "--kinds", kind] + common, 240)
        if a.parent_lib:
            base = {k: v for k, v in os.environ.items() if k != "RRTMGPNN_LIB"}
            for kind in ("lw_pair", "sw_pair"):
                print("== (a) %s: the parent library's route against (m16), fresh processes in turn" % kind, flush=True)
                for r in range(2):
                    for who in (("parent", "this") if r % 2 == 0 else ("this", "parent")):
                        env = dict(base, RRTMGPNN_LIB=a.parent_lib) if who == "parent" else base
                        spawn(["--child", "route", "--kinds", kind, "--tag", who, "--mode", "-1" if who == "parent" else "1"]
                              + common, 180, env)
    if a.only in (None, "step"):
        print("== (b) the fused clear-sky step, captured", flush=True)
        spawn(["--child", "step"] + common, 420)


if __name__ == "__main__":
    main()
