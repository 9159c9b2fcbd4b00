"""GPU: the paths whose global streams carry a non-default cache policy (CachePolicy, csrc/rte_device.hpp; DESIGN.md
section 3, "Cache policies per stream") give the oracle's fluxes bit for bit.  A policy cannot change a value; what it
could do is leave a line behind that a later launch into the same buffers then reads, so every case launches three
times into one step's buffers with three different column sets and compares after each launch.

The fused step's entry points (rrtmgpnn_lw_solver_noscat_planck[_inc], rrtmgpnn_sw_solver_2stream_rfmip) with the
shipped NN gas optics, at the smallest shapes that reach all their branches: 3 columns (an odd count: the SW block's
last column slot is idle and its stores go to the out-of-range offset), 7 and 4 layers (no multiple of the SW chunk of 3
or the LW ring of 8: the last chunk is partial), both orientations; clear sky (the small-grid SW instance and the fused
clear-sky LW instance) and all sky (the band-increment instances of both solvers).  As shipped the SW instances'
last-use loads carry `nt`; the LW instances run here too, so that a policy set on them later is covered as well.
The cases run once more in a fresh child process with RRTMGPNN_SW_NO_PLANES=1 (read once per process, as
tests/test_gpu_sw_planes.py does): the all-sky SW instance then runs without its workspace planes.  The large-grid clear-sky instance cannot be reached at
these sizes; tests/test_gpu_fullsize.py and tests/test_gpu_chunked.py cover it."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COL0 = (0, 1000, 5000)  # three column sets of the synthetic problem (three different random-stream blocks)


def _flip(prob):
    out = dict(prob)
    for k in ("play", "plev", "tlay", "tlev"):
        out[k] = np.ascontiguousarray(prob[k][:, ::-1])
    out["gases"] = {k: np.ascontiguousarray(v[:, ::-1]) for k, v in prob["gases"].items()}
    out["top_at_1"] = False
    return out


def _problems(nlay, top_at_1, allsky):
    from rrtmgpnn import data
    out = []
    for col0 in COL0:
        prob = data.synthetic_problem(3, nlay, seed=20251020, col0=col0)
        if not top_at_1:
            prob = _flip(prob)
        out.append((prob, data.allsky_clouds(prob, data.load_cloud_optics("lw")) if allsky else None))
    return out


def _reference(orc, prob, clouds):
    from rrtmgpnn import data
    m = {k: data.load_model(k) for k in ("lw_abs", "lw_pfrac", "sw_abs", "sw_ray")}
    kl, ks = data.load_kdist("lw"), data.load_kdist("sw")
    if clouds is None:
        lu, ld, _ = orc.clear_sky_lw(prob, [m["lw_abs"], m["lw_pfrac"]], kl)
        su, sd, sr, _ = orc.clear_sky_sw(prob, [m["sw_abs"], m["sw_ray"]], ks, zero_unused=False)
    else:
        co_lw, co_sw = data.load_cloud_optics("lw"), data.load_cloud_optics("sw")
        lu, ld, _ = orc.all_sky_lw(prob, [m["lw_abs"], m["lw_pfrac"]], kl, co_lw, clouds)
        su, sd, sr, _ = orc.all_sky_sw(prob, [m["sw_abs"], m["sw_ray"]], ks, co_sw, clouds)
    return {"lw_up": lu, "lw_dn": ld, "sw_up": su, "sw_dn": sd, "sw_dir": sr}


@pytest.mark.parametrize("allsky", [False, True], ids=["clear", "allsky"])
@pytest.mark.parametrize("top_at_1", [True, False], ids=["top1", "top0"])
@pytest.mark.parametrize("nlay", [7, 4])
def test_three_launches_into_one_step_match_oracle_bitwise(orc, nlay, top_at_1, allsky):
    from rrtmgpnn.pipeline import ClearSkyStep
    torch.cuda.set_device(0)
    probs = _problems(nlay, top_at_1, allsky)
    if allsky:
        assert any((c[0] > 0).any() or (c[1] > 0).any() for _, c in probs), "no cloud in any column set"
    step = ClearSkyStep(probs[0][0], device=0, clouds=probs[0][1])
    entries = {fn.__name__ for _, fn, _ in step.calls}
    assert "rrtmgpnn_sw_solver_2stream_rfmip" in entries
    assert ("rrtmgpnn_lw_solver_noscat_planck_inc" if allsky else "rrtmgpnn_lw_solver_noscat_planck") in entries
    ins, _ = step.io_tensors()
    seen = []
    for prob, clouds in probs:
        for d, x in zip(ins, step.inputs_for(prob, clouds)):
            d.copy_(x)
        torch.cuda.synchronize()
        step.step()
        torch.cuda.synchronize()
        got = step.fluxes()
        ref = _reference(orc, prob, clouds)
        use = prob["usecol"]
        np.testing.assert_array_equal(got["lw_up"], ref["lw_up"], err_msg="lw_up")
        np.testing.assert_array_equal(got["lw_dn"], ref["lw_dn"], err_msg="lw_dn")
        if allsky:  # the oracle's all-sky SW fluxes: night columns' up and down zeroed, the beam on the day columns
            for k in ("sw_up", "sw_dn"):
                g = got[k].copy()
                g[~use] = 0.0
                np.testing.assert_array_equal(g, ref[k], err_msg=k)
            np.testing.assert_array_equal(got["sw_dir"][use], ref["sw_dir"][use], err_msg="sw_dir")
        else:  # rte_sw's raw output on every column, night columns (solved with mu0 = 1) included
            for k in ("sw_up", "sw_dn", "sw_dir"):
                np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
        seen.append(got["lw_dn"])
    # the three column sets are different problems: a launch that changed nothing would not pass as the next one
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])


def test_same_cases_without_sw_workspace_planes():
    env = dict(os.environ)
    env["RRTMGPNN_SW_NO_PLANES"] = "1"
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider",
                        "-k", "three_launches", os.path.abspath(__file__)],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-2000:])
    assert "8 passed" in r.stdout, r.stdout[-1000:]
