"""GPU: ClearSkyStep(upper_bc=True) on 36 RFMIP columns without their topmost layer -- clear sky at one and two angles,
one McICA (seeded) all-sky set, the LW-only step, fused and unfused -- every comparison bit for bit: the step's LW fluxes
against the oracle's rte_lw with inc_flux = the comparator's boundary flux (tests/compute_bc_ref.py, flux units), a
captured graph against the eager step, the SW fluxes against the same step without the option; the downward LW flux at
the model's top is no longer zero.  And the call plan of every upper_bc=True option set against
tests/golden/step_plan_upper_bc.json."""
import json
import os

import numpy as np
import pytest

import compute_bc_ref as B
import mcica_ref as M
import philox_ref as PH
import step_plan_upper_bc as PU

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "step_plan_upper_bc.json")
FLUX = ("lw_up", "lw_dn", "sw_up", "sw_dn", "sw_dir")
SEED = 20261020


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a device"
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def case(rfmip, orc):
    """36 columns under the removed top layer, their clouds, cloud fraction and overlap parameter, the oracle's LW gas
    optics (shared by every mode) and the comparator's boundary fluxes at one and two angles."""
    from conftest import subset
    from rrtmgpnn import data
    prob = subset(PU.without_top(rfmip), np.arange(3, 1800, 50))
    ncol, nlay = prob["ncol"], prob["nlay"]
    clouds = data.allsky_clouds(prob, data.load_cloud_optics("lw"))
    cloudy = (clouds[0] > 0) | (clouds[1] > 0)
    assert cloudy.any()
    rng = np.random.default_rng(63)
    cf = np.where(cloudy, rng.uniform(0.2, 0.9, cloudy.shape), 0).astype(np.float32)
    ov = rng.uniform(-1, 1, (ncol, nlay - 1)).astype(np.float32)
    kd = data.load_kdist("lw")
    go = orc.lw_gas_optics(prob, [data.load_model("lw_abs"), data.load_model("lw_pfrac")], kd)
    inc = {n: B.in_flux_units(B.lw(orc, prob, n), n) for n in (1, 2)}
    return dict(prob=prob, clouds=clouds, cf=cf, ov=ov, kd=kd, go=go, inc=inc)


def _lw_oracle(orc, c, nmus, mcica=False):
    """rte_lw with the boundary flux as inc_flux, on the gas optical depth or the McICA-sampled all-sky one."""
    from rrtmgpnn import data
    prob, go, kd = c["prob"], c["go"], c["kd"]
    ncol, nlay, ng = go["tau"].shape
    tau = go["tau"]
    if mcica:
        (ct,) = orc.cloud_optics(data.load_cloud_optics("lw"), *c["clouds"], nstr=1, lut=True, icergh=2)
        mask = M.sampled_mask(PH.randoms(SEED, 0, 0, ng, nlay, ncol), c["cf"], c["ov"])
        ident = np.stack([np.arange(1, ng + 1)] * 2, axis=1).astype(np.int32)
        (tau,) = orc.increment_bybnd(ident, (tau,), (M.draw(mask, ct, kd["band_lims_gpt"]),))
    emis = np.repeat(np.asarray(prob["sfc_emis"], np.float32)[:, None], ng, axis=1)
    return orc.lw_solver(tau, go["lay_source"], go["lev_source"], emis, go["sfc_source"], prob["top_at_1"], nmus,
                         inc_flux=c["inc"][nmus])


def _kwargs(c, mode):
    if mode == "mcica":
        return {"clouds": c["clouds"], "mcica": {"cloud_frac": c["cf"], "overlap_param": c["ov"], "seed": SEED}}
    return {"nmus": 2} if mode == "clear2" else {}


def _run(step, replay=False):
    for k in FLUX if step.sw else FLUX[:2]:  # (an LW-only step's SW fluxes are zeros written once)
        getattr(step, k).fill_(float("nan"))
    if getattr(step, "lw_inc_flux", None) is not None:
        step.lw_inc_flux.fill_(float("nan"))
    step.replay() if replay else step.step()
    torch.cuda.synchronize()
    return step.fluxes()


@pytest.mark.parametrize("mode", ["clear1", "clear2", "mcica"])
def test_step_with_upper_bc(dev, orc, case, mode):
    from rrtmgpnn import _lib
    from rrtmgpnn.pipeline import ClearSkyStep
    c, prob = case, case["prob"]
    nmus = 2 if mode == "clear2" else 1
    step = ClearSkyStep(prob, device=0, upper_bc=True, **_kwargs(c, mode))
    names = [n for n, _, _ in step.calls]
    fns = {n: f for n, f, _ in step.calls}
    assert fns["lw_upper_bc"] is _lib.lib().rrtmgpnn_compute_bc_lw
    assert names.index("lw_upper_bc") < names.index("predict_nn_lw") < names.index("lw_solver")
    eager = _run(step)
    np.testing.assert_array_equal(step.lw_inc_flux.cpu().numpy(), c["inc"][nmus], err_msg="the step's lw_inc_flux")
    up, dn = _lw_oracle(orc, c, nmus, mode == "mcica")
    np.testing.assert_array_equal(eager["lw_up"], up, err_msg="fused eager lw_up against the oracle")
    np.testing.assert_array_equal(eager["lw_dn"], dn, err_msg="fused eager lw_dn against the oracle")
    top = 0 if prob["top_at_1"] else prob["nlay"]
    assert (eager["lw_dn"][:, top] > 0).all(), "the downward LW flux at the model's top"
    bare = ClearSkyStep(prob, device=0, **_kwargs(c, mode))
    plain = _run(bare)
    bare.close()
    assert (plain["lw_dn"][:, top] == 0).all()
    for k in ("sw_up", "sw_dn", "sw_dir"):
        np.testing.assert_array_equal(eager[k], plain[k], err_msg="the SW fluxes without the option: " + k)
    step.capture()
    again = _run(step, replay=True)
    for k in FLUX:
        np.testing.assert_array_equal(again[k], eager[k], err_msg="captured against eager: " + k)
    step.close()
    unf = ClearSkyStep(prob, device=0, upper_bc=True, fused=False, **_kwargs(c, mode))
    got = _run(unf)
    unf.close()
    for k in FLUX:
        np.testing.assert_array_equal(got[k], eager[k], err_msg="fused=False against fused: " + k)


def test_lw_only_step_and_refusals(dev, orc, case, rfmip):
    from conftest import subset
    from rrtmgpnn.pipeline import ClearSkyStep
    c, prob = case, case["prob"]
    step = ClearSkyStep(prob, device=0, upper_bc=True, sw=False)
    got = _run(step)
    up, dn = _lw_oracle(orc, c, 1)
    np.testing.assert_array_equal(got["lw_up"], up)
    np.testing.assert_array_equal(got["lw_dn"], dn)
    assert not got["sw_dn"].any()
    # new pressures come in through inputs_for: the unmodified columns are refused there as at construction
    full = subset(rfmip, np.arange(3, 1800, 50))
    shaped = dict(prob, plev=np.ascontiguousarray(full["plev"][:, :-1]))
    with pytest.raises(ValueError, match="pressures are too close"):
        step.inputs_for(shaped)
    assert len(step.inputs_for(prob)) == len(step.io_tensors()[0])
    step.close()
    with pytest.raises(ValueError, match="pressures are too close"):
        ClearSkyStep(full, device=0, upper_bc=True)


# ---- the call plan ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def env(dev, rfmip):
    return PU.environment(rfmip)


@pytest.mark.parametrize("cid,build", PU.CASES, ids=[k for k, _ in PU.CASES])
def test_step_plan(cid, build, env, golden):
    want = golden[cid]
    got = json.loads(json.dumps(PU.run_case(build, env)))
    if "raises" in want:
        assert got == want
        return
    assert "raises" not in got, got
    assert got["schedule"] == want["schedule"]
    assert got["buffers"] == want["buffers"]
    assert [c.split()[0] for c in got["calls"]] == [c.split()[0] for c in want["calls"]]
    for g, w in zip(got["calls"], want["calls"]):
        assert g == w
    assert got == want
