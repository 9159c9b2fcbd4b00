"""GPU: ClearSkyStep(clouds=..., lw_scattering=True) on 12 RFMIP columns -- overcast, McICA (random-number arrays), and
with clear-sky fluxes -- the LW fluxes bit for bit against the composed oracle (gas optics, two-stream cloud optics by
band, the -- sampled -- increment of (tau, 0, 0), the rescaled solver; the clear set: the no-scattering solver); a
captured graph replayed twice with lwp changed in between against fresh eager steps; the refusals; and the SW fluxes and
the default step's fluxes as without the option."""
import numpy as np
import pytest

import mcica_ref as M

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
FLUX = ("lw_up", "lw_dn", "sw_up", "sw_dn", "sw_dir")
MODES = ("overcast", "mcica", "clrsky", "mcica_clrsky")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a device"
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def case(rfmip, orc):
    """12 columns, the all-sky example's clouds, a cloud fraction, overlap parameter and random numbers; the oracle's gas
    optics and cloud optics, computed once."""
    from conftest import subset
    from rrtmgpnn import data
    prob = subset(rfmip, np.arange(7, 1800, 150))
    ncol, nlay = prob["ncol"], prob["nlay"]
    kl, ks = data.load_kdist("lw"), data.load_kdist("sw")
    clouds = data.allsky_clouds(prob, data.load_cloud_optics("lw"))
    cloudy = (clouds[0] > 0) | (clouds[1] > 0)
    assert cloudy.any()
    rng = np.random.default_rng(63)
    cf = np.where(cloudy, rng.uniform(0.2, 0.9, cloudy.shape), 0).astype(np.float32)
    ov = rng.uniform(-1, 1, (ncol, nlay - 1)).astype(np.float32)
    r_lw = rng.random((ncol, nlay, kl["ngpt"]), dtype=np.float32)
    r_sw = rng.random((ncol, nlay, ks["ngpt"]), dtype=np.float32)
    go = orc.lw_gas_optics(prob, [data.load_model("lw_abs"), data.load_model("lw_pfrac")], kl)
    return dict(prob=prob, clouds=clouds, cf=cf, ov=ov, r_lw=r_lw, r_sw=r_sw, go=go, kl=kl)


def _kwargs(c, mode, clouds=None):
    kw = {"clouds": c["clouds"] if clouds is None else clouds}
    if mode.startswith("mcica"):
        kw["mcica"] = {"cloud_frac": c["cf"], "overlap_param": c["ov"], "randoms_lw": c["r_lw"], "randoms_sw": c["r_sw"]}
        if mode == "mcica_clrsky":
            kw["mcica"]["clrsky"] = True
    elif mode == "clrsky":
        kw["clrsky"] = True
    return kw


def _ident(ng):
    return np.stack([np.arange(1, ng + 1)] * 2, axis=1).astype(np.int32)


def _lw_oracle(orc, c, mode, clouds=None):
    """The composed oracle's LW fluxes: lw_up / lw_dn under scattering clouds, and the clear set."""
    from rrtmgpnn import data
    prob, go, kl = c["prob"], c["go"], c["kl"]
    ng = go["tau"].shape[-1]
    cld = orc.cloud_optics(data.load_cloud_optics("lw"), *(c["clouds"] if clouds is None else clouds), nstr=2, lut=True,
                           icergh=2)
    z = np.zeros_like(go["tau"])
    if mode.startswith("mcica"):
        mask = M.sampled_mask(c["r_lw"], c["cf"], c["ov"])
        io = orc.increment_bybnd(_ident(ng), (go["tau"], z, z), [M.draw(mask, a, kl["band_lims_gpt"]) for a in cld])
    else:
        io = orc.increment_bybnd(kl["band_lims_gpt"], (go["tau"], z, z), cld)
    emis = np.repeat(np.asarray(prob["sfc_emis"], np.float32)[:, None], ng, axis=1)
    src = (go["lay_source"], go["lev_source"], emis, go["sfc_source"], prob["top_at_1"], 1)
    out = {}
    out["lw_up"], out["lw_dn"] = orc.lw_solver(io[0], *src, ssa=io[1], g=io[2])
    out["lw_up_clr"], out["lw_dn_clr"] = orc.lw_solver(go["tau"], *src)
    return out


def _poison(step):
    for k in FLUX:
        getattr(step, k).fill_(float("nan"))
        if step.clrsky:
            getattr(step, k + "_clr").fill_(float("nan"))


def _outputs(step):
    torch.cuda.synchronize()
    out = dict(step.fluxes())
    if step.clrsky:
        out.update(step.clrsky_fluxes())
    return out


def _run(step):
    _poison(step)
    step.step()
    return _outputs(step)


def _equal(got, want, what, keys):
    for k in keys:
        np.testing.assert_array_equal(got[k], want[k], err_msg="%s %s" % (what, k))


@pytest.mark.parametrize("mode", MODES)
def test_step_with_lw_scattering(dev, orc, case, mode):
    from rrtmgpnn import _lib
    from rrtmgpnn.pipeline import ClearSkyStep
    c, L = case, _lib.lib()
    prob = c["prob"]
    clr = mode.endswith("clrsky")
    lw_keys = ("lw_up", "lw_dn") + (("lw_up_clr", "lw_dn_clr") if clr else ())
    step = ClearSkyStep(prob, device=0, lw_scattering=True, **_kwargs(c, mode))
    names = [n for n, _, _ in step.calls]
    fns = {n: f for n, f, _ in step.calls}
    assert fns["lw_solver"] is L.rrtmgpnn_lw_solver_1rescl_planck_inc
    assert not [n for n in names if n.startswith("increment") or n.startswith("draw_samples")]
    if mode.startswith("mcica"):  # the mask request right before the all-sky solver, after the clear launch
        assert names.index("lw_mask") == names.index("lw_solver") - 1
    if clr:
        assert fns["lw_solver_clr"] is L.rrtmgpnn_lw_solver_noscat_planck
        assert names.index("predict_nn_lw") < names.index("lw_solver_clr") < names.index("lw_solver")
        assert "lw_mask" not in names or names.index("lw_solver_clr") < names.index("lw_mask")
    assert step.cld_ssa_lw.shape == step.cld_tau_lw.shape == step.cld_g_lw.shape
    eager = _run(step)
    want = _lw_oracle(orc, c, mode)
    _equal(eager, want, "fused eager against the oracle:", lw_keys)
    # the default step: its LW fluxes are those of absorbing clouds, its SW fluxes this step's
    plain = ClearSkyStep(prob, device=0, **_kwargs(c, mode))
    assert not hasattr(plain, "cld_ssa_lw")
    base = _run(plain)
    plain.close()
    sw_keys = tuple(k for k in base if k.startswith("sw"))
    _equal(eager, base, "the SW fluxes beside the default step's:", sw_keys)
    assert (eager["lw_dn"] != base["lw_dn"]).any() and (eager["lw_up"] != base["lw_up"]).any(), "scattering does not show"
    if clr:
        _equal(eager, base, "the clear LW set beside the default step's:", ("lw_up_clr", "lw_dn_clr"))
    # a captured graph, replayed twice with lwp changed in between
    step.capture()
    _poison(step)
    step.replay()
    _equal(_outputs(step), eager, "captured against eager:", tuple(eager))
    clouds_b = (c["clouds"][0] * np.float32(0.5),) + tuple(c["clouds"][1:])
    step.lwp.copy_(torch.as_tensor(np.array(clouds_b[0], np.float32), device=dev))
    torch.cuda.synchronize()
    _poison(step)
    step.replay()
    again = _outputs(step)
    step.close()
    _equal(again, _lw_oracle(orc, c, mode, clouds_b), "replay after a new lwp against the oracle:", lw_keys)
    assert (again["lw_dn"] != eager["lw_dn"]).any()


def test_default_step_is_unchanged(dev, orc, case):
    """lw_scattering=False is the default and the step of before: absorbing clouds against the composed oracle."""
    from rrtmgpnn import data
    from rrtmgpnn.pipeline import ClearSkyStep
    c = case
    a = ClearSkyStep(c["prob"], device=0, clouds=c["clouds"])
    b = ClearSkyStep(c["prob"], device=0, clouds=c["clouds"], lw_scattering=False)
    assert [(n, f) for n, f, _ in a.calls] == [(n, f) for n, f, _ in b.calls]
    fa, fb = _run(a), _run(b)
    a.close()
    b.close()
    _equal(fa, fb, "default against lw_scattering=False:", FLUX)
    go, kl = c["go"], c["kl"]
    (ct,) = orc.cloud_optics(data.load_cloud_optics("lw"), *c["clouds"], nstr=1, lut=True, icergh=2)
    (tau,) = orc.increment_bybnd(kl["band_lims_gpt"], (go["tau"],), (ct,))
    emis = np.repeat(np.asarray(c["prob"]["sfc_emis"], np.float32)[:, None], go["tau"].shape[-1], axis=1)
    up, dn = orc.lw_solver(tau, go["lay_source"], go["lev_source"], emis, go["sfc_source"], c["prob"]["top_at_1"], 1)
    np.testing.assert_array_equal(fa["lw_up"], up)
    np.testing.assert_array_equal(fa["lw_dn"], dn)


def test_step_refusals(dev, case):
    from rrtmgpnn.pipeline import ClearSkyStep
    from rrtmgpnn import data
    c = case
    nb_lw, nb_sw = data.load_kdist("lw")["nband"], data.load_kdist("sw")["nband"]
    ncol, nlay = c["prob"]["ncol"], c["prob"]["nlay"]
    aer = {"lw_tau": np.zeros((ncol, nlay, nb_lw), np.float32), "sw_tau": np.zeros((ncol, nlay, nb_sw), np.float32),
           "sw_ssa": np.zeros((ncol, nlay, nb_sw), np.float32), "sw_g": np.zeros((ncol, nlay, nb_sw), np.float32)}
    mc = {"cloud_frac": c["cf"], "overlap_param": None, "randoms_lw": c["r_lw"], "randoms_sw": c["r_sw"], "byband": True}
    for kw in ({"clouds": c["clouds"], "fused": False}, {"clouds": c["clouds"], "byband": True},
               {"clouds": c["clouds"], "mcica": mc}, {"clouds": c["clouds"], "jacobian": True},
               {"clouds": c["clouds"], "aerosols": aer}, {}):
        with pytest.raises(ValueError, match="lw_scattering"):
            ClearSkyStep(c["prob"], device=0, lw_scattering=True, **kw)
