"""CPU: compute_bc (extensions/mo_compute_bc.F90) -- the comparator's solver half against the reference's own rte_lw /
rte_sw at nlay = 1, the class layer's refusals with the reference's strings, the two entries in the built library, and
the fixture of the upper_bc=True step plans."""
import ctypes
import json
import os

import numpy as np
import pytest

import compute_bc_ref as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOO_CLOSE = "compute_bc: pressures are too close to (or less than) min in gas optics "


def test_comparator_solver_half_is_the_reference_at_one_layer(orc, rfmip, tmp_path):
    """rte_lw and rte_sw of the reference on the one-layer problem's optical properties and sources, g-point outputs
    (ty_fluxes_flexible), both orientations: every level of the comparator's solver call, bit for bit.  The reference
    runs in a process of its own (compute_bc_ref.reference_main says why)."""
    import subprocess
    import sys
    import oracle as O
    if not os.path.exists(O.REF_SO):
        pytest.skip("reference library not built (oracle/_ref)")
    src, want, probs = {"tags": np.array(["t1", "tN"])}, {}, {}
    for tag, top_at_1 in (("t1", True), ("tN", False)):
        prob = probs[tag] = B.truncated(rfmip, B.COLS["c7"], 1, 2, top_at_1)
        kd, go = B.lw_solver_inputs(orc, prob)
        kds, gs, inc = B.sw_solver_inputs(orc, prob)
        ncol, _, ngpt = go["tau"].shape
        for nmus in (1, 3):
            want[tag, "lw%d" % nmus] = orc.lw_solver(go["tau"], go["lay_source"], go["lev_source"],
                                                     np.ones((ncol, ngpt), np.float32), go["sfc_source"], top_at_1, nmus,
                                                     gpt=True)
        ones = np.ones_like(inc)
        want[tag, "sw"] = orc.sw_solver(gs["tau"], gs["ssa"], gs["g"], prob["mu0"], inc, ones, ones, top_at_1, gpt=True)
        src.update({tag + "_" + k: v for k, v in dict(
            top_at_1=np.array(top_at_1), lw_tau=go["tau"], lay=go["lay_source"], lev=go["lev_source"],
            sfc=go["sfc_source"], jac=go["sfc_source_Jac"], sw_tau=gs["tau"], ssa=gs["ssa"], g=gs["g"],
            mu0=prob["mu0"], inc=inc).items()})
    fin, fout = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(fin, **src)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "compute_bc_ref.py"), fin, fout],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.load(fout)
    for (tag, what), arrays in want.items():
        for i, a in enumerate(arrays):
            np.testing.assert_array_equal(a, got["%s_%s_%d" % (tag, what, i)], err_msg="%s %s output %d" % (tag, what, i))
    for tag, prob in probs.items():
        bottom = 1 if prob["top_at_1"] else 0
        for nmus in (1, 3):
            np.testing.assert_array_equal(B.lw(orc, prob, nmus), got["%s_lw%d_3" % (tag, nmus)][:, bottom])
        np.testing.assert_array_equal(B.sw(orc, prob), got["%s_sw_5" % tag][:, bottom])


def test_comparator_values(orc, rfmip):
    """Finite, not negative, and at one angle a radiance: its g-point sum times pi is the broadband flux of the same
    solve (the solver's fac is 2 pi * 0.5)."""
    for top_at_1 in (True, False):
        prob = B.truncated(rfmip, B.COLS["c7"], 3, 5, top_at_1)
        radn = B.lw(orc, prob)
        assert np.isfinite(radn).all() and (radn >= 0).all() and (radn.max(axis=1) > 0).all()
        flux = B.in_flux_units(radn)
        np.testing.assert_array_equal(flux, (np.float32(2) * np.float32(np.pi) * np.float32(0.5) * radn))
        kd, go = B.lw_solver_inputs(orc, prob)
        ones = np.ones(go["sfc_source"].shape, np.float32)
        dn = orc.lw_solver(go["tau"], go["lay_source"], go["lev_source"], ones, go["sfc_source"], top_at_1)[1]
        np.testing.assert_allclose(flux.astype(np.float64).sum(axis=1), dn[:, 1 if top_at_1 else 0], rtol=1e-5)
        assert 0.05 < dn[:, 1 if top_at_1 else 0].min() and dn.max() < 20.0  # W/m2: a thin layer near the model top
        beam = B.sw(orc, prob)
        assert np.isfinite(beam).all() and (beam >= 0).all() and (beam.max(axis=1) > 0).all()


def _class_args(prob, which):
    """compute_bc's arguments on host tensors: every refusal returns before anything touches a device."""
    torch = pytest.importorskip("torch")
    from rrtmgpnn import api
    kd = api.GasOpticsRRTMGP()
    assert kd.load(which, device="cpu") == ""
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32))  # noqa: E731
    ncol = prob["play"].shape[0]
    return kd, t(prob["play"]), t(prob["plev"]), t(prob["tlay"]), torch.empty((ncol, kd.get_ngpt()))


def test_class_layer_refusals(rfmip):
    from conftest import subset
    from rrtmgpnn.compute_bc import compute_bc, pressure_check
    full = subset(rfmip, B.COLS["c7"])
    kd, play, plev, tlay, out = _class_args(full, "lw")
    # RFMIP's own top level is press_ref_min + eps: refused as the reference would
    assert compute_bc(kd, play, plev, tlay, None, out) == TOO_CLOSE
    # reversed, the check reads plev(:, nlay), the second level from the top (20 Pa), and passes: the next check speaks
    fl = B.flip(full)
    kd, fplay, fplev, ftlay, out = _class_args(fl, "lw")
    assert compute_bc(kd, fplay, fplev, ftlay, None, out).startswith("gas_optics(): the lookup-table branch")
    assert compute_bc(kd, play, plev[:, :-1], tlay, None, out) == "compute_bc: array plev has wrong dimensions"
    assert compute_bc(kd, play, plev, tlay[:, 1:], None, out) == "compute_bc: array tlay has wrong dimensions"
    assert compute_bc(kd, play, plev, tlay, None, out, mu0=tlay[:3, 0]) == "compute bc: array mu0 has wrong dimensions"
    trunc = B.truncated(rfmip, B.COLS["c7"], 1, 2)
    kds, play, plev, tlay, out = _class_args(trunc, "sw")
    assert compute_bc(kds, play, plev, tlay, None, out) == "compute_bc: have to supply mu0 for solar calculations"
    pmin = np.float32(kd.get_press_min())
    sp = np.nextafter(pmin, np.float32(np.inf)) - pmin
    assert pressure_check([pmin + np.float32(2) * sp], pmin) == TOO_CLOSE
    assert pressure_check([pmin + np.float32(3) * sp, 20.0], pmin) == ""


def test_library_exports_both_entries():
    from rrtmgpnn import _lib
    h = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("rrtmgpnn_compute_bc_lw", "rrtmgpnn_compute_bc_sw"):
        assert hasattr(h, name), name
        assert name in _lib.SIGNATURES
    L = _lib.lib()
    assert L.rrtmgpnn_compute_bc_lw(None, 1, 1, 256, 18, 1, 1.0, *([None] * 7), 2, 16, 196, None, 160.0, 1.0, None, 1,
                                    None, None, 0, None) != 0
    assert b"null context" in L.rrtmgpnn_last_error()


def test_step_plan_fixture_holds_the_cases():
    """tests/golden/step_plan_upper_bc.json has exactly the cases of tests/step_plan_upper_bc.py; in every plan the
    boundary call stands ahead of the LW network, issued on the LW stream in flux units at the step's angles, and every
    LW solver call takes the step's lw_inc_flux as inc_flux; no SW call mentions it."""
    import step_plan_upper_bc as PU
    with open(os.path.join(ROOT, "tests", "golden", "step_plan_upper_bc.json")) as f:
        golden = json.load(f)
    assert sorted(golden) == sorted(k for k, _ in PU.CASES)
    assert {k for k, v in golden.items() if "raises" in v} == {k for k, _ in PU.CASES if k.startswith("refused-")}
    for k, v in golden.items():
        if "raises" in v:
            assert v == {"raises": "ValueError", "message": TOO_CLOSE}, k
            continue
        names = [c.split()[0] for c in v["calls"]]
        assert names.count("lw_upper_bc") == 1, k
        assert names.index("lw_upper_bc") < names.index("predict_nn_lw"), k
        assert v["buffers"]["lw_inc_flux"] == [[4, 256], "float32"], k
        for c in v["calls"]:
            name, entry, stream = c.split(":")[0].split()
            args = c.split(": ", 1)[1].split(", ")
            if name == "lw_upper_bc":
                assert entry == "rrtmgpnn_compute_bc_lw" and stream == "lw", k
                assert args[-1] == "lw_inc_flux" and args[-2] == "1", k  # as_flux
            elif name in ("lw_solver", "lw_solver_clr"):
                assert args[8] == "lw_inc_flux", (k, c)
            else:
                assert "lw_inc_flux" not in c, (k, c)
