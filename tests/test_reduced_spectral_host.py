"""CPU: the reduced-resolution spectral configuration (the 2021 networks: LW g128, SW g112) on the host side -- the four
model fixtures through the native reader, the surrogate k-distribution tables of tools/make_reduced_kdist.py, and the
oracle pinned to the reference Fortran on these models (what lets tests/test_gpu_reduced_spectral.py trust the oracle at
these shapes).  ClearSkyStep(spectral=None) against the committed step plans needs a device context and stands with the
GPU tests (test_gpu_reduced_spectral.py::test_spectral_none_plans_equal_the_goldens)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import subset  # (run as a program: tests/ is the script's directory)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES = os.path.join(ROOT, "tests", "golden", "reference_files")
LW_ABS = os.path.join(FILES, "lw-g128-210809_absorption_BEST.nc")
LW_PFRAC = os.path.join(FILES, "lw-g128-210809_planck_frac_BEST.nc")
SW_ABS = os.path.join(FILES, "sw-g112-210809_absorption_BEST.nc")
SW_RAY = os.path.join(FILES, "sw-g112-210809_rayleigh_BEST.nc")
LW_NAMES = ["tlay", "play", "h2o", "o3", "co2", "ch4", "n2o", "cfc11", "cfc12", "co", "ccl4", "cfc22", "hfc143a",
            "hfc125", "hfc23", "hfc32", "hfc134a", "cf4"]
SW_NAMES = ["tlay", "play", "h2o", "o3", "co2", "n2o", "ch4"]
MODELS = ((LW_ABS, [18, 72, 72, 128], LW_NAMES, True), (LW_PFRAC, [18, 24, 24, 128], LW_NAMES, False),
          (SW_ABS, [7, 32, 32, 112], SW_NAMES, True), (SW_RAY, [7, 32, 32, 112], SW_NAMES, True))
REF_SO = os.path.join(ROOT, "oracle", "_ref", "librrtmgp_ref.so")


@pytest.mark.parametrize("path,dims,names,scaled", MODELS, ids=[os.path.basename(m[0]) for m in MODELS])
def test_fixture_loads_natively(path, dims, names, scaled):
    from rrtmgpnn import data, ncio, rbin
    assert os.path.getsize(path) < 1 << 20
    with ncio.DataFile(path) as f:
        assert [int(f.read("nn_input_coeffs_min").size)] + [int(v) for v in f.read("nn_dimsize")] == dims
        assert f.strings("nn_activation_char") == ["softsign", "softsign", "linear"]
        assert f.strings("nn_inputs_char") == names
        assert ("nn_output_coeffs_mean" in f) == scaled
        w3 = f.read("nn_weights_3", np.float32)
    m = data.load_model(path)
    assert [int(v) for v in m["dims"]] == dims and [int(v) for v in m["activation"]] == [1, 1, 0]
    assert rbin.unchars(m["input_names"]) == names
    assert m["w3"].shape == (dims[2], dims[3]) and m["w3"].dtype == np.float32
    np.testing.assert_array_equal(m["w3"], w3)
    assert ("output_mean" in m) == scaled and ("output_std" in m) == scaled
    # the same dict as the class layer holds: one mapping (ncio.read_model) behind both
    want = ncio.read_model(path)
    assert list(m) == list(want)
    for k in want:
        np.testing.assert_array_equal(m[k], want[k], err_msg=k)


def test_load_model_is_the_network_class_mapping():
    """RrtmgpNetwork.load_netcdf and data.load_model read a model through the same function."""
    import inspect
    from rrtmgpnn import api, data
    assert "ncio.read_model(" in inspect.getsource(api.RrtmgpNetwork.load_netcdf)
    assert "ncio.read_model(" in inspect.getsource(data.load_model)
    assert "nn_weights" not in inspect.getsource(api.RrtmgpNetwork.load_netcdf)
    # the shipped models still come from their RBIN files, by key
    assert [int(v) for v in data.load_model("lw_abs")["dims"]] == [18, 58, 58, 256]


def test_reduced_kdist_invariants():
    from rrtmgpnn import data
    for which, ngpt, nband in (("lw", 128, 16), ("sw", 112, 14)):
        full, red = data.load_kdist(which), data.load_kdist(which, ngpt)
        lims = red["band_lims_gpt"]
        assert red["ngpt"] == ngpt and red["nband"] == nband == full["nband"] and lims.dtype == np.int32
        assert lims[0, 0] == 1 and lims[-1, 1] == ngpt
        np.testing.assert_array_equal(lims[1:, 0], lims[:-1, 1] + 1)  # contiguous
        np.testing.assert_array_equal(lims[:, 1] - lims[:, 0] + 1, 8)  # 8 per band
        for k in ("band_lims_wvn", "temp_ref_min", "temp_ref_max", "press_ref_min"):
            np.testing.assert_array_equal(red[k].view(np.uint32), full[k].view(np.uint32), err_msg=k)
        assert list(red) == list(full)
    lw, lw_full = data.load_kdist("lw", 128), data.load_kdist("lw")
    np.testing.assert_array_equal(lw["totplnk"].view(np.uint32), lw_full["totplnk"].view(np.uint32))
    assert lw["totplnk_delta"] == lw_full["totplnk_delta"] and lw["nPlanckTemp"] == lw_full["nPlanckTemp"]
    s112, s224 = data.load_kdist("sw", 112)["solar_source"], data.load_kdist("sw")["solar_source"]
    assert s112.shape == (112,) and s112.dtype == np.float32
    for b in range(14):
        for i in range(8):
            assert s112[8 * b + i] == np.float32(s224[16 * b + 2 * i] + s224[16 * b + 2 * i + 1])
    # The two totals are float32 sums in index order of the same 224 terms, grouped differently.  Every float32 add
    # rounds by at most half an ulp of its result, which is at most the total: 223 adds on one side, 112 + 111 on the
    # other, so the totals differ by at most 223 ulp(total); against the exact (float64) sum each is within half of it.
    # Observed: 1364.2382 (g112) and 1364.2363 (g224), 16 ulp apart; the float64 sum of the 224 terms lies between.
    t112, t224 = data.seqsum(s112)[()], data.seqsum(s224)[()]
    ulp = np.spacing(np.float32(max(t112, t224)))
    print("solar source totals: g112 %.7g g224 %.7g, %.1f ulp apart" % (t112, t224, abs(float(t112) - float(t224)) / ulp))
    assert abs(float(t112) - float(t224)) <= 223 * float(ulp)
    exact = float(np.sum(s224.astype(np.float64)))
    assert abs(float(t112) - exact) <= 111.5 * float(ulp) and abs(float(t224) - exact) <= 111.5 * float(ulp)


def test_load_kdist_refuses_other_grids():
    from rrtmgpnn import data
    assert data.load_kdist("lw", None)["ngpt"] == 256 and data.load_kdist("sw")["ngpt"] == 224
    for which, ngpt in (("lw", 112), ("sw", 128), ("lw", 256), ("sw", 224), ("lw", 64), ("sw", 0)):
        with pytest.raises(ValueError):
            data.load_kdist(which, ngpt)


def test_generator_reproduces_the_committed_tables(tmp_path):
    from rrtmgpnn import data
    assert not [f for f in os.listdir(data.DATA_DIR) if "g128.rbin" in f and f.startswith("kdist")]
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_reduced_kdist.py"), str(tmp_path)], check=True)
    for name in ("kdist_lw_g128.rbin", "kdist_sw_g112.rbin"):
        with open(os.path.join(str(tmp_path), name), "rb") as a, open(os.path.join(ROOT, "tests", "golden", name), "rb") as b:
            assert a.read() == b.read(), name
    # ... and they are the tables load_kdist forms in memory
    from rrtmgpnn import rbin
    for which, ngpt, name in (("lw", 128, "kdist_lw_g128.rbin"), ("sw", 112, "kdist_sw_g112.rbin")):
        kd = data.load_kdist(which, ngpt)
        for k, v in rbin.read(os.path.join(ROOT, "tests", "golden", name)).items():
            assert v.dtype == kd[k].dtype and v.tobytes() == kd[k].tobytes(), (name, k)


def pin_to_reference():
    """60 RFMIP columns (every 30th): oracle == reference Fortran on the four reduced-resolution networks (MLP) and on
    the clear-sky fluxes with the reduced tables (rte_lw, rte_sw), bit for bit."""
    import oracle as O
    from rrtmgpnn import data
    orc, ref = O.Oracle(), O.Reference()
    kd, kds = data.load_kdist("lw", 128), data.load_kdist("sw", 112)
    lw = [data.load_model(LW_ABS), data.load_model(LW_PFRAC)]
    sw = [data.load_model(SW_ABS), data.load_model(SW_RAY)]
    prob = subset(data.rfmip_problem(), np.arange(0, 1800, 30))
    assert prob["ncol"] == 60
    up, dn, go = orc.clear_sky_lw(prob, lw, kd)
    assert go["tau"].shape == (60, 60, 128)
    x = go["nn_inputs"].reshape(-1, 18)
    for m in lw:
        np.testing.assert_array_equal(orc.mlp(m, x).view(np.uint32), ref.mlp(m, x).view(np.uint32))
    emis_band = np.repeat(prob["sfc_emis"][:, None], 16, axis=1)
    ur, dr_ = ref.rte_lw(kd, go["tau"], go["lay_source"], go["lev_source"], go["sfc_source"], go["sfc_source_Jac"],
                         emis_band, True, 1)
    np.testing.assert_array_equal(up.view(np.uint32), ur.view(np.uint32))
    np.testing.assert_array_equal(dn.view(np.uint32), dr_.view(np.uint32))
    ups, dns, drs, gs = orc.clear_sky_sw(prob, sw, kds)
    assert gs["tau"].shape == (60, 60, 112)
    xs = gs["nn_inputs"].reshape(-1, 7)
    for m in sw:
        np.testing.assert_array_equal(orc.mlp(m, xs).view(np.uint32), ref.mlp(m, xs).view(np.uint32))
    toa = data.toa_flux(prob, kds)
    alb = np.repeat(prob["sfc_alb"][:, None], 112, axis=1)
    u2, d2, r2 = ref.rte_sw(kds, gs["tau"], gs["ssa"], gs["g"], prob["mu0"], toa, alb, alb, True)
    m = ~prob["usecol"]
    assert m.any() and (~m).any()
    u2[m] = 0
    d2[m] = 0
    np.testing.assert_array_equal(ups.view(np.uint32), u2.view(np.uint32))
    np.testing.assert_array_equal(dns.view(np.uint32), d2.view(np.uint32))
    np.testing.assert_array_equal(drs.view(np.uint32), r2.view(np.uint32))
    print("reduced models: oracle == reference, bit for bit")


@pytest.mark.skipif(not os.path.exists(REF_SO), reason="reference oracle (oracle/_ref) not built")
def test_oracle_bitwise_vs_reference_reduced_models():
    """pin_to_reference() in an interpreter of its own.  The reference's sw_solver_2stream declares `logical ::
    save_gpt_flux = .false.` (rte/kernels/mo_rte_solver_kernels.F90:567), an initialised and so saved local: once any
    call in a process asked for g-point fluxes (tests/test_oracle.py does), every later plain rte_sw in that process
    dereferences its absent g-point arguments.  The pin below needs plain rte_sw, so it does not share a process with
    the other reference tests."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "bit for bit" in r.stdout


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(ROOT, "rte-rrtmgp-nn_amd"))
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    pin_to_reference()
