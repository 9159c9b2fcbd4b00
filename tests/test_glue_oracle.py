"""CPU tests of the oracle's gas-optics glue: compute_nn_inputs, get_col_dry, the output scaling, the Planck source,
the tlev interpolation and the single-model ("both") split.

The modules holding this glue (mod_network_rrtmgp, mo_gas_optics_rrtmgp, mo_gas_optics_kernels) `use netcdf`
unconditionally and cannot be built here, so the glue is pinned by
  * the one execution of the reference's glue on record: the SURVEY.md section 0.4 probe, which ran the reference's
    own compute_nn_inputs -> get_col_dry -> predict_nn_{lw,sw}_blas -> compute_Planck_source_nn -> rte_{lw,sw} on
    RFMIP expt 1 (column 0 below) and printed five fluxes to two decimals.  The SW harness of that probe used a
    flat solar_source (one value for every g-point, renormalised to the column's TSI), not the 5778 K blackbody
    surrogate the build ships: with a flat source the restatement reproduces all five printed values;
  * operation-by-operation restatements in numpy float32 of the Fortran expressions (tlev, the "both" split); the
    Planck source's own (interpolate1D and compute_Planck_source_nn, at every table and temperature edge, with a
    float64 reference beside it) is planck_edges.planck_source_f32, held in tests/test_planck_edges_host.py.
"""
import numpy as np
import pytest

from conftest import subset

# reference execution on RFMIP expt 1, column 0 (W/m2, printed to 2 decimals)
PROBE = {"lw_toa_up": 289.75, "lw_sfc_dn": 339.35, "sw_toa_dn": 757.35, "sw_toa_up": 56.82, "sw_sfc_dn": 225.74}
PROBE_TOL = 6e-3  # half a unit of the printed last digit, plus float32 noise


@pytest.fixture(scope="module")
def models():
    from rrtmgpnn import data
    return {k: data.load_model(k) for k in ("lw_abs", "lw_pfrac", "sw_abs", "sw_ray", "lw_g128_both")}


def test_lw_glue_reproduces_reference_probe(orc, rfmip, models):
    from rrtmgpnn import data
    prob = subset(rfmip, [0])
    up, dn, _ = orc.clear_sky_lw(prob, [models["lw_abs"], models["lw_pfrac"]], data.load_kdist("lw"))
    assert abs(float(up[0, 0]) - PROBE["lw_toa_up"]) <= PROBE_TOL, float(up[0, 0])
    assert abs(float(dn[0, -1]) - PROBE["lw_sfc_dn"]) <= PROBE_TOL, float(dn[0, -1])


def test_sw_glue_reproduces_reference_probe_with_flat_solar_source(orc, rfmip, models):
    from rrtmgpnn import data
    prob = subset(rfmip, [0])
    kd = dict(data.load_kdist("sw"))
    kd["solar_source"] = np.ones(224, np.float32)  # the probe harness's source (see module docstring)
    up, dn, _, _ = orc.clear_sky_sw(prob, [models["sw_abs"], models["sw_ray"]], kd)
    assert abs(float(dn[0, 0]) - PROBE["sw_toa_dn"]) <= PROBE_TOL, float(dn[0, 0])
    assert abs(float(up[0, 0]) - PROBE["sw_toa_up"]) <= PROBE_TOL, float(up[0, 0])
    assert abs(float(dn[0, -1]) - PROBE["sw_sfc_dn"]) <= PROBE_TOL, float(dn[0, -1])
    # with the shipped blackbody surrogate only TOA down (set by mu0 and TSI alone) is the probe's
    up2, dn2, _, _ = orc.clear_sky_sw(prob, [models["sw_abs"], models["sw_ray"]], data.load_kdist("sw"))
    assert abs(float(dn2[0, 0]) - PROBE["sw_toa_dn"]) <= PROBE_TOL
    assert abs(float(up2[0, 0]) - PROBE["sw_toa_up"]) > 1.0


def _tlev_numpy(play, plev, tlay):
    """rrtmgp/mo_gas_optics_rrtmgp.F90:327-334 in numpy float32, one Fortran operation per numpy operation."""
    pa, pv, ta = (np.asarray(a, np.float32) for a in (play, plev, tlay))
    nlay = pa.shape[1]
    out = np.empty((pa.shape[0], nlay + 1), np.float32)
    out[:, 0] = ta[:, 0] + ((pv[:, 0] - pa[:, 0]) * (ta[:, 1] - ta[:, 0])) / (pa[:, 1] - pa[:, 0])
    a, b = pa[:, :-1], pa[:, 1:]
    out[:, 1:nlay] = ((a * ta[:, :-1]) * (pv[:, 1:nlay] - b) + (b * ta[:, 1:]) * (a - pv[:, 1:nlay])) / \
        (pv[:, 1:nlay] * (a - b))
    out[:, nlay] = ta[:, -1] + ((pv[:, nlay] - pa[:, -1]) * (ta[:, -1] - ta[:, -2])) / (pa[:, -1] - pa[:, -2])
    return out


@pytest.mark.parametrize("flip", [False, True])
def test_tlev_interpolation_restatement(orc, rfmip, flip):
    prob = subset(rfmip, np.arange(0, 1800, 5))
    play, plev, tlay = prob["play"], prob["plev"], prob["tlay"]
    if flip:
        play, plev, tlay = play[:, ::-1], plev[:, ::-1], tlay[:, ::-1]
    got = orc.interpolate_tlev(play, plev, tlay)
    np.testing.assert_array_equal(got, _tlev_numpy(play, plev, tlay))
    # property: inside the column the pressure-weighted interpolation stays close to the file's own level
    # temperatures (RFMIP gives both); the ends (extrapolated, or next to the 1 Pa top) differ more
    ref = prob["tlev"][:, ::-1] if flip else prob["tlev"]
    inner = slice(2, -2)
    assert float(np.max(np.abs(got[:, inner] - ref[:, inner]))) < 6.0
    assert float(np.median(np.abs(got[:, 1:-1] - ref[:, 1:-1]))) < 0.5


def test_both_split_restatement(orc, models):
    m = models["lw_g128_both"]
    ngpt = int(m["dims"][-1]) // 2
    rng = np.random.default_rng(3)
    x = rng.uniform(0, 1, size=(500, int(m["dims"][0]))).astype(np.float32)
    y = orc.mlp(m, x)
    cd = rng.uniform(1e20, 1e24, size=500).astype(np.float32)
    tau, pf = orc.both_post(m, y, cd)
    sd, mn = np.asarray(m["output_std"], np.float32)[:ngpt], np.asarray(m["output_mean"], np.float32)[:ngpt]
    t = sd * y[:, :ngpt]
    t = t + mn
    t2 = t * t
    t4 = t2 * t2
    np.testing.assert_array_equal(tau, (t4 * t4) * cd[:, None])
    np.testing.assert_array_equal(pf, y[:, ngpt:] * y[:, ngpt:])


def test_user_col_dry_is_honoured(orc, rfmip, models):
    # quirk B-3 fixed: an explicit col_dry replaces get_col_dry's; tau scales with it exactly (one product per element)
    from rrtmgpnn import data
    prob = subset(rfmip, np.arange(0, 1800, 97))
    kd = data.load_kdist("lw")
    base = orc.lw_gas_optics(prob, [models["lw_abs"], models["lw_pfrac"]], kd)
    cd = (base["col_dry"] * np.float32(2.0)).astype(np.float32)
    go = orc.lw_gas_optics(prob, [models["lw_abs"], models["lw_pfrac"]], kd, col_dry=cd)
    np.testing.assert_array_equal(go["tau"], base["tau"] * np.float32(2.0))
    np.testing.assert_array_equal(go["pfrac"], base["pfrac"])


def test_scalar_and_1d_gases_equal_their_2d_expansion(orc, rfmip, models):
    # compute_nn_inputs (:724-753): a scalar or (nlay) concentration reads as the (nlay, ncol) field it stands for
    prob = subset(rfmip, np.arange(0, 1800, 101))
    ncol, nlay = prob["ncol"], prob["nlay"]
    g2 = dict(prob["gases"])
    g2["co2"] = np.full((ncol, nlay), 4.1e-4, np.float32)
    g2["ch4"] = np.repeat(np.linspace(1.6e-6, 1.9e-6, nlay, dtype=np.float32)[None], ncol, axis=0)
    g1 = dict(prob["gases"])
    g1["co2"] = np.float32(4.1e-4)
    g1["ch4"] = np.linspace(1.6e-6, 1.9e-6, nlay, dtype=np.float32)
    a = orc.nn_inputs(prob["play"], prob["tlay"], g2, models["lw_abs"])
    b = orc.nn_inputs(prob["play"], prob["tlay"], g1, models["lw_abs"])
    np.testing.assert_array_equal(a, b)
