"""CPU: the compact McICA mask entries are declared, bound and exported; their restatement (one column at a time, from
the source column's own inputs and global counter word) is the full mask's rows at idx[:nday]; the expected values of
tests/test_gpu_mcica_daylit_step.py hold on the oracle alone -- sampled clouds behind an aerosol on the daylit columns
by themselves, scattered with zeros, are the same on every column with the driver's zeroing
(rrtmgp_rfmip_sw.F90:456-463) -- and the step's refusals come before any device object exists."""
import ctypes
import os
import re

import numpy as np
import pytest

import mcica_daylit_cases as C
import mcica_ref as M
import philox_ref as P
from conftest import subset
from test_daylit_host import scattered

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# entry -> number of arguments
NEW = {"rrtmgpnn_sampled_mask_max_ran_active": 9, "rrtmgpnn_sampled_mask_exp_ran_active": 10,
       "rrtmgpnn_sampled_mask_max_ran_seeded_active": 9, "rrtmgpnn_sampled_mask_exp_ran_seeded_active": 10}
COLS = np.arange(3, 1800, 45)  # day and night columns (tests/test_night_columns_host.py)


def test_new_entries_are_declared_bound_and_exported():
    from rrtmgpnn import _lib, daylit
    header = open(os.path.join(ROOT, "include", "rrtmgpnn.h")).read()
    fortran = open(os.path.join(ROOT, "rte-rrtmgp-nn_amd", "fortran", "mo_rrtmgpnn_c.F90")).read()
    api_cpp = open(os.path.join(ROOT, "rte-rrtmgp-nn_amd", "csrc", "api.cpp")).read()
    h = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in NEW.items():
        m = re.search(r"int %s\(([^;]*)\);" % name, header)
        assert m, name + " is not declared in include/rrtmgpnn.h"
        assert len(m.group(1).split(",")) == nargs, name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
        assert 'name="%s"' % name in fortran and "c_" + name in fortran, name
        assert re.search(r"^int %s\(" % name, api_cpp, re.M), name + " is not defined in csrc/api.cpp"
        assert hasattr(h, name), name + " is not exported by librrtmgpnn.so"
    for name in NEW:   # each entry cites the driver's lines, as the other daylit entries do
        at = header.index("int %s(" % name)
        comment = re.sub(r"\s*\n \*\s*", " ", header[header.rindex("/*", 0, at):at])
        assert "rrtmgp_rfmip_sw.F90:285-287, 433, 456-463" in comment, name
    for f in ("sampled_mask_active", "sampled_mask_seeded_active"):
        assert callable(getattr(daylit, f))
    # the solver family the masked and aerosol active-count instances form
    assert re.search(r"^ \*   8 sw_2stream_ck_kernel", header, re.M), "family 8 is not documented"
    internal = open(os.path.join(ROOT, "rte-rrtmgp-nn_amd", "csrc", "internal.hpp")).read()
    assert re.search(r"kSolverSwCkActiveSky\s*=\s*8\b", internal)


@pytest.mark.parametrize("route", ["array", "seeded"])
@pytest.mark.parametrize("overlap", ["max_ran", "exp_ran"])
@pytest.mark.parametrize("shape", C.CASES, ids=lambda s: "g%d-l%d-c%d" % s)
def test_compact_mask_restatement_is_the_full_masks_rows(shape, overlap, route):
    from rrtmgpnn import daylit
    ngpt, nlay, ncol = shape
    r, cf, ov = C.inputs(ngpt, nlay, ncol)
    ov = ov if overlap == "exp_ran" else None
    counts = set()
    for col0 in C.COL0 if route == "seeded" else (0,):
        full = C.full_mask(route, col0, ngpt, r, cf, ov)
        if ncol > 1:   # the case is not vacuous: set and clear elements, mixed words, a column without a draw group
            assert full.any() and not full.all()
            assert M.non_vacuity(full, M.bands(ngpt))[2] >= 1
        for pattern in C.PATTERNS:
            idx, slot, nday = daylit.plan_host(C.sun(ncol, pattern), daylit.KIND_LT, daylit.SZA_BOUND)
            counts.add(nday)
            got = C.compact_mask(route, col0, ngpt, r, cf, ov, idx, nday)
            np.testing.assert_array_equal(got, full[idx[:nday]], err_msg="%s col0 %d" % (pattern, col0))
    assert {0, 1, ncol - 1, ncol} <= counts


def test_cases_hold_the_seeded_skip_and_the_clear_gap():
    """A column with a clear layer between cloudy ones and a whole clear group of four layers, in every multi-layer
    case; the wrapping col0 wraps inside the 65-column cases."""
    for ngpt, nlay, ncol in C.CASES:
        _, cf, _ = C.inputs(ngpt, nlay, ncol)
        cl = cf > 0
        if nlay >= 5:
            gap = any(cl[i, 0] and not cl[i, 1] and cl[i, 2] for i in range(ncol))
            group = any(cl[i].any() and not cl[i, 4:8].any() for i in range(ncol))
            assert gap and group, (ngpt, nlay, ncol)
    assert C.COL0[1] + 65 > 2 ** 32
    w = P.words(C.SEED, C.STREAM, C.COL0[1], 33, 5, 5)
    np.testing.assert_array_equal(w[3:], P.words(C.SEED, C.STREAM, 0, 33, 5, 2))


@pytest.mark.parametrize("overlap", ["max_ran", "exp_ran"])
def test_oracle_with_sampled_clouds_and_aerosols_is_column_independent(orc, rfmip, overlap):
    """Sampled clouds behind an aerosol increment, then sw_solver: on the daylit columns alone and scattered with zeros,
    bit for bit what the same gives on every column with the driver's zeroing -- on up and dn everywhere, on dir at the
    daylit columns.  The clouds of a column are those of its global index (the seeded numbers of column i)."""
    from rrtmgpnn import data
    prob = subset(rfmip, COLS)
    use = prob["usecol"]
    ncol, nlay = prob["ncol"], prob["nlay"]
    assert use.any() and (~use).any()
    models, kd = [data.load_model("sw_abs"), data.load_model("sw_ray")], data.load_kdist("sw")
    ngpt, lims = kd["ngpt"], kd["band_lims_gpt"]
    clouds = data.allsky_clouds(prob, data.load_cloud_optics("lw"))
    cloudy = (clouds[0] > 0) | (clouds[1] > 0)
    rng = np.random.default_rng(77)
    cf = np.where(cloudy, rng.uniform(0.2, 0.9, cloudy.shape), 0).astype(np.float32)
    ov = rng.uniform(-1, 1, (ncol, nlay - 1)).astype(np.float32) if overlap == "exp_ran" else None
    aer = (rng.lognormal(-2, 1, (ncol, nlay, len(lims))).astype(np.float32),
           rng.uniform(0.6, 1, (ncol, nlay, len(lims))).astype(np.float32),
           rng.uniform(0.3, 0.8, (ncol, nlay, len(lims))).astype(np.float32))
    mask = M.sampled_mask(P.randoms(2026, 1, 0, ngpt, nlay, ncol), cf, ov)
    assert mask[use].any() and not mask[use][cf[use] > 0].all()
    ident = np.stack([np.arange(1, ngpt + 1)] * 2, axis=1).astype(np.int32)

    def solve(p, cl, mk, ae):
        go = orc.sw_gas_optics(p, models)
        cld = orc.delta_scale(*orc.cloud_optics(data.load_cloud_optics("sw"), *cl, nstr=2, lut=True, icergh=2))
        io = orc.increment_bybnd(lims, (go["tau"], go["ssa"], go["g"]), ae)
        io = orc.increment_bybnd(ident, io, [M.draw(mk, a, lims) for a in cld])
        alb = np.repeat(np.asarray(p["sfc_alb"], np.float32)[:, None], ngpt, axis=1)
        return orc.sw_solver(*io, p["mu0"], data.toa_flux(p, kd), alb, alb, p["top_at_1"])

    full = solve(prob, clouds, mask, aer)
    for f in full[:2]:
        f[~use] = 0.0   # the driver's zeroing (rrtmgp_rfmip_sw.F90:456-463)
    part = solve(subset(prob, np.flatnonzero(use)), tuple(c[use] for c in clouds), mask[use], tuple(a[use] for a in aer))
    for k, f, p in zip(("up", "dn"), full, part):
        np.testing.assert_array_equal(scattered(p, use, ncol).view(np.uint32), f.view(np.uint32), err_msg=k)
    np.testing.assert_array_equal(part[2].view(np.uint32), full[2][use].view(np.uint32), err_msg="dir")
    assert (full[0][use] > 0).any()


def test_step_refusals_come_before_any_device_object():
    """The refusals of mcica={..., "daylit": True} name the pair, and daylit=True beside mcica is refused as ever."""
    from rrtmgpnn.pipeline import ClearSkyStep
    prob = {"ncol": 1, "nlay": 1}
    mc = {"cloud_frac": None, "seed": 1, "daylit": True}
    for kw, word in ((dict(mcica=dict(mc, byband=True)), "mcica['byband']"), (dict(mcica=mc, sw_dual=True), "sw_dual"),
                     (dict(mcica=mc, fused=False), "fused=False")):
        with pytest.raises(ValueError, match=re.escape("mcica['daylit'] with ") + ".*" + re.escape(word)):
            ClearSkyStep(prob, clouds=(None,) * 4, **kw)
    with pytest.raises(ValueError, match="daylit=True with .*mcica"):
        ClearSkyStep(prob, daylit=True, clouds=(None,) * 4, mcica=mc)
    with pytest.raises(ValueError, match="daylit=True with .*mcica"):
        ClearSkyStep(prob, daylit=True, mcica={})
    # capture_chains / run_blocks: refused by name before they touch the step's graphs
    step = ClearSkyStep.__new__(ClearSkyStep)
    step.mcica_daylit, step.daylit, step.overlap, step.sw = True, False, True, True
    for call in (step.capture_chains, lambda: step.run_blocks(1)):
        with pytest.raises(ValueError, match=re.escape("mcica['daylit'] with capture_chains / run_blocks")):
            call()
