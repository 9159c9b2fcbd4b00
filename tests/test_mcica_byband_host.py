"""CPU: rrtmgpnn_solver_request_byband_mcica is declared, bound and exported, and the composed-oracle expectation of
tests/test_gpu_mcica_byband.py is deterministic and depends on the mask: in some band the sampled mask's by-band down
flux is neither the all-ones nor the all-zeros one (the GPU tests' non-vacuity condition, established without a GPU)."""
import ctypes
import os
import re

import numpy as np
import pytest

import byband_ref as R
import mcica_byband_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"rrtmgpnn_solver_request_byband_mcica": 10}


def test_new_entry_is_declared_bound_and_exported():
    from rrtmgpnn import _lib
    header = open(os.path.join(ROOT, "include", "rrtmgpnn.h")).read()
    fortran = open(os.path.join(ROOT, "rte-rrtmgp-nn_amd", "fortran", "mo_rrtmgpnn_c.F90")).read()
    h = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in NEW.items():
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert len(_lib.SIGNATURES[name][1]) == nargs
        assert 'name="%s"' % name in fortran and "c_" + name in fortran
        assert hasattr(h, name), name + " is not exported by librrtmgpnn.so"
    # the header's argument list is the issue's: the by-band request's arguments, then the mask request's
    m = re.search(r"int rrtmgpnn_solver_request_byband_mcica\(([^;]*)\);", header)
    args = [a.strip().split()[-1].lstrip("*") for a in m.group(1).replace("\n", " ").split(",")]
    assert args == ["ctx", "nbnd", "band_lims_gpt", "bnd_flux_up", "bnd_flux_dn", "bnd_flux_dir", "ngpt", "nlay", "ncol",
                    "mask_bits"]
    from rrtmgpnn import cloud_sampling
    assert callable(cloud_sampling.arm_cloud_mask_byband)


def _differs_in_a_band(a, b, c):
    """Some band (last axis) in which a differs from both b and c."""
    return bool((((a != b).reshape(-1, a.shape[-1]).any(axis=0)) & ((a != c).reshape(-1, a.shape[-1]).any(axis=0))).any())


@pytest.mark.parametrize("nmus", [1, 3])
def test_lw_expectation_depends_on_the_mask(orc, nmus):
    c = C.lw_inputs()
    masks = {k: C.mask_for(c["ng"], C.LW_MASK_SEED, k) for k in ("sampled", "ones", "zeros")}
    share, cols, mixed = C.M.non_vacuity(masks["sampled"], c["kd"]["band_lims_gpt"])
    assert 0.1 < share < 0.9 and cols == 1.0 and mixed > 0
    exp = {k: C.lw_expect(orc, c, m, True, nmus) for k, m in masks.items()}
    again = C.lw_expect(orc, c, C.mask_for(c["ng"], C.LW_MASK_SEED), True, nmus)
    for a, b in zip(exp["sampled"], again):  # deterministic
        np.testing.assert_array_equal(a, b)
    for name, lims in C.byband_layouts(c["kd"]).items():
        dn = {k: R.sum_byband(v[3], lims) for k, v in exp.items()}
        assert np.isfinite(dn["sampled"]).all()
        assert _differs_in_a_band(dn["sampled"], dn["ones"], dn["zeros"]), name


@pytest.mark.parametrize("seed", [C.SW_MASK_SEED, C.RFMIP_MASK_SEED])
@pytest.mark.parametrize("layout", ["pair", "general"])
def test_sw_expectation_depends_on_the_mask(orc, layout, seed):
    c = C.sw_inputs()
    cl = c["lims"][layout]
    masks = {k: C.mask_for(c["ng"], seed, k) for k in ("sampled", "ones", "zeros")}
    exp = {k: C.sw_expect(orc, c, m, cl, True, True) for k, m in masks.items()}
    again = C.sw_expect(orc, c, C.mask_for(c["ng"], seed), cl, True, True)
    for a, b in zip(exp["sampled"][1], again[1]):
        np.testing.assert_array_equal(a, b)
    for name, lims in C.byband_layouts(c["kd"]).items():
        dn = {k: R.sum_byband(v[1][1], lims) for k, v in exp.items()}
        assert np.isfinite(dn["sampled"]).all()
        assert _differs_in_a_band(dn["sampled"], dn["ones"], dn["zeros"]), name
    # the uncovered layout really leaves g-points outside every band, and those g-points carry flux
    covered = np.zeros(c["ng"], bool)
    for lo, hi in R.uncovered_limits(c["ng"]):
        covered[lo - 1:hi] = True
    assert not covered.all() and (exp["sampled"][1][1][..., ~covered] != 0).any()
