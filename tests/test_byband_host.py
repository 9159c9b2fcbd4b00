"""CPU: the by-band reference helper is pinned to the oracle, and the by-band entries exist in the header, the ctypes
table and the class layer."""
import os
import re

import numpy as np
import pytest

import byband_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lw_case(ngpt, seed=7, ncol=3, nlay=6):
    rng = np.random.default_rng(seed)
    tau = rng.lognormal(-1, 1.5, size=(ncol, nlay, ngpt)).astype(np.float32)
    lay = rng.uniform(1, 50, size=(ncol, nlay, ngpt)).astype(np.float32)
    lev = rng.uniform(1, 50, size=(ncol, nlay + 1, ngpt)).astype(np.float32)
    emis = rng.uniform(0.8, 1.0, size=(ncol, ngpt)).astype(np.float32)
    sfc = rng.uniform(1, 50, size=(ncol, ngpt)).astype(np.float32)
    return tau, lay, lev, emis, sfc


@pytest.mark.parametrize("top_at_1", [True, False])
@pytest.mark.parametrize("ngpt", [256, 32, 130])
def test_one_angle_terms_reduce_to_the_oracle_broadband(orc, ngpt, top_at_1):
    """fac * radiance (the helper's rounding of fac), reduced in the reference's broadband order, is the oracle's
    broadband flux bit for bit; for ngpt % 4 != 0 the bare radiances summed sequentially are."""
    from oracle import gauss
    tau, lay, lev, emis, sfc = _lw_case(ngpt)
    up, dn, gu, gd = orc.lw_solver(tau, lay, lev, emis, sfc, top_at_1, 1, gpt=True)
    w = gauss(1)[1][0]
    red = R.broadband_4partials if ngpt % 4 == 0 else R.broadband_sequential
    np.testing.assert_array_equal(red(R.lw_one_angle_terms(gu, w, ngpt)), up)
    np.testing.assert_array_equal(red(R.lw_one_angle_terms(gd, w, ngpt)), dn)


def test_sum_byband_helper_is_sequential():
    """Against a plain Python loop in float32, on values whose pairwise sum differs."""
    rng = np.random.default_rng(1)
    x = (rng.uniform(0, 1, size=(2, 3, 40)) * 10.0 ** rng.integers(-3, 4, size=(2, 3, 40))).astype(np.float32)
    lims = R.irregular_limits(40)
    want = np.empty((2, 3, len(lims)), np.float32)
    for i in range(2):
        for j in range(3):
            for b, (lo, hi) in enumerate(lims):
                s = x[i, j, lo - 1]
                for g in range(lo, hi):
                    s = np.float32(s + x[i, j, g])
                want[i, j, b] = s
    np.testing.assert_array_equal(R.sum_byband(x, lims), want)
    assert lims[0].tolist() == [1, 1] and lims[-1, 1] == 40 and (np.diff(lims.ravel())[1::2] == 1).all()
    assert any(lo % 2 == 0 for lo, _ in lims) and any(lo % 2 == 1 for lo, _ in lims)


def test_header_and_signatures_declare_the_byband_entries():
    from rrtmgpnn import _lib
    hdr = open(os.path.join(ROOT, "include", "rrtmgpnn.h")).read()
    for name in ("rrtmgpnn_solver_request_byband", "rrtmgpnn_sum_byband"):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["rrtmgpnn_solver_request_byband"][1]) == 6
    assert len(_lib.SIGNATURES["rrtmgpnn_sum_byband"][1]) == 8
    # the reference routines are cited, as for every entry
    assert "mo_fluxes_byband_kernels.F90:31-50" in hdr and "mo_fluxes_byband.F90" in hdr


def test_fluxes_byband_class_exists():
    from rrtmgpnn import api
    assert issubclass(api.FluxesByBand, api.FluxesFlexible)
    fl = api.FluxesByBand()
    for k in ("bnd_flux_up", "bnd_flux_dn", "bnd_flux_dn_dir", "bnd_flux_net"):
        assert getattr(fl, k) is None
    assert not fl.are_desired()
    assert api.FluxesByBand(bnd_flux_up=np.zeros((1, 2, 3), np.float32)).are_desired()


def test_clear_sky_step_takes_byband():
    import inspect
    from rrtmgpnn.pipeline import ClearSkyStep
    assert inspect.signature(ClearSkyStep.__init__).parameters["byband"].default is False
