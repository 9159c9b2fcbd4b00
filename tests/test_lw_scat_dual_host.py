"""CPU: what tests/test_gpu_lw_scat_dual.py's bitwise comparisons rest on, established on the oracle alone with the
inputs of tests/lw_scat_dual_cases.py --

1. the 2str-by-1scl increment (inc_2stream_by_1scalar_bybnd) leaves ssa and g as +0 bit patterns and its tau is the
   1scl increment's, so the kernel may feed literal zeros into its two-stream increment;
2. the rescaled solve of (tau + tau_aer, 0, 0) equals the no-scattering solve bit for bit, so the clear set may be
   compared against rrtmgpnn_lw_solver_noscat_planck[_inc];
3. the aerosol changes flux bits in every column (clear and all-sky);
4. for nlay >= 7 (top_at_1, one angle, unmasked) both the cloud-before-aerosol order and one pre-summed increment change
   all-sky flux bits: a kernel that computes either cannot pass --

and that the built library exports the entry and the knob, the header declares them and the Fortran binding names them."""
import ctypes
import os

import numpy as np
import pytest

import lw_scat_cases as S
import lw_scat_dual_cases as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = pytest.mark.parametrize("ng,nlay", D.CASES)
ENTRY = "rrtmgpnn_lw_solver_1rescl_planck_clr_all"
KNOB = "rrtmgpnn_context_set_lw_scat_clr_all"


@CASES
def test_2str_by_1scl_increment_keeps_zero_ssa_and_g(orc, ng, nlay):
    c = S.case(ng, nlay)
    aer = D.aerosol(ng, nlay)
    z = np.zeros_like(c["tau"])
    t, w, g = orc.increment_bybnd(c["lims"], [c["tau"], z, z], [aer])
    assert (w.view(np.uint32) == 0).all() and (g.view(np.uint32) == 0).all(), "ssa / g are not +0 bit patterns"
    np.testing.assert_array_equal(t.view(np.uint32), D.clear_tau(orc, c, aer).view(np.uint32))
    np.testing.assert_array_equal(t, c["tau"] + S.expand(aer, c["lims"], ng))
    if nlay >= 7:
        assert (aer[1, nlay // 2] == 0).all() and (aer[1, :nlay // 2] > 0).all()


@CASES
@pytest.mark.parametrize("top_at_1", [True, False], ids=["top1", "top0"])
@pytest.mark.parametrize("nmus", [1, 3])
@pytest.mark.parametrize("kind", [None, "sampled"], ids=["unmasked", "sampled"])
def test_rescaled_clear_is_noscat_and_the_aerosol_shows(orc, ng, nlay, top_at_1, nmus, kind):
    c = S.case(ng, nlay)
    aer = D.aerosol(ng, nlay)
    lay, lev, sfc, _ = S.sources(orc, c, top_at_1)
    emis = S.expand(c["emis_bnd"], c["lims"], ng)
    z = np.zeros_like(c["tau"])
    with_aer = D.expect(orc, c, kind, True, top_at_1, nmus)
    without = D.expect(orc, c, kind, False, top_at_1, nmus)
    # 2: the rescaled solver on the 1scl atmosphere [+ aerosol] against the no-scattering clear set
    for a, want in ((aer, with_aer), (None, without)):
        t = D.clear_tau(orc, c, a)
        resc = orc.lw_solver(t, lay, lev, emis, sfc, top_at_1=top_at_1, nmus=nmus, ssa=z, g=z)
        for q in range(2):
            np.testing.assert_array_equal(resc[q].view(np.uint32), want[2 + q].view(np.uint32))
    # 3: the aerosol in every column of all four arrays
    assert all(np.isfinite(f).all() for f in with_aer)
    for q in range(4):
        assert (with_aer[q] != without[q]).any(axis=1).all(), "a column of array %d shows no aerosol" % q
    # the clear set is the unmasked call's, the cloud shows beside it
    np.testing.assert_array_equal(with_aer[2], D.expect(orc, c, None, True, top_at_1, nmus)[2])
    assert (with_aer[1] != with_aer[3]).any()


@pytest.mark.parametrize("ng,nlay", [k for k in D.CASES if k[1] >= 7])
def test_increment_order_and_presum_change_bits(orc, ng, nlay):
    c = S.case(ng, nlay)
    aer = D.aerosol(ng, nlay)
    lay, lev, sfc, _ = S.sources(orc, c, True)
    emis = S.expand(c["emis_bnd"], c["lims"], ng)
    want = D.expect(orc, c, None, True, True, 1)
    for order in ("cloud_first", "presummed"):
        io = D.props(orc, c, None, aer, order)
        got = orc.lw_solver(io[0], lay, lev, emis, sfc, top_at_1=True, nmus=1, ssa=io[1], g=io[2])
        assert any((got[q] != want[q]).any() for q in range(2)), "%s gives the entry's bits" % order


def test_library_header_and_fortran_name_the_entry_and_the_knob():
    from rrtmgpnn import _lib
    assert ENTRY in _lib.SIGNATURES and KNOB in _lib.SIGNATURES
    # the arguments of _1rescl_planck_inc in its order, then flux_up_clr, flux_dn_clr
    base = _lib.SIGNATURES["rrtmgpnn_lw_solver_1rescl_planck_inc"][1]
    assert _lib.SIGNATURES[ENTRY][1] == base + [_lib.c_vp, _lib.c_vp]
    assert _lib.SIGNATURES[KNOB] == _lib.SIGNATURES["rrtmgpnn_context_set_sw_clr_all"]
    h = ctypes.CDLL(_lib.LIB_PATH)
    for name in (ENTRY, KNOB):
        assert hasattr(h, name), "librrtmgpnn.so does not export %s" % name
    with open(os.path.join(ROOT, "include", "rrtmgpnn.h")) as f:
        text = f.read()
    assert "int %s(" % ENTRY in text and "int %s(" % KNOB in text
    for cite in ("extensions/mo_rrtmgp_clr_all_sky.F90:146-172", "rte/kernels/mo_optical_props_kernels.F90:426-484",
                 "rte/mo_rte_lw.F90:372-387"):
        assert cite in text[text.index("Clear-sky beside all-sky LW fluxes for scattering clouds"):text.index(
            "int %s(" % ENTRY)], cite
    with open(os.path.join(ROOT, "rte-rrtmgp-nn_amd", "fortran", "mo_rrtmgpnn_c.F90")) as f:
        text = f.read()
    for name in (ENTRY, KNOB):
        assert 'bind(C, name="%s")' % name in text and "function c_%s(" % name in text
