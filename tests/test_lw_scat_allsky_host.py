"""CPU: the composed oracle of tests/lw_scat_cases.py tells apart what the fused all-sky LW solve with scattering clouds
(rrtmgpnn_lw_solver_1rescl_planck_inc) must tell apart -- the mask, ssa_bnd and g_bnd all show in the expected fluxes --
so that tests/test_gpu_lw_scat_allsky.py's bitwise comparisons cannot pass on a kernel that ignores one of them.  Also:
the designed layers are present, the composition equals the reference's own increment + rte_lw where oracle/_ref is
built, and the library exports the entry."""
import ctypes
import os

import numpy as np
import pytest

import lw_scat_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORIENT = pytest.mark.parametrize("top_at_1", [True, False], ids=["top1", "top0"])
NMUS = pytest.mark.parametrize("nmus", [1, 3])
CASES = pytest.mark.parametrize("ng,nlay", S.CASES)


def _differ_enough(a, b, nlay, what):
    """At least 7/8 of the (column, level) values of each flux for nlay >= 7 (the top level's incident flux is the same
    in both), at least one value per column for one layer."""
    for k, (x, y) in enumerate(zip(a, b)):
        ne = x != y
        if nlay >= 7:
            assert ne.sum() * 8 >= 7 * ne.size, "%s [%d]: only %d of %d values differ" % (what, k, ne.sum(), ne.size)
        else:
            assert ne.any(axis=1).all(), "%s [%d]: a column shows no difference" % (what, k)


@CASES
@ORIENT
@NMUS
def test_composed_oracle_tells_the_variants_apart(orc, ng, nlay, top_at_1, nmus):
    c = S.case(ng, nlay)
    got = {k: S.expect(orc, c, k, top_at_1, nmus) for k in S.MASKS}
    clear = S.clear_expect(orc, c, top_at_1, nmus)
    for k, fl in got.items():
        assert all(np.isfinite(f).all() for f in fl), "non-finite fluxes under mask %r" % (k,)
    for q in range(2):
        np.testing.assert_array_equal(got["ones"][q], got[None][q], err_msg="all ones against unmasked")
        np.testing.assert_array_equal(got["zeros"][q], clear[q], err_msg="all zeros against the no-scattering clear sky")
        assert (got["sampled"][q] != got[None][q]).any(), "the sampled mask does not show against the unmasked set"
        assert (got["sampled"][q] != clear[q]).any(), "the sampled mask does not show against the clear set"
    no_ssa = S.expect(orc, c, None, top_at_1, nmus, wb=np.zeros_like(c["wb"]))
    no_g = S.expect(orc, c, None, top_at_1, nmus, gb=np.zeros_like(c["gb"]))
    _differ_enough(got[None], no_ssa, nlay, "ssa_bnd = 0")
    _differ_enough(got[None], no_g, nlay, "g_bnd = 0")


@CASES
def test_designed_layers_are_present(orc, ng, nlay):
    c = S.case(ng, nlay)
    l0, le, lg = S.designed(nlay)
    assert (c["tb"][2, l0] == 0).any() and (c["gb"][2, l0][c["tb"][2, l0] == 0] < 0).any()
    if nlay >= 7:
        prod = c["tb"][2, le] * c["wb"][2, le]
        assert ((c["tb"][2, le] > 0) & (prod < S.EPS)).any(), "no layer where max(eps, tau * ssa) bites"
    assert (c["gb"][2, lg] < 0).any()
    assert c["wb"].max() <= 0.95 and c["gb"].max() <= 0.95
    # the zero-tau, negative-g layer: the incremented g is +0 there (with the gas operands dropped it would be -0)
    _, _, g = S.props(orc, c, None)
    b0 = slice(c["lims"][0][0] - 1, c["lims"][0][1])
    z = g[2, l0, b0]
    assert (z == 0).all() and not np.signbit(z).any()


@ORIENT
@NMUS
def test_composition_against_the_reference(orc, top_at_1, nmus):
    """The unmasked composition on the shipped bands against the reference's own increment (by band) and rte_lw on
    two-stream properties; the incremented properties compared as bit patterns (the sign of a zero g counts)."""
    import oracle as O
    try:
        ref = O.Reference()
    except FileNotFoundError as e:
        pytest.skip(str(e))
    c = S.case(256, 7)
    kd = c["kd"]
    z = np.zeros_like(c["tau"])
    io = ref.increment_bybnd(kd, [c["tau"], z, z], [c["tb"], c["wb"], c["gb"]])
    for a, b in zip(io, S.props(orc, c, None)):
        np.testing.assert_array_equal(a.view(np.int32), b.view(np.int32))
    lay, lev, sfc, jac = S.sources(orc, c, top_at_1)
    want = ref.rte_lw_2str(kd, *io, lay, lev, sfc, jac, c["emis_bnd"], top_at_1=top_at_1, nmus=nmus)
    got = S.expect(orc, c, None, top_at_1, nmus)
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)


def test_library_exports_the_entry():
    from rrtmgpnn import _lib
    name = "rrtmgpnn_lw_solver_1rescl_planck_inc"
    assert name in _lib.SIGNATURES
    # the arguments of _noscat_planck_inc with ssa_bnd and g_bnd after tau_bnd
    base = _lib.SIGNATURES["rrtmgpnn_lw_solver_noscat_planck_inc"][1]
    assert _lib.SIGNATURES[name][1] == base[:11] + [_lib.c_vp, _lib.c_vp] + base[11:]
    h = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(h, name), "librrtmgpnn.so does not export %s" % name
    with open(os.path.join(ROOT, "include", "rrtmgpnn.h")) as f:
        assert "int %s(" % name in f.read()
