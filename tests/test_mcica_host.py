"""CPU: the numpy restatement of mo_cloud_sampling (tests/mcica_ref.py) against the fixture made from the reference's
own module (tests/golden/mcica_masks.npz, tests/golden/make_mcica_golden.py), the bit packing, and the conditions that
keep the GPU cases of tests/test_gpu_mcica.py from being vacuous."""
import os
import re

import numpy as np
import pytest

import mcica_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "mcica_masks.npz")))


def test_fixture_inputs_are_the_builders(golden):
    r, cf, ov = M.build(*M.FIXTURE_SHAPE, M.FIXTURE_SEED)
    np.testing.assert_array_equal(golden["randoms"], r)
    np.testing.assert_array_equal(golden["cloud_frac"], cf)
    np.testing.assert_array_equal(golden["overlap_param"], ov)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "mcica_masks.npz")) < 256 * 1024


@pytest.mark.parametrize("overlap", ["max_ran", "exp_ran"])
def test_restatement_equals_reference_fixture(golden, overlap):
    ov = golden["overlap_param"] if overlap == "exp_ran" else None
    got = M.sampled_mask(golden["randoms"], golden["cloud_frac"], ov)
    want = golden["mask_" + overlap]
    assert set(np.unique(want)) <= {0, 1}
    np.testing.assert_array_equal(got, want.astype(bool))


def test_overlaps_differ_and_quirk_layers_are_false(golden):
    """exp_ran is not max_ran on these inputs, and the clear layers between cloudy ones (which the reference's exp_ran
    never assigns; the generator pre-fills .false.) are false in both."""
    assert (golden["mask_max_ran"] != golden["mask_exp_ran"]).any()
    cf = golden["cloud_frac"]
    n = 0
    for ic in range(cf.shape[0]):
        idx = np.nonzero(cf[ic] > 0)[0]
        if len(idx) < 2:
            continue
        gap = [il for il in range(idx[0], idx[-1]) if cf[ic, il] == 0]
        n += len(gap)
        for k in ("mask_max_ran", "mask_exp_ran"):
            assert not golden[k][ic, gap].any()
    assert n > 0


@pytest.mark.parametrize("ngpt", [1, 31, 32, 33, 40, 64, 224, 256])
def test_packing_round_trips(ngpt):
    rng = np.random.default_rng(ngpt)
    m = rng.random((3, 5, ngpt)) < 0.5
    b = M.pack_bits(m)
    nw = (ngpt + 31) // 32
    assert b.shape == (3, 5, nw) and b.dtype == np.uint32
    np.testing.assert_array_equal(M.unpack_bits(b, ngpt), m)
    if ngpt % 32:
        assert not (b[..., -1] >> np.uint32(ngpt % 32)).any(), "unused high bits must be zero"
    g = ngpt - 1
    one = np.zeros((1, 1, ngpt), bool)
    one[0, 0, g] = True
    w = M.pack_bits(one)
    assert w[0, 0, g // 32] == np.uint32(1) << np.uint32(g % 32) and w.astype(np.uint64).sum() == 1 << (g % 32)


def test_builders_reach_every_required_case(golden):
    cov = M.coverage(golden["randoms"], golden["cloud_frac"], golden["overlap_param"])
    assert all(cov.values()), cov
    # and the largest GPU cases on their own (the small ones cannot hold every design)
    for ngpt in (256, 224, 40, 33):
        r, cf, ov = M.build(ngpt, 12, 5, M.case_seed(ngpt, 12, 5))
        cov = M.coverage(r, cf, ov)
        for k in ("no_cloud", "adjacent", "gap", "frac1_rand0", "rand_eq_thresh", "rho_pm1_0", "rho_generic"):
            assert cov[k], (ngpt, k)
    # the designed comparisons come out as the strict float32 comparison says
    r, cf, ov = golden["randoms"], golden["cloud_frac"], golden["overlap_param"]
    assert cf[1, 0] == 1 and r[1, 0, 0] == 0 and not golden["mask_max_ran"][1, 0, 0]
    assert r[1, 0, 1] == np.float32(1) - cf[1, 0] and not golden["mask_max_ran"][1, 0, 1]
    tiny = (cf > 0) & ((np.float32(1) - cf) == 1)
    # (exp_ran's correlated deviates are not confined to [0, 1), so only max_ran's mask is necessarily false there)
    assert tiny.any() and not golden["mask_max_ran"][tiny].any()


@pytest.mark.parametrize("shape", M.CASES + [M.FIXTURE_SHAPE], ids=lambda s: "g%d-l%d-c%d" % s)
def test_cases_are_not_vacuous(shape):
    """Every GPU mask case, both overlaps: 20-80 % of the bits set, at least a third of the columns with a layer whose
    bits differ inside one band, at least one mixed 32-bit word."""
    ngpt, nlay, ncol = shape
    seed = M.FIXTURE_SEED if shape == M.FIXTURE_SHAPE else M.case_seed(*shape)
    r, cf, ov = M.build(ngpt, nlay, ncol, seed)
    for o in (None, ov):
        share, cols, mixed = M.non_vacuity(M.sampled_mask(r, cf, o), M.bands(ngpt))
        assert 0.2 <= share <= 0.8, share
        assert cols >= 1 / 3, cols
        assert mixed >= 1


def test_bands_cover_and_layouts():
    for ngpt in (256, 224, 40, 33):
        b = M.bands(ngpt)
        assert b[0, 0] == 1 and b[-1, 1] == ngpt and (b[1:, 0] == b[:-1, 1] + 1).all()
    assert ((M.bands(224)[:, 0] - 1) % 2 == 0).all()      # band-pair layout
    assert ((M.bands(40)[:, 0] - 1) % 2 == 1).any()       # general layout: odd band starts
    assert len(set((M.bands(40)[:, 1] - M.bands(40)[:, 0]).tolist())) > 1


def test_new_entries_are_declared_and_bound():
    """include/rrtmgpnn.h, the ctypes table and the Fortran interface module all carry the four new entries."""
    from rrtmgpnn import _lib
    header = open(os.path.join(ROOT, "include", "rrtmgpnn.h")).read()
    fortran = open(os.path.join(ROOT, "rte-rrtmgp-nn_amd", "fortran", "mo_rrtmgpnn_c.F90")).read()
    for name, nargs in (("rrtmgpnn_sampled_mask_max_ran", 8), ("rrtmgpnn_sampled_mask_exp_ran", 9),
                        ("rrtmgpnn_draw_samples", 13), ("rrtmgpnn_solver_request_cloud_mask", 5)):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert len(_lib.SIGNATURES[name][1]) == nargs
        assert 'name="%s"' % name in fortran
    assert "mo_cloud_sampling.F90" in header and "QUIRK" in header
