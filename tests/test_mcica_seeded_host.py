"""CPU: the seeded McICA route's generator as restated in tests/philox_ref.py (Philox4x32-10 and the counter layout of
include/rrtmgpnn.h), the conditions that keep the GPU cases of tests/test_gpu_mcica_seeded.py from being vacuous, and
the new entries in the header, the ctypes table and the library."""
import ctypes
import os
import re

import numpy as np
import pytest

import mcica_ref as M
import mcica_seeded_cases as C
import philox_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"rrtmgpnn_mcica_rng_set": 5, "rrtmgpnn_mcica_randoms": 6, "rrtmgpnn_sampled_mask_max_ran_seeded": 8,
       "rrtmgpnn_sampled_mask_exp_ran_seeded": 9}


def _hex(words):
    return " ".join("%08x" % int(w) for w in words)


@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_known_answers(counter, key, want):
    assert _hex(P.philox4x32_10(counter, key)) == want


def test_numbers_lie_in_unit_interval():
    r = P.randoms(2026, 0, 0, 40, 12, 50)
    assert r.dtype == np.float32 and r.shape == (50, 12, 40)
    assert (r >= 0).all() and (r < 1).all()
    # the conversion's extremes: exact, and the largest is 1 - 2^-24
    ext = P.to_float(np.array([0, 0xFF, 0x100, 0xFFFFFFFF], np.uint32))
    assert ext.tolist() == [0.0, 0.0, 2.0 ** -24, 1.0 - 2.0 ** -24]


def test_word_and_group_layout():
    """Layer l of g-point g of column icol is word l & 3 of the call with counter (g, l >> 2, col0 + icol, stream)."""
    seed, stream, col0, ngpt, nlay, ncol = (7 << 32) | 11, 9, 100, 3, 5, 2
    w = P.words(seed, stream, col0, ngpt, nlay, ncol)
    r = P.randoms(seed, stream, col0, ngpt, nlay, ncol)
    assert w.shape == r.shape == (ncol, nlay, ngpt)
    for icol in range(ncol):
        for l in range(nlay):
            for g in range(ngpt):
                one = P.philox4x32_10((g, l >> 2, col0 + icol, stream), (11, 7))
                assert int(w[icol, l, g]) == int(one[l & 3]), (icol, l, g)
                assert r[icol, l, g] == np.float32(int(one[l & 3]) >> 8) * np.float32(2.0 ** -24)
    # stream and seed matter
    assert (P.words(seed, stream + 1, col0, ngpt, nlay, ncol) != w).any()
    assert (P.words(seed + (1 << 32), stream, col0, ngpt, nlay, ncol) != w).any()


def test_decomposition_and_wrap():
    whole = P.randoms(5, 1, 0, 40, 5, 7)
    np.testing.assert_array_equal(whole[3:], P.randoms(5, 1, 3, 40, 5, 4))
    wrap = P.randoms(5, 1, 2 ** 32 - 2, 40, 5, 3)
    for i, col in enumerate((2 ** 32 - 2, 2 ** 32 - 1, 0)):
        np.testing.assert_array_equal(wrap[i], P.randoms(5, 1, col, 40, 5, 1)[0])


def test_layout_sanity_cloud_share():
    """cloud_frac 0.3 everywhere in one layer: the share of set elements is 0.30 +- 0.02 (5.6 binomial standard
    deviations of 256 * 64 elements)."""
    r = P.randoms(2026, 0, 0, 256, 1, 64)
    share = float(M.sampled_mask(r, np.full((64, 1), 0.3, np.float32)).mean())
    print("share of set mask elements: %.5f" % share)
    assert abs(share - 0.30) <= 0.02


def test_case_seeds_are_the_search_result():
    for ngpt, nlay in C.CASES:
        for ncol in C.NCOL:
            want = C.first_build_seed(ngpt, nlay, ncol)
            assert C.BUILD_SEED.get((ngpt, nlay, ncol), M.case_seed(ngpt, nlay, ncol)) == want, (ngpt, nlay, ncol)


def test_cases_are_not_vacuous_and_reach_the_group_paths():
    for ngpt, nlay in C.CASES:
        for ncol in C.NCOL:
            assert C.holds(ngpt, nlay, ncol, None), (ngpt, nlay, ncol)
    # 3 columns x 12 layers: a group of 4 layers that draws nothing, and one cloudy only in its last layer
    cf, _ = C.inputs(40, 12, 3)
    cl = cf[2] > 0
    assert cl[0:4].any() and not cl[4:8].any() and cl[8:12].tolist() == [False, False, False, True]
    # clear layers above, between and below cloudy ones somewhere in the 12-layer inputs
    gen = np.concatenate([C.inputs(g, 12, 3)[0] for g in C.NGPT]) > 0
    assert (~gen[:, 0]).any() and (~gen[:, -1]).any()


def test_new_entries_are_declared_bound_and_exported():
    from rrtmgpnn import _lib
    header = open(os.path.join(ROOT, "include", "rrtmgpnn.h")).read()
    fortran = open(os.path.join(ROOT, "rte-rrtmgp-nn_amd", "fortran", "mo_rrtmgpnn_c.F90")).read()
    h = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in NEW.items():
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert len(_lib.SIGNATURES[name][1]) == nargs
        assert 'name="%s"' % name in fortran
        assert hasattr(h, name), name + " is not exported by librrtmgpnn.so"
    # the header states the counter layout, the wrap and that there is no reference counterpart
    assert "(g, l >> 2, (col0 + icol) mod 2^32, stream)" in header
    assert "wraps modulo 2^32" in header and "No reference counterpart" in header
