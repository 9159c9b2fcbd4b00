"""The cases of the seeded McICA mask tests (tests/test_gpu_mcica_seeded.py), shared with the CPU test that keeps them
from being vacuous (tests/test_mcica_seeded_host.py).

Shapes: the smallest at which each mechanism of the seeded kernels can go wrong.
  ngpt 1, 33, 40, 224, 256, 300: a partial wave, a partial last word, the SW and LW counts (256: exactly the block),
       and more than the 256-lane block;
  nlay 1, 3, 4, 5, 12: the edges of the groups of 4 layers one Philox call serves;
  ncol 1, 3; col0 0, 5, 2^32 - 2 (the global column wraps); two seeds, one with a non-zero high word.
A test case is (ngpt, nlay, overlap); it runs every (ncol, col0, seed) combination.  The cloud fractions and overlap
parameters come from mcica_ref.build (its random numbers are not used): with 3 columns and nlay 12, column 2 is cloudy
in layers 0, 2, 3 and 11 only, so its middle group of 4 layers draws nothing and its last group is cloudy only in its
last layer.

Non-vacuity (a condition on the inputs, checked on the CPU for every combination): with more than one g-point, the mask
of every combination has a 32-bit word with both set and clear bits, that is a cloudy layer with both set and clear
elements (mcica_ref.non_vacuity's third figure); with one g-point a layer is one element, so the set and clear elements
are looked for among the cloudy layers of all the case's combinations together.  BUILD_SEED picks, per (ngpt, nlay,
ncol), the first builder seed at or after mcica_ref.case_seed for which that holds with both Philox seeds, all three
col0 and both overlaps (found by first_build_seed below; the host test asserts the table is what the search gives)."""
import numpy as np

import mcica_ref as M
import philox_ref as P

NGPT = (1, 33, 40, 224, 256, 300)
NLAY = (1, 3, 4, 5, 12)
NCOL = (1, 3)
COL0 = (0, 5, 2 ** 32 - 2)
SEEDS = (2026, 0x9E3779B97F4A7C15)  # the second: a non-zero high word
STREAM = 3
CASES = [(g, l) for g in NGPT for l in NLAY]


def inputs(ngpt, nlay, ncol, build_seed=None):
    """(cloud_frac, overlap_param) of a combination."""
    seed = BUILD_SEED.get((ngpt, nlay, ncol), M.case_seed(ngpt, nlay, ncol)) if build_seed is None else build_seed
    _, cf, ov = M.build(ngpt, nlay, ncol, seed)
    return cf, ov


def want_mask(seed, col0, ngpt, cf, ov):
    ncol, nlay = cf.shape
    return M.sampled_mask(P.randoms(seed, STREAM, col0, ngpt, nlay, ncol), cf, ov)


def combos():
    return [(ncol, col0, seed) for ncol in NCOL for col0 in COL0 for seed in SEEDS]


def holds(ngpt, nlay, ncol, build_seed):
    """The non-vacuity condition of one (ngpt, nlay, ncol) for a builder seed: every (col0, seed, overlap)."""
    cf, ov = inputs(ngpt, nlay, ncol, build_seed)
    if not (cf > 0).any():
        return False
    for o in (None, ov):
        elems = []
        for col0 in COL0:
            for seed in SEEDS:
                m = want_mask(seed, col0, ngpt, cf, o)
                if ngpt > 1 and M.non_vacuity(m, M.bands(ngpt))[2] < 1:
                    return False
                elems.append(m[cf > 0].ravel())
        e = np.concatenate(elems)
        if ngpt == 1 and (e.all() or not e.any()):
            return False
    return True


def first_build_seed(ngpt, nlay, ncol):
    s = M.case_seed(ngpt, nlay, ncol)
    while not holds(ngpt, nlay, ncol, s):
        s += 1
    return s


# (ngpt, nlay, ncol) -> builder seed, where it is not mcica_ref.case_seed itself
BUILD_SEED = {(33, 3, 1): 33032, (256, 1, 3): 256014, (300, 1, 1): 300012}
