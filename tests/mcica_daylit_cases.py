"""The cases of the compact McICA mask tests (tests/test_gpu_mcica_daylit.py), shared with the CPU test that restates
the compact mask and keeps the cases from being vacuous (tests/test_mcica_daylit_host.py).

Shapes: the smallest at which the compact instances of the mask kernel can go wrong.
  ngpt 33, 112, 224: one, four and seven 32-bit words per (layer, column), each with a partial last wave of 64 lanes;
  nlay 1, 5, 9: overlap_param is empty (NULL) at 1; neither 5 nor 9 is a multiple of the four-layer group one Philox
       call serves;
  ncol 1, 5, 65: one block, a few, and more columns than a wave has lanes;
  the day / night patterns of tests/test_daylit_host.py, which give the counts 0 (night), 1 (last), ncol (day) and,
       with a plan made for it here, ncol - 1 (all but the first column); `alternating` and `random` lie in between;
  both overlaps, the array and the seeded route, col0 = 0 and a col0 whose global column wraps modulo 2^32.
The cloud fraction of column i depends on i alone (cloud_frac below): every third column has clear layers between
cloudy ones and whole clear groups of four layers (the seeded kernel's skip), the others are generic with about 30 % of
the layers clear."""
import numpy as np

import mcica_ref as M
import philox_ref as P

F = np.float32
NGPT = (33, 112, 224)
NLAY = (1, 5, 9)
NCOL = (1, 5, 65)
PATTERNS = ("day", "night", "alternating", "last", "random", "all_but_first")
COL0 = (0, 2 ** 32 - 3)
SEED, STREAM = 0x9E3779B97F4A7C15, 3
PREFILL = 0xDEADBEEF
CASES = [(g, l, c) for g in NGPT for l in NLAY for c in NCOL]


def inputs(ngpt, nlay, ncol):
    """(randoms, cloud_frac, overlap_param): mcica_ref.build's generic inputs with designed columns: column i with
    i % 3 == 1 is cloudy in layers 0 and 2 alone (a clear layer between cloudy ones, then clear groups of four) and, where
    there are nine layers, in the last one too; column i with i % 3 == 2 is overcast in part: fraction 1 in its first
    layer."""
    r, cf, ov = M.build(ngpt, nlay, ncol, 7000 * ngpt + 70 * nlay + ncol)
    for i in range(ncol):
        if i % 3 == 1 or ncol == 1:
            cf[i] = 0
            cf[i, 0] = F(0.6)
            if nlay > 2:
                cf[i, 2] = F(0.7)
            if nlay > 8:
                cf[i, 8] = F(0.5)
        elif i % 3 == 2:
            cf[i, 0] = F(1.0)
    return r, cf, ov


def sun(ncol, pattern):
    """The zenith angles of a pattern (tests/test_daylit_host.values with the driver's kind and bound)"""
    from rrtmgpnn import daylit
    from test_daylit_host import values
    if pattern == "all_but_first":
        v = np.full(ncol, 30.0, F)
        v[0] = 120.0
        return v
    return values(ncol, pattern, daylit.KIND_LT, daylit.SZA_BOUND, seed=ncol)


def full_mask(route, col0, ngpt, r, cf, ov):
    """The full-extent mask (ncol, nlay, ngpt) bool of a route: the caller's randoms, or the seeded numbers"""
    ncol, nlay = cf.shape
    if route == "seeded":
        r = P.randoms(SEED, STREAM, col0, ngpt, nlay, ncol)
    return M.sampled_mask(r, cf, ov)


def compact_mask(route, col0, ngpt, r, cf, ov, idx, nday):
    """The compact entries restated: dense row j < nday from source column i = idx[j] alone -- its cloud_frac,
    overlap_param and randoms, or the seeded numbers of global column (col0 + i) mod 2^32 -- as a one-column problem."""
    ncol, nlay = cf.shape
    out = np.zeros((nday, nlay, ngpt), bool)
    for j in range(nday):
        i = int(idx[j])
        rr = P.randoms(SEED, STREAM, (col0 + i) % 2 ** 32, ngpt, nlay, 1) if route == "seeded" else r[i:i + 1]
        out[j] = M.sampled_mask(rr, cf[i:i + 1], None if ov is None else ov[i:i + 1])[0]
    return out
