"""The by-band tests' reference: a float32 numpy sum_byband (extensions/mo_fluxes_byband_kernels.F90:31-50 of the
reference: start from the band's first g-point, add the others one by one in increasing g), the band layouts the tests
use, and the one-angle LW g-point terms.  Shared by tests/test_byband_host.py, tests/test_gpu_byband.py and
tests/test_fortran_byband.py."""
import numpy as np

PI_F = np.float32(3.14159265358979323846)


def sum_byband(gpt, lims):
    """gpt (..., ngpt) float32, lims (nbnd, 2) 1-based inclusive -> (..., nbnd) float32.  np.add.accumulate is a
    sequential left-to-right sum (np.sum pairs and would differ in the last bits)."""
    gpt = np.ascontiguousarray(gpt, np.float32)
    lims = np.asarray(lims).reshape(-1, 2)
    out = np.empty(gpt.shape[:-1] + (len(lims),), np.float32)
    for b, (lo, hi) in enumerate(lims):
        out[..., b] = np.add.accumulate(gpt[..., lo - 1:hi], axis=-1, dtype=np.float32)[..., -1]
    return out


def lw_one_angle_terms(rad, weight, ngpt):
    """The float32 terms lw_solver_noscat's broadband sum adds at one angle: fac * radiance with fac = 2.0f * PI_F *
    weight (oracle/rrtmgpnn_oracle.c:386), or the bare radiance when ngpt % 4 != 0 (quirk B-5)."""
    rad = np.ascontiguousarray(rad, np.float32)
    if ngpt % 4 != 0:
        return rad
    fac = np.float32(np.float32(2.0) * PI_F) * np.float32(weight)
    return (np.float32(fac) * rad).astype(np.float32)


def broadband_4partials(terms):
    """The reference's broadband order for ngpt % 4 == 0: partial j sums g = j, j+4, ... in increasing g, then
    ((p0 + p1) + p2) + p3."""
    t = np.ascontiguousarray(terms, np.float32)
    p = [np.add.accumulate(t[..., j::4], axis=-1, dtype=np.float32)[..., -1] for j in range(4)]
    return ((p[0] + p[1]) + p[2]) + p[3]


def broadband_sequential(terms):
    return np.add.accumulate(np.ascontiguousarray(terms, np.float32), axis=-1, dtype=np.float32)[..., -1]


def irregular_limits(ngpt):
    """Bands covering every g-point with widths 1, 3, 2, 7, 16, 5, ... repeated: widths of 1, odd starts."""
    widths, lims, g = (1, 3, 2, 7, 16, 5), [], 1
    k = 0
    while g <= ngpt:
        w = min(widths[k % len(widths)], ngpt - g + 1)
        lims.append((g, g + w - 1))
        g += w
        k += 1
    return np.asarray(lims, np.int32)


def one_band(ngpt):
    return np.asarray([(1, ngpt)], np.int32)


def even_limits(ngpt, width=16):
    """Bands of `width` g-points (the shipped k-distributions' layout when ngpt is a multiple of 16)."""
    return np.asarray([(g, min(g + width - 1, ngpt)) for g in range(1, ngpt + 1, width)], np.int32)


def uncovered_limits(ngpt):
    """The irregular layout with every third band left out: g-points outside every band."""
    lims = irregular_limits(ngpt)
    return np.ascontiguousarray(lims[np.arange(len(lims)) % 3 != 1])
