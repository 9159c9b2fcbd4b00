"""CPU: the inputs of tests/test_gpu_sw_clr_all.py tell the two skies apart, and the three entries are declared in every
binding layer."""
import os
import re

import numpy as np
import pytest

import sw_clr_all_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("rrtmgpnn_sw_solver_2stream_clr_all", "rrtmgpnn_sw_solver_2stream_rfmip_clr_all",
           "rrtmgpnn_context_set_sw_clr_all")


def _cases(orc):
    for nlay in (1, 7, 19):
        yield "nn %d" % nlay, S.nn_case(orc, nlay)
    for ngpt in sorted(S.LAYOUTS):
        yield "seeded %d" % ngpt, S.seeded_case(orc, ngpt, S.LAYOUTS[ngpt])


def test_clear_and_all_sky_differ_in_a_third_of_the_columns(orc):
    """A condition on the inputs: a dual kernel that stored one sky twice, or swapped the two, would not pass the GPU
    tests.  (Cloud-free columns are not asserted equal: in the SW a zero increment still rounds.)"""
    for name, c in _cases(orc):
        for kw in ({}, {"aer": True}, {"mask": c["masks"][0]}, {"aer": True, "mask": c["masks"][0]}):
            up, dn, dr, upc, dnc, drc = S.expect(orc, c, True, **kw)
            for a, b in ((up, upc), (dn, dnc), (dr, drc)):
                differ = (a != b).any(axis=1)
                assert 3 * differ.sum() >= c["ncol"], (name, sorted(kw), differ)


def test_masks_differ_and_sample_the_clouds(orc):
    for name, c in _cases(orc):
        m0, m1 = c["masks"]
        assert (m0 != m1).any(), name
        cloudy = c["bt"][..., 0] > 0
        assert m0[cloudy].any() and not m0[cloudy].all(), name
        assert not m0[~cloudy].any(), name


def test_every_layer_declares_the_entries():
    from rrtmgpnn import _lib
    with open(os.path.join(ROOT, "include", "rrtmgpnn.h")) as f:
        header = f.read()
    with open(os.path.join(ROOT, "rte-rrtmgp-nn_amd", "fortran", "mo_rrtmgpnn_c.F90")) as f:
        fortran = f.read()
    for e in ENTRIES:
        assert re.search(r"\bint %s\(" % e, header), e
        assert e in _lib.SIGNATURES, e
        assert 'bind(C, name="%s")' % e in fortran and "public ::" in fortran and "c_" + e in fortran, e
    # the clear outputs follow the arguments of the entry each extends
    n_inc, n_rfmip = len(_lib.SIGNATURES["rrtmgpnn_sw_solver_2stream_inc"][1]), \
        len(_lib.SIGNATURES["rrtmgpnn_sw_solver_2stream_rfmip"][1])
    assert _lib.SIGNATURES[ENTRIES[0]][1][:n_inc] == _lib.SIGNATURES["rrtmgpnn_sw_solver_2stream_inc"][1]
    assert len(_lib.SIGNATURES[ENTRIES[0]][1]) == n_inc + 3
    assert _lib.SIGNATURES[ENTRIES[1]][1][:n_rfmip] == _lib.SIGNATURES["rrtmgpnn_sw_solver_2stream_rfmip"][1]
    assert len(_lib.SIGNATURES[ENTRIES[1]][1]) == n_rfmip + 3
