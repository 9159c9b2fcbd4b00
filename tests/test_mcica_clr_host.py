"""CPU: the C ABI of the clear-sky + McICA all-sky LW entry (rrtmgpnn_lw_solver_noscat_planck_clr_all_mcica) in the
ctypes table, the header and the Fortran binding, and the class layer's mask checks, which return before anything
touches a device."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "rrtmgpnn_lw_solver_noscat_planck_clr_all_mcica"


def test_signature_is_clr_all_plus_one_pointer():
    from rrtmgpnn import _lib
    res, args = _lib.SIGNATURES[ENTRY]
    res0, args0 = _lib.SIGNATURES["rrtmgpnn_lw_solver_noscat_planck_clr_all"]
    assert res is res0 is _lib.c_int
    assert len(args) == 29 and len(args0) == 28
    assert list(args[:-1]) == list(args0) and args[-1] is _lib.c_vp


def _params(text, name):
    m = re.search(r"\b%s\s*\(([^;{]*?)\)\s*[;{]" % name, text, re.S)
    assert m, name
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_header_and_library_source_declare_the_same_arguments():
    header = open(os.path.join(ROOT, "include", "rrtmgpnn.h")).read()
    source = open(os.path.join(ROOT, "rte-rrtmgp-nn_amd", "csrc", "api.cpp")).read()
    h, h0 = _params(header, ENTRY), _params(header, "rrtmgpnn_lw_solver_noscat_planck_clr_all")
    assert h[:-1] == h0 and h[-1] == "const unsigned int *mask_bits"
    assert _params(source, ENTRY) == h
    # the entry is on the operand-bound comment's list, and its mode-0 meaning is stated
    assert "_planck_clr_all_mcica" in header.split("OPERAND BOUND")[1].split("*/")[0]
    doc = header.split("int " + ENTRY)[0].rsplit("/*", 1)[1]
    assert "Mode 0" in doc and "RRTMGPNN_ERR_ARGUMENT" in doc


def test_fortran_binding_mirrors_the_entry():
    f90 = open(os.path.join(ROOT, "rte-rrtmgp-nn_amd", "fortran", "mo_rrtmgpnn_c.F90")).read()
    assert 'bind(C, name="%s")' % ENTRY in f90
    m = re.search(r"function c_%s\((.*?)\)\s*&?\s*bind" % ENTRY, f90, re.S)
    names = [a.strip() for a in m.group(1).replace("&", " ").split(",")]
    assert len(names) == 29 and names[-1] == "mask_bits"
    assert re.search(r"public ::.*c_%s\b" % ENTRY, f90)


class _Spec:
    def __init__(self, ngpt, nband):
        self._g, self._b = ngpt, nband

    def get_ngpt(self):
        return self._g

    def get_nband(self):
        return self._b


def test_class_layer_mask_extents_strings():
    torch = pytest.importorskip("torch")
    from rrtmgpnn import clr_all_sky
    ncol, nlay, ngpt = 3, 5, 40
    k = _Spec(ngpt, 6)
    z = lambda *s: torch.zeros(s)  # noqa: E731
    lw = lambda **kw: clr_all_sky.rte_lw(k, None, z(ncol, nlay), z(ncol, nlay), z(ncol, nlay + 1), z(ncol),  # noqa: E731
                                         z(ncol, 6), None, None, None, **kw)
    sw = lambda **kw: clr_all_sky.rte_sw(k, None, z(ncol, nlay), z(ncol, nlay), z(ncol, nlay + 1), z(ncol),  # noqa: E731
                                         z(ncol, 6), z(ncol, 6), None, None, None, **kw)
    bits = lambda *s: torch.zeros(s, dtype=torch.int32)  # noqa: E731
    for f, who in ((lw, "rte_lw"), (sw, "rte_sw")):
        msg = "%s: mask_bits is not (ncol, nlay, ceil(ngpt/32)) 32-bit words" % who
        assert f(mask_bits=bits(ncol, nlay, 1)) == msg          # 40 g-points are two words
        assert f(mask_bits=bits(ncol, nlay + 1, 2)) == msg
        assert f(mask_bits=bits(nlay, ncol, 2)) == msg
        assert f(mask_bits=torch.zeros((ncol, nlay, 2), dtype=torch.int64)) == msg
        assert f(cloud_mask=torch.zeros((ncol, nlay, ngpt - 1), dtype=torch.uint8)) == \
            "%s: cloud_mask is not (ncol, nlay, ngpt) bytes" % who
        assert f(mask_bits=bits(ncol, nlay, 4)[:, :, ::2]) == "%s: arrays must be contiguous" % who
    # the reference's own checks keep their precedence
    assert lw(t_lev=z(ncol, nlay), mask_bits=bits(1, 1, 1)) == "rrtmpg_lw: t_lev inconsistently sized"
