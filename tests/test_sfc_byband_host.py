"""CPU: surface by-band SW fluxes from the fused solvers (rrtmgpnn_solver_request_sfc_byband) without a device.

  * the request is declared, bound (ctypes, Fortran) and numbered (family 9, option bit 4096);
  * the rows of tests/sfc_byband_cases.py are not vacuous, on the oracle alone: the sequential band sum differs in bits
    from numpy's pairwise sum, the masked values from both the unmasked-cloud and the cloud-free ones, the aerosol rows
    from the aerosol-free ones, and every daylit column has a positive direct sum in some band;
  * tests/sfc_byband_policy_host.cpp walks the new request against every cell of the five others on every row of the
    policy table (csrc/requests.cpp): not armed, nothing changes; armed, the accepted cells are those the header names
    and set the new fields beside the others; once more under the address and undefined-behaviour sanitizers."""
import os
import re
import subprocess

import numpy as np
import pytest

import sfc_byband_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "rte-rrtmgp-nn_amd")
CSRC = os.path.join(PKG, "csrc")
OK, ERR_ARGUMENT, ERR_UNSUPPORTED = 0, 1, 4
TAKERS = ("sw_solver_2stream_inc", "sw_solver_2stream_rfmip")


def read(*parts):
    return open(os.path.join(*parts)).read()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- declared, bound, numbered ------------------------------------------------------------------------------------------
def test_declared_bound_and_numbered():
    from rrtmgpnn import _lib, cloud_sampling
    m = re.search(r"int rrtmgpnn_solver_request_sfc_byband\(([^;]*)\);", read(ROOT, "include", "rrtmgpnn.h"))
    assert m and len(m.group(1).split(",")) == 7
    assert len(_lib.SIGNATURES["rrtmgpnn_solver_request_sfc_byband"][1]) == 7
    f90 = read(PKG, "fortran", "mo_rrtmgpnn_c.F90")
    assert 'bind(C, name="rrtmgpnn_solver_request_sfc_byband")' in f90
    assert re.search(r"public ::[^\n]*c_rrtmgpnn_solver_request_sfc_byband", f90)
    internal = read(CSRC, "internal.hpp")
    assert re.search(r"kSolverSwCkSfcBand\s*=\s*9\b", internal) and re.search(r"kSwCkSfcBand\s*=\s*4096\b", internal)
    assert callable(cloud_sampling.arm_sfc_byband)


# ---- the cases --------------------------------------------------------------------------------------------------------
def test_rows_cover_the_ring_and_the_instance_list():
    assert len({r["name"] for r in S.ROWS}) == len(S.ROWS)
    here = {(r["ngpt"], r["nlay"], r["top"], r["kind"], r["form"]) for r in S.HERE_ROWS}
    assert len(here) == len(S.NGPTS) * len(S.NLAYS) * 2 * len(S.KINDS) * len(S.FORMS)
    assert S.NCOL % 2 == 1 and set(S.NLAYS) == {1, 4, 7, 9, 10}
    assert {r["kind"] for r in S.CHILD_ROWS} == set(S.KINDS)
    for ngpt in S.NGPTS:   # the band-pair layout: every band starts at an odd 1-based g-point
        lims = S.inputs("inc-mask-g%d-l4-top1" % ngpt)[1]
        assert (lims[:, 0] % 2 == 1).all() and lims[0, 0] == 1 and lims[-1, 1] == ngpt


@pytest.mark.parametrize("name", [r["name"] for r in S.ROWS])
def test_row_is_not_vacuous(name):
    r, lims, p = S.inputs(name)
    gpt, want = S.expected(name)
    for g, w in zip(gpt, want):
        pairwise = np.stack([g[:, lo - 1:hi].sum(axis=1, dtype=np.float32) for lo, hi in lims], axis=1)
        np.testing.assert_allclose(w, pairwise, rtol=1e-5)
        assert w.shape == (S.NCOL, len(lims)) and np.isfinite(w).all()
    # the order of the additions is under test: in some (column, band) the two sums differ in bits
    assert any((bits(w) != bits(np.stack([g[:, lo - 1:hi].sum(axis=1, dtype=np.float32) for lo, hi in lims], axis=1))).any()
               for g, w in zip(gpt, want)), name
    aer = "aer" in r["kind"]
    sums = lambda a, c: [S.B.sum_byband(g, lims) for g in S.gpt_fluxes(name, a, c)]  # noqa: E731
    if "mask" in r["kind"]:
        for other in ("whole", None):
            assert all((bits(w) != bits(o)).any() for w, o in zip(want, sums(aer, other))), (name, other)
    if aer:
        cloud = "masked" if "mask" in r["kind"] else "whole"
        assert all((bits(w) != bits(o)).any() for w, o in zip(want, sums(False, cloud))), name
    assert p["daylit"].any() and (want[2][p["daylit"]] > 0).any(axis=1).all(), name
    # the total down flux holds the direct one
    assert (want[1] >= want[2]).all()


# ---- the policy ---------------------------------------------------------------------------------------------------------
def build_and_run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    cmd = [os.environ.get("CXX", "c++"), "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-I", CSRC,
           os.path.join(ROOT, "tests", "sfc_byband_policy_host.cpp"), os.path.join(CSRC, "requests.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and not r.stderr, r.stderr[-3000:]
    return r.stdout


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    return build_and_run(tmp_path_factory.mktemp("sfc_byband_policy"), "plain", [])


def parse(text):
    """-> entry -> (cell, sfc) -> (status, the rest of the line)"""
    out = {}
    for line in text.splitlines():
        entry, *cell, status, rest = line.split(" ", 8)
        out.setdefault(entry, {})[(tuple(int(v) for v in cell[:5]), int(cell[5]))] = (int(status), rest)
    return out


def test_every_row_and_cell_is_walked(output):
    import request_policy_cells as C
    got = parse(output)
    assert len(got) == 15 and set(TAKERS) < set(got)
    assert {e for e in got} == {s for s in C.SYMBOLS if not s.endswith("_gpt")}
    for e in got:
        assert sorted({c for c, _ in got[e]}) == C.CELLS and {s for _, s in got[e]} == {0, 1, 2, 3, 4}


def test_not_armed_changes_nothing(output):
    for e, cells in parse(output).items():
        for (cell, s), answer in cells.items():
            if s == 1:
                assert answer == cells[(cell, 0)], (e, cell)
            if s == 0:
                assert "sfc_bnd" not in answer[1] or answer[0] != OK, (e, cell, answer)


def test_armed_answers(output):
    accepted = 0
    for e, cells in parse(output).items():
        for (cell, s), (status, rest) in cells.items():
            if s < 2:
                continue
            base = cells[(cell, 0)]
            byband, mask, jacobian, aerosol, active = cell
            if base[0] != OK:   # an earlier request's refusal stands, word for word
                assert (status, rest) == base, (e, cell, s)
            elif e not in TAKERS:
                assert status == ERR_ARGUMENT and all(t in rest for t in TAKERS), (e, cell, s, rest)
            elif byband:   # alone, or beside the mask as the _byband_mcica pair
                assert mask in (0, 2) and not aerosol, (e, cell)
                assert status == ERR_UNSUPPORTED and "by-band" in rest, (e, cell, s, rest)
            elif not mask and not aerosol:
                assert status == ERR_UNSUPPORTED and "rrtmgpnn_solver_request_byband" in rest, (e, cell, s, rest)
            elif s == 3:
                assert status == ERR_ARGUMENT and "ncol" in rest, (e, cell, s, rest)
            elif s == 4:
                assert status == ERR_ARGUMENT and "band limits" in rest, (e, cell, s, rest)
            else:
                assert not jacobian and mask in (0, 1) and aerosol in (0, 2) and active in (0, 1), (e, cell)
                assert status == OK and rest == base[1] + "sfc_bnd,", (e, cell, rest)
                accepted += 1
    # {mask, mask + aerosol, aerosol} x {the count or not} on the two entries
    assert accepted == 2 * 3 * 2


def test_under_the_sanitizers(tmp_path, output):
    flags = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    assert build_and_run(tmp_path, "sanitized", flags) == output
