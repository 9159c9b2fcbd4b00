"""CPU: the request policy (csrc/requests.cpp) without a device.  tests/request_policy_host.cpp walks the cells of
tests/request_policy_cells.py through apply_requests for every row of the table; the refusals are held to
tests/golden/request_policy.json (the parent commit's answers, recorded from its library) under the two rules of
request_policy_cells.compare, the accepted cells to the extras they must set.  The program is built with the host
compiler alone -- the unit includes no HIP header -- and once more with the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

import request_policy_cells as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rte-rrtmgp-nn_amd", "csrc")

def build_and_run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    cmd = [os.environ.get("CXX", "c++"), "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-I", CSRC,
           os.path.join(ROOT, "tests", "request_policy_host.cpp"), os.path.join(CSRC, "requests.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and not r.stderr, r.stderr[-3000:]
    return r.stdout


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    return build_and_run(tmp_path_factory.mktemp("request_policy"), "plain", [])


def parse(text):
    """-> symbol -> cell -> (status, the rest of the line)"""
    out = {}
    for line in text.splitlines():
        symbol, *cell, status, rest = line.split(" ", 7)
        out.setdefault(symbol, {})[tuple(int(v) for v in cell)] = (int(status), rest)
    return out


def test_refusals_follow_the_parent(output):
    got = parse(output)
    assert sorted(got) == sorted(C.SYMBOLS) and all(sorted(got[s]) == C.CELLS for s in got)
    # the entry itself turns an accepted cell into its "bad argument" (tau is null in the recorded calls)
    new = {s: [C.accepted(s) if got[s][c][0] == 0 else got[s][c] for c in C.CELLS] for s in C.SYMBOLS}
    failures, cells, groups = C.rule_b_summary(C.golden(), new)
    assert not failures, "%d cells, the first: %s" % (len(failures), failures[:3])
    assert cells == C.RULE_B_CELLS and groups == C.RULE_B_GROUPS, (cells, sorted(groups ^ C.RULE_B_GROUPS))


def test_accepted_cells_set_what_was_armed_and_nothing_else(output):
    got, n = parse(output), 0
    for s in C.SYMBOLS:
        for cell, (status, rest) in got[s].items():
            if status:
                continue
            byband, mask, jacobian, aerosol, active = cell
            want = set()
            want |= {"byband"} if byband else set()
            want |= {"mask_bits"} if mask else set()
            want |= {"jac_up"} | ({"sfc_jac"} if jacobian == 1 else set()) if jacobian else set()
            want |= {"aer_tau"} | ({"aer_ssa", "aer_g"} if C.aerosol_is_2str(s, aerosol) else set()) if aerosol else set()
            want |= {"nact"} if active else set()
            assert set(filter(None, rest.split(","))) == want, (s, cell, rest)
            n += 1
    assert n == sum(a == C.accepted(s) for s, answers in C.golden().items() for a in answers)


def test_under_the_sanitizers(tmp_path, output):
    flags = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    assert build_and_run(tmp_path, "sanitized", flags) == output
