"""GPU: the shortened correctly-rounded sequences the kernels use (libm_ref.hpp rcp_rn_normal, sqrt_rn_normal,
div_rn_normal as solver_div, div_softsign; x2_device.hpp rcp2, sqrt2, div2 on both lanes)
equal the IEEE results on EVERY float of their domains, and the libm restatements (ref_expf_neg, ref_expf_neg_batch<4>,
ref_logf_nb, ref_cosf, ref_tanhf) equal the host's libm, checked on the device itself (v_rcp_f32 is a hardware approximation no
host can emulate bit for bit): tools/exhaustive_ops.hip, built by __graft_entry__.build() against the product's own
headers -- the "shipped:" rows call the functions the kernels call, not copies of them.  The reference column (the
compiler's IEEE sequence) is cross-checked against a double-precision evaluation rounded once.

One measured run of the whole tool on an MI355X box took 2 s (19e9 device evaluations; 4.3e9 host libm calls on 16
threads); the subprocess gets MEASURED_RUN_S (that, rounded up) times 40, the old 120 s, so that a loaded host's slower
libm threads do not fail the test."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tools", "exhaustive_ops")
MEASURED_RUN_S = 3
SW_NUMERATORS = 8


def test_shortened_division_sequences_are_exact_on_their_domains():
    if not os.path.exists(EXE):
        pytest.skip("tools/exhaustive_ops not built (__graft_entry__.build())")
    r = subprocess.run(["timeout", "-k", "10", str(40 * MEASURED_RUN_S), EXE], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    res = {}
    for line in r.stdout.splitlines():
        m = re.match(r"(\S+)\s+(\S+)\s+inputs (\d+) mismatches (\d+)", line)
        if m:
            res[(m.group(1), m.group(2))] = (int(m.group(3)), int(m.group(4)))
    shipped = [("rcp", "newton+1corr"), ("sqrt", "current"), ("soft+<", "2corr-negres"), ("soft-<", "2corr-negres")]
    for key in shipped + [k for k in res if k[1] == "ref-vs-double"]:
        n, bad = res[key]
        assert n > 100_000_000 and bad == 0, (key, n, bad)
    # the product's own functions, through its headers
    by_header = [("rcp", "shipped:rcp_rn_normal"), ("rcp", "shipped:rcp2.x"), ("rcp", "shipped:rcp2.y"),
                 ("sqrt", "shipped:sqrt_rn_normal"), ("sqrt", "shipped:sqrt2.x"), ("sqrt", "shipped:sqrt2.y"),
                 ("sqrt<", "shipped:sqrt_rn_normal"), ("sqrt<", "shipped:sqrt2.x"), ("sqrt<", "shipped:sqrt2.y"),
                 ("soft+<", "shipped:div_softsign"), ("soft-<", "shipped:div_softsign")]
    # the solvers' divisions in the LW use, (1 - T) / t on every t of (sqrt(FLT_EPSILON), 2^126] (past 2^126 the tool
    # reports solver_div for the record: every quotient differs there, which is the operand bound include/rrtmgpnn.h
    # states for the LW entry points)
    by_header += [("divlw", "shipped:" + v) for v in ("solver_div", "div2.x", "div2.y", "div2(scalar)")]
    # ... and in the SW use: every denominator of [eps, 1] and [-4, -eps] under eight numerators
    for i in range(SW_NUMERATORS):
        by_header += [("divsw%s%d" % (s, i), "shipped:" + v) for s in "+-"
                      for v in ("solver_div", "div2.x", "div2.y", "div2(scalar)")]
    by_header += [("exp", "shipped:ref_expf_neg"), ("exp", "shipped:ref_expf_neg_batch4"),
                  ("log", "shipped:ref_logf_nb"), ("log", "shipped:ref_logf"), ("cos", "shipped:ref_cosf"),
                  # the MLPs' tanh activation: glibc's tanhf on every float of [-10, 10]
                  ("tanh+", "shipped:ref_tanhf"), ("tanh-", "shipped:ref_tanhf")]
    for key in by_header:
        n, bad = res[key]
        assert n > 100_000_000 and bad == 0, (key, n, bad)
    # the short runs: the strided sample of exp below -105, and -inf
    for key, least in ((("exp<", "shipped:ref_expf_neg"), 1_000_000),
                       (("exp<", "shipped:ref_expf_neg_batch4"), 1_000_000), (("exp-inf", "shipped:ref_expf_neg"), 1),
                       (("exp-inf", "shipped:ref_expf_neg_batch4"), 1)):
        n, bad = res[key]
        assert n >= least and bad == 0, (key, n, bad)
