"""GPU: which solver kernel instance serves which call (rrtmgpnn_context_get_solver_path), family by family.

Every solver kernel family takes one compile-time options value and compiles one list of instances; a launcher maps the
call to the value and the list to the kernel.  The plane / plane-free, band-pair / general, dual / two-launch and
one- / two-per-lane instances give the same bits by design, so a wrong instance passes every flux comparison: only the
path tells.  Each row below is one public call, the (family, options, launches) it must report, and the lines of the
launch ladders it was read from -- the ladders of the commit before the options existed (b84c312):

  LW no scattering    csrc/kernels_rte.hip:735-803       lw_noscat_kernel<kFused, kInc, PF, kMulti, kBand, kDual, kMask,
                                                         kMaskS, kJac, kAer>
  SW checkpointed     csrc/kernels_sw_ck.hip:826-1026    sw_2stream_ck_kernel<kHasG, kInc, K, kGpt, R, WAVES, kTn, V, kEmk,
                                                         kBandPair, P1C, AHEAD, kBand, kMask, kAer, kDual>
  LW rescaled, fused  csrc/kernels_lw_scat.hip:865-876   lw_rescl_planck_inc_kernel<kMask, PF, kAer, kDual>
  LW rescaled         csrc/kernels_lw_scat.hip:804-815   lw_rescl_kernel<kBand, kJac>
  SW one per lane     csrc/kernels_rte.hip:1237-1246     sw_2stream_kernel<kHasG, kInc, PF, kGpt, kBand>
  SW two per lane     csrc/kernels_sw_x2.hip:336-345     sw_2stream_x2_kernel<kHasG, kInc, PF, kBand>

The option bits are those include/rrtmgpnn.h documents with the getter.  path[3] is the number of instances the family
compiles: every family's rows must reach that many different options values, so an instance without a row fails the
test, and so does a row that reaches an instance outside the table.

Rows that solve the same problem (same inputs, same physics) through different instances also compare their fluxes bit
for bit with the first such row: the check the existing tests make pairwise, here across the whole table.

Shapes: 3 columns, 4 layers, 32 g-points in two bands of 16 (the band-pair layout) unless the branch needs another:
bands 1-15 / 16-32 for the general increment, 64 g-points for the wave-uniform mask pair, 31 for the odd-ngpt SW kernel,
and ncol * ngpt / 2 above 64 * 16 * CUs (the device's count) for the large-grid SW instances.  The plane-free SW
instances run in a child process with RRTMGPNN_SW_NO_PLANES=1, as tests/test_gpu_sw_planes.py runs them.
"""
import ctypes
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32

# families and option bits (include/rrtmgpnn.h, rrtmgpnn_context_get_solver_path)
LW_NOSCAT, SW_CK, LW_RESCL_INC, LW_RESCL, SW_1, SW_X2 = 1, 2, 3, 4, 5, 6
FUSED, INC, MULTI, BAND, DUAL, MASK, MASKS, JAC, AER = 1, 2, 4, 8, 16, 32, 64, 128, 256          # lw_noscat_kernel
FI = FUSED | INC
CK_G, CK_INC, CK_GPT, CK_TN, CK_EMK, CK_PAIR, CK_BAND, CK_MASK, CK_AER, CK_DUAL, CK_SMALL = (
    1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024)                                                   # sw_2stream_ck_kernel
# the planes each instance family keeps (kCkTn* / kCkEmk* of kernels_sw_ck.hip): all sky and dual the transmittances,
# the small-grid and the large clear-sky NN instance both
PL_INC, PL_DUAL, PL_SMALL, PL_NN = CK_TN, CK_TN, CK_TN | CK_EMK, CK_TN | CK_EMK
SC_MASK, SC_AER, SC_DUAL = 1, 2, 4                                                                 # lw_rescl_planck_inc_kernel
RS_BAND, RS_JAC = 1, 2                                                                             # lw_rescl_kernel
SW_G, SW_INC, SW_GPT, SW_BAND = 1, 2, 4, 8                                                         # sw_2stream(_x2)_kernel

PAIR_LIMS = ((1, 16), (17, 32))
GENERAL_LIMS = ((1, 15), (16, 32))   # band 2 starts at an even 1-based g-point: fails the band-pair test
ODD_LIMS = ((1, 16), (17, 31))
LIMS64 = ((1, 32), (33, 64))


def R(name, call, family, options, launches=1, same=None, **kw):
    return dict(name=name, call=call, family=family, options=options, launches=launches, same=same, kw=kw)


def _lw_base(call, base, tag):
    """{one angle, several} x {broadband, by band, Jacobian}: kernels_rte.hip:798-803 at <kFused, kInc> of `base`"""
    same = lambda n: (tag, n)
    return [R("%s-%s" % (tag, s), call, LW_NOSCAT, base | o, same=same(n), nmus=n, **kw)
            for s, o, n, kw in (("1", 0, 1, {}), ("3", MULTI, 3, {}), ("bb1", BAND, 1, dict(bb=True)),
                                ("bb3", BAND | MULTI, 3, dict(bb=True)), ("jac1", JAC, 1, dict(jac=True)),
                                ("jac3", JAC | MULTI, 3, dict(jac=True)))]


LW_ROWS = (
    _lw_base("lw_arrays", 0, "arrays") + _lw_base("lw_planck", FUSED, "planck") + _lw_base("lw_planck_inc", FI, "inc") + [
        # masked twins, kernels_rte.hip:776-793
        R("inc-mask1", "lw_planck_inc", LW_NOSCAT, FI | MASK, same=("incm", 1), nmus=1, mask=True),             # :791
        R("inc-mask3", "lw_planck_inc", LW_NOSCAT, FI | MASK | MULTI, same=("incm", 3), nmus=3, mask=True),     # :790
        R("inc-mask-bb1", "lw_planck_inc", LW_NOSCAT, FI | MASK | BAND, same=("incm", 1), nmus=1, mask=True, bb=True),   # :789
        R("inc-mask-bb3", "lw_planck_inc", LW_NOSCAT, FI | MASK | BAND | MULTI, same=("incm", 3), nmus=3, mask=True,
          bb=True),                                                                                             # :788
        R("inc-mask-jac1", "lw_planck_inc", LW_NOSCAT, FI | MASK | JAC, same=("incm", 1), nmus=1, mask=True, jac=True),  # :783
        R("inc-mask-jac3", "lw_planck_inc", LW_NOSCAT, FI | MASK | JAC | MULTI, same=("incm", 3), nmus=3, mask=True,
          jac=True),                                                                                            # :782
        # aerosol twins, :766-773
        R("inc-aer1", "lw_planck_inc", LW_NOSCAT, FI | AER, same=("inca", 1), nmus=1, aer=True),                # :771
        R("inc-aer3", "lw_planck_inc", LW_NOSCAT, FI | AER | MULTI, same=("inca", 3), nmus=3, aer=True),        # :770
        R("inc-aer-mask1", "lw_planck_inc", LW_NOSCAT, FI | AER | MASK, same=("incam", 1), nmus=1, aer=True, mask=True),  # :769
        R("inc-aer-mask3", "lw_planck_inc", LW_NOSCAT, FI | AER | MASK | MULTI, same=("incam", 3), nmus=3, aer=True,
          mask=True),                                                                                           # :768
        # clear beside all sky: the dual instances, :736-763 (mode 1), and the two launches of mode 2 or several angles
        R("dual", "lw_clr_all", LW_NOSCAT, FI | DUAL, same=("inc", 1), nmus=1, mode=1),                         # :760
        R("dual-mask-word", "lw_clr_all", LW_NOSCAT, FI | DUAL | MASK, same=("incm", 1), nmus=1, mode=1, mask=True),  # :756
        R("dual-mask-pair", "lw_clr_all", LW_NOSCAT, FI | DUAL | MASK | MASKS, nmus=1, mode=1, mask=True, ngpt=64,
          same=("incm64", 1)),                                                                                  # :754
        R("dual-mask-word64", "lw_clr_all", LW_NOSCAT, FI | DUAL | MASK, nmus=1, mode=1, mask=True, ngpt=64,
          mask_offset=1, same=("incm64", 1)),                                          # :756, the pointer one word off 8 bytes
        R("dual-aer", "lw_clr_all", LW_NOSCAT, FI | DUAL | AER, same=("inca", 1), nmus=1, mode=1, aer=True),    # :746
        R("dual-aer-mask-word", "lw_clr_all", LW_NOSCAT, FI | DUAL | AER | MASK, same=("incam", 1), nmus=1, mode=1,
          aer=True, mask=True),                                                                                 # :744
        R("dual-aer-mask-pair", "lw_clr_all", LW_NOSCAT, FI | DUAL | AER | MASK | MASKS, nmus=1, mode=1, aer=True,
          mask=True, ngpt=64),                                                                                  # :742
        R("two-launch", "lw_clr_all", LW_NOSCAT, FI, 2, same=("inc", 1), nmus=1, mode=2),                       # :844-845
        R("two-launch-angles", "lw_clr_all", LW_NOSCAT, FI | MULTI, 2, same=("inc", 3), nmus=3, mode=1),        # :828
        R("two-launch-mask", "lw_clr_all", LW_NOSCAT, FI | MASK, 2, same=("incm", 1), nmus=1, mode=2, mask=True),
        R("two-launch-aer", "lw_clr_all", LW_NOSCAT, FI | AER, 2, same=("inca", 1), nmus=1, mode=2, aer=True),  # :841-842
    ])

# kernels_lw_scat.hip:865-876 (dual: mode 1 of rrtmgpnn_context_set_lw_scat_clr_all; mode 2: the no-scattering clear
# launch, then the instance without kDual) and :804-815
SCAT_ROWS = [
    R("scat", "lw_scat_inc", LW_RESCL_INC, 0, same=("scat",), nmus=1),                                          # :875
    R("scat-mask", "lw_scat_inc", LW_RESCL_INC, SC_MASK, same=("scatm",), nmus=1, mask=True),                   # :874
    R("scat-angles", "lw_scat_inc", LW_RESCL_INC, 0, nmus=3),                                                   # :875
    R("scat-aer", "lw_scat_clr_all", LW_RESCL_INC, SC_AER, 2, same=("scata",), nmus=1, mode=2, aer=True),       # :872
    R("scat-aer-mask", "lw_scat_clr_all", LW_RESCL_INC, SC_AER | SC_MASK, 2, same=("scatam",), nmus=1, mode=2, aer=True,
      mask=True),                                                                                               # :871
    R("scat-two-launch", "lw_scat_clr_all", LW_RESCL_INC, 0, 2, same=("scat",), nmus=1, mode=2),
    R("scat-dual", "lw_scat_clr_all", LW_RESCL_INC, SC_DUAL, same=("scat",), nmus=1, mode=1),                   # :869
    R("scat-dual-mask", "lw_scat_clr_all", LW_RESCL_INC, SC_DUAL | SC_MASK, same=("scatm",), nmus=1, mode=1, mask=True),  # :868
    R("scat-dual-aer", "lw_scat_clr_all", LW_RESCL_INC, SC_DUAL | SC_AER, same=("scata",), nmus=1, mode=1, aer=True),  # :867
    R("scat-dual-aer-mask", "lw_scat_clr_all", LW_RESCL_INC, SC_DUAL | SC_AER | SC_MASK, same=("scatam",), nmus=1,
      mode=1, aer=True, mask=True),                                                                             # :866
    R("scat-dual-angles", "lw_scat_clr_all", LW_RESCL_INC, 0, 2, nmus=3, mode=1),          # :893: one angle only
]
RESCL_ROWS = [
    R("rescl", "lw_rescl", LW_RESCL, 0, same=("rescl", 1), nmus=1),                                             # :813
    R("rescl-angles", "lw_rescl", LW_RESCL, 0, same=("rescl", 3), nmus=3),
    R("rescl-bb", "lw_rescl", LW_RESCL, RS_BAND, same=("rescl", 1), nmus=1, bb=True),                           # :809
    R("rescl-jac", "lw_rescl", LW_RESCL, RS_JAC, same=("rescl", 1), nmus=1, jac=True),                          # :805
    R("rescl-jac-angles", "lw_rescl", LW_RESCL, RS_JAC, same=("rescl", 3), nmus=3, jac=True),
]


def _sw_key(g=False, lims=None, mask=False, aer=False, ngpt=32, large=False, gpt=False, **_):
    return ("sw", bool(g), lims, bool(mask), bool(aer), ngpt, bool(large), bool(gpt))


def S(name, call, family, options, launches=1, **kw):
    return R(name, call, family, options, launches, same=_sw_key(**kw), **kw)


def _sw_lane_rows(family, kernel, tag, gpt_rows):
    """kernels_rte.hip:1237-1246 (mode 1, or odd ngpt) and kernels_sw_x2.hip:336-345 (mode 2): {gas g} x {increment} x
    {broadband, by band}; the one-per-lane kernel also has the g-point instances, which only odd ngpt reaches"""
    rows = []
    for g in (False, True):
        o = SW_G if g else 0
        rows += [S("%s-%s" % (tag, "g" if g else "nog"), "sw", family, o, kernel=kernel, g=g),
                 S("%s-bb-%s" % (tag, "g" if g else "nog"), "sw", family, o | SW_BAND, kernel=kernel, g=g, bb=True),
                 S("%s-inc-%s" % (tag, "g" if g else "nog"), "sw_inc", family, o | SW_INC, kernel=kernel, g=g,
                   lims=PAIR_LIMS),
                 S("%s-inc-bb-%s" % (tag, "g" if g else "nog"), "sw_inc", family, o | SW_INC | SW_BAND, kernel=kernel,
                   g=g, lims=GENERAL_LIMS, bb=True)]
        if gpt_rows:
            rows += [S("%s-gpt-%s" % (tag, "g" if g else "nog"), "sw_gpt", family, o | SW_GPT, kernel=0, g=g, ngpt=31,
                       gpt=True)]
    return rows


SW1_ROWS = _sw_lane_rows(SW_1, 1, "sw1", True) + [
    S("sw1-odd", "sw", SW_1, SW_G, kernel=0, g=True, ngpt=31),                                    # odd ngpt, any mode
    S("sw1-odd-inc", "sw_inc", SW_1, SW_INC, kernel=0, g=False, ngpt=31, lims=ODD_LIMS)]
SWX2_ROWS = _sw_lane_rows(SW_X2, 2, "x2", False)


def _ck_rows(planes):
    """The instances whose workspace planes launch_sw_2stream's fallback drops (kernels_sw_ck.hip at the parent): with
    the planes of their family, or (the child process) without"""
    t = "" if planes else "-noplanes"
    pd, pi, pn = (PL_DUAL, PL_INC, PL_NN) if planes else (0, 0, 0)
    rows = []
    for g in (False, True):
        og, tg = (CK_G if g else 0), ("g" if g else "nog")
        for mask in (False, True):
            om, tm = (CK_MASK if mask else 0), ("-mask" if mask else "")
            for aer in (False, True):
                oa, ta = (CK_AER if aer else 0), ("-aer" if aer else "")
                # :851-865, the dual instances (mode 1 of rrtmgpnn_context_set_sw_clr_all)
                rows.append(S("ck-dual%s%s-%s%s" % (tm, ta, tg, t), "sw_clr_all", SW_CK,
                              CK_DUAL | CK_INC | pd | og | om | oa, g=g, mask=mask, aer=aer, lims=PAIR_LIMS, mode=1))
            # :886-909, aerosol + (masked) cloud, the band-pair layout
            rows.append(S("ck-aer%s-%s%s" % (tm, tg, t), "sw_inc", SW_CK, CK_AER | CK_INC | CK_PAIR | pi | og | om, g=g,
                          mask=mask, aer=True, lims=PAIR_LIMS))
        for lims, op, tp in ((PAIR_LIMS, CK_PAIR, "pair"), (GENERAL_LIMS, 0, "general")):
            # :935-958, the masked increment; :1000-1015, the increment
            rows.append(S("ck-mask-%s-%s%s" % (tp, tg, t), "sw_inc", SW_CK, CK_MASK | CK_INC | pi | op | og, g=g,
                          mask=True, lims=lims))
            rows.append(S("ck-inc-%s-%s%s" % (tp, tg, t), "sw_inc", SW_CK, CK_INC | pi | op | og, g=g, lims=lims))
    # :1024-1026, the large-grid clear-sky NN instance
    rows.append(S("ck-nn-large%s" % t, "sw", SW_CK, pn, g=False, large=True))
    return rows


CK_ROWS = _ck_rows(True) + [
    # by band under the mask, no planes either way: :923-933
    S("ck-mask-bb-pair-g", "sw_inc", SW_CK, CK_MASK | CK_INC | CK_BAND | CK_PAIR | CK_G, g=True, mask=True, bb=True,
      lims=PAIR_LIMS),
    S("ck-mask-bb-pair-nog", "sw_inc", SW_CK, CK_MASK | CK_INC | CK_BAND | CK_PAIR, g=False, mask=True, bb=True,
      lims=PAIR_LIMS),
    S("ck-mask-bb-general-g", "sw_inc", SW_CK, CK_MASK | CK_INC | CK_BAND | CK_G, g=True, mask=True, bb=True,
      lims=GENERAL_LIMS),
    S("ck-mask-bb-general-nog", "sw_inc", SW_CK, CK_MASK | CK_INC | CK_BAND, g=False, mask=True, bb=True,
      lims=GENERAL_LIMS),
    # g-point outputs (even ngpt takes the checkpointed kernel whatever the mode): :962-963
    S("ck-gpt-g", "sw_gpt", SW_CK, CK_GPT | CK_G, g=True, gpt=True),
    S("ck-gpt-nog", "sw_gpt", SW_CK, CK_GPT, g=False, gpt=True, kernel=2),
    # by band: :969-993
    S("ck-bb-small", "sw", SW_CK, CK_BAND | CK_SMALL | PL_SMALL, g=False, bb=True),                             # :970
    S("ck-bb-pair-g", "sw_inc", SW_CK, CK_BAND | CK_INC | CK_PAIR | CK_G, g=True, bb=True, lims=PAIR_LIMS),     # :978
    S("ck-bb-pair-nog", "sw_inc", SW_CK, CK_BAND | CK_INC | CK_PAIR, g=False, bb=True, lims=PAIR_LIMS),         # :981
    S("ck-bb-general-g", "sw_inc", SW_CK, CK_BAND | CK_INC | CK_G, g=True, bb=True, lims=GENERAL_LIMS),         # :984
    S("ck-bb-general-nog", "sw_inc", SW_CK, CK_BAND | CK_INC, g=False, bb=True, lims=GENERAL_LIMS),             # :987
    S("ck-bb-g", "sw", SW_CK, CK_BAND | CK_G, g=True, bb=True),                                                 # :990
    S("ck-bb-large", "sw", SW_CK, CK_BAND, g=False, bb=True, large=True),                                       # :992
    # clear sky: :1017-1023
    S("ck-g", "sw", SW_CK, CK_G, g=True),                                                                       # :1017
    S("ck-small", "sw", SW_CK, CK_SMALL | PL_SMALL, g=False),                                                   # :1021
    # the clear + all-sky entry's two launches (mode 2): the all-sky launch, then the clear one (api.cpp)
    S("ck-two-launch", "sw_clr_all", SW_CK, CK_SMALL | PL_SMALL, 2, g=False, lims=PAIR_LIMS, mode=2),
    S("ck-two-launch-aer", "sw_clr_all", SW_CK, CK_INC | CK_PAIR | PL_INC | CK_G, 2, g=True, aer=True, lims=PAIR_LIMS,
      mode=2),
]
CK_CHILD_ROWS = _ck_rows(False)

FAMILY_ROWS = {"lw_noscat": (LW_NOSCAT, LW_ROWS), "lw_rescl_planck_inc": (LW_RESCL_INC, SCAT_ROWS),
               "lw_rescl": (LW_RESCL, RESCL_ROWS), "sw_2stream": (SW_1, SW1_ROWS), "sw_2stream_x2": (SW_X2, SWX2_ROWS),
               "sw_2stream_ck": (SW_CK, CK_ROWS + CK_CHILD_ROWS)}


# ---- inputs: built once per shape, read-only ---------------------------------------------------------------------
def _large_shape():
    """(ncol, nlay, ngpt) past the small-grid bound ncol * ngpt / 2 <= 64 * 16 * CUs of this device"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    ngpt = 256
    return 64 * 16 * cus // (ngpt // 2) + 52, 3, ngpt


@functools.lru_cache(maxsize=None)
def problem(ncol, nlay, ngpt, nb):
    from rrtmgpnn import data
    kl = data.load_kdist("lw")
    rng = np.random.default_rng(1000 * ngpt + 10 * nlay + nb)
    u = lambda lo, hi, *s: rng.uniform(lo, hi, s).astype(F32)
    p = dict(tau=rng.lognormal(-2, 1.5, (ncol, nlay, ngpt)).astype(F32), ssa=u(0.1, 0.95, ncol, nlay, ngpt),
             g=u(0, 0.9, ncol, nlay, ngpt), mu0=u(0.1, 1, ncol), toa=u(0.1, 10, ncol, ngpt), alb=u(0, 0.9, ncol, ngpt),
             tb=rng.lognormal(-1, 1, (ncol, nlay, nb)).astype(F32), wb=u(0.3, 0.95, ncol, nlay, nb),
             gb=u(0.3, 0.9, ncol, nlay, nb), ta=rng.lognormal(-2, 1, (ncol, nlay, nb)).astype(F32),
             wa=u(0.5, 0.95, ncol, nlay, nb), ga=u(0.3, 0.8, ncol, nlay, nb),
             mask=rng.integers(0, 2 ** 32, (ncol, nlay, (ngpt + 31) // 32), dtype=np.uint32),
             pfrac=u(0, 0.2, ncol, nlay, ngpt), tlay=u(200, 300, ncol, nlay), tlev=u(200, 300, ncol, nlay + 1),
             tsfc=u(250, 310, ncol), emis=u(0.9, 1, ncol, ngpt), inc=u(0, 2, ncol, ngpt), lay=u(1, 3, ncol, nlay, ngpt),
             lev=u(1, 3, ncol, nlay + 1, ngpt), sfc=u(1, 3, ncol, ngpt), sfc_jac=u(0.01, 0.1, ncol, ngpt),
             totplnk=np.ascontiguousarray(kl["totplnk"][:nb]))
    for a in p.values():
        a.setflags(write=False)
    p["planck"] = (int(kl["nPlanckTemp"]), float(kl["temp_ref_min"][0]), float(kl["totplnk_delta"]))
    return p


class Runner:
    """One context of its own (the modes are set on it, not on the library defaults) and the device copies."""

    def __init__(self):
        from rrtmgpnn import _lib, api
        self.L, self.lib = _lib.lib(), _lib
        self.ctx = api.Context(0)
        self.dev = torch.device("cuda", 0)
        self._dev = {}

    def arrays(self, ncol, nlay, ngpt, nb):
        key = (ncol, nlay, ngpt, nb)
        if key not in self._dev:
            p = problem(*key)
            self._dev[key] = {k: torch.as_tensor(np.array(v), device=self.dev) for k, v in p.items() if k != "planck"}
        return self._dev[key], problem(*key)["planck"]

    def path(self):
        out = (ctypes.c_int * 4)()
        self.lib.check(self.L.rrtmgpnn_context_get_solver_path(self.ctx.h, out), "get_solver_path")
        return list(out)

    def run(self, row):
        """The row's call -> (path, {output name: numpy array})"""
        kw = dict(row["kw"])
        call = row["call"]
        sw = call.startswith("sw")
        large = kw.get("large", False)
        ncol, nlay, ngpt = _large_shape() if large else (3, 4, kw.get("ngpt", 32))
        lims = kw.get("lims") or (LIMS64 if ngpt == 64 else (ODD_LIMS if ngpt == 31 else PAIR_LIMS))
        nb = len(lims)
        a, (ntemp, tmin, tdelta) = self.arrays(ncol, nlay, ngpt, nb)
        P = lambda t: t.data_ptr() if t is not None else None
        new = lambda *s: torch.full(s, float("nan"), device=self.dev)
        L, c, check = self.L, self.ctx.h, self.lib.check
        lims_c = self.lib.int_array(np.asarray(lims).ravel())
        out = {}
        # modes, then requests (armed for the next call)
        check(L.rrtmgpnn_context_set_sw_kernel(c, kw.get("kernel", 0)), "set_sw_kernel")
        mode = kw.get("mode", 0)
        check(L.rrtmgpnn_context_set_lw_clr_all(c, mode), "set_lw_clr_all")
        check(L.rrtmgpnn_context_set_lw_scat_clr_all(c, mode), "set_lw_scat_clr_all")
        check(L.rrtmgpnn_context_set_sw_clr_all(c, mode), "set_sw_clr_all")
        mask = None
        if kw.get("mask"):
            off = kw.get("mask_offset", 0)
            buf = torch.zeros(a["mask"].numel() + off, dtype=torch.int32, device=self.dev)
            buf[off:] = a["mask"].view(torch.int32).ravel()
            mask = buf.data_ptr() + 4 * off
            out["_keep"] = buf
        nlev = nlay + 1
        if kw.get("bb"):
            bnd = [new(ncol, nlev, nb) for _ in range(3 if sw else 2)]
            bp = [P(t) for t in bnd] + ([] if sw else [None])
            if mask is not None:
                check(L.rrtmgpnn_solver_request_byband_mcica(c, nb, lims_c, *bp, ngpt, nlay, ncol, mask), "byband_mcica")
            else:
                check(L.rrtmgpnn_solver_request_byband(c, nb, lims_c, *bp), "byband")
            out.update({"bnd%d" % i: t for i, t in enumerate(bnd)})
        elif mask is not None and call not in ("lw_clr_all",):
            check(L.rrtmgpnn_solver_request_cloud_mask(c, ngpt, nlay, ncol, mask), "cloud_mask")
        if kw.get("jac"):
            out["jac"] = new(ncol, nlev)
            fused = call in ("lw_planck", "lw_planck_inc")
            check(L.rrtmgpnn_solver_request_jacobian(c, ngpt, nlay, ncol, None if fused else P(a["sfc_jac"]),
                                                     P(out["jac"])), "jacobian")
        if kw.get("aer"):
            check(L.rrtmgpnn_solver_request_aerosol(c, nb, nlay, ncol, P(a["ta"]), P(a["wa"]) if sw else None,
                                                    P(a["ga"]) if sw else None), "aerosol")
        names = ("up", "dn", "dir") if sw else ("up", "dn")
        fl = [new(ncol, nlev) for _ in names]
        out.update(zip(names, fl))
        clr = []
        if call.endswith("clr_all"):
            clr = [new(ncol, nlev) for _ in names]
            out.update(zip(["clr_" + n for n in names], clr))
        if sw:
            head = [c, ngpt, nlay, ncol, 1, P(a["toa"]), None, P(a["tau"]), P(a["ssa"]), P(a["g"]) if kw.get("g") else None]
            tail = [P(a["mu0"]), P(a["alb"]), P(a["alb"])] + [P(t) for t in fl]
            bands = [nb, lims_c, P(a["tb"]), P(a["wb"]), P(a["gb"])]
            if call == "sw":
                check(L.rrtmgpnn_sw_solver_2stream(*head, *tail), row["name"])
            elif call == "sw_gpt":
                gp = [new(ncol, nlev, ngpt) for _ in range(3)]
                out.update({"gpt%d" % i: t for i, t in enumerate(gp)})
                check(L.rrtmgpnn_sw_solver_2stream_gpt(*head, *tail, *[P(t) for t in gp]), row["name"])
            elif call == "sw_inc":
                check(L.rrtmgpnn_sw_solver_2stream_inc(*head, *bands, *tail), row["name"])
            else:
                check(L.rrtmgpnn_sw_solver_2stream_clr_all(*head, *bands, *tail, *[P(t) for t in clr]), row["name"])
        else:
            from rrtmgpnn.api import GAUSS_DS, GAUSS_WTS
            nmus = kw["nmus"]
            head = [c, ngpt, nlay, ncol, 1, nmus, self.lib.float_array(GAUSS_DS[nmus]),
                    self.lib.float_array(GAUSS_WTS[nmus]), P(a["inc"]), P(a["tau"])]
            planck = [P(a["pfrac"]), nb, ntemp, P(a["tlay"]), P(a["tlev"]), P(a["tsfc"]), nlay, lims_c, tmin, tdelta,
                      P(a["totplnk"]), 0, P(a["emis"])]
            srcs = [P(a["lay"]), P(a["lev"]), P(a["emis"]), P(a["sfc"])]
            ud = [P(t) for t in fl]
            if call == "lw_arrays":
                check(L.rrtmgpnn_lw_solver_noscat(*head, *srcs, *ud), row["name"])
            elif call == "lw_planck":
                check(L.rrtmgpnn_lw_solver_noscat_planck(*head, *planck, *ud), row["name"])
            elif call == "lw_planck_inc":
                check(L.rrtmgpnn_lw_solver_noscat_planck_inc(*head, P(a["tb"]), *planck, *ud), row["name"])
            elif call == "lw_clr_all" and mask is not None:
                check(L.rrtmgpnn_lw_solver_noscat_planck_clr_all_mcica(*head, P(a["tb"]), *planck, *ud,
                                                                       *[P(t) for t in clr], mask), row["name"])
            elif call == "lw_clr_all":
                check(L.rrtmgpnn_lw_solver_noscat_planck_clr_all(*head, P(a["tb"]), *planck, *ud, *[P(t) for t in clr]),
                      row["name"])
            elif call == "lw_rescl":
                check(L.rrtmgpnn_lw_solver_1rescl(*head, P(a["ssa"]), P(a["g"]), *srcs, *ud), row["name"])
            elif call == "lw_scat_inc":
                check(L.rrtmgpnn_lw_solver_1rescl_planck_inc(*head, P(a["tb"]), P(a["wb"]), P(a["gb"]), *planck, *ud),
                      row["name"])
            else:
                assert call == "lw_scat_clr_all", call
                check(L.rrtmgpnn_lw_solver_1rescl_planck_clr_all(*head, P(a["tb"]), P(a["wb"]), P(a["gb"]), *planck, *ud,
                                                                 *[P(t) for t in clr]), row["name"])
        torch.cuda.synchronize()
        path = self.path()
        return path, {k: v.cpu().numpy() for k, v in out.items() if not k.startswith("_")}


def run_rows(rows):
    r = Runner()
    return {row["name"]: r.run(row) for row in rows}


def child_main(out_json, out_npz):
    """The plane-free rows (the parent process set RRTMGPNN_SW_NO_PLANES=1): paths to JSON, the broadband fluxes to npz"""
    torch.cuda.set_device(0)
    res = run_rows(CK_CHILD_ROWS)
    json.dump({k: v[0] for k, v in res.items()}, open(out_json, "w"))
    np.savez(out_npz, **{"%s/%s" % (k, n): a for k, v in res.items() for n, a in v[1].items() if n in ("up", "dn", "dir")})


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    """Every row's (path, outputs): the rows of this process, then the child's with RRTMGPNN_SW_NO_PLANES=1"""
    assert torch.cuda.is_available(), "GPU tests need a device"
    torch.cuda.set_device(0)
    assert "RRTMGPNN_SW_NO_PLANES" not in os.environ
    res = run_rows(LW_ROWS + SCAT_ROWS + RESCL_ROWS + SW1_ROWS + SWX2_ROWS + CK_ROWS)
    d = tmp_path_factory.mktemp("noplanes")
    oj, on = str(d / "paths.json"), str(d / "flux.npz")
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_gpu_solver_dispatch as D; D.child_main(%r, %r)"
            % (os.path.join(ROOT, "tests"), os.path.join(ROOT, "rte-rrtmgp-nn_amd"), oj, on))
    env = dict(os.environ, RRTMGPNN_SW_NO_PLANES="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    paths, flux = json.load(open(oj)), np.load(on)
    for row in CK_CHILD_ROWS:
        res[row["name"]] = (paths[row["name"]], {n: flux["%s/%s" % (row["name"], n)] for n in ("up", "dn", "dir")})
    return res


def test_row_names_are_unique():
    names = [row["name"] for _, rows in FAMILY_ROWS.values() for row in rows]
    assert len(names) == len(set(names))


@pytest.mark.parametrize("family", sorted(FAMILY_ROWS))
def test_solver_dispatch(results, family):
    """Every row reports its table entry; the family's rows reach every instance it compiles; rows of one problem agree
    bit for bit."""
    fam, rows = FAMILY_ROWS[family]
    wrong = []
    for row in rows:
        path, out = results[row["name"]]
        print("%-28s family %d options %4d launches %d (of %d instances)" % ((row["name"],) + tuple(path)))
        if path[:3] != [row["family"], row["options"], row["launches"]]:
            wrong.append("%s: got family %d options %d launches %d, table says %d / %d / %d"
                         % ((row["name"],) + tuple(path[:3]) + (row["family"], row["options"], row["launches"])))
        for n in ("up", "dn", "dir"):
            if n in out:
                assert np.isfinite(out[n]).all(), "%s: flux_%s" % (row["name"], n)
        for n, a in out.items():
            assert not np.isnan(a).any(), "%s: output %s was not written everywhere" % (row["name"], n)
    assert not wrong, "\n".join(wrong)
    listed = {results[row["name"]][0][3] for row in rows}
    assert len(listed) == 1, listed
    reached = {row["options"] for row in rows if row["family"] == fam}
    assert len(reached) == listed.pop(), "%s: the rows reach %d instances: %s" % (family, len(reached), sorted(reached))


def test_same_problem_same_bits(results):
    """Rows that solve one problem through different instances (planes or not, band pair or not, dual or two launches,
    one or two g-points per lane, with or without by-band / Jacobian outputs) give the same broadband fluxes."""
    first = {}
    for _, rows in FAMILY_ROWS.values():
        for row in rows:
            if row["same"] is None:
                continue
            out = results[row["name"]][1]
            ref = first.setdefault(row["same"], (row["name"], out))
            for n in ("up", "dn", "dir"):
                if n in out:
                    np.testing.assert_array_equal(out[n].view(np.uint32), ref[1][n].view(np.uint32),
                                                  err_msg="%s against %s: flux_%s" % (row["name"], ref[0], n))
