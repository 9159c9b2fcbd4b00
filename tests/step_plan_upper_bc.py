"""ClearSkyStep(upper_bc=True): the option sets whose call plan tests/golden/step_plan_upper_bc.json pins, in the form of
tests/step_plan.py (whose describe and run_case serve here too).  CASES: (id, builder) pairs; builder(env) -> the
constructor's keyword arguments.  The environment is step_plan's on the RFMIP columns without their topmost layer (the
unmodified columns' top level is the gas optics' minimum pressure itself, which compute_bc refuses: the one refusal
case).  Every LW solver entry the option sets select -- fused or not, one angle and three, by-band, Jacobian, overcast and
McICA clouds with clear-sky outputs, aerosols, scattering clouds, the dual entries -- an LW-only step and one without
stream overlap.  Nothing is ever launched."""
import numpy as np

import step_plan as P
from step_plan_aerosol import aerosols

DROP = 1  # topmost layers removed


def without_top(rfmip, drop=DROP):
    """The RFMIP problem (top at index 0) without its `drop` topmost layers."""
    assert rfmip["top_at_1"]
    out = dict(rfmip, nlay=rfmip["nlay"] - drop)
    for k in ("play", "plev", "tlay", "tlev"):
        out[k] = np.ascontiguousarray(rfmip[k][:, drop:])
    out["gases"] = {k: np.ascontiguousarray(v[:, drop:]) for k, v in rfmip["gases"].items()}
    return out


def environment(rfmip):
    from conftest import subset
    env = P.environment(without_top(rfmip))
    env["full"] = subset(rfmip, P.COLS)
    return env


def _bc(build, aer=False, **more):
    def b(e):
        kw = dict(build(e), upper_bc=True, **more)
        if aer:
            kw["aerosols"] = aerosols(e, kw.get("sw", True))
        return kw
    return b


SCAT = {"lw_scattering": True}
MODES = [
    ("bc-clear", _bc(lambda e: {})),
    ("bc-clear-lw", _bc(lambda e: {"sw": False})),
    ("bc-clear-nmus3", _bc(lambda e: {"nmus": 3})),
    ("bc-clear-byband", _bc(lambda e: {"byband": True})),
    ("bc-clear-jacobian", _bc(lambda e: {"jacobian": True})),
    ("bc-aer-clear", _bc(lambda e: {}, aer=True)),
    ("bc-allsky", _bc(P._allsky())),
    ("bc-allsky-clrsky", _bc(P._allsky(clrsky=True))),
    ("bc-allsky-clrsky-nmus3", _bc(P._allsky(clrsky=True, nmus=3))),
    ("bc-mcica-seeded", _bc(P._mcica(seeded=True, ov=True))),
    ("bc-mcica-clrsky-seeded", _bc(P._mcica(seeded=True, ov=True, clrsky=True))),
]
FUSED_ONLY = [
    ("bc-scat-clrsky", _bc(P._allsky(clrsky=True), **SCAT)),
    ("bc-scat-dual-aer", _bc(P._allsky(clrsky=True), aer=True, lw_dual=True, **SCAT)),
]
NO_OVERLAP = ("bc-clear", "bc-allsky-clrsky")

REFUSALS = [
    ("top-at-press-min", lambda e: {"upper_bc": True, "prob": e["full"]}),
    ("top-at-press-min-unfused-lw", lambda e: {"upper_bc": True, "fused": False, "sw": False, "prob": e["full"]}),
]

CASES = [("%s-%s" % (m, "fused" if fused else "unfused"), P._with(b, fused=fused))
         for m, b in MODES for fused in (True, False)]
CASES += [(m + "-fused", b) for m, b in FUSED_ONLY]
CASES += [("%s-%s-serial" % (m, "fused" if fused else "unfused"), P._with(b, fused=fused, overlap=False))
          for m, b in MODES if m in NO_OVERLAP for fused in (True, False)]
CASES += [("refused-" + k, b) for k, b in REFUSALS]
assert len({k for k, _ in CASES}) == len(CASES)


def run_case(build, env):
    """step_plan.run_case on the case's own problem (the key "prob" of its arguments) or the environment's."""
    kw = build(env)
    prob = kw.pop("prob", env["prob"])
    return P.run_case(lambda e: kw, dict(env, prob=prob))
