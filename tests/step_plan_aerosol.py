"""ClearSkyStep(aerosols=...): the option sets whose call plan tests/golden/step_plan_aerosol.json pins, in the form of
tests/step_plan.py (whose environment, describe and run_case serve here too).  CASES: (id, builder) pairs;
builder(env) -> the constructor's keyword arguments.  Modes x fused / unfused, two of them without stream overlap, and
the constructor's refusals.  Nothing is ever launched."""
import numpy as np

import step_plan as P

AER_SEED = 97


def aerosols(e, sw=True):
    """Aerosol band properties of the environment's 4 columns (any values: a plan holds addresses, not contents)."""
    from rrtmgpnn import data
    prob = e["prob"]
    ncol, nlay = prob["ncol"], prob["nlay"]
    nb_lw, nb_sw = data.load_kdist("lw")["nband"], data.load_kdist("sw")["nband"]
    rng = np.random.default_rng(AER_SEED)
    a = {"lw_tau": rng.lognormal(-3, 1, (ncol, nlay, nb_lw)).astype(np.float32)}
    if sw:
        a.update(sw_tau=rng.lognormal(-3, 1, (ncol, nlay, nb_sw)).astype(np.float32),
                 sw_ssa=rng.uniform(0.6, 1, (ncol, nlay, nb_sw)).astype(np.float32),
                 sw_g=rng.uniform(0.3, 0.8, (ncol, nlay, nb_sw)).astype(np.float32))
    return a


def _aer(build, sw=True):
    return lambda e: dict(build(e), aerosols=aerosols(e, sw))


MODES = [
    ("aer-clear", _aer(lambda e: {})),
    ("aer-clear-lw", _aer(lambda e: {"sw": False}, sw=False)),
    ("aer-clear-nmus3", _aer(lambda e: {"nmus": 3})),
    ("aer-allsky", _aer(P._allsky())),
    ("aer-allsky-lw", _aer(P._allsky(sw=False), sw=False)),
    ("aer-allsky-clrsky", _aer(P._allsky(clrsky=True))),
    ("aer-allsky-clrsky-nmus3", _aer(P._allsky(clrsky=True, nmus=3))),
    ("aer-mcica-arrays-maxran", _aer(P._mcica())),
    ("aer-mcica-seeded-expran", _aer(P._mcica(seeded=True, ov=True))),
    ("aer-mcica-clrsky-seeded", _aer(P._mcica(seeded=True, ov=True, clrsky=True))),
]
NO_OVERLAP = ("aer-clear", "aer-mcica-clrsky-seeded")


def _bad_shape(e):
    a = aerosols(e)
    a["sw_g"] = a["sw_g"][:, 1:]
    return {"aerosols": a}


def _missing_key(e):
    a = aerosols(e)
    del a["sw_ssa"]
    return {"aerosols": a}


REFUSALS = [
    ("aer-byband", _aer(lambda e: {"byband": True})),
    ("aer-jacobian", _aer(lambda e: {"jacobian": True})),
    ("aer-mcica-byband", _aer(P._mcica(ov=True, byband=True))),
    ("aer-sw-keys-lw-step", _aer(lambda e: {"sw": False})),
    ("aer-missing-key", _missing_key),
    ("aer-shape", _bad_shape),
]

CASES = [("%s-%s" % (m, "fused" if fused else "unfused"), P._with(b, fused=fused))
         for m, b in MODES for fused in (True, False)]
CASES += [("%s-%s-serial" % (m, "fused" if fused else "unfused"), P._with(b, fused=fused, overlap=False))
          for m, b in MODES if m in NO_OVERLAP for fused in (True, False)]
CASES += [("refused-" + k, b) for k, b in REFUSALS]
assert len({k for k, _ in CASES}) == len(CASES)
