"""ClearSkyStep(lw_scattering=True, lw_dual=True): the option sets whose call plan tests/golden/step_plan_lw_dual.json
pins, in the form of tests/step_plan.py (whose environment, describe and run_case serve here too).  CASES: (id, builder)
pairs; builder(env) -> the constructor's keyword arguments.  Overcast and McICA clouds with clear-sky outputs, with and
without aerosols, one without stream overlap, one LW-only, one with three angles; and the constructor's refusals.  Nothing
is ever launched."""
import step_plan as P
from step_plan_aerosol import aerosols

DUAL = {"lw_scattering": True, "lw_dual": True}


def _dual(build, aer=False, sw=True):
    def b(e):
        kw = dict(build(e), **DUAL)
        if aer:
            kw["aerosols"] = aerosols(e, sw)
        return kw
    return b


MODES = [
    ("dual-clrsky", _dual(P._allsky(clrsky=True))),
    ("dual-clrsky-lw", _dual(P._allsky(clrsky=True, sw=False))),
    ("dual-clrsky-nmus3", _dual(P._allsky(clrsky=True, nmus=3))),
    ("dual-mcica-arrays", _dual(P._mcica(ov=True, clrsky=True))),
    ("dual-mcica-seeded", _dual(P._mcica(seeded=True, ov=True, clrsky=True))),
    ("dual-aer-clrsky", _dual(P._allsky(clrsky=True), aer=True)),
    ("dual-aer-clrsky-lw", _dual(P._allsky(clrsky=True, sw=False), aer=True, sw=False)),
    ("dual-aer-mcica-arrays", _dual(P._mcica(ov=True, clrsky=True), aer=True)),
    ("dual-aer-mcica-seeded", _dual(P._mcica(seeded=True, ov=True, clrsky=True), aer=True)),
]
NO_OVERLAP = ("dual-aer-mcica-seeded",)

REFUSALS = [
    ("no-scattering", lambda e: dict(P._allsky(clrsky=True)(e), lw_dual=True)),
    ("no-clrsky", _dual(P._allsky())),
    ("mcica-no-clrsky", _dual(P._mcica(ov=True))),
    ("unfused", P._with(_dual(P._allsky(clrsky=True)), fused=False)),
    ("byband", _dual(P._allsky(byband=True))),
    ("jacobian", _dual(P._allsky(clrsky=True, jacobian=True))),
    ("mcica-byband", _dual(P._mcica(ov=True, byband=True, clrsky=True))),
]

CASES = [(m, b) for m, b in MODES]
CASES += [(m + "-serial", P._with(b, overlap=False)) for m, b in MODES if m in NO_OVERLAP]
CASES += [("refused-" + k, b) for k, b in REFUSALS]
assert len({k for k, _ in CASES}) == len(CASES)
