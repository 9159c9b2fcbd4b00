"""ClearSkyStep's call plan over its whole option matrix, shared by tests/golden/make_step_plan_golden.py (which records
it from the commit the fixture is pinned to) and tests/test_gpu_step_plan.py (which compares the tree with it).

CASES: (id, builder) pairs; builder(env) -> the constructor's keyword arguments.  env (environment()) holds 4 RFMIP
columns spread over the 1800, the all-sky example's clouds for them (at least one layer cloudy) and McICA inputs of the
step's shapes.  Modes x fused / unfused, the same without stream overlap, the schedule knobs on the fused all-sky step,
and every refusal of the constructor.  Nothing is ever launched: a case builds the step, describes it and closes it.

describe(step): the plan as JSON-serialisable data with no device address in it: every call as one string "name entry
stream: arguments" (a device pointer is written as the name of the step's tensor it addresses, a handle by its name, a
ctypes array by its values in brackets, None as null), every tensor attribute's shape and dtype, and the schedule
attributes.  It reads only public attributes and step.calls; what it cannot name is an error, never a literal."""
import ctypes

import numpy as np

COLS = np.arange(4) * 400
SCHEDULE = ("overlap", "lw_after", "sw_after", "lw_net_cus", "sw_net_cus", "fused", "sw", "allsky", "clrsky", "byband",
            "mcica", "seeded")
HANDLES = ("cloud_lw", "cloud_sw")
CTX_CUS = 40  # the cap the caller-supplied context of the "ctx" case carries


def environment(rfmip):
    from conftest import subset
    from rrtmgpnn import data
    prob = subset(rfmip, COLS)
    ncol, nlay = prob["ncol"], prob["nlay"]
    clouds = data.allsky_clouds(prob, data.load_cloud_optics("lw"))
    cloudy = (clouds[0] > 0) | (clouds[1] > 0)
    assert cloudy.any()
    rng = np.random.default_rng(41)
    cf = np.where(cloudy, rng.uniform(0.2, 0.9, cloudy.shape), 0).astype(np.float32)
    ng_lw, ng_sw = data.load_kdist("lw")["ngpt"], data.load_kdist("sw")["ngpt"]
    return {"prob": prob, "clouds": clouds, "cloud_frac": cf,
            "overlap_param": rng.uniform(-1, 1, (ncol, nlay - 1)).astype(np.float32),
            "randoms_lw": np.zeros((ncol, nlay, ng_lw), np.float32),
            "randoms_sw": np.zeros((ncol, nlay, ng_sw), np.float32), "ctxs": []}


def _mc(e, seeded=False, ov=False, **keys):
    d = {"cloud_frac": e["cloud_frac"], "overlap_param": e["overlap_param"] if ov else None}
    d.update({"seed": 2026} if seeded else {"randoms_lw": e["randoms_lw"], "randoms_sw": e["randoms_sw"]})
    d.update(keys)
    return d


def _caller_ctx(e):
    from rrtmgpnn.api import Context
    ctx = Context(0)
    ctx.set_mlp_max_cus(CTX_CUS)
    e["ctxs"].append(ctx)
    return ctx


def _allsky(**kw):
    return lambda e: dict(kw, clouds=e["clouds"])


def _mcica(kw=None, **mc):
    return lambda e: dict(kw or {}, clouds=e["clouds"], mcica=_mc(e, **mc))


MODES = [
    ("clear", lambda e: {}),
    ("clear-byband", lambda e: {"byband": True}),
    ("clear-lw", lambda e: {"sw": False}),
    ("clear-lw-byband", lambda e: {"sw": False, "byband": True}),
    ("allsky", _allsky()),
    ("allsky-byband", _allsky(byband=True)),
    ("allsky-lw", _allsky(sw=False)),
    ("allsky-clrsky", _allsky(clrsky=True)),
    ("allsky-clrsky-lw", _allsky(clrsky=True, sw=False)),
    ("allsky-clrsky-nmus3", _allsky(clrsky=True, nmus=3)),
    ("mcica-arrays-maxran", _mcica()),
    ("mcica-arrays-expran", _mcica(ov=True)),
    ("mcica-seeded-maxran", _mcica(seeded=True)),
    ("mcica-seeded-expran", _mcica(seeded=True, ov=True)),
    ("mcica-clrsky-arrays", _mcica(ov=True, clrsky=True)),
    ("mcica-clrsky-seeded", _mcica(seeded=True, ov=True, clrsky=True)),
    ("mcica-byband-arrays", _mcica(ov=True, byband=True)),
    ("mcica-byband-seeded", _mcica(seeded=True, ov=True, byband=True)),
]
NO_OVERLAP = ("clear", "allsky", "mcica-seeded-expran", "allsky-clrsky")
KNOBS = [
    ("lw_after-none", _allsky(lw_after="")),
    ("lw_after-cloud_optics_sw", _allsky(lw_after="cloud_optics_sw")),
    ("sw_after-predict_nn_lw", _allsky(sw_after="predict_nn_lw")),
    ("lw_net_cus-64", _allsky(lw_net_cus=64)),
    ("sw_net_cus-32", _allsky(sw_net_cus=32)),
    ("sw_priority-high", _allsky(sw_priority=-1)),
    ("ctx", lambda e: {"clouds": e["clouds"], "ctx": _caller_ctx(e)}),
]


def _wrong(key):
    def build(e):
        mc = _mc(e, ov=True)
        mc[key] = mc[key][:, 1:]
        return {"clouds": e["clouds"], "mcica": mc}
    return build


REFUSALS = [
    ("mcica-without-clouds", lambda e: {"mcica": _mc(e)}),
    ("mcica-with-clrsky-flag", _mcica({"clrsky": True})),
    ("mcica-with-byband-flag", _mcica({"byband": True})),
    ("mcica-lw", _mcica({"sw": False})),
    ("clrsky-without-clouds", lambda e: {"clrsky": True}),
    ("clrsky-with-byband", _allsky(clrsky=True, byband=True)),
    ("mcica-byband-with-clrsky", _mcica(byband=True, clrsky=True)),
    ("mcica-seed-with-randoms", lambda e: {"clouds": e["clouds"], "mcica": dict(_mc(e), seed=7)}),
    ("mcica-shape-cloud_frac", _wrong("cloud_frac")),
    ("mcica-shape-randoms_lw", _wrong("randoms_lw")),
    ("mcica-shape-randoms_sw", _wrong("randoms_sw")),
    ("mcica-shape-overlap_param", _wrong("overlap_param")),
    ("lw_net_cus-without-overlap", _allsky(overlap=False, lw_net_cus=64)),
    ("sw_net_cus-without-overlap", _allsky(overlap=False, sw_net_cus=32)),
    ("lw_after-not-sw-chain", _allsky(lw_after="predict_nn_lw")),
    ("lw_after-unfused", _allsky(fused=False, lw_after="predict_nn_sw")),
    ("sw_after-not-lw-chain", _allsky(sw_after="predict_nn_sw")),
    ("sw_after-after-the-solver", _allsky(lw_after="sw_solver", sw_after="predict_nn_lw")),
]


def _with(build, **more):
    return lambda e: dict(build(e), **more)


CASES = [("%s-%s" % (m, "fused" if fused else "unfused"), _with(b, fused=fused))
         for m, b in MODES for fused in (True, False)]
CASES += [("%s-%s-serial" % (m, "fused" if fused else "unfused"), _with(b, fused=fused, overlap=False))
          for m, b in MODES if m in NO_OVERLAP for fused in (True, False)]
CASES += [("knob-" + k, b) for k, b in KNOBS]
CASES += [("refused-" + k, b) for k, b in REFUSALS]
assert len({k for k, _ in CASES}) == len(CASES)


def _tensors(step):
    import torch
    out = {k: v for k, v in vars(step).items() if isinstance(v, torch.Tensor) and not k.startswith("_")}
    out.update({"gases[%s]" % k: v for k, v in step.gases.items()})
    return out


def _handles(step):
    out = {"ctx": step.ctx.h}
    if step.ctx2 is not None:
        out["ctx2"] = step.ctx2.h
    for k in HANDLES:
        if getattr(step, k, None) is not None:
            out[k] = getattr(step, k)
    for k in ("lw_nets", "sw_nets"):
        out.update({"%s[%d]" % (k, i): h for i, h in enumerate(getattr(step, k))})
    return {(h.value if isinstance(h, ctypes.c_void_p) else int(h)): k for k, h in out.items()}


def _text(a):
    """A rendered argument as text: a name bare, a list in brackets, None as null, a number by its repr."""
    if isinstance(a, list):
        return "[%s]" % ",".join(map(_text, a))
    return "null" if a is None else a if isinstance(a, str) else repr(a)


def describe(step):
    """The plan of a built step (module docstring)."""
    ptrs = {}
    for k, t in sorted(_tensors(step).items(), reverse=True):
        ptrs[t.data_ptr()] = k  # two names of one buffer: the first in sorted order
    handles = _handles(step)
    assert not set(ptrs) & set(handles)

    def address(v, where):
        if v is None or v == 0:
            return None
        if v in handles:
            return handles[v]
        if v in ptrs:
            return ptrs[v]
        raise ValueError("describe: %s is no tensor or handle of the step (%#x)" % (where, v))

    def render(a, where):
        if a is None:
            return None
        if isinstance(a, ctypes.c_void_p):
            return address(a.value, where)
        if isinstance(a, ctypes.Array):
            if a._type_ is ctypes.c_void_p:
                return [address(v, where) for v in a]
            if a._type_ in (ctypes.c_int, ctypes.c_float):
                return list(a)
            raise ValueError("describe: %s is a ctypes array of %r" % (where, a._type_))
        if isinstance(a, (bool, int, np.bool_, np.integer)):
            a = int(a)
            if a in handles or a in ptrs:
                return address(a, where)
            if abs(a) >= 1 << 31:  # no count or size of a 4-column step: an address the step does not own
                raise ValueError("describe: %s is no tensor or handle of the step (%#x)" % (where, a))
            return a
        if isinstance(a, (float, np.floating)):
            return float(a)
        raise ValueError("describe: %s is a %s" % (where, type(a).__name__))

    lw = step.ctx.stream.cuda_stream
    calls = []
    for name, fn, args in step.calls:
        s = step.stream_for(name).cuda_stream
        if s != lw and (step.ctx2 is None or s != step.ctx2.stream.cuda_stream):
            raise ValueError("describe: %s is issued on a stream of neither context" % name)
        args = [render(a, "%s argument %d" % (name, i)) for i, a in enumerate(args)]
        calls.append("%s %s %s: %s" % (name, fn.__name__, "lw" if s == lw else "sw", ", ".join(map(_text, args))))
    buffers = {k: [list(t.shape), str(t.dtype).replace("torch.", "")] for k, t in sorted(_tensors(step).items())}
    schedule = {k: getattr(step, k) for k in SCHEDULE if hasattr(step, k)}
    schedule["sw_priority"] = getattr(step, "sw_priority", 0)  # (an LW-only step has no SW stream to give one)
    for k, v in schedule.items():
        if not isinstance(v, (bool, int, str)):
            raise ValueError("describe: schedule attribute %s is a %s" % (k, type(v).__name__))
    return {"calls": calls, "buffers": buffers, "schedule": schedule}


def run_case(build, env, cls=None):
    """Build the case's step, describe it, close it (and a context the case made for it); a refusal is described by
    its exception."""
    if cls is None:
        from rrtmgpnn.pipeline import ClearSkyStep as cls
    try:
        try:
            step = cls(env["prob"], device=0, **build(env))
        except ValueError as e:
            return {"raises": "ValueError", "message": str(e)}
        try:
            return describe(step)
        finally:
            step.close()
    finally:
        while env["ctxs"]:
            env["ctxs"].pop().close()
