"""The cells of the request policy (csrc/requests.cpp): every public solver symbol with every combination of request
states, walked through a built library, and the two rules that hold a library's answers to the recorded ones.  Shared by
tests/golden/make_request_policy_golden.py (the recording), tests/test_gpu_request_policy.py and
tests/test_request_policy_host.py.

A call uses ngpt 4, nbnd 2 with limits (1,2),(3,4), nlay 2, ncol 3 and passes tau as null, so an accepted combination
comes back as the entry's own "<entry>: bad argument" and nothing is ever launched."""
import ctypes
import itertools
import json
import os

NGPT, NBND, NLAY, NCOL, NTEMP = 4, 2, 2, 3, 4
LIMS, LIMS_PAST_NGPT = (1, 2, 3, 4), (1, 2, 3, 5)
ERR_ARGUMENT = 1

# state 0 of every request: not armed
KINDS = ("byband", "mask", "jacobian", "aerosol", "active")
STATES = {"byband": ("off", "armed", "last limit above ngpt"),
          "mask": ("off", "armed", "the byband_mcica pair", "other ncol"),
          "jacobian": ("off", "with sfc_source_Jac", "without sfc_source_Jac", "other ncol"),
          "aerosol": ("off", "1scl", "2str", "other ncol (of the entry's kind: LW 1scl, SW 2str)"),
          "active": ("off", "armed", "other ncol")}
PAIR = 2
# the arming calls make one thing impossible: the pair is armed by one call, which holds its limits to its ngpt, so a
# paired mask of the call's extents has a by-band request within ngpt beside it
CELLS = [c for c in itertools.product(*[range(len(STATES[k])) for k in KINDS]) if c[1] != PAIR or c[0] == 1]
INDEX = {c: i for i, c in enumerate(CELLS)}

# The arguments after the context: G L C B T the extents, 1 an int flag (top_at_1, nmus, sfc_lay, emis_by_band), h a host
# float array (Ds, weights), l the band limits, f a float (temp_ref_min, totplnk_delta), p a device pointer, 0 tau.
_PLANCK = "B T p p p 1 l f f p 1 p"  # nbnd nPlanckTemp tlay tlev tsfc sfc_lay lims tmin tdelta totplnk emis_by_band emis
SYMBOLS = {
    "lw_solver_noscat": "G L C 1 1 h h p 0 p p p p p p",
    "lw_solver_noscat_gpt": "G L C 1 1 h h p p 0 p p p p p p p p",
    "lw_solver_noscat_planck": "G L C 1 1 h h p 0 p " + _PLANCK + " p p",
    "lw_solver_noscat_planck_gpt": "G L C 1 1 h h p p 0 p " + _PLANCK + " p p p p",
    "lw_solver_noscat_planck_inc": "G L C 1 1 h h p 0 p p " + _PLANCK + " p p",
    "lw_solver_noscat_planck_clr_all": "G L C 1 1 h h p 0 p p " + _PLANCK + " p p p p",
    "lw_solver_noscat_planck_clr_all_mcica": "G L C 1 1 h h p 0 p p " + _PLANCK + " p p p p p",
    "lw_solver_1rescl": "G L C 1 1 h h p 0 p p p p p p p p",
    "lw_solver_1rescl_gpt": "G L C 1 1 h h p 0 p p p p p p p p p p",
    "lw_solver_1rescl_planck_inc": "G L C 1 1 h h p 0 p p p p " + _PLANCK + " p p",
    "lw_solver_1rescl_planck_clr_all": "G L C 1 1 h h p 0 p p p p " + _PLANCK + " p p p p",
    "lw_solver_2stream": "G L C 1 p 0 p p p p p p p",
    "lw_solver_2stream_gpt": "G L C 1 p 0 p p p p p p p p p",
    "sw_solver_2stream": "G L C 1 p p 0 p p p p p p p p",
    "sw_solver_2stream_gpt": "G L C 1 p p 0 p p p p p p p p p p p",
    "sw_solver_noscat": "G L C 1 p 0 p p",
    "sw_solver_noscat_gpt": "G L C 1 p 0 p p p",
    "sw_solver_2stream_inc": "G L C 1 p p 0 p p B l p p p p p p p p p",
    "sw_solver_2stream_clr_all": "G L C 1 p p 0 p p B l p p p p p p p p p p p p",
    "sw_solver_2stream_rfmip": "G L C 1 p p p p 0 p p B l p p p p p p p p p",
    "sw_solver_2stream_rfmip_clr_all": "G L C 1 p p p p 0 p p B l p p p p p p p p p p p p",
}


def entry_of(symbol):
    return symbol[:-4] if symbol.endswith("_gpt") else symbol


def accepted(symbol):
    """What a call gives when its requests (if any) were all taken: its own refusal of the null tau"""
    return (ERR_ARGUMENT, entry_of(symbol) + ": bad argument")


def aerosol_is_2str(symbol, state):
    return state == 2 or (state == 3 and symbol.startswith("sw_"))


class Walker:
    """The cells through a loaded librrtmgpnn.so (a ctypes handle with the argument types of rrtmgpnn._lib.SIGNATURES
    set), on a context and one small device allocation of its own."""

    def __init__(self, L):
        self.L = L
        self.ctx = ctypes.c_void_p()
        assert L.rrtmgpnn_context_create(0, None, ctypes.byref(self.ctx)) == 0, self.error()
        mem = ctypes.c_void_p()
        assert L.rrtmgpnn_malloc(self.ctx, 4096, ctypes.byref(mem)) == 0, self.error()
        self.mem = mem.value
        i, f = ctypes.c_int, ctypes.c_float
        self.lims, self.lims_past = (i * 4)(*LIMS), (i * 4)(*LIMS_PAST_NGPT)
        self.host = (f * 4)(1.0, 1.0, 1.0, 1.0)
        self.value = {"G": NGPT, "L": NLAY, "C": NCOL, "B": NBND, "T": NTEMP, "1": 1, "h": self.host, "l": self.lims,
                      "f": 1.0, "p": self.mem, "0": None}

    def close(self):
        self.L.rrtmgpnn_free(self.ctx, self.mem)
        self.L.rrtmgpnn_context_destroy(self.ctx)

    def error(self):
        return self.L.rrtmgpnn_last_error().decode()

    def path(self):
        p = (ctypes.c_int * 4)()
        assert self.L.rrtmgpnn_context_get_solver_path(self.ctx, p) == 0, self.error()
        return list(p)

    def arm(self, symbol, cell):
        L, c, p = self.L, self.ctx, self.mem
        byband, mask, jacobian, aerosol, active = cell
        if mask == PAIR:
            assert L.rrtmgpnn_solver_request_byband_mcica(c, NBND, self.lims, p, p, p, NGPT, NLAY, NCOL, p) == 0
        else:
            if byband:
                assert L.rrtmgpnn_solver_request_byband(c, NBND, self.lims if byband == 1 else self.lims_past, p, p, p) == 0
            if mask:
                assert L.rrtmgpnn_solver_request_cloud_mask(c, NGPT, NLAY, NCOL + (mask == 3), p) == 0
        if jacobian:
            assert L.rrtmgpnn_solver_request_jacobian(c, NGPT, NLAY, NCOL + (jacobian == 3), None if jacobian == 2 else p,
                                                      p) == 0
        if aerosol:
            sg = p if aerosol_is_2str(symbol, aerosol) else None
            assert L.rrtmgpnn_solver_request_aerosol(c, NBND, NLAY, NCOL + (aerosol == 3), p, sg, sg) == 0
        if active:
            assert L.rrtmgpnn_solver_request_active_columns(c, NCOL + (active == 2), p) == 0

    def call(self, symbol):
        rc = getattr(self.L, "rrtmgpnn_" + symbol)(self.ctx, *[self.value[t] for t in SYMBOLS[symbol].split()])
        return (rc, self.error())

    def walk(self, symbol):
        """-> the (status, message) of every cell, in the order of CELLS.  The call after each cell, with nothing armed,
        must give the nothing-armed answer (every request was taken and cleared, whatever the call returned), and the
        context's launch record must not have moved."""
        before, plain, out = self.path(), accepted(symbol), []
        assert self.call(symbol) == plain, (symbol, self.error())
        for cell in CELLS:
            self.arm(symbol, cell)
            out.append(self.call(symbol))
            again = self.call(symbol)
            assert again == plain, "%s %s: something stayed armed: %s" % (symbol, cell, again)
        assert self.path() == before, "%s launched something" % symbol
        return out


def load(path):
    """A ctypes handle of the library at `path` with the declared argument types"""
    from rrtmgpnn import _lib
    L = ctypes.CDLL(path)
    for name, (res, args) in _lib.SIGNATURES.items():
        f = getattr(L, name)
        f.restype, f.argtypes = res, args
    return L


def sub_cells(cell):
    """The cell with one or more of its armed requests switched off (the pair without its by-band half is a mask)"""
    on = [k for k in range(len(KINDS)) if cell[k]]
    for n in range(1, len(on) + 1):
        for off in itertools.combinations(on, n):
            s = [0 if k in off else v for k, v in enumerate(cell)]
            if s[1] == PAIR and not s[0]:
                s[1] = 1
            yield tuple(s)


def compare(symbol, parent, new):
    """Rules A and B on one symbol's answers (lists over CELLS of (status, message)).
    -> (failures, the cells that pass by rule B with another answer than the parent's)"""
    ok, failures, by_rule_b = accepted(symbol), [], []
    for i, cell in enumerate(CELLS):
        p, n = tuple(parent[i]), tuple(new[i])
        if n == p:
            continue
        below = [tuple(parent[INDEX[s]]) for s in sub_cells(cell)]
        one_reason = all(b == ok or b == p for b in below)
        if p == ok or n == ok or one_reason:  # rule A; acceptance and refusal never stand in for each other
            failures.append((symbol, cell, "A", p, n))
        elif n not in below:  # rule B: a refusal the parent gives for part of what was armed
            failures.append((symbol, cell, "B", p, n))
        else:
            by_rule_b.append(cell)
    return failures, by_rule_b


def group_of(symbol, cell, parent, new):
    """The smallest sets of request kinds, armed together within `cell`, at which the two libraries already differ"""
    differing = [s for s in list(sub_cells(cell)) + [cell] if tuple(parent[INDEX[s]]) != tuple(new[INDEX[s]])]
    fewest = min(sum(1 for v in s if v) for s in differing)
    return {(entry_of(symbol), "+".join(KINDS[k] for k, v in enumerate(s) if v))
            for s in differing if sum(1 for v in s if v) == fewest}


# The cells whose refusal differs from the parent's and passes by rule B, and the (entry, requests armed together) groups
# they fall into: what the one fixed order of apply_requests changed ("Solver dispatch")
RULE_B_CELLS = 221
_SKY = ("sw_solver_2stream_inc", "sw_solver_2stream_rfmip")
_SW_CLR_ALL = ("sw_solver_2stream_clr_all", "sw_solver_2stream_rfmip_clr_all")
_LW_CLR_ALL = ("lw_solver_noscat_planck_clr_all", "lw_solver_noscat_planck_clr_all_mcica")
RULE_B_GROUPS = (
    {(e, "mask+jacobian") for e in ("lw_solver_noscat_planck_inc", "lw_solver_1rescl_planck_inc",
                                    "lw_solver_1rescl_planck_clr_all") + _SKY + _SW_CLR_ALL}
    | {(e, "byband+mask+jacobian") for e in ("lw_solver_noscat_planck_inc",) + _SKY}
    | {(e, "jacobian+aerosol") for e in ("lw_solver_1rescl_planck_clr_all",) + _LW_CLR_ALL + _SKY + _SW_CLR_ALL})


def golden():
    """symbol -> the parent's (status, message) over CELLS (tests/golden/request_policy.json)"""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "request_policy.json")) as f:
        g = json.load(f)
    assert [tuple(c) for c in g["cells"]] == CELLS and list(g["symbols"]) == list(SYMBOLS)
    return {s: [tuple(g["answers"][i]) for i in idx] for s, idx in g["symbols"].items()}


def rule_b_summary(parent, new):
    """-> (failures of either rule, the number of cells that pass by rule B, their groups) over every symbol"""
    failures, cells, groups = [], 0, set()
    for s in SYMBOLS:
        f, b = compare(s, parent[s], new[s])
        failures += f
        cells += len(b)
        for cell in b:
            groups |= group_of(s, cell, parent[s], new[s])
    return failures, cells, groups
