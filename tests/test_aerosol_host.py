"""CPU: rrtmgpnn_solver_request_aerosol is declared, bound and exported; the composed-oracle expectations of
tests/test_gpu_aerosol.py tell the right order of the two increments from the swapped one, from their sum and from no
aerosol at all, for every (orientation, nmus, mask, ngpt / layout) case the GPU file runs -- so no GPU case can pass
with the increments swapped, pre-summed or the aerosol ignored; and the class layers' routing predicate."""
import ctypes
import os
import re

import numpy as np
import pytest

import aerosol_cases as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"rrtmgpnn_solver_request_aerosol": 7}


def test_new_entry_is_declared_bound_and_exported():
    from rrtmgpnn import _lib, cloud_sampling
    header = open(os.path.join(ROOT, "include", "rrtmgpnn.h")).read()
    fortran = open(os.path.join(ROOT, "rte-rrtmgp-nn_amd", "fortran", "mo_rrtmgpnn_c.F90")).read()
    h = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in NEW.items():
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert len(_lib.SIGNATURES[name][1]) == nargs
        assert 'name="%s"' % name in fortran and "c_" + name in fortran
        assert hasattr(h, name), name + " is not exported by librrtmgpnn.so"
    m = re.search(r"int rrtmgpnn_solver_request_aerosol\(([^;]*)\);", header)
    args = [a.strip().split()[-1].lstrip("*") for a in m.group(1).replace("\n", " ").split(",")]
    assert args == ["ctx", "nbnd", "nlay", "ncol", "tau_aer", "ssa_aer", "g_aer"]
    assert callable(cloud_sampling.arm_aerosol)


def _some_value_differs(a, b):
    return any((x != y).any() for x, y in zip(a, b))


def _every_column_differs(a, b):
    """Every column differs in some broadband value of some flux."""
    d = np.zeros(a[0].shape[0], bool)
    for x, y in zip(a, b):
        d |= (x != y).any(axis=1)
    return bool(d.all())


@pytest.mark.parametrize("kind", [None, "sampled", "ones"], ids=["unmasked", "sampled", "ones"])
@pytest.mark.parametrize("nmus", [1, 3])
@pytest.mark.parametrize("top_at_1", [True, False], ids=["top1", "top0"])
@pytest.mark.parametrize("ng", A.LW_NGPTS)
def test_lw_expectation_tells_the_orders_apart(orc, ng, top_at_1, nmus, kind):
    c = A.lw_case(ng)
    mask = A.lw_mask(c, kind)
    exp = {o: A.lw_expect(orc, c, mask, top_at_1, nmus, o)[:2] for o in A.ORDERS}
    assert all(np.isfinite(x).all() for v in exp.values() for x in v)
    assert _some_value_differs(exp["right"], exp["swapped"]), "the swapped order gives the same broadband bits"
    assert _some_value_differs(exp["right"], exp["presummed"]), "the pre-summed increment gives the same broadband bits"
    assert _every_column_differs(exp["right"], exp["noaer"]), "a column does not see the aerosol"


@pytest.mark.parametrize("nmus", [1, 3])
@pytest.mark.parametrize("ng", A.LW_NGPTS)
def test_lw_zero_mask_and_clear_set(orc, ng, nmus):
    """An all-zero mask: the all-sky set is the clear one (tau + aerosol), which is not the set without aerosols."""
    c = A.lw_case(ng)
    up, dn, upc, dnc = A.lw_expect(orc, c, A.lw_mask(c, "zeros"), True, nmus)
    np.testing.assert_array_equal(up, upc)
    np.testing.assert_array_equal(dn, dnc)
    bare = A.lw_expect(orc, c, A.lw_mask(c, "zeros"), True, nmus, "noaer")[:2]
    assert _every_column_differs((up, dn), bare)


@pytest.mark.parametrize("kind", [None, "sampled"], ids=["unmasked", "sampled"])
@pytest.mark.parametrize("with_g", [True, False], ids=["g", "nog"])
@pytest.mark.parametrize("top_at_1", [True, False], ids=["top1", "top0"])
def test_sw_expectation_tells_the_orders_apart(orc, top_at_1, with_g, kind):
    c = A.sw_case()
    mask = A.sw_mask(c, kind)
    exp = {o: A.sw_expect(orc, c, mask, with_g, top_at_1, o) for o in ("right", "swapped", "noaer")}
    assert all(np.isfinite(x).all() for v in exp.values() for x in v)
    assert _some_value_differs(exp["right"], exp["swapped"]), "the swapped order gives the same broadband bits"
    assert _every_column_differs(exp["right"], exp["noaer"]), "a column does not see the aerosol"


@pytest.mark.parametrize("bound", [False, True], ids=["sza", "sza_bound"])
@pytest.mark.parametrize("kind", [None, "sampled"], ids=["unmasked", "sampled"])
@pytest.mark.parametrize("with_g", [True, False], ids=["g", "nog"])
@pytest.mark.parametrize("top_at_1", [True, False], ids=["top1", "top0"])
def test_sw_rfmip_expectation_tells_the_orders_apart(orc, top_at_1, with_g, kind, bound):
    """The same with the _rfmip entry's boundary conditions, for both zenith-angle sets of the GPU file."""
    c = A.sw_case()
    bc = A.rfmip_bc(c, A.bound_sza() if bound else None)
    if bound:
        assert bc[0][0] < 1e-5 and bc[0][1] == 1 and bc[0][2] == 1
    mask = A.sw_mask(c, kind)
    exp = {o: A.sw_expect(orc, c, mask, with_g, top_at_1, o, bc=bc) for o in ("right", "swapped", "noaer")}
    assert all(np.isfinite(x).all() for v in exp.values() for x in v)
    assert _some_value_differs(exp["right"], exp["swapped"]), "the swapped order gives the same broadband bits"
    assert _every_column_differs(exp["right"], exp["noaer"]), "a column does not see the aerosol"


@pytest.mark.parametrize("with_g", [True, False], ids=["g", "nog"])
def test_sw_zero_mask_leaves_the_aerosol(orc, with_g):
    """An all-zero mask switches the cloud off and leaves the aerosol in place."""
    c = A.sw_case()
    zero = A.sw_mask(c, "zeros")
    assert _every_column_differs(A.sw_expect(orc, c, zero, with_g, True), A.sw_expect(orc, c, zero, with_g, True, "noaer"))
    assert _every_column_differs(A.sw_expect(orc, c, zero, with_g, True),
                                 A.sw_expect(orc, c, A.sw_mask(c, "sampled"), with_g, True))


def _props(api, kind, ncol, nlay, lims_wvn, lims_gpt=None):
    import torch  # CPU tensors: the predicate looks at classes, bands and extents only
    op = kind()
    assert op.init(lims_wvn, lims_gpt) == ""
    assert (op.alloc_2str if kind is api.OpticalProps2str else op.alloc_1scl)(ncol, nlay, device=torch.device("cpu")) == ""
    return op


def test_class_layer_routing_predicate():
    """Which aer_props go to the request: the solve's own kind, by band on its bands, the same extents."""
    pytest.importorskip("torch")
    from rrtmgpnn import api, clr_all_sky
    wv = np.stack([np.arange(1, 5) * 100.0, np.arange(2, 6) * 100.0], axis=1)
    gp = np.array([[1, 4], [5, 8], [9, 12], [13, 16]], np.int32)
    one, two = api.OpticalProps1scl, api.OpticalProps2str
    ok = clr_all_sky.aerosol_by_request
    gas1, gas2 = _props(api, one, 3, 5, wv, gp), _props(api, two, 3, 5, wv, gp)
    assert ok(_props(api, one, 3, 5, wv), gas1, one)
    assert ok(_props(api, two, 3, 5, wv), gas2, two)
    assert not ok(None, gas1, one)
    assert not ok(_props(api, two, 3, 5, wv), gas1, one)  # 2str aerosols in the LW: the rescaled solver's case
    assert not ok(_props(api, one, 3, 5, wv), gas2, two)  # 1scl aerosols in the SW
    assert not ok(_props(api, one, 3, 5, wv, gp), gas1, one)  # on g-points
    assert not ok(_props(api, one, 3, 5, wv + 1.0), gas1, one)  # other bands
    assert not ok(_props(api, one, 3, 5, wv[:3]), gas1, one)  # fewer bands
    assert not ok(_props(api, one, 2, 5, wv), gas1, one) and not ok(_props(api, one, 3, 4, wv), gas1, one)  # extents
    assert clr_all_sky.AEROSOL_REQUEST is True


def test_step_plan_fixture_holds_the_cases():
    """tests/golden/step_plan_aerosol.json has exactly the cases of tests/step_plan_aerosol.py, refusals as refusals; in
    the fused plans with clouds each chain's aerosol request stands right before its solver and nothing materialises an
    increment; the unfused ones increment by the aerosol right after gas optics."""
    import json
    import step_plan_aerosol as PA
    with open(os.path.join(ROOT, "tests", "golden", "step_plan_aerosol.json")) as f:
        golden = json.load(f)
    assert sorted(golden) == sorted(k for k, _ in PA.CASES)
    assert {k for k, v in golden.items() if "raises" in v} == {k for k, _ in PA.CASES if k.startswith("refused-")}
    for k, v in golden.items():
        if "raises" in v:
            assert v["raises"] == "ValueError" and "aerosols" in v["message"], k
            continue
        names = [c.split()[0] for c in v["calls"]]
        entry = {c.split()[0]: c.split()[1] for c in v["calls"]}
        assert "aer_tau_lw" in v["buffers"]
        if "-unfused" in k:
            assert names.index("increment_aer_lw") == names.index("predict_nn_lw") + 1, k
            assert "lw_aerosol" not in names and "sw_aerosol" not in names, k
            continue
        assert not [n for n in names if n.startswith("increment")], k
        if k.startswith("aer-clear"):
            assert "lw_aerosol" not in names and entry["lw_solver"] == "rrtmgpnn_lw_solver_noscat_planck_inc", k
        else:
            assert names.index("lw_aerosol") == names.index("lw_solver") - 1, k
            assert entry["lw_aerosol"] == "rrtmgpnn_solver_request_aerosol", k
            if "sw_solver" in names:
                assert names.index("sw_aerosol") == names.index("sw_solver") - 1, k


def test_resolve_options_refusals():
    pytest.importorskip("torch")
    from types import SimpleNamespace
    from rrtmgpnn.pipeline import ClearSkyStep
    aer = {"lw_tau": 0, "sw_tau": 0, "sw_ssa": 0, "sw_g": 0}
    clouds = (0, 0, 0, 0)

    def resolve(aerosols=aer, clouds=None, sw=True, byband=False, clrsky=False, mcica=None, jacobian=False):
        s = SimpleNamespace()
        ClearSkyStep._resolve_options(s, True, clouds, sw, 0, byband, clrsky, mcica, aerosols, jacobian)
        return s

    assert resolve().aerosols and not resolve(aerosols=None).aerosols
    assert resolve(clouds=clouds, clrsky=True).aerosols
    assert resolve(clouds=clouds, mcica={"seed": 1, "clrsky": True}).aerosols
    assert resolve(aerosols={"lw_tau": 0}, sw=False).aerosols
    for kw in ({"byband": True}, {"jacobian": True}, {"clouds": clouds, "mcica": {"seed": 1, "byband": True}}):
        with pytest.raises(ValueError, match="aerosols with byband=True, jacobian=True or mcica"):
            resolve(**kw)
    with pytest.raises(ValueError, match="aerosols: expected the keys"):
        resolve(aerosols={"lw_tau": 0})
    with pytest.raises(ValueError, match="aerosols: expected the keys"):
        resolve(sw=False)
