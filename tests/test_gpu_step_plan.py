"""GPU: ClearSkyStep builds, for every option set of tests/step_plan.py, the call list, buffers and schedule recorded in
tests/golden/step_plan.json from the constructor as it stood before it was split into steps
(tests/golden/make_step_plan_golden.py): names, entries, arguments, order and stream, and every refusal with its
message.  No case launches anything."""
import json
import os

import pytest

import step_plan as P

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "step_plan.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def env(rfmip):
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "GPU tests need a device"
    torch.cuda.set_device(0)
    return P.environment(rfmip)


def test_cases_and_fixture_hold_the_same_keys(golden):
    assert sorted(golden) == sorted(k for k, _ in P.CASES)


@pytest.mark.gpu
@pytest.mark.parametrize("cid,build", P.CASES, ids=[k for k, _ in P.CASES])
def test_step_plan(cid, build, env, golden):
    want = golden[cid]
    got = json.loads(json.dumps(P.run_case(build, env)))
    if "raises" in want:
        assert got == want
        return
    assert "raises" not in got, got
    assert got["schedule"] == want["schedule"]
    assert got["buffers"] == want["buffers"]
    assert [c.split()[0] for c in got["calls"]] == [c.split()[0] for c in want["calls"]]
    for g, w in zip(got["calls"], want["calls"]):
        assert g == w
    assert got == want
