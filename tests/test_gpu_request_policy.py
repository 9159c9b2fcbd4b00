"""GPU (host work only): what every public solver symbol answers to every combination of armed requests, through the
built library, against tests/golden/request_policy.json -- the parent commit's answers, recorded from its library by
tests/golden/make_request_policy_golden.py.  No call reaches a launcher (tau is null), every call is followed by the
same call with nothing armed, which must give the nothing-armed answer, and the context's launch record must not move
(request_policy_cells.Walker.walk).

Rule A: a cell the parent accepts, or refuses for exactly one reason, gives the parent's status and message.  Rule B:
where several reasons apply, the answer is one the parent gives for the same symbol with part of the requests switched
off; acceptance and refusal never stand in for each other.  The cells that pass by rule B with another answer than the
parent's are counted, and fall into the groups of request_policy_cells.RULE_B_GROUPS."""
import pytest

import request_policy_cells as C

pytestmark = pytest.mark.gpu


def test_every_cell_follows_the_parent():
    from rrtmgpnn import _lib
    w = C.Walker(C.load(_lib.LIB_PATH))
    try:
        new = {s: w.walk(s) for s in C.SYMBOLS}
    finally:
        w.close()
    failures, cells, groups = C.rule_b_summary(C.golden(), new)
    assert not failures, "%d cells, the first: %s" % (len(failures), failures[:3])
    assert cells == C.RULE_B_CELLS and groups == C.RULE_B_GROUPS, (cells, sorted(groups ^ C.RULE_B_GROUPS))
