"""engine.check_candidates on the host: the one place where the candidate table of Engine.edit_curves /
counterfactual_search / integrated_gradients is checked.  A table of malformed inputs (tests/candidate_cases.py) per
method name, the exception type and the whole message compared — the messages are written out in the table, not read
from the code under test.  tests/test_gpu_ops_refusals.py sends the same table through the three methods."""
import numpy as np
import pytest

from iddgcn_amd import _lib as L
from iddgcn_amd.engine import Engine, check_candidates
from tests import candidate_cases as CC

CASES = list(CC.cases())


def check(who, cand, Q=CC.Q):
    return check_candidates(who, cand, Q, CC.N, CC.R, CC.EXTRA[who], CC.K if who == "edit_curves" else None)


@pytest.mark.parametrize("who, cand, message", [pytest.param(*c[1:], id=c[0]) for c in CASES])
def test_candidate_table(who, cand, message):
    if message is None:
        qp, C = check(who, cand)
        assert qp.dtype == np.int64 and np.array_equal(qp, cand["qptr"]) and C == len(cand["rel"])
        return
    with pytest.raises(L.IddgcnError) as e:
        check(who, cand)
    assert type(e.value) is L.IddgcnError and str(e.value) == message


def test_the_table_has_every_kind_of_case():
    """Not vacuous: each message occurs for each method it can occur for, and accepted cases exist beside them."""
    seen = {(who, message) for _, who, _, message in CASES}
    for who in CC.EXTRA:
        for text in (CC.QPTR, CC.LENGTH, CC.RANGE):
            assert (who, text.format(who=who, clause=CC.CLAUSE[who])) in seen
        assert sum(1 for _, w, _, message in CASES if w == who and message is None) == 3
    assert ("counterfactual_search", CC.SYMMETRY.format(who="counterfactual_search")) in seen
    base = CC.base("counterfactual_search")
    assert (len(base["rel"]), len(base["qptr"]) - 1) == (CC.C, CC.Q) and base["qptr"].tolist() == [0, 3, 5]


@pytest.mark.parametrize("who", list(CC.EXTRA))
def test_no_query(who):
    empty = {k: (v[:1] if k == "qptr" else v[:0]) for k, v in CC.base(who).items()}
    qp, C = check(who, empty, Q=0)
    assert qp.tolist() == [0] and C == 0 and Engine._query_chunks(qp, 10) == []
    with pytest.raises(L.IddgcnError) as e:       # two queries' table for none
        check(who, CC.base(who), Q=0)
    assert str(e.value) == CC.QPTR.format(who=who)


def test_step_needs_K():
    with pytest.raises(TypeError):
        check_candidates("edit_curves", CC.base("edit_curves"), CC.Q, CC.N, CC.R, ("step",))
