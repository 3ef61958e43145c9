"""The candidate table of Engine.edit_curves / counterfactual_search / integrated_gradients, well formed and malformed
— a test helper.  One table for engine.check_candidates on the host (tests/test_candidate_checks_host.py) and for the
three Engine methods on the GPU (tests/test_gpu_ops_refusals.py).  The messages are the ones the three methods raised
when each carried its own copy of the checks, written out here: a reworded refusal fails both tests.

The base case: N = 8, R = 2, two queries with 3 and 2 candidates (qptr = [0, 3, 5]); relations ascend inside a query
and fall back across the boundary; candidates 0 and 1 are partners; K = 3."""
import numpy as np

N, R, Q, C, K = 8, 2, 2, 5, 3
TRIPLES = np.array([[0, 0, 2], [1, 1, 3]], np.int64)
# the per-candidate arrays each method reads beside rel / col / role / val
EXTRA = {"edit_curves": ("step",), "counterfactual_search": ("partner", "eligible"),
         "integrated_gradients": ("eligible",)}
CLAUSE = {"edit_curves": ", step in [-1, K)", "counterfactual_search": ", partner in [-1, n)",
          "integrated_gradients": ""}
QPTR = "{who}: cand['qptr'] must be (Q + 1,), ascending from 0 to the candidate count"
LENGTH = "{who}: the candidate arrays must be of one length"
RANGE = "{who}: candidate out of range (rel, col, role in 1..3{clause}) or relations not ascending inside a query"
SYMMETRY = "{who}: partner must be symmetric"


def base(who):
    full = dict(qptr=np.array([0, 3, 5], np.int64), rel=np.array([0, 0, 1, 0, 1], np.int32),
                col=np.array([1, 2, 3, 4, 5], np.int32), role=np.array([1, 2, 3, 1, 2], np.int32),
                val=np.array([1.0, 0.5, 2.0, 1.0, 0.25], np.float32), step=np.array([0, 1, -1, 0, 2], np.int32),
                partner=np.array([1, 0, -1, -1, -1], np.int32), eligible=np.array([True, True, False, True, True]))
    return {k: full[k] for k in ("qptr", "rel", "col", "role", "val") + EXTRA[who]}


def put(name, at, value):
    """cand[name][at] = value."""
    def change(cand):
        cand[name] = cand[name].copy()
        cand[name][at] = value
    return change


def whole(name, values):
    def change(cand):
        cand[name] = np.asarray(values, cand[name].dtype)
    return change


def one_short(name):
    def change(cand):
        cand[name] = cand[name][:-1]
    return change


def no_candidates(cand):
    for k in cand:
        cand[k] = np.zeros(3, np.int64) if k == "qptr" else cand[k][:0]


EVERY = tuple(EXTRA)
# (id, the methods it applies to, the change to the base case, the refusal's message or None: accepted)
CASES = [
    ("base", EVERY, lambda cand: None, None),
    ("qptr one too long", EVERY, whole("qptr", [0, 3, 5, 5]), QPTR),
    ("qptr one too short", EVERY, whole("qptr", [0, 5]), QPTR),
    ("qptr starts at 1", EVERY, whole("qptr", [1, 3, 5]), QPTR),
    ("qptr ends short of C", EVERY, whole("qptr", [0, 3, 4]), QPTR),
    ("qptr descends", EVERY, whole("qptr", [0, 6, 5]), QPTR),
    ("col one short", EVERY, one_short("col"), LENGTH),
    ("role one short", EVERY, one_short("role"), LENGTH),
    ("val one short", EVERY, one_short("val"), LENGTH),
    ("step one short", ("edit_curves",), one_short("step"), LENGTH),
    ("partner one short", ("counterfactual_search",), one_short("partner"), LENGTH),
    ("eligible one short", ("counterfactual_search", "integrated_gradients"), one_short("eligible"), LENGTH),
    ("rel = -1", EVERY, put("rel", 0, -1), RANGE),
    ("rel = R", EVERY, put("rel", 4, R), RANGE),
    ("col = N", EVERY, put("col", 2, N), RANGE),
    ("col = -1", EVERY, put("col", 3, -1), RANGE),
    ("role = 0", EVERY, put("role", 1, 0), RANGE),
    ("role = 4", EVERY, put("role", 4, 4), RANGE),
    ("relations descend inside the first query", EVERY, whole("rel", [0, 1, 0, 0, 1]), RANGE),
    ("relations descend inside the last query", EVERY, whole("rel", [0, 0, 1, 1, 0]), RANGE),
    ("relations descend only across the boundary", EVERY, whole("rel", [1, 1, 1, 0, 0]), None),
    ("step = K", ("edit_curves",), put("step", 3, K), RANGE),
    ("step = -2", ("edit_curves",), put("step", 2, -2), RANGE),
    ("partner = the segment's length", ("counterfactual_search",), put("partner", 3, 2), RANGE),
    ("partner = -2", ("counterfactual_search",), put("partner", 2, -2), RANGE),
    ("partner not symmetric", ("counterfactual_search",), whole("partner", [1, -1, -1, -1, -1]), SYMMETRY),
    ("partners in a cycle of three", ("counterfactual_search",),
     whole("partner", [1, 2, 0, -1, -1]), SYMMETRY),
    ("no candidates", EVERY, no_candidates, None),
]


def cases():
    """(id, who, cand, message or None) of every case and method it applies to."""
    for name, methods, change, message in CASES:
        for who in methods:
            cand = base(who)
            change(cand)
            yield f"{who}: {name}", who, cand, message and message.format(who=who, clause=CLAUSE[who])
