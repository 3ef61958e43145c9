"""The counterfactual search's host side: candidate rules, the restatement's own properties (stop rules, tie rule,
prefix consistency, non-vacuous inputs), counterfactual_summary and the C entry's refusals.  No GPU."""
import ctypes

import numpy as np
import pytest

import iddgcn_amd
from iddgcn_amd import _lib
from iddgcn_amd import explain as X
from iddgcn_amd.graph import DeviceAdjacency, get_adj_mats
from tests import ref_counterfactual as RC
from tests import ref_fidelity as RF

ENTRY = "iddgcn_explain_counterfactual_f32"


def _graph():
    """tests/test_fidelity_host.py's hand graph, N = 12, R = 2.  Row 3: (3,0,1) (3,0,4) (3,1,4) (3,1,3); row 4:
    (4,0,3) (4,0,9); others: (1,0,3) (9,1,4) (7,0,7) (5,1,6)."""
    tri = np.array([(3, 0, 1), (3, 0, 4), (3, 1, 4), (3, 1, 3), (4, 0, 3), (4, 0, 9), (1, 0, 3), (9, 1, 4), (7, 0, 7),
                    (5, 1, 6)], np.int64)
    return tri, DeviceAdjacency(get_adj_mats(tri, 12, 2), 12, "cpu")


def _table(c, q, field):
    """{(row, rel, col): field} of query q's candidates; partner as the partner's (row, rel, col)."""
    sl = slice(c["qptr"][q], c["qptr"][q + 1])
    keys = [(int(a), int(b), int(d)) for a, b, d in zip(c["row"][sl], c["rel"][sl], c["col"][sl])]
    vals = c[field][sl]
    if field == "partner":
        vals = [keys[p] if p >= 0 else None for p in vals]
    return dict(zip(keys, (v if field == "partner" else v.item() for v in vals)))


def test_candidates_rules():
    tri, dadj = _graph()
    q = np.array([(3, 0, 4), (3, 1, 3), (7, 0, 7), (11, 0, 5), (11, 1, 10)], np.int64)
    c = X.counterfactual_candidates(dadj, q)
    s = X.curve_steps(dadj, q, [np.array([(0, 0, 0)])] * 5)
    for k in ("qptr", "entry", "rel", "col", "role", "val"):                    # curve_steps' candidates, its order
        assert np.array_equal(c[k], s[k]) and c[k].dtype == s[k].dtype, k
    assert c["qptr"].tolist() == [0, 6, 10, 11, 12, 12]                         # (11, 1, 10): both rows empty
    assert c["partner"].dtype == np.int32 and c["eligible"].dtype == bool
    assert (c["partner"] == -1).all() and c["eligible"].all()                   # directed, nothing excluded
    assert list(_table(c, 0, "eligible")) == [(3, 0, 1), (3, 0, 4), (4, 0, 3), (4, 0, 9), (3, 1, 3), (3, 1, 4)]
    # undirected: (3,0,4) <-> (4,0,3), the only pair between h and t; (3,1,4) has no stored reverse, (3,1,3) and
    # (7,0,7) are their own reverse
    u = X.counterfactual_candidates(dadj, q, undirected=True)
    assert _table(u, 0, "partner") == {(3, 0, 1): None, (3, 0, 4): (4, 0, 3), (4, 0, 3): (3, 0, 4), (4, 0, 9): None,
                                      (3, 1, 3): None, (3, 1, 4): None}
    assert all(v is None for j in (1, 2, 3) for v in _table(u, j, "partner").values())
    for j in range(len(q)):                                                     # symmetric, inside the segment
        p = u["partner"][u["qptr"][j]:u["qptr"][j + 1]]
        has = np.flatnonzero(p >= 0)
        assert (p < len(p)).all() and np.array_equal(p[p[has]], has)
    # h == t: every candidate feeds both rows, a self loop has no partner
    assert (u["role"][u["qptr"][1]:u["qptr"][2]] == X.ROLE_HEAD | X.ROLE_TAIL).all()
    # exclude_target: (h, r, t) and (t, r, h) of the query's own relation only
    e = X.counterfactual_candidates(dadj, q, exclude_target=True)
    assert [k for k, v in _table(e, 0, "eligible").items() if not v] == [(3, 0, 4), (4, 0, 3)]
    assert [k for k, v in _table(e, 1, "eligible").items() if not v] == [(3, 1, 3)]
    assert _table(e, 2, "eligible") == {(7, 0, 7): False} and _table(e, 3, "eligible") == {(5, 1, 6): True}
    # relations
    r = X.counterfactual_candidates(dadj, q, relations=[1])
    assert np.array_equal(r["eligible"], r["rel"] == 1)
    assert not X.counterfactual_candidates(dadj, q, relations=[])["eligible"].any()
    both = X.counterfactual_candidates(dadj, q, exclude_target=True, relations=[0, 1], undirected=True)
    assert np.array_equal(both["eligible"], e["eligible"]) and np.array_equal(both["partner"], u["partner"])
    with pytest.raises(X.IddgcnError):
        X.counterfactual_candidates(dadj, q, relations=[2])
    z = X.counterfactual_candidates(dadj, np.zeros((0, 3), np.int64), undirected=True)
    assert z["qptr"].tolist() == [0] and len(z["partner"]) == 0


def test_public_names():
    for name in ("counterfactual_batched", "occlusion_batched", "counterfactual_summary"):
        assert getattr(iddgcn_amd, name) is getattr(X, name)


# -- the restatement ---------------------------------------------------------------------------------------------
def test_restatement_stop_rules_and_prefix():
    c = RC.case(64, 4)
    params, q, cand, thr = c["params"], c["q"], c["cand"], c["threshold"]
    r = c["ref64"]
    n = np.diff(cand["qptr"])
    p0 = r["path"][:, 0]
    assert np.array_equal(r["lower"], p0 > thr)
    for j in range(RC.NQ):
        k = r["n_steps"][j]
        path, low = r["path"][j], r["lower"][j]
        # never a step from the target side, never more steps than candidates, a stop before K only for a reason
        assert all(not RC.crossed(path[i], low, thr) for i in range(k))
        assert r["flipped"][j] == RC.crossed(path[k], low, thr)
        assert k == RC.K_SMALL or r["flipped"][j] or k == n[j]
        assert (path[k:] == path[k]).all() and (r["chosen"][j, k:] == -1).all()
        ch = r["chosen"][j, :k]
        assert len(set(ch.tolist())) == k and np.array_equal(r["cstep"][j][ch], np.arange(k))
        assert (np.delete(r["cstep"][j], ch) == -1).all()
        # every step took the best of its table, the lowest index among equals
        for live, pj, b in r["tables"][j]:
            key = pj if low else -pj
            assert key[b] == key.min() and b == np.flatnonzero(key == key.min())[0]
        assert np.isfinite(r["loo"][j]).all()
    assert n[3] < 8 and n[5] == 0 and r["n_steps"][5] == 0                     # the empty rows of small_case
    assert r["n_steps"][3] == n[3] and not r["flipped"][3]                     # .. run out of candidates
    # a shorter search is the prefix of the longer one
    s = RC.search(params, q, cand, 3, "flip", thr)
    assert np.array_equal(s["chosen"], r["chosen"][:, :3]) and np.array_equal(s["path"], r["path"][:, :4])
    assert np.array_equal(s["n_steps"], np.minimum(r["n_steps"], 3))
    z = RC.search(params, q, cand, 0, "flip", thr)
    assert z["path"].shape == (RC.NQ, 1) and np.array_equal(z["path"][:, 0], p0)
    assert all(np.array_equal(a, b) for a, b in zip(z["loo"], r["loo"]))
    # fixed directions: a query already on the target side takes no step and counts as flipped
    lo = RC.search(params, q, cand, 2, "lower", thr)
    neg = ~(p0 > thr)
    assert neg.any() and (lo["n_steps"][neg] == 0).all() and lo["flipped"][neg].all()
    ra = RC.search(params, q, cand, 2, "raise", thr)
    assert (ra["n_steps"][~neg] == 0).all() and ra["flipped"][~neg].all() and (ra["n_steps"][neg & (n > 0)] > 0).all()
    # replay along the search's own choices reproduces it
    rp = RC.replay(params, q, cand, r["chosen"], "flip", thr)
    assert np.array_equal(rp["path"], r["path"]) and np.array_equal(rp["n_steps"], r["n_steps"])


def test_restatement_tie_rule():
    """Two entries of one row and relation whose columns have the same E row: removing either gives the same sets of
    addends, so the same float64 probability, and the lower index wins."""
    rng = np.random.default_rng(5)
    N, R, D = 8, 2, 32
    tri = np.array([(0, 1, 3), (0, 1, 5), (0, 0, 2), (1, 0, 4), (1, 0, 6)], np.int64)
    params = RF.make_params(N, R, D, rng)
    params["E"][5] = params["E"][3]
    host = DeviceAdjacency(get_adj_mats(tri, N, R), N, "cpu")
    q = np.array([(0, 0, 1)], np.int64)
    cand = X.counterfactual_candidates(host, q, relations=[1])
    assert cand["eligible"].tolist() == [False, False, False, True, True]
    for toward in ("lower", "raise"):
        r = RC.search(params, q, cand, 2, toward, 2.0 if toward == "raise" else -1.0)
        live, pj, b = r["tables"][0][0]
        assert live.tolist() == [3, 4] and pj[0] == pj[1] and r["chosen"][0].tolist() == [3, 4]


@pytest.mark.parametrize("d,R,saturate", RC.SEARCH_CASES)
def test_inputs_are_not_vacuous(d, R, saturate):
    """Asserted on the float64 restatement alone.  Measured: flips 7 / 5 / 11 / 6, full runs 30 / 32 / 24 / 32, and
    0 / 0 / 0 / 2 queries with a runner-up closer than 1e-6 at some step."""
    c = RC.case(d, R, saturate)
    r = c["ref64"]
    flips, full = int(r["flipped"].sum()), int((r["n_steps"] == RC.K_SMALL).sum())
    counts = sorted(set(r["n_steps"][r["flipped"]].tolist()))
    close = int((r["gap"].min(1) <= 1e-6).sum())
    print(f"d={d} R={R} saturate={saturate} threshold={c['threshold']:.6f}: {flips} flips at step counts {counts}, "
          f"{full} full runs, {close} queries with a runner-up within 1e-6")
    assert flips >= 5 and len(counts) >= 3 and full >= 20 and close <= 4
    assert (r["lower"].sum() > 0) and (~r["lower"]).sum() > 0                   # both directions searched


def test_summary_by_hand():
    res = dict(p=np.array([0.9, 0.2, 0.7, 0.6], np.float32),
               path=np.array([[0.9, 0.6, 0.4], [0.2, 0.3, 0.3], [0.7, 0.7, 0.65], [0.6, 0.6, 0.6]], np.float32),
               n_edges=np.array([2, 1, 2, 0]), flipped=np.array([True, False, False, False]),
               edges=[np.array([(1, 0, 2), (1, 3, 4)]), np.array([(5, 3, 6)]), np.array([(7, 1, 8), (7, 3, 9)]),
                      np.zeros((0, 3), np.int64)])
    s = X.counterfactual_summary(res)
    assert s["n"] == 4 and s["flip_rate"] == 0.25 and s["mean_size"] == 2.0 and s["median_size"] == 2.0
    assert abs(s["mean_shift"] - (0.5 + 0.1 + 0.05 + 0.0) / 4) < 1e-7
    assert s["relation_share"] == {0: 0.2, 1: 0.2, 3: 0.6}
    res["flipped"] = np.array([True, True, False, False])
    s = X.counterfactual_summary(res)
    assert s["flip_rate"] == 0.5 and s["mean_size"] == 1.5 and s["median_size"] == 1.5
    empty = X.counterfactual_summary(dict(p=np.zeros(0), path=np.zeros((0, 3)), n_edges=np.zeros(0, int),
                                          flipped=np.zeros(0, bool), edges=[]))
    assert empty == dict(n=0, flip_rate=0.0, mean_size=0.0, median_size=0.0, mean_shift=0.0, relation_share={})
    with pytest.raises(ValueError):
        X.counterfactual_summary(dict(res, edges=res["edges"][:2]))


# -- the C entry -------------------------------------------------------------------------------------------------
def _args(d=64, R=2, k=10, Q=1, N=10, mode=0, max_cand=8, ptr=None):
    a = _lib.CounterfactualArgs()
    a.N, a.d, a.R, a.k, a.Q, a.mode, a.threshold, a.max_cand = N, d, R, k, Q, mode, 0.5, max_cand
    for f, _ in _lib.CounterfactualArgs._fields_[8:]:
        if f in ("K", "S", "Wa", "ba"):
            setattr(a, f, (ctypes.c_void_p * 3)(ptr, ptr, ptr))
        else:
            setattr(a, f, ptr)
    return a


def test_symbol_and_rejections_before_launch():
    """Null stream, null or stand-in pointers: every return below happens on the host, before any launch."""
    lib = _lib.load()
    assert ENTRY in _lib.SIGNATURES and hasattr(lib, ENTRY)
    assert lib.iddgcn_abi_version() == _lib.ABI_VERSION == 13              # added symbol only
    fn = getattr(lib, ENTRY)
    call = lambda **kw: fn(None, ctypes.byref(_args(**kw)))  # noqa: E731
    ok = 4096                                                              # a stand-in address, never read
    for d in (16, 48, 128):
        assert call(d=d, ptr=ok) == -1
    for R in (0, 9):
        assert call(R=R, ptr=ok) == -2
    assert call(d=16, R=9, k=-1) == -1 and call(R=9, k=-1) == -2           # BAD_DIM before BAD_REL before BAD_ARG
    for k in (-1, _lib.TOPK_MAX + 1):
        assert call(k=k, ptr=ok) == -3
    for mode in (-1, 3):
        assert call(mode=mode, ptr=ok) == -3
    assert call(Q=-1, ptr=ok) == -3 and call(N=0, ptr=ok) == -3 and call(max_cand=-1, ptr=ok) == -3
    assert call(Q=0) == 0 and call(Q=0, k=0) == 0 and call(Q=0, k=_lib.TOPK_MAX) == 0     # nothing to do
    assert call() == -3 and call(k=0) == -3                                # null pointers
    assert fn(None, None) == -3
    a = _args(ptr=ok)
    a.E = ok + 4                                                           # a misaligned E
    assert fn(None, ctypes.byref(a)) == -3
    a = _args(ptr=ok)
    a.S[1] = None
    assert fn(None, ctypes.byref(a)) == -3
    for field in ("path", "chosen", "n_steps", "flipped", "scratch"):      # a missing output or scratch
        a = _args(ptr=ok)
        setattr(a, field, None)
        assert fn(None, ctypes.byref(a)) == -3, field
