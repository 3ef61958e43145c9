"""The counterfactual search on the GPU (ops.explain_counterfactual, Engine.counterfactual_search,
explain.counterfactual_batched / occlusion_batched).

Two anchors.  (1) Every probability of the search is fidelity_curves' deletion forward, so the returned path IS the
deletion curve of the returned edges and every step's table can be recomputed by fidelity_curves, bit for bit.  (2) The
float64 restatement of tests/ref_counterfactual.py (tests/test_counterfactual_host.py asserts its inputs are not
vacuous), at tests/test_gpu_fidelity.py's bar: a probability may deviate from float64 by max(4 x the float32
restatement's own deviation, 1e-6)."""
import numpy as np
import pytest
import torch

from iddgcn_amd import _lib as L
from iddgcn_amd import explain as X
from iddgcn_amd import get_IDDGCN_Model
from iddgcn_amd.graph import DeviceAdjacency, get_adj_mats
from tests import ref_counterfactual as RC
from tests import ref_fidelity as RF

pytestmark = pytest.mark.gpu
K = RC.K_SMALL
NQ = RC.NQ
CASES = [(d, R, False) for d in (32, 64) for R in (1, 2, 4, 8)] + [(64, 4, True), (32, 2, True)]   # test_gpu_fidelity's
N_ENT, N_REL = 845, 4
_RUNS = {}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def same(a, b, keys=("p", "path", "chosen", "n_edges", "flipped")):
    """Two results agree bit for bit (probabilities compared as bit patterns)."""
    for k in keys:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and np.array_equal(bits(x) if x.dtype == np.float32 else x,
                                                     bits(y) if y.dtype == np.float32 else y), k
    if "occlusion" in a and "occlusion" in b:
        for x, y in zip(a["occlusion"][1], b["occlusion"][1]):
            assert np.array_equal(bits(x), bits(y))
    return True


def run(d, R, saturate, cuda, undirected=False):
    """A case's first 40 queries searched with K = 8 on the fused route, computed once.  The threshold is 0.5 at
    d = 64 and the median unedited probability at d = 32 (nothing crosses 0.5 there)."""
    key = (d, R, saturate, undirected)
    if key not in _RUNS:
        N, tri, params, q = RF.small_case(d, R, saturate)
        q = q[:NQ]
        model = RF.model_with(params, N, R, d)
        if (d, R, saturate) in RC.SEARCH_CASES:
            thr = RC.case(d, R, saturate)["threshold"]
        else:
            z = X.counterfactual_batched(model, tri, q, 0, fused=True)
            thr = 0.5 if d == 64 else float(np.median(z["p"]))
        stats = {}
        res = X.counterfactual_batched(model, tri, q, K, threshold=thr, undirected=undirected, fused=True,
                                       return_occlusion=True, stats=stats)
        assert stats["fused"] is True and res["path"].shape == (NQ, K + 1) and res["path"].dtype == np.float32
        _RUNS[key] = dict(N=N, tri=tri, params=params, q=q, model=model, threshold=thr, res=res)
    return _RUNS[key]


def check_path_is_deletion(model, tri, q, res, undirected, what):
    """Check 1: the deletion curve of the returned edges equals the path on every column, bit for bit."""
    assert max(len(e) for e in res["edges"]) >= 1, what
    cur = X.fidelity_curves(model, tri, q, res["edges"], undirected=undirected, fused=True)
    k = cur["deletion"].shape[1] - 1
    assert k == res["n_edges"].max() and np.array_equal(bits(cur["p"]), bits(res["p"])), what
    assert np.array_equal(bits(cur["deletion"]), bits(res["path"][:, :k + 1])), what
    assert np.array_equal(bits(res["path"][:, k:]), bits(np.repeat(res["path"][:, k:k + 1], res["path"].shape[1] - k, 1)))
    for j, e in enumerate(res["edges"]):                       # every listed edge removed something, none twice
        assert len(e) == res["n_edges"][j] and cur["effective"][j, :len(e)].all(), (what, j)
        assert np.array_equal(bits(res["path"][j, len(e):]), bits(np.full(res["path"].shape[1] - len(e),
                                                                          res["path"][j, len(e)]))), (what, j)


def check_bookkeeping(res, threshold, toward="flip"):
    """path, chosen, n_edges, flipped and direction are consistent with the stop rules, in fp32."""
    thr = np.float32(threshold)
    for j in range(len(res["p"])):
        low = {"flip": bool(res["p"][j] > thr), "lower": True, "raise": False}[toward]
        assert res["direction"][j] == (1 if low else -1)
        k = int(res["n_edges"][j])
        path = res["path"][j]
        assert all(not RC.crossed(path[i], low, thr) for i in range(k)), j
        assert bool(res["flipped"][j]) == RC.crossed(path[k], low, thr), j
        ch = res["chosen"][j]
        assert (ch[:k] >= 0).all() and (ch[k:] == -1).all() and len(set(ch[:k].tolist())) == k, j


# -- 1. the path is the deletion curve -----------------------------------------------------------------------------
@pytest.mark.parametrize("d,R,saturate", CASES)
def test_path_is_the_deletion_curve(d, R, saturate, cuda):
    for undirected in (False, True):
        c = run(d, R, saturate, cuda, undirected)
        check_path_is_deletion(c["model"], c["tri"], c["q"], c["res"], undirected, (d, R, saturate, undirected))
        check_bookkeeping(c["res"], c["threshold"])
    # the queries' own edges stored in both directions: pairs that go as one step
    c = run(d, R, saturate, cuda)
    tri2 = np.concatenate([c["tri"], c["q"][6:16], c["q"][6:16][:, ::-1]])
    host = DeviceAdjacency(get_adj_mats(tri2, c["N"], R), c["N"], "cpu")
    cand = X.counterfactual_candidates(host, c["q"], undirected=True)
    assert (cand["partner"] >= 0).sum() >= 12
    res = X.counterfactual_batched(c["model"], tri2, c["q"], K, threshold=c["threshold"], undirected=True)
    check_path_is_deletion(c["model"], tri2, c["q"], res, True, (d, R, saturate, "both directions"))
    check_bookkeeping(res, c["threshold"])
    qp = cand["qptr"]
    pair_steps = sum(int(cand["partner"][qp[j] + ch] >= 0) for j in range(NQ) for ch in res["chosen"][j] if ch >= 0)
    print(f"d={d} R={R} saturate={saturate}: {int(res['flipped'].sum())} flips, {pair_steps} steps removed a pair")
    directed = X.counterfactual_batched(c["model"], tri2, c["q"], K, threshold=c["threshold"])
    check_path_is_deletion(c["model"], tri2, c["q"], directed, False, (d, R, saturate, "both directions, directed"))


# -- 2. every step takes the best candidate ------------------------------------------------------------------------
@pytest.mark.parametrize("d,R", [(64, 4), (32, 8)])
def test_every_step_takes_the_best_candidate(d, R, cuda):
    """Per step one fidelity_curves call whose pseudo-queries are (query, edges[:i] + [j]) for every remaining j: its
    last deletion point is p(F_i + {j})."""
    c = run(d, R, False, cuda)
    model, tri, q, res = c["model"], c["tri"], c["q"], c["res"]
    cand_edges, loo = res["occlusion"]
    steps = 0
    for i in range(K):
        took = np.flatnonzero(res["n_edges"] > i)
        pq, pe, owner = [], [], []
        for j in took:
            left = [x for x in range(len(cand_edges[j])) if x not in set(res["chosen"][j, :i].tolist())]
            for x in left:
                pq.append(q[j])
                pe.append(np.concatenate([res["edges"][j][:i], cand_edges[j][x:x + 1]]))
                owner.append((j, x))
        if not pq:
            break
        val = X.fidelity_curves(model, tri, np.array(pq), pe, fused=True)["deletion"][:, i + 1]
        owner = np.array(owner)
        for j in took:
            m = owner[:, 0] == j
            xs, pj = owner[m, 1], val[m]
            key = bits(pj).astype(np.int64) * (1 if res["direction"][j] > 0 else -1)       # p >= 0: the bits order it
            best = xs[np.flatnonzero(key == key.min())[0]]
            assert res["chosen"][j, i] == best, (i, j)
            assert bits(res["path"][j, i + 1:i + 2])[0] == bits(pj[xs == best])[0], (i, j)
            if i == 0:
                assert np.array_equal(bits(loo[j]), bits(pj)), j
            steps += 1
    assert steps == res["n_edges"].sum() and steps > 200


def test_bitwise_tie_goes_to_the_lower_entry(cuda):
    """Row 0 of relation 1 holds exactly two entries whose columns have identical E rows: removing either leaves the
    same addends in the same order, so the two probabilities are the same bits and the lower candidate goes first."""
    rng = np.random.default_rng(5)
    N, R = 8, 2
    tri = np.array([(0, 1, 3), (0, 1, 5), (0, 0, 2), (1, 0, 4), (1, 0, 6)], np.int64)
    q = np.array([(0, 0, 1)], np.int64)
    for D in (32, 64):
        params = RF.make_params(N, R, D, rng)
        params["E"][5] = params["E"][3]
        model = RF.model_with(params, N, R, D)
        for toward, thr in (("lower", 0.0), ("raise", 1.0)):              # never crossed: both steps are taken
            res = X.counterfactual_batched(model, tri, q, 2, toward=toward, threshold=thr, relations=[1],
                                           return_occlusion=True)
            loo = res["occlusion"][1][0]
            assert np.isnan(loo[:3]).all() and bits(loo[3:4])[0] == bits(loo[4:5])[0]
            assert res["chosen"][0].tolist() == [3, 4] and res["edges"][0].tolist() == [[0, 1, 3], [0, 1, 5]]
            assert loo[3] != res["p"][0]                                   # the tie is not the trivial one
            check_path_is_deletion(model, tri, q, res, False, ("tie", D, toward))


# -- 3. against the float64 restatement ------------------------------------------------------------------------------
def check_along_choices(params, q, cand, res, threshold, toward, floor, what):
    """3(a): along the kernel's own choices every path value is within the bar of float64, and the chosen candidate's
    float64 value is within its own plus the optimum's bar of the float64 optimum.  bar = max(4 |p32 - p64|, floor)."""
    r64 = RC.replay(params, q, cand, res["chosen"], toward, threshold)
    r32 = RC.replay(params, q, cand, res["chosen"], toward, threshold, torch.float32)
    err = np.abs(res["path"].astype(np.float64) - r64["path"])
    bar = np.maximum(4 * np.abs(r32["path"].astype(np.float64) - r64["path"]), floor)
    assert (err <= bar).all(), (what, np.argwhere(err > bar)[:5].tolist(), err[err > bar][:5], bar[err > bar][:5])
    worst_gap = 0.0
    for j in range(len(q)):
        assert len(r64["tables"][j]) == res["n_edges"][j]
        sign = 1.0 if res["direction"][j] > 0 else -1.0
        for (live, p64, b), (_, p32, _) in zip(r64["tables"][j], r32["tables"][j]):
            tb = np.maximum(4 * np.abs(p32.astype(np.float64) - p64), floor)
            o = int(np.argmin(sign * p64))
            gap = sign * (p64[b] - p64[o])
            assert gap <= tb[b] + tb[o], (what, j, gap, tb[b], tb[o])
            worst_gap = max(worst_gap, gap)
    return float((err / bar).max()), worst_gap


@pytest.mark.parametrize("d,R,saturate", RC.SEARCH_CASES)
def test_against_the_restatement(d, R, saturate, cuda):
    ref = RC.case(d, R, saturate)
    params, q, cand, thr, r64 = ref["params"], ref["q"], ref["cand"], ref["threshold"], ref["ref64"]
    # (b) the queries the independent float64 greedy decides with room to spare, fixed before looking at the kernel:
    # along ITS choices, dev = the largest |p32 - p64| of any probability the query met; every step's runner-up gap
    # and every path value's distance from the threshold must exceed 1e-6 + 8 dev
    along32 = RC.replay(params, q, cand, r64["chosen"], "flip", thr, torch.float32)
    decided = np.ones(NQ, bool)
    for j in range(NQ):
        dev = abs(float(along32["path"][j, 0]) - r64["path"][j, 0])
        for (_, p64, _), (_, p32, _) in zip(r64["tables"][j], along32["tables"][j]):
            dev = max(dev, float(np.abs(p32.astype(np.float64) - p64).max()))
        room = 1e-6 + 8 * dev
        k = r64["n_steps"][j]
        decided[j] = (r64["gap"][j, :k] > room).all() and (np.abs(r64["path"][j, :k + 1] - thr) > room).all()
    assert (~decided).sum() <= 4, np.flatnonzero(~decided)
    c = run(d, R, saturate, cuda)
    res = c["res"]
    worst, gap = check_along_choices(params, q, cand, res, thr, "flip", 1e-6, (d, R, saturate))     # (a): all 40
    agree = (res["chosen"] == r64["chosen"]).all(1)
    print(f"d={d} R={R} saturate={saturate}: worst path error / bar {worst:.3f}, worst chosen-to-optimum gap {gap:.2e}; "
          f"{int(decided.sum())} of {NQ} queries decided, {int(agree.sum())} agree with the float64 greedy")
    assert agree[decided].all(), np.flatnonzero(decided & ~agree)
    assert np.array_equal(res["n_edges"][decided], r64["n_steps"][decided])
    assert np.array_equal(res["flipped"][decided], r64["flipped"][decided])
    assert res["flipped"].sum() >= 5 - (~decided).sum()


# -- 4. independence -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,R", [(64, 4), (32, 8)])
def test_independence(d, R, cuda):
    c = run(d, R, False, cuda)
    model, tri, q, res, thr = c["model"], c["tri"], c["q"], c["res"], c["threshold"]
    go = lambda qq, k=K, **kw: X.counterfactual_batched(model, tri, qq, k, threshold=thr, fused=True,  # noqa: E731
                                                        return_occlusion=True, **kw)
    pick = lambda r, idx: dict({k: np.asarray(r[k])[idx] for k in ("p", "path", "chosen", "n_edges", "flipped")},  # noqa
                               occlusion=(None, [r["occlusion"][1][j] for j in idx]))
    for j in (0, 2, 3, 5, 17, 39):                                          # a query alone
        assert same(go(q[j:j + 1]), pick(res, [j]))
    assert same(pick(res, [0]), pick(res, [1]))                             # the repeated query of small_case
    rev = go(q[::-1])
    assert same(rev, pick(res, list(range(NQ))[::-1]))
    assert same(go(np.concatenate([q[7:9]] * 3)), pick(res, [7, 8] * 3))
    short = go(q, 3)                                                        # K = 3 is the prefix of K = 8
    assert np.array_equal(bits(short["path"]), bits(res["path"][:, :4]))
    assert np.array_equal(short["chosen"], res["chosen"][:, :3])
    assert np.array_equal(short["n_edges"], np.minimum(res["n_edges"], 3))
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(short["occlusion"][1], res["occlusion"][1]))
    # chunks: max_entries small enough to split the batch several times
    eng, params = X._model_state(model)
    dadj = DeviceAdjacency(get_adj_mats(tri, c["N"], R), c["N"], eng.device)
    cand = X.counterfactual_candidates(dadj, q)
    whole = eng.counterfactual_search(params, dadj, q, cand, K, "flip", thr)
    parts = eng.counterfactual_search(params, dadj, q, cand, K, "flip", thr, max_entries=50)
    assert len(eng._query_chunks(cand["qptr"], 50)) >= 5
    for k in whole:
        a, b = whole[k].cpu().numpy(), parts[k].cpu().numpy()
        assert np.array_equal(bits(a) if a.dtype == np.float32 else a, bits(b) if b.dtype == np.float32 else b), k
    assert np.array_equal(bits(whole["path"].cpu().numpy()), bits(res["path"]))
    assert np.array_equal(whole["cstep"].cpu().numpy() >= 0,
                          np.isin(np.arange(len(cand["entry"])),
                                  np.concatenate([cand["qptr"][j] + res["chosen"][j, :res["n_edges"][j]]
                                                  for j in range(NQ)])))


# -- 5. rules ----------------------------------------------------------------------------------------------------------
def test_rules(cuda):
    c = run(64, 4, False, cuda)
    model, tri, q, res, thr, N = c["model"], c["tri"], c["q"], c["res"], c["threshold"], c["N"]
    host = DeviceAdjacency(get_adj_mats(tri, N, 4), N, "cpu")
    n = np.diff(X.counterfactual_candidates(host, q)["qptr"])
    # small_case: q[2] is h == t, q[3] / q[4] have an empty head / tail row, q[5] both
    assert n[5] == 0 and res["n_edges"][5] == 0 and not res["flipped"][5] and len(res["edges"][5]) == 0
    assert np.array_equal(bits(res["path"][5]), bits(np.full(K + 1, res["p"][5])))
    assert 0 < n[3] < K and res["n_edges"][3] == n[3] and not res["flipped"][3]      # K > n: runs out of candidates
    assert res["n_edges"][2] > 0 and res["n_edges"][4] > 0
    for toward in ("lower", "raise"):
        r = X.counterfactual_batched(model, tri, q, 3, toward=toward, threshold=thr)
        check_bookkeeping(r, thr, toward)
        there = ~(r["p"] > np.float32(thr)) if toward == "lower" else r["p"] > np.float32(thr)
        assert there.any() and (~there).any()
        assert (r["n_edges"][there] == 0).all() and r["flipped"][there].all()        # already on the target side
        assert (r["n_edges"][~there & (n > 0)] > 0).all()
        assert r["flipped"][5] == there[5]                                           # n = 0: from p alone
        check_path_is_deletion(model, tri, q, r, False, toward)
    # exclude_target / relations on an adjacency that stores the queries themselves, both ways
    tri2 = np.concatenate([tri, q[6:16], q[6:16][:, ::-1]])
    host2 = DeviceAdjacency(get_adj_mats(tri2, N, 4), N, "cpu")
    for kw in (dict(exclude_target=True), dict(relations=[1, 3]), dict(exclude_target=True, undirected=True)):
        cand = X.counterfactual_candidates(host2, q, **kw)
        assert 0 < (~cand["eligible"]).sum() < len(cand["eligible"])
        r = X.counterfactual_batched(model, tri2, q, K, threshold=thr, return_occlusion=True, **kw)
        for j in range(NQ):
            el = cand["eligible"][cand["qptr"][j]:cand["qptr"][j + 1]]
            assert np.array_equal(np.isnan(r["occlusion"][1][j]), ~el), (kw, j)
            assert el[r["chosen"][j, :r["n_edges"][j]]].all(), (kw, j)
        check_path_is_deletion(model, tri2, q, r, bool(kw.get("undirected")), kw)
        check_bookkeeping(r, thr)
    none = X.counterfactual_batched(model, tri, q, K, threshold=thr, relations=[], return_occlusion=True)
    assert (none["n_edges"] == 0).all() and not none["flipped"].any()
    assert np.array_equal(bits(none["p"]), bits(res["p"])) and all(np.isnan(x).all() for x in none["occlusion"][1])
    # K = 0: the occlusion table and p alone
    z = X.counterfactual_batched(model, tri, q, 0, threshold=thr, return_occlusion=True)
    assert z["path"].shape == (NQ, 1) and z["chosen"].shape == (NQ, 0) and (z["n_edges"] == 0).all()
    assert np.array_equal(bits(z["p"]), bits(res["p"])) and all(len(e) == 0 for e in z["edges"])
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(z["occlusion"][1], res["occlusion"][1]))
    assert not z["flipped"].any()
    # occlusion_batched: the table, ranked
    preds, scores = X.occlusion_batched(model, tri, q, 5, threshold=thr)
    lay_p, lay_s = X.occlusion_batched(model, tri, q[:6], 5, threshold=thr, fused=False)
    for j in range(NQ):
        loo, edges = res["occlusion"][1][j], res["occlusion"][0][j]
        sc = (res["p"][j] - loo) * np.float32(res["direction"][j])
        o = np.lexsort((np.arange(len(sc)), -sc))[:5]
        assert np.array_equal(preds[j], edges[o]) and np.array_equal(bits(scores[j]), bits(sc[o])), j
        if j < 6:
            assert len(lay_p[j]) == len(o) and np.abs(lay_s[j] - sc[o]).max(initial=0) <= 1e-4
    assert X.counterfactual_summary(res)["flip_rate"] == res["flipped"].mean()
    for bad in (dict(max_edges=65), dict(max_edges=-1), dict(toward="up")):
        with pytest.raises(L.IddgcnError):
            X.counterfactual_batched(model, tri, q, **bad)
    e = X.counterfactual_batched(model, tri, np.zeros((0, 3), np.int64), K)
    assert e["path"].shape == (0, K + 1) and e["edges"] == []


# -- 6. large rows -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,big", [(64, 330), (32, 650)])
def test_large_rows(D, big, cuda):
    """tests/test_gpu_mask_batched.py's kind of graph: one query whose candidates exceed the E rows the kernel stages
    in LDS (320 at D = 64, 640 at D = 32: the others come from global memory) and rows of degree 63, 64 and 65."""
    rng = np.random.default_rng(3)
    N, R = 700, 3
    rows = []
    for node, deg in ((1, 1), (2, 63), (3, 64), (4, 65)):
        cols = np.sort(rng.choice(np.arange(7, N), deg, replace=False))
        rows.append(np.stack([np.full(deg, node), np.zeros(deg, np.int64), cols], 1))
    half = big // 2
    rows.append(np.stack([np.full(half, 5), np.zeros(half, np.int64), np.arange(10, 10 + half)], 1))
    rows.append(np.stack([np.full(big - half, 5), np.ones(big - half, np.int64), np.arange(20, 20 + big - half)], 1))
    rows.append(np.array([[0, 0, 9], [8, 1, 0]]))
    tri = np.concatenate(rows).astype(np.int64)
    mats = get_adj_mats(tri, N, R)
    assert mats[2].nnz == 1 and mats[2].values[0] == 0                # relation 2 is empty: a placeholder, no candidate
    params = RF.make_params(N, R, D, rng)
    q = np.array([(5, 0, 6), (1, 0, 2), (2, 1, 3), (3, 0, 4)], np.int64)
    host = DeviceAdjacency(mats, N, "cpu")
    cand = X.counterfactual_candidates(host, q)
    assert np.diff(cand["qptr"]).tolist() == [big, 64, 127, 129] and big > (80 * 1024) // (4 * D)
    ref = RC.search(params, q, cand, 2, "lower", 0.0)
    assert ref["gap"].min() > 1e-5                                    # measured: 1.7e-5 at least, |p32 - p64| 1.2e-7
    model = RF.model_with(params, N, R, D)
    res = X.counterfactual_batched(model, tri, q, 2, toward="lower", threshold=0.0, fused=True)   # never crossed
    assert np.array_equal(res["chosen"], ref["chosen"])
    assert (res["n_edges"] == 2).all() and not res["flipped"].any()
    check_path_is_deletion(model, tri, q, res, False, ("large rows", D))
    worst, gap = check_along_choices(params, q, cand, res, 0.0, "lower", 1e-6, ("large rows", D))
    print(f"large rows D={D}: candidates {np.diff(cand['qptr']).tolist()}, chosen {res['chosen'].tolist()}, worst path "
          f"error / bar {worst:.3f}, worst chosen-to-optimum gap {gap:.2e}, drop {res['p'] - res['path'][:, -1]}")
    assert (res["p"] - res["path"][:, -1] > 1e-4).sum() >= 3


# -- 7. fold 4, bundled weights ------------------------------------------------------------------------------------
def test_fold4(golden, cuda):
    d, ex = golden("fold4_data.npz"), golden("explain_fold4.npz")
    model = get_IDDGCN_Model(N_ENT, N_REL, 64, 64, 123, None, 0, 4)
    model.load_weights("tests/golden/weights_fold4.npz")
    test = ex["test_triples"].astype(np.int64)
    adjacency = np.concatenate([d["X_train"].astype(np.int64), test])
    stats = {}
    res = X.counterfactual_batched(model, adjacency, test, 10, undirected=True, stats=stats)
    assert stats["fused"] is True and res["path"].shape == (288, 11)
    check_path_is_deletion(model, adjacency, test, res, True, "fold 4")
    check_bookkeeping(res, 0.5)
    s = X.counterfactual_summary(res)
    print(f"fold 4: {stats['candidates']} candidates, flip rate {s['flip_rate']:.4f}, mean / median flipping set "
          f"{s['mean_size']:.2f} / {s['median_size']:.1f}, mean |p - path[-1]| {s['mean_shift']:.4f}, relation share "
          f"{s['relation_share']}")
    assert res["flipped"].any() and not res["flipped"].all()
    # the first 8 triples on the layered route, along the fused path's choices: the per-variant deletion curve of the
    # fused edges, and the layered search itself (compared up to the first step it decides otherwise, that step's
    # probability included: both are the minimum of tables that agree within the bar)
    lay = X.fidelity_curves(model, adjacency, test[:8], res["edges"][:8], undirected=True, fused=False)
    k = lay["deletion"].shape[1] - 1
    assert np.abs(lay["deletion"] - res["path"][:8, :k + 1]).max() <= 1e-4
    ls = X.counterfactual_batched(model, adjacency, test[:8], 10, undirected=True, fused=False)
    same_steps = 0
    for j in range(8):
        assert abs(ls["p"][j] - res["p"][j]) <= 1e-4
        for i in range(min(int(ls["n_edges"][j]), int(res["n_edges"][j]))):
            assert abs(ls["path"][j, i + 1] - res["path"][j, i + 1]) <= 1e-4, (j, i)
            if ls["chosen"][j, i] != res["chosen"][j, i]:
                break
            same_steps += 1
    print(f"fold 4, layered route: {same_steps} of {int(res['n_edges'][:8].sum())} steps of the first 8 triples compared")
    assert same_steps >= res["n_edges"][:8].sum() // 2
    # occlusion as an explainer, beside the random baseline
    host = DeviceAdjacency(get_adj_mats(adjacency, N_ENT, N_REL), N_ENT, "cpu")
    fplus = {}
    for name, preds in (("occlusion", X.occlusion_batched(model, adjacency, test, 10, undirected=True)[0]),
                        ("occlusion toward=lower", X.occlusion_batched(model, adjacency, test, 10, toward="lower",
                                                                         undirected=True)[0]),
                        ("counterfactual", res["edges"]),
                        ("explaiNE", ex["explaine_preds"]),
                        ("random", X.random_explanations(host, test, 10, seed=0))):
        preds = [p if len(p) else np.full((1, 3), -1, np.int64) for p in preds]
        fplus[name] = X.fidelity_summary(X.fidelity_curves(model, adjacency, test, preds,
                                                           undirected=True))["mean"]["fidelity_plus"]
    print("fold 4 fidelity+: " + ", ".join(f"{k} {v:.4f}" for k, v in fplus.items()))
    assert fplus["occlusion"] >= fplus["random"]


# -- 8. outside the envelope -----------------------------------------------------------------------------------------
def test_outside_the_envelope(cuda):
    """D = 128: fused=True raises, fused=None takes the layered route and agrees with the restatement (1e-4)."""
    N, tri, _, q = RF.small_case(64, 2)
    params = RF.make_params(N, 2, 128, np.random.default_rng(9))
    q = q[[0, 2, 3]]
    model = RF.model_with(params, N, 2, 128)
    with pytest.raises(L.IddgcnError, match="fused=False"):
        X.counterfactual_batched(model, tri, q, 2, fused=True)
    with pytest.raises(L.IddgcnError, match="fused=False"):
        X.occlusion_batched(model, tri, q, 2, fused=True)
    stats = {}
    res = X.counterfactual_batched(model, tri, q, 2, toward="lower", threshold=0.0, return_occlusion=True, stats=stats)
    assert stats["fused"] is False and (res["n_edges"] == 2).all()
    host = DeviceAdjacency(get_adj_mats(tri, N, 2), N, "cpu")
    cand = X.counterfactual_candidates(host, q)
    worst, gap = check_along_choices(params, q, cand, res, 0.0, "lower", 1e-4, "D = 128")
    r64 = RC.replay(params, q, cand, res["chosen"], "lower", 0.0)
    for j in range(3):
        assert np.abs(res["occlusion"][1][j] - r64["loo"][j]).max() <= 1e-4
    assert np.abs(r64["path"][:, -1] - r64["path"][:, 0]).max() > 1e-3
    check_bookkeeping(res, 0.0, "lower")


# -- 9. ops.explain_counterfactual's refusals ------------------------------------------------------------------------
def test_ops_refusals(cuda, monkeypatch):
    """Wrong devices, dtypes, shapes and (with the range checks on) indices are refused before anything is launched;
    the unmodified arguments run."""
    from iddgcn_amd import ops
    N, D, R, Q, k = 6, 32, 2, 2, 3
    z = lambda *s: torch.zeros(*s, device=cuda)  # noqa: E731
    ints = lambda v: torch.tensor(v, dtype=torch.int32, device=cuda)  # noqa: E731
    good = dict(E=z(N, D), K=[z(R, D, D)] * 3, S=[z(D, D)] * 3, Wa=[z(D, R)] * 3, ba=[z(R)] * 3, rel=z(R, D),
                h=ints([0, 1]), r=ints([0, 1]), t=ints([1, 2]), qptr=torch.tensor([0, 3, 5], device=cuda),
                crel=ints([0, 0, 1, 0, 1]), ccol=ints([1, 2, 3, 0, 4]), crole=ints([1, 2, 1, 3, 3]),
                cpartner=ints([1, 0, -1, -1, -1]), celig=ints([1, 1, 1, 0, 1]), cval=z(5) + 1, k=k)
    out = ops.explain_counterfactual(**good)
    assert out["path"].shape == (Q, k + 1) and out["chosen"].shape == (Q, k) and out["loo"].shape == (5,)
    # zero weights: every p is 0.5, not above the threshold, so the search raises and every step is an all-way tie
    assert out["n_steps"].tolist() == [2, 1] and out["flipped"].tolist() == [0, 0]
    assert out["chosen"].tolist() == [[0, 2, -1], [1, -1, -1]] and out["cstep"].tolist() == [0, 0, 1, -1, 0]
    assert (out["path"] == 0.5).all() and torch.isnan(out["loo"]).tolist() == [False, False, False, True, False]
    cases = [(dict(E=good["E"].cpu()), "GPU tensor", False), (dict(cval=good["cval"].double()), "cval: expected", False),
             (dict(cpartner=good["cpartner"][:4]), "cpartner: expected shape", False),
             (dict(celig=good["celig"].long()), "celig: expected", False), (dict(k=65), "k must be", False),
             (dict(k=-1), "k must be", False), (dict(toward="up"), "toward must be", False),
             (dict(max_cand=-1), "max_cand", False), (dict(path=z(Q, k)), "path: expected shape", False),
             (dict(chosen=z(Q, k)), "chosen: expected", False), (dict(S=good["S"][:2]), "must hold", False),
             (dict(cpartner=ints([3, 0, -1, -1, -1])), "cpartner must lie", True),
             (dict(cpartner=ints([1, 0, -1, -1, 2])), "cpartner must lie", True),
             (dict(ccol=ints([1, 2, 3, 0, N])), "ccol: index out of range", True),
             (dict(qptr=torch.tensor([0, 3, 6], device=cuda)), "qptr must ascend", True)]
    for change, match, ranges in cases:
        monkeypatch.setattr(ops, "CHECK_INDEX_RANGES", ranges)
        with pytest.raises(L.IddgcnError, match=match):
            ops.explain_counterfactual(**dict(good, **change))
    monkeypatch.setattr(ops, "CHECK_INDEX_RANGES", True)
    ops.explain_counterfactual(**good)
