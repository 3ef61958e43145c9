"""Host side of the batched mask explainers (no GPU): the candidate lists, the level schedule, the selection and the
return_masks layout, against explain.get_computation_graph / get_adj_mats and the explainer oracle."""
import numpy as np
import pytest

from iddgcn_amd import explain as X
from iddgcn_amd.graph import DeviceAdjacency, get_adj_mats
from oracle import ref_explain

N_ENT, N_REL = 845, 4


def make_params(N, R, D, rng):
    p = {"E": rng.standard_normal((N, D)) / 8}
    for l in (1, 2, 3):
        p.update({f"K{l}": rng.standard_normal((R, D, D)) / D, f"S{l}": rng.standard_normal((D, D)) / 8,
                  f"relw{l}": np.zeros(R), f"Wa{l}": rng.standard_normal((D, R)) / 8,
                  f"ba{l}": rng.standard_normal(R) / 8})
    p["rel"] = rng.standard_normal((R, D)) / np.sqrt(D / 64)
    return {k: v.astype(np.float32) for k, v in p.items()}


def synthetic_case(R=3, D=32, N=40, seed=0):
    """About 260 stored entries over nodes 1 .. N-2; a self loop at node 7; relation R-1 holds the real entry (0, 0)
    and nothing else (R > 1); node N-1 has no entry.  12 triples in a row that share heads and tails: h == t, triples
    at the (0,0)-only relation, and (index 8) a triple whose computation graph is empty.  init[0, 0] = 1, so the
    (0, 0) entry passes every threshold used here and its relation is then skipped.
    Returns (adjacency triples, query triples, init (N, N) fp32, params)."""
    rng = np.random.default_rng(seed)
    tri = np.stack([rng.integers(1, N - 1, 260), rng.integers(0, max(R - 1, 1), 260), rng.integers(1, N - 1, 260)], 1)
    r1 = min(1, R - 1)
    tri = np.concatenate([tri, [[7, 0, 7], [0, R - 1, 0], [0, 0, 5], [9, r1, 0]]]).astype(np.int64)
    q = np.array([(3, 0, 4), (4, r1, 9), (3, r1, 4), (7, 0, 7), (N - 1, 0, 3), (0, R - 1, 5), (0, 0, 0),
                  (9, R - 1, N - 1), (N - 1, r1, N - 1), (4, 0, 3), (20, r1, 21), (5, 0, 0)], np.int64)
    init = rng.standard_normal((N, N)).astype(np.float32)
    init[0, 0] = 1.0
    return tri, q, init, make_params(N, R, D, rng)


EMPTY = 8      # synthetic_case's triple without a candidate


def fold4_case(golden):
    d, ex = golden("fold4_data.npz"), golden("explain_fold4.npz")
    adjacency = np.concatenate([d["X_train"].astype(np.int64), ex["test_triples"]])
    return adjacency, ex["test_triples"].astype(np.int64)


def reference_candidates(adjacency, tr, N, R):
    """(rel, row, col) of the non-placeholder entries of get_adj_mats(get_computation_graph(..)), in its order."""
    mats = get_adj_mats(X.get_computation_graph(int(tr[0]), int(tr[1]), int(tr[2]), adjacency), N, R)
    out = []
    for r, m in enumerate(mats):
        real = m.values != 0
        out.append(np.stack([np.full(real.sum(), r), m.rows[real], m.cols[real]], 1))
    return np.concatenate(out).astype(np.int64)


def check_candidates(adjacency, q, N, R):
    dadj = DeviceAdjacency(get_adj_mats(adjacency, N, R), N, "cpu")
    row, col, rel, real = X._entry_table(dadj)
    qptr, entry, crel, ccol, crole = X.mask_candidates(dadj, q)
    assert qptr.dtype == np.int64 and qptr[0] == 0 and qptr[-1] == len(entry) and len(qptr) == len(q) + 1
    assert all(a.dtype == np.int32 for a in (entry, crel, ccol, crole))
    for j, tr in enumerate(q):
        e = entry[qptr[j]:qptr[j + 1]].astype(np.int64)
        assert np.all(np.diff(e) > 0), (j, tr)                     # ascending, distinct
        assert real[e].all()
        ref = reference_candidates(adjacency, tr, N, R)
        assert np.array_equal(np.stack([rel[e], row[e], col[e]], 1).reshape(-1, 3), ref), (j, tr)
        sl = slice(qptr[j], qptr[j + 1])
        assert np.array_equal(crel[sl], rel[e]) and np.array_equal(ccol[sl], col[e])
        want = (row[e] == tr[0]) * X.ROLE_HEAD | (row[e] == tr[2]) * X.ROLE_TAIL
        assert np.array_equal(crole[sl], want)
        assert np.all((want != 0) | (col[e] == tr[0]) | (col[e] == tr[2]))
    return qptr, entry, dadj


def test_candidates_synthetic():
    tri, q, _, _ = synthetic_case(R=3)
    N, R = 40, 3
    qptr, entry, dadj = check_candidates(tri, q, N, R)
    n = np.diff(qptr)
    assert n[EMPTY] == 0 and (np.delete(n, EMPTY) > 0).all()
    row, col, rel, real = X._entry_table(dadj)
    assert real.all() and dadj.nnz[R - 1] == 1 and row[-1] == 0 and col[-1] == 0    # the real (0, 0) of relation R-1
    assert not ((row == N - 1) | (col == N - 1)).any()
    e3 = entry[qptr[3]:qptr[4]]                                    # h == t == 7: the self loop feeds both rows
    assert ((row[e3] == 7) & (col[e3] == 7)).sum() == 1
    # an empty relation's placeholder is stored in the full adjacency but is never a candidate
    tri2 = tri[tri[:, 1] != R - 1]
    dadj2 = DeviceAdjacency(get_adj_mats(tri2, N, R), N, "cpu")
    _, _, _, real2 = X._entry_table(dadj2)
    assert (~real2).sum() == 1
    _, entry2, crel2, _, _ = X.mask_candidates(dadj2, q)
    assert real2[entry2].all() and not (crel2 == R - 1).any()
    with pytest.raises(X.IddgcnError):
        X.mask_candidates(dadj, np.array([[N, 0, 1]]))


def test_candidates_fold4(golden):
    adjacency, test = fold4_case(golden)
    check_candidates(adjacency, test[:20], N_ENT, N_REL)


def check_schedule(qptr, entry, levels):
    assert levels[0] == 1
    sets = [set(entry[qptr[j]:qptr[j + 1]].tolist()) for j in range(len(levels))]
    for j in range(len(levels)):
        want = 1 + max((levels[i] for i in range(j) if sets[i] & sets[j]), default=0)
        assert levels[j] == want, j                                  # the greedy rule; sharing => strictly increasing


def test_schedule_synthetic():
    tri, q, _, _ = synthetic_case(R=3)
    dadj = DeviceAdjacency(get_adj_mats(tri, 40, 3), 40, "cpu")
    qptr, entry, *_ = X.mask_candidates(dadj, q)
    levels = X.mask_schedule(qptr, entry, dadj.total_nnz)
    check_schedule(qptr, entry, levels)
    assert levels[EMPTY] == 1 and levels.max() > 2 and len(set(levels.tolist())) < len(q)
    assert np.array_equal(X.mask_schedule(qptr, entry, dadj.total_nnz, "sequential"), np.arange(1, len(q) + 1))
    with pytest.raises(ValueError):
        X.mask_schedule(qptr, entry, dadj.total_nnz, "other")


def test_schedule_fold4(golden):
    adjacency, test = fold4_case(golden)
    assert len(test) == 288
    dadj = DeviceAdjacency(get_adj_mats(adjacency, N_ENT, N_REL), N_ENT, "cpu")
    qptr, entry, *_ = X.mask_candidates(dadj, test)
    levels = X.mask_schedule(qptr, entry, dadj.total_nnz)
    assert levels.max() == 155
    assert levels[:8].tolist() == [1, 2, 2, 3, 4, 1, 3, 5]
    check_schedule(qptr, entry, levels)
    n = np.diff(qptr)
    assert n.min() == 37 and n.max() == 467


@pytest.mark.parametrize("kind", ["gnnexplainer", "iddgcn"])
def test_selection_and_layout_against_oracle(kind):
    """select_candidates / masks_layout on the oracle's own final values give the oracle's triples, scores and
    return_masks layout: the (0,0)-only relation is kept by the threshold and then skipped, relations that are empty
    in a computation graph show their placeholder 0."""
    N, R = 40, 3
    tri, q, init, params = synthetic_case(R=R)
    kw = dict(num_epochs=5, threshold=0.2)
    if kind == "iddgcn":
        q = np.delete(q, EMPTY, 0)
        kw = dict(num_epochs=10, threshold=0.15, target_ratios=(0.5, 0.3, 0.2))
    ref_p, ref_s, ref_m = ref_explain.mask_explainer(params, tri, q, N, R, init, top_k=100, **kw)
    dadj = DeviceAdjacency(get_adj_mats(tri, N, R), N, "cpu")
    row, col, rel, _ = X._entry_table(dadj)
    qptr, entry, crel, _, _ = X.mask_candidates(dadj, q)
    skipped = placeholders = 0
    for j, tr in enumerate(q):
        sl = slice(qptr[j], qptr[j + 1])
        mats = get_adj_mats(X.get_computation_graph(tr[0], tr[1], tr[2], tri), N, R)
        real = np.concatenate([m.values != 0 for m in mats])
        assert len(ref_m[j]) == len(real)
        vals = ref_m[j][real]
        lay = X.masks_layout(crel[sl], vals, R)
        assert lay.dtype == np.float32 and np.array_equal(lay, ref_m[j].astype(np.float32))
        placeholders += int((~real).sum())
        for top_k in (3, 10, 100):
            p_, s_ = X.select_candidates(entry[sl].astype(np.int64), crel[sl], vals, row, col, R, kw["threshold"],
                                         top_k)
            assert p_.dtype == np.int64 and s_.dtype == np.float32 and p_.shape == (len(s_), 3)
            assert np.array_equal(p_, ref_p[j][:top_k]) and np.array_equal(s_, ref_s[j][:top_k].astype(np.float32))
        e = entry[sl]
        at00 = (rel[e] == R - 1) & (row[e] == 0) & (col[e] == 0)
        if at00.any():
            assert vals[at00][0] > kw["threshold"] and not (ref_p[j][:, 1] == R - 1).any()
            skipped += 1
    assert skipped >= 3 and placeholders > 0


def test_alpha_table_is_mask_adams():
    """The step-size table is MaskAdam.apply's fp32 expression, bit for bit."""
    f = np.float32
    lr, b1, b2 = 1e-3, 0.9, 0.999
    tab = X.mask_adam_alphas(lr, b1, b2, 5, 3000)
    assert tab.dtype == np.float32 and tab.shape == (3000,)
    for i in (0, 1, 2, 7, 100, 999, 2999):
        t = f(5 + i)
        assert tab[i] == f(lr) * np.sqrt(f(1) - f(b2) ** t) / (f(1) - f(b1) ** t)
