"""The greedy counterfactual search restated on top of tests/ref_fidelity.curves (a test helper, CPU).

p(F) of a query is the last deletion point of a K = 1 explanation whose step-0 candidates are exactly F, so every
probability here goes through ref_fidelity.curves' op order (held to oracle.ref_explain.forward_with_values by
tests/test_fidelity_host.py).  ``search`` is the independent greedy (its own choices), ``replay`` follows a GIVEN
sequence of choices and returns every step's candidate probabilities."""
import numpy as np
import torch

from tests import ref_fidelity as RF

CHUNK = 1 << 14          # pseudo-candidates per ref_fidelity.curves call

def probs(params, triples, cand, items, dtype=torch.float64):
    """p(F) for every (query, F) of ``items`` (F: a bool mask over the query's candidates), float64 numpy, computed in
    ``dtype``: one ref_fidelity.curves call over pseudo-queries."""
    if not items:
        return np.zeros(0, np.float64)
    tr = np.asarray(triples, np.int64)
    qp = np.asarray(cand["qptr"], np.int64)
    sizes = np.cumsum([qp[q + 1] - qp[q] for q, _ in items])
    if sizes[-1] > CHUNK and len(items) > 1:        # curves builds a (candidates, 4, D) tensor: bounded pieces
        cut = max(1, int(np.searchsorted(sizes, CHUNK, side="right")))
        return np.concatenate([probs(params, tr, cand, items[:cut], dtype), probs(params, tr, cand, items[cut:], dtype)])
    sl = [slice(qp[q], qp[q + 1]) for q, _ in items]
    pseudo = dict(qptr=np.concatenate([[0], np.cumsum([s.stop - s.start for s in sl])]).astype(np.int64),
                  step=np.concatenate([np.where(m, 0, -1) for _, m in items]).astype(np.int32))
    for k in ("rel", "col", "role", "val"):
        pseudo[k] = np.concatenate([np.asarray(cand[k])[s] for s in sl])
    return RF.curves(params, tr[[q for q, _ in items]], pseudo, 1, dtype)[0][:, 1]


def _removed(mask, j, part):
    m = mask.copy()
    m[j] = True
    if part[j] >= 0:
        m[part[j]] = True
    return m


def crossed(p, lower, threshold):
    return (not p > threshold) if lower else bool(p > threshold)


def lowering(p0, toward, threshold):
    return {"flip": bool(p0 > threshold), "lower": True, "raise": False}[toward]


def _run(params, triples, cand, K, toward, threshold, dtype, given=None):
    """The search (``given`` None) or the replay of the (n, K) choices ``given`` (-1: no step).  Numbers are float64
    when computed in float64 and float32 (value and comparisons) when computed in float32."""
    cast = np.float64 if dtype == torch.float64 else np.float32
    thr = cast(threshold)
    n = len(triples)
    qp = np.asarray(cand["qptr"], np.int64)
    part = [np.asarray(cand["partner"][qp[q]:qp[q + 1]], np.int64) for q in range(n)]
    elig = [np.asarray(cand["eligible"][qp[q]:qp[q + 1]], bool) for q in range(n)]
    gone = [np.zeros(qp[q + 1] - qp[q], bool) for q in range(n)]
    base = probs(params, triples, cand, [(q, gone[q]) for q in range(n)], dtype).astype(cast)
    out = dict(path=np.repeat(base[:, None], K + 1, 1), chosen=np.full((n, K), -1, np.int64),
               n_steps=np.zeros(n, np.int64), flipped=np.zeros(n, bool),
               cstep=[np.full(len(g), -1, np.int64) for g in gone],
               loo=[np.full(len(g), np.nan, cast) for g in gone], lower=np.zeros(n, bool),
               tables=[[] for _ in range(n)], gap=np.full((n, K), np.inf))
    p = base.copy()
    for q in range(n):
        out["lower"][q] = lowering(p[q], toward, thr)
    for i in range(max(K, 1)):
        if given is None:
            active = [q for q in range(n) if i == 0 or (out["n_steps"][q] == i and
                                                        not crossed(p[q], out["lower"][q], thr))]
        else:
            active = [q for q in range(n) if i == 0 or (i < K and given[q, i] >= 0)]
        live = {q: np.flatnonzero(elig[q] & ~gone[q]) for q in active}
        items = [(q, _removed(gone[q], j, part[q])) for q in active for j in live[q]]
        vals = probs(params, triples, cand, items, dtype).astype(cast)
        at = 0
        for q in active:
            pj = vals[at:at + len(live[q])]
            at += len(live[q])
            if i == 0:
                out["loo"][q][live[q]] = pj
            if K == 0:
                continue
            if given is None:
                if crossed(p[q], out["lower"][q], thr) or not len(live[q]):
                    continue
                order = np.lexsort((live[q], pj if out["lower"][q] else -pj))
                b = order[0]
                if len(order) > 1:
                    out["gap"][q, i] = abs(float(pj[order[1]]) - float(pj[b]))
            else:
                if given[q, i] < 0:
                    continue
                b = int(np.flatnonzero(live[q] == given[q, i])[0])      # the given choice must be live
            out["tables"][q].append((live[q], pj, b))
            j = int(live[q][b])
            gone[q] = _removed(gone[q], j, part[q])
            out["cstep"][q][gone[q] & (out["cstep"][q] < 0)] = i
            p[q] = pj[b]
            out["chosen"][q, i], out["path"][q, i + 1:], out["n_steps"][q] = j, pj[b], i + 1
    for q in range(n):
        out["flipped"][q] = crossed(p[q], out["lower"][q], thr)
    return out


def search(params, triples, cand, K, toward="flip", threshold=0.5, dtype=torch.float64):
    """The greedy search of include/iddgcn_explain.h.  Returns a dict: ``path`` (n, K + 1), ``chosen`` (n, K),
    ``n_steps``, ``flipped``, ``lower`` (n,), per query ``cstep`` and ``loo`` arrays, ``tables``: per query one
    (live candidate indices, their probabilities, position of the choice) per step taken, and ``gap`` (n, K): the
    distance between the best and the second-best probability of each step taken (inf: no second candidate)."""
    return _run(params, triples, cand, K, toward, threshold, dtype)


def replay(params, triples, cand, chosen, toward="flip", threshold=0.5, dtype=torch.float64):
    """The same quantities along the GIVEN choices ``chosen`` (n, K; -1: no step): nothing is decided here, so the
    probabilities of the sets another implementation visited can be compared one by one."""
    chosen = np.asarray(chosen, np.int64)
    return _run(params, triples, cand, chosen.shape[1], toward, threshold, dtype, given=chosen)


# -- the shared small cases --------------------------------------------------------------------------------------
NQ, K_SMALL = 40, 8
# (d, R, saturate): at (64, 4) predictions cross 0.5; at d = 32 nothing does, so those cases take the median of the
# 40 unedited float64 probabilities as threshold
SEARCH_CASES = [(64, 4, False), (64, 4, True), (32, 3, False), (32, 8, False)]
_CASES = {}


def case(d, R, saturate=False, undirected=False):
    """The first 40 queries of ref_fidelity.small_case with their candidates, the case's threshold and the float64
    and float32 restatements of the K = 8 search, computed once."""
    from iddgcn_amd import explain as X
    from iddgcn_amd.graph import DeviceAdjacency, get_adj_mats
    key = (d, R, saturate, undirected)
    if key not in _CASES:
        N, tri, params, q = RF.small_case(d, R, saturate)
        q = q[:NQ]
        host = DeviceAdjacency(get_adj_mats(tri, N, R), N, "cpu")
        cand = X.counterfactual_candidates(host, q, undirected=undirected)
        thr = 0.5
        if d == 32:
            p0 = probs(params, q, cand, [(j, np.zeros(cand["qptr"][j + 1] - cand["qptr"][j], bool))
                                         for j in range(NQ)])
            thr = float(np.float32(np.median(p0)))
        _CASES[key] = dict(N=N, tri=tri, params=params, q=q, host=host, cand=cand, threshold=thr,
                           ref64=search(params, q, cand, K_SMALL, "flip", thr),
                           ref32=search(params, q, cand, K_SMALL, "flip", thr, torch.float32))
    return _CASES[key]
