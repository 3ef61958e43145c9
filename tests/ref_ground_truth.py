"""CPU restatement of the explanation ground truth (the five steps of include/iddgcn_ground_truth.h), written from
the semantics with dict lookups and the GENERAL `added` set of pairs (so it also says what the reference does when
mutation and drug ids overlap).  A helper for the ground-truth tests, not a test module."""
import functools
import os
from collections import Counter, defaultdict

import numpy as np

from tests.conftest import GOLDEN, REFERENCE


def similar_lists(sim):
    """node -> [b of the rows (a, _, b) with a == node, table order] + [a of the rows with b == node, table order]"""
    fwd, rev = defaultdict(list), defaultdict(list)
    for a, _, b in np.asarray(sim, dtype=np.int64).reshape(-1, 3).tolist():
        fwd[a].append(b)
        rev[b].append(a)
    return {v: fwd.get(v, []) + rev.get(v, []) for v in set(fwd) | set(rev)}


def ground_truth(dc, mu_sim, drug_sim, queries=None, drug_rel=2, mu_rel=3):
    """List (one entry per query, default the rows of dc) of int64 (n, 3) arrays."""
    dc = np.asarray(dc, dtype=np.int64).reshape(-1, 3)
    count = Counter(map(tuple, dc.tolist()))
    sm_of, sd_of = similar_lists(mu_sim), similar_lists(drug_sim)
    out = []
    for mu0, rel0, drug0 in (dc if queries is None else np.asarray(queries, dtype=np.int64).reshape(-1, 3)).tolist():
        sm, sd = sm_of.get(mu0, []), sd_of.get(drug0, [])
        gt, added = [], set()
        for m in sm:                                   # step 1
            c = count.get((m, rel0, drug0), 0)
            gt += [(m, rel0, drug0)] * c
            if c:
                added.add((drug0, mu0))
        for d in sd:                                   # step 2
            c = count.get((mu0, rel0, d), 0)
            gt += [(mu0, rel0, d)] * c
            if c:
                added.add((d, mu0))
        for d in sd:                                   # step 3
            for m in sm:
                c = count.get((m, rel0, d), 0)
                gt += [(m, rel0, d)] * c
                if c:
                    added.add((d, m))
        for d in sd:                                   # step 4
            if any(count.get((m, rel0, d), 0) for m in [mu0] + sm) and (drug0, d) not in added:
                gt.append((drug0, drug_rel, d))
                added.add((drug0, d))
        for m in sm:                                   # step 5
            if any(count.get((m, rel0, d), 0) for d in [drug0] + sd) and (mu0, m) not in added:
                gt.append((mu0, mu_rel, m))
                added.add((mu0, m))
        out.append(np.asarray(gt, dtype=np.int64).reshape(-1, 3))
    return out


def as_csr(gts):
    """(ptr int64 [Q+1], triples int64 [total, 3]) of a list of per-query arrays."""
    ptr = np.concatenate([[0], np.cumsum([len(g) for g in gts])]).astype(np.int64)
    tri = np.concatenate(gts).astype(np.int64) if len(gts) else np.zeros((0, 3), np.int64)
    return ptr, tri.reshape(-1, 3)


def fixture_lists(gt_all):
    """The fixture's gt_all (int32, -1 padded) as (queries (Q, 3), list of per-query (n, 3) int64 arrays)."""
    gt_all = np.asarray(gt_all, dtype=np.int64)
    rest = gt_all[:, 3:].reshape(len(gt_all), -1, 3)
    n = (rest[:, :, 0] >= 0).sum(1)
    for row, k in zip(rest, n):                        # the padding is a suffix and whole triples
        assert (row[:k] >= 0).all() and (row[k:] == -1).all()
    return gt_all[:, :3], [row[:k] for row, k in zip(rest, n)]


@functools.lru_cache(maxsize=None)
def bundled():
    """(dc, mu_sim, drug_sim) of the bundled prediction datasets, loaded the way the reference loads them."""
    from iddgcn_amd import ground_truth as G
    return (G.load_response_csv(os.path.join(REFERENCE, "triplets_dc.csv")),
            G.load_similarity_csv(os.path.join(REFERENCE, "mu_similar0.97.csv")),
            G.load_similarity_csv(os.path.join(REFERENCE, "drug_similar0.78.csv")))


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(os.path.join(GOLDEN, "ground_truth.npz"), allow_pickle=False))
