"""The counterfactual search (explain.counterfactual_batched) on fold 4 with the bundled weights: the reference's 288
test triples, K = 10, undirected (N = 845, R = 4, D = 64, about 114 candidates per triple).  Three routes in one
process, interleaved round by round:

(a) the new call, split into its launches (device events around them) and the host preparation around them;
(b) what a user had before it, written from the earlier API alone: K rounds of ``fidelity_curves`` with one
    pseudo-explanation per (triple, remaining candidate) — the last deletion point is p(F + {j}) — read back, arg-min on
    the host, lists rebuilt.  It makes the same choices bit for bit (``parent_route_agrees``);
(c) the layered route (``fused=False``: one set_values + predict per evaluated variant) on the first 8 triples,
    scaled to the batch.

Every timed region is a whole call between two device events and ends in a synchronise; per route the median and
spread over the rounds after one warm-up call of each.  The findings beside the timings: flip rate, size of the
flipping sets, and the fidelity+ of the counterfactual and occlusion lists next to explaiNE's and the random baseline's.

usage: python tools/bench_counterfactual.py [rounds] [triples] [out.json]   -> one JSON line, also written to out.json
       (default profiles/r17/counterfactual.json)
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from iddgcn_amd import explain as X  # noqa: E402
from iddgcn_amd import get_IDDGCN_Model  # noqa: E402
from iddgcn_amd.graph import DeviceAdjacency, get_adj_mats  # noqa: E402
from tools.bench_fidelity import summary, timed  # noqa: E402

K, THRESHOLD, LAYERED_TRIPLES = 10, 0.5, 8


def parent_route(model, adjacency, test, N, R):
    """Route (b).  Returns (edges per triple, path (n, K + 1), flipped (n,))."""
    host = DeviceAdjacency(get_adj_mats(adjacency, N, R), N, "cpu")
    n = len(test)
    c = X.curve_steps(host, test, [np.full((1, 3), -1, np.int64)] * n)          # the candidate lists
    row = X._entry_table(host, real=False)[0][c["entry"]]
    edges_of = np.stack([row, c["rel"], c["col"]], 1).astype(np.int64)
    qp = c["qptr"]
    left = [list(range(qp[j], qp[j + 1])) for j in range(n)]
    edges = [np.zeros((0, 3), np.int64) for _ in range(n)]
    path = np.zeros((n, K + 1), np.float32)
    lower = flipped = None
    for i in range(K):
        if i == 0:
            active = [j for j in range(n)]
        else:
            active = [j for j in range(n) if not flipped[j] and len(edges[j]) == i and left[j]]
        pq, pe, owner = [], [], []
        for j in active:
            if not left[j]:                                   # step 0 needs p of every triple: an inert pseudo-edge
                pq.append(test[j]), pe.append(np.full((1, 3), -1, np.int64)), owner.append((j, -1))
            for e in left[j]:
                pq.append(test[j]), pe.append(np.concatenate([edges[j], edges_of[e:e + 1]])), owner.append((j, e))
        if not pq:
            path[:, i + 1:] = path[:, i:i + 1]
            break
        cur = X.fidelity_curves(model, adjacency, np.array(pq), pe, undirected=True)
        val, owner = cur["deletion"][:, i + 1], np.array(owner)
        if i == 0:
            first = np.unique(owner[:, 0], return_index=True)[1]
            path[:, 0] = cur["p"][first]
            lower = path[:, 0] > np.float32(THRESHOLD)
            flipped = np.zeros(n, bool)                       # toward="flip": nobody starts on the target side
        path[:, i + 1] = path[:, i]
        for j in active:
            m = (owner[:, 0] == j) & (owner[:, 1] >= 0)
            if not m.any():
                continue
            pj, es = val[m], owner[m, 1]
            b = int(np.lexsort((es, pj if lower[j] else -pj))[0])
            e = edges_of[es[b]]
            edges[j] = np.concatenate([edges[j], e[None]])
            gone = {tuple(e), (e[2], e[1], e[0])}
            left[j] = [x for x in left[j] if tuple(edges_of[x]) not in gone]
            path[j, i + 1] = pj[b]
            flipped[j] = (not pj[b] > np.float32(THRESHOLD)) if lower[j] else bool(pj[b] > np.float32(THRESHOLD))
    return edges, path, flipped


def main(rounds=5, n_triples=None, out_path=None):
    g = lambda n: dict(np.load(os.path.join(ROOT, "tests", "golden", n)))  # noqa: E731
    d, ex = g("fold4_data.npz"), g("explain_fold4.npz")
    N, R = 845, 4
    test = ex["test_triples"].astype(np.int64)[:n_triples]
    adjacency = np.concatenate([d["X_train"].astype(np.int64), ex["test_triples"].astype(np.int64)])
    model = get_IDDGCN_Model(N, R, 64, 64, 123, None, 0, 4)
    model.load_weights(os.path.join(ROOT, "tests", "golden", "weights_fold4.npz"))
    Q = len(test)
    nl = min(LAYERED_TRIPLES, Q)
    stats = {}
    new = lambda: X.counterfactual_batched(model, adjacency, test, K, undirected=True, stats=stats)  # noqa: E731
    old = lambda: parent_route(model, adjacency, test, N, R)  # noqa: E731
    lay = lambda: X.counterfactual_batched(model, adjacency, test[:nl], K, undirected=True, fused=False)  # noqa: E731
    ours, theirs, layered = new(), old(), lay()             # warm-up: device state, workspaces, allocator pools
    ta, tb, tc, dev_ms = [], [], [], []
    for _ in range(rounds):                                 # interleave the three routes
        ta.append(timed(new)[0])
        a, b = stats["launch_events"]
        dev_ms.append(a.elapsed_time(b))
        tb.append(timed(old)[0])
        tc.append(timed(lay)[0])
    agrees = (all(np.array_equal(x, y) for x, y in zip(ours["edges"], theirs[0])) and
              np.array_equal(ours["path"].view(np.int32), theirs[1].view(np.int32)) and
              np.array_equal(ours["flipped"], theirs[2]))
    same_choice = (layered["chosen"] == ours["chosen"][:nl]).all(1)
    sa, sb, sc = summary(ta, Q), summary(tb, Q), summary(tc, nl)
    # findings: what the search found, and the fidelity of its lists beside the other explainers'
    s = X.counterfactual_summary(ours)
    host = DeviceAdjacency(get_adj_mats(adjacency, N, R), N, "cpu")
    pad = lambda preds: [p if len(p) else np.full((1, 3), -1, np.int64) for p in preds]  # noqa: E731
    lists = {"counterfactual": ours["edges"],
             "occlusion": X.occlusion_batched(model, adjacency, test, K, undirected=True)[0],
             "occlusion_toward_lower": X.occlusion_batched(model, adjacency, test, K, toward="lower",
                                                           undirected=True)[0],
             "explaine": list(ex["explaine_preds"][:n_triples]),
             "random": X.random_explanations(host, test, K, seed=0)}
    fidelity = {}
    for name, preds in lists.items():
        fs = X.fidelity_summary(X.fidelity_curves(model, adjacency, test, pad(preds), undirected=True))
        fidelity[name] = dict(fs["mean"], effective_share=fs["effective_share"])
    res = {"rounds": rounds, "Q": Q, "K": K, "undirected": True, "threshold": THRESHOLD,
           "candidates": stats["candidates"], "launches": 2 * K,
           "fused": sa, "fused_launches_device_ms": summary(dev_ms, Q),
           "fused_host_ms_median": sa["median_ms"] - float(np.median(dev_ms)),
           "parent_route": sb, "parent_route_agrees": bool(agrees),
           "layered": dict(sc, triples=nl, scaled_median_ms=sc["median_ms"] * Q / nl,
                           same_choices_as_fused=int(same_choice.sum()),
                           max_abs_p_difference=float(np.abs(layered["p"] - ours["p"][:nl]).max())),
           "speedup_over_parent_route": sb["median_ms"] / sa["median_ms"],
           "speedup_over_layered_scaled": sc["median_ms"] * Q / nl / sa["median_ms"],
           "findings": dict(s, relation_share={str(k): v for k, v in s["relation_share"].items()},
                            steps_taken=int(ours["n_edges"].sum()), fidelity=fidelity),
           "config": {"device": torch.cuda.get_device_name(0),
                      "timed": "whole call incl. adjacency build, candidate lists and copy to numpy, device events"}}
    line = json.dumps(res)
    print(line, flush=True)
    out_path = out_path or os.path.join(ROOT, "profiles", "r17", "counterfactual.json")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    a = sys.argv[1:]
    main(int(a[0]) if a else 5, int(a[1]) if len(a) > 1 and a[1] != "all" else None, a[2] if len(a) > 2 else None)
