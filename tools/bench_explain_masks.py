"""Batched mask explainers (explain.gnn_explainer_batched / iddgcn_explainer_batched) next to the per-triple path
(explain.gnn_explainer / iddgcn_explainer), in one process, alternating between the two, on fold 4 with the bundled
weights and the reference's 288 test triples (N = 845, R = 4, D = 64, 37.8k stored entries).

Every timed region is a whole call (adjacency build, candidate lists and schedule, launches, selection, copy to numpy)
and ends in a synchronise.  Per path and explainer kind: median and spread (min, max) over the rounds after one
warm-up call of each.  The batched path's own split: device-event time around its launches (one per schedule level)
against the host time of the whole call.  Acceptance: the batched call's slowest round is faster than the per-triple
path's fastest round, for both kinds (``accepted``).

usage: python tools/bench_explain_masks.py [rounds] [triples]   -> one JSON line
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from iddgcn_amd import explain as X  # noqa: E402
from iddgcn_amd import get_IDDGCN_Model  # noqa: E402

KINDS = {"gnnexplainer": (X.gnn_explainer, X.gnn_explainer_batched),
         "iddgcn": (X.iddgcn_explainer, X.iddgcn_explainer_batched)}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def summary(ts, Q):
    ts = np.asarray(ts) * 1e3
    return {"median_ms": float(np.median(ts)), "min_ms": float(ts.min()), "max_ms": float(ts.max()),
            "median_us_per_triple": float(np.median(ts)) / Q * 1e3}


def main(rounds=5, n_triples=None):
    g = lambda n: dict(np.load(os.path.join(ROOT, "tests", "golden", n)))  # noqa: E731
    d, ex = g("fold4_data.npz"), g("explain_fold4.npz")
    test = ex["test_triples"].astype(np.int64)[:n_triples]
    adjacency = np.concatenate([d["X_train"].astype(np.int64), ex["test_triples"].astype(np.int64)])
    model = get_IDDGCN_Model(845, 4, 64, 64, 123, None, 0, 4)
    model.load_weights(os.path.join(ROOT, "tests", "golden", "weights_fold4.npz"))
    init = np.random.default_rng(123).standard_normal((845, 845)).astype(np.float32)
    Q = len(test)
    res = {"rounds": rounds, "Q": Q, "kinds": {}}
    for kind, (per_triple, batched) in KINDS.items():
        stats = {}
        base = lambda: per_triple(model, adjacency, test, init_value=init)  # noqa: E731
        new = lambda: batched(model, adjacency, test, init_value=init, stats=stats)  # noqa: E731
        base()                                          # warm-up: device state, workspaces, allocator pools
        new()
        tb, tn, dev_ms = [], [], []
        for _ in range(rounds):                         # alternate the two paths
            tb.append(timed(base)[0])
            tn.append(timed(new)[0])
            a, b = stats["launch_events"]
            dev_ms.append(a.elapsed_time(b))
        b, n = summary(tb, Q), summary(tn, Q)
        res["kinds"][kind] = {
            "per_triple": b, "batched": n, "speedup_median": b["median_ms"] / n["median_ms"],
            "levels": stats["levels"], "candidates": stats["candidates"],
            "batched_launches_device_ms_median": float(np.median(dev_ms)),
            "batched_host_ms_median": n["median_ms"] - float(np.median(dev_ms)),
            "accepted": n["max_ms"] < b["min_ms"]}
    res["accepted"] = all(k["accepted"] for k in res["kinds"].values())
    res["config"] = {"top_k": 10, "device": torch.cuda.get_device_name(0),
                     "timed": "whole call incl. adjacency build, schedule and copy to numpy, synchronised"}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    a = sys.argv[1:]
    main(int(a[0]) if a else 5, int(a[1]) if len(a) > 1 else None)
