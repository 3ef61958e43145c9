"""Batched explaiNE (explain.explaine_batched) next to the per-triple path (explain.explaine(graph=True)), in one
process, alternating between the two, on three shapes:

  fold4       fold 4, bundled weights, the reference's 288 test triples (N = 845, R = 4, D = 64, 37.8k entries)
  fold4x16    the same triples tiled to Q = 4,608 (a timed window of more than a fraction of a millisecond)
  synth20k    a seeded synthetic graph, N = 20,000, about 400k entries, R = 4, D = 64, Q = 512

Every timed region is a whole call (adjacency build, launches, ranking, copy to numpy) and ends in a synchronise.
Per path: median and spread (min, max) over the rounds after one warm-up call of every shape.  The batched path's
own split comes from device events around its launches (node tables, seeds, row gradients, top-k) and a host timer
around the completion of triples with fewer than k positive candidates.

usage: python tools/bench_explain_batched.py [rounds] [shape ...]   -> one JSON line
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
from iddgcn_amd.utils import synthetic_graph  # noqa: E402


def shapes():
    g = lambda n: dict(np.load(os.path.join(ROOT, "tests", "golden", n)))  # noqa: E731
    d, ex = g("fold4_data.npz"), g("explain_fold4.npz")
    test = ex["test_triples"].astype(np.int64)
    adjacency = np.concatenate([d["X_train"].astype(np.int64), test])
    model = get_IDDGCN_Model(845, 4, 64, 64, 123, None, 0, 4)
    model.load_weights(os.path.join(ROOT, "tests", "golden", "weights_fold4.npz"))
    yield "fold4", model, adjacency, test
    yield "fold4x16", model, adjacency, np.tile(test, (16, 1))
    N, R = 20000, 4
    pos, _ = synthetic_graph(N, R, 400000, seed=7)
    big = get_IDDGCN_Model(N, R, 64, 64, 123, None, 0, 0, init="independent")
    yield "synth20k", big, pos, pos[np.random.default_rng(7).choice(len(pos), 512, replace=False)]


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


def main(rounds=5, only=()):
    res = {"rounds": rounds, "shapes": {}}
    for name, model, adjacency, triples in shapes():
        if only and name not in only:
            continue
        Q = len(triples)
        base = lambda: X.explaine(model, adjacency, triples, top_k=10, graph=True)  # noqa: E731
        stats = {}
        new = lambda: X.explaine_batched(model, adjacency, triples, top_k=10, stats=stats)  # noqa: E731
        base()                                          # warm-up: device state, workspaces, graph capture
        new()
        eng = model._device_state()
        tb, tn, split, nnz_c = [], [], {}, None
        for _ in range(rounds):                         # alternate the two paths
            tb.append(timed(base)[0])
            eng.probe = {}
            tn.append(timed(new)[0])
            for k, evs in eng.probe.items():
                split.setdefault(k[3:] + "_ms", []).append(sum(a.elapsed_time(b) for a, b in evs))
            eng.probe = None
            split.setdefault("host_completion_ms", []).append(stats["host_complete_s"] * 1e3)
        b, n = summary(tb, Q), summary(tn, Q)
        res["shapes"][name] = {
            "Q": Q, "num_entities": model.num_entities, "per_triple_graph": b, "batched": n,
            "speedup_median": b["median_ms"] / n["median_ms"],
            "batched_split_median": {k: float(np.median(v)) for k, v in split.items()},
            "host_completed_triples": stats["host_completed"]}
    res["config"] = {"top_k": 10, "device": torch.cuda.get_device_name(0),
                     "timed": "whole call incl. adjacency build and copy to numpy, synchronised"}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    a = sys.argv[1:]
    main(int(a[0]) if a else 5, tuple(a[1:]))
