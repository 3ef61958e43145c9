"""All-candidate ranking A/B on one GPU: the fused chain kernel, the layered path and the parent's only way
(predict on the materialised Q x N triples, ScoredEdges build included).

usage: python tools/screen_bench.py [--shapes a,b,c] [--rounds 5] [--out profiles/r08/screen_bench.json]

  a. N = 845,     R = 4, D = 64,  Q = 4096 tail side, bundled fold-0 weights and graph (3.5M candidates)
  b. N = 100 000, R = 2, D = 64,  Q = 64   synthetic graph, smoke-recipe parameters
  c. N = 100 000, R = 2, D = 256, Q = 32   layered and predict only (the fused kernel is D <= 64), gemm = bf16x3

Every path of a shape is warmed up once, then the paths alternate within each round.  A time is the device-event
interval around one whole call on an idle stream, the stream synchronised before and after (so host work inside the
call — the triple materialisation and the edge build of the predict path — counts).  Reports median, min, max and
candidates per second per path, and max |fused - layered| over all Q x N logits.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from iddgcn_amd.engine import Engine, FlatParams  # noqa: E402
from iddgcn_amd.graph import get_adj_mats  # noqa: E402
from iddgcn_amd.utils import synthetic_graph  # noqa: E402


def smoke_params(N, R, D, rng):
    p = {"E": rng.standard_normal((N, D)) / 8}
    for l in (1, 2, 3):
        p.update({f"K{l}": rng.standard_normal((R, D, D)) / D, f"S{l}": rng.standard_normal((D, D)) / 8,
                  f"Wa{l}": rng.standard_normal((D, R)) / 8, f"ba{l}": np.zeros(R)})
    p["rel"] = rng.standard_normal((R, D)) / np.sqrt(D / 64) * 8
    return {k: v.astype(np.float32) for k, v in p.items()}


def shape(name):
    """(N, R, D, params, graph triples, queries, engine kwargs, paths)"""
    if name == "a":
        g = os.path.join(ROOT, "tests", "golden")
        d, w = np.load(os.path.join(g, "fold0_data.npz")), dict(np.load(os.path.join(g, "weights_fold0.npz")))
        known = np.concatenate([d["X_train"], d["X_test"]]).astype(np.int64)
        q = np.resize(d["X_test"].astype(np.int64), (4096, 3))
        return 845, 4, 64, w, known, q, {}, ("fused", "layered", "predict")
    rng = np.random.default_rng(0)
    N, R = 100_000, 2
    D, Q = (64, 64) if name == "b" else (256, 32)
    pos, _ = synthetic_graph(N, R, 400_000, seed=3)
    q = pos[rng.choice(len(pos), Q, replace=False)]
    kw = {} if name == "b" else {"gemm": "bf16x3"}
    return N, R, D, smoke_params(N, R, D, rng), pos, q, kw, (("fused", "layered", "predict") if name == "b" else
                                                             ("layered", "predict"))


def timed(fn):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="a,b,c")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08", "screen_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    record = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "shapes": {}}
    for name in args.shapes.split(","):
        N, R, D, params, graph, q, kw, paths = shape(name)
        Q = len(q)
        eng = Engine(N, R, D, dev, **kw)
        P = FlatParams(N, R, D, dev)
        P.load(params)
        adj = eng.adjacency(get_adj_mats(graph, N, R))

        def predict():
            # what a user of predict has to do: every (h, r, c) on the host, then the scored-edge build and forward
            tri = np.stack([np.repeat(q[:, 0], N), np.repeat(q[:, 1], N), np.tile(np.arange(N), Q)], 1)
            return eng.predict(P, adj, eng.edges(tri)).cpu().numpy()

        run = {"fused": lambda: eng.rank_candidates(P, adj, q, fused=True),
               "layered": lambda: eng.rank_candidates(P, adj, q, fused=False),
               "predict": predict}
        times = {p: [] for p in paths}
        for p in paths:                  # warm-up of every path (workspaces, code objects)
            timed(run[p])
        for _ in range(args.rounds):
            for p in paths:
                times[p].append(timed(run[p])[0])
        rec = {"N": N, "R": R, "D": D, "Q": Q, "candidates": Q * N, "engine": kw, "paths": {}}
        for p in paths:
            t = np.array(times[p])
            rec["paths"][p] = {"median_ms": float(np.median(t)), "min_ms": float(t.min()), "max_ms": float(t.max()),
                               "candidates_per_s": Q * N / (float(np.median(t)) * 1e-3), "all_ms": t.tolist()}
        if "fused" in paths:
            f = eng.rank_candidates(P, adj, q, fused=True, return_scores=True)
            l = eng.rank_candidates(P, adj, q, fused=False, return_scores=True)
            rec["max_abs_fused_minus_layered"] = float((f["scores"] - l["scores"]).abs().max())
            # a rank is discontinuous: logits 1e-6 apart can order two near-tied candidates differently
            rec["queries_with_other_rank_counts"] = int(((f["greater"] != l["greater"]) |
                                                         (f["equal"] != l["equal"])).sum())
            rec["max_greater_difference"] = int((f["greater"] - l["greater"]).abs().max())
            rec["max_equal_difference"] = int((f["equal"] - l["equal"]).abs().max())
            fm, lm = rec["paths"]["fused"], rec["paths"]["layered"]
            rec["fused_beats_layered_by_more_than_its_spread"] = bool(
                lm["median_ms"] - fm["median_ms"] > lm["max_ms"] - lm["min_ms"])
            del f, l
        record["shapes"][name] = rec
        print(json.dumps({name: rec}), flush=True)
        del eng, P, adj
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(record, fh, indent=1)


if __name__ == "__main__":
    main()
