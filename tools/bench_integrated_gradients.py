"""Integrated-gradients edge attributions (explain.integrated_gradients_batched) on fold 4 with the bundled weights:
the reference's 288 test triples, Gauss-Legendre with 256 nodes (N = 845, R = 4, D = 64).  Two routes in one process,
alternating round by round:

(a) the new call (fused kernels), split into its launches (device events around them) and the host work around them;
(b) the best route the earlier API allows, valid when every candidate is eligible: per node one ``set_values`` that
    scales every row that is a head or a tail of some triple, one ``Engine.value_grads_batch``, and the weighted sum
    kept on the device; Engine.predict for the two end points.

Every timed region is a whole call between two device events and ends in a synchronise; per route the median and
spread over the rounds after one warm-up call of each.  Beside the timings: the completeness gap at 64, 128 and 256
nodes for both rules, and the fidelity of the top-10 lists next to explaiNE's, occlusion's and random edges' of the
same rows.

usage: python tools/bench_integrated_gradients.py [rounds] [triples] [out.json]   -> one JSON line, also written to
       out.json (default profiles/r18/integrated_gradients.json)
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

K, STEPS = 10, 256


def parent_route(model, adjacency, test, N, R, alpha, omega):
    """Route (b).  Returns a dict of host arrays: attr in value_grads_batch's candidate order with its qptr / entry,
    total, p, p_baseline, gap."""
    eng, params = X._model_state(model)
    dadj = DeviceAdjacency(get_adj_mats(adjacency, N, R), N, eng.device)
    base = dadj.base_values.to(torch.float32)
    row = torch.as_tensor(X._entry_table(dadj, real=False)[0], device=eng.device)
    nodes = torch.as_tensor(np.unique(test[:, [0, 2]]), device=eng.device)
    on_path = torch.isin(row, nodes)
    ed = eng.edges(test)
    ends = []
    for a in (0.0, 1.0):
        dadj.set_values(torch.where(on_path, base * a, base))
        ends.append(eng.predict(params, dadj, ed).clone())
    acc = None
    for a, w in zip(alpha.astype(np.float32), omega.astype(np.float32)):
        dadj.set_values(torch.where(on_path, base * float(a), base))
        out = eng.value_grads_batch(params, dadj, test)
        acc = out["grad"] * float(w) if acc is None else acc + out["grad"] * float(w)
    dadj.set_values(base)
    attr = acc * base[out["entry"].long()]
    lens = out["qptr"][1:] - out["qptr"][:-1]
    q_of = torch.repeat_interleave(torch.arange(len(test), device=eng.device), lens)
    total = torch.zeros(len(test), dtype=torch.float32, device=eng.device).index_add_(0, q_of, attr)
    gap = total - (ends[1] - ends[0])
    return {k: v.cpu().numpy() for k, v in dict(attr=attr, qptr=out["qptr"], entry=out["entry"], total=total,
                                                 p=ends[1], p_baseline=ends[0], gap=gap).items()}


def gap_stats(gap):
    g = np.abs(np.asarray(gap, np.float64))
    return {"max": float(g.max()), "median": float(np.median(g)), "mean": float(g.mean()),
            "share_within_1e-3": float((g <= 1e-3).mean())}


def main(rounds=5, n_triples=None, out_path=None):
    g = lambda n: dict(np.load(os.path.join(ROOT, "tests", "golden", n)))  # noqa: E731
    d, ex = g("fold4_data.npz"), g("explain_fold4.npz")
    N, R = 845, 4
    test = ex["test_triples"].astype(np.int64)[:n_triples]
    adjacency = np.concatenate([d["X_train"].astype(np.int64), ex["test_triples"].astype(np.int64)])
    model = get_IDDGCN_Model(N, R, 64, 64, 123, None, 0, 4)
    model.load_weights(os.path.join(ROOT, "tests", "golden", "weights_fold4.npz"))
    Q = len(test)
    rule = X.quadrature_rule(STEPS, "gauss")
    stats = {}
    new = lambda: X.integrated_gradients_batched(model, adjacency, test, K, steps=STEPS, stats=stats,  # noqa: E731
                                                 return_attributions=True)
    old = lambda: parent_route(model, adjacency, test, N, R, *rule)  # noqa: E731
    ours, theirs = new(), old()                             # warm-up: device state, workspaces, allocator pools
    ta, tb, dev_ms = [], [], []
    for _ in range(rounds):                                 # the two routes alternate
        ta.append(timed(new)[0])
        a, b = stats["launch_events"]
        dev_ms.append(a.elapsed_time(b))
        tb.append(timed(old)[0])
    # the two routes against each other: per triple, the attributions matched by entry id
    host = DeviceAdjacency(get_adj_mats(adjacency, N, R), N, "cpu")
    cand = X.counterfactual_candidates(host, test)
    mine = np.concatenate(ours["attributions"][1])
    worst = 0.0
    for j in range(Q):
        e = theirs["entry"][theirs["qptr"][j]:theirs["qptr"][j + 1]]
        v = theirs["attr"][theirs["qptr"][j]:theirs["qptr"][j + 1]]
        sl = slice(cand["qptr"][j], cand["qptr"][j + 1])
        at = np.searchsorted(np.sort(e), cand["entry"][sl])
        worst = max(worst, float(np.abs(v[np.argsort(e, kind="stable")][at] - mine[sl]).max()) if sl.stop > sl.start
                    else 0.0)
    gaps = {}
    for name in ("gauss", "midpoint"):
        for m in (64, 128, 256):
            r = X.integrated_gradients_batched(model, adjacency, test, K, steps=m, quadrature=name)
            gaps[f"{name}_{m}"] = gap_stats(r["gap"])
    pad = lambda preds: [p if len(p) else np.full((1, 3), -1, np.int64) for p in preds]  # noqa: E731
    lists = {"integrated_gradients": ours["edges"],
             "integrated_gradients_toward_lower": X.integrated_gradients_batched(model, adjacency, test, K, steps=STEPS,
                                                                                 toward="lower")["edges"],
             "occlusion": X.occlusion_batched(model, adjacency, test, K)[0],
             "explaine": list(ex["explaine_preds"][:n_triples]),
             "random": X.random_explanations(host, test, K, seed=0)}
    fidelity = {}
    for name, preds in lists.items():
        fs = X.fidelity_summary(X.fidelity_curves(model, adjacency, test, pad(preds)))
        fidelity[name] = dict(fs["mean"], effective_share=fs["effective_share"])
    sa, sb = summary(ta, Q), summary(tb, Q)
    s = X.integrated_gradients_summary(ours)
    res = {"rounds": rounds, "Q": Q, "steps": STEPS, "quadrature": "gauss", "top_k": K,
           "candidates": stats["candidates"], "launches": 2,
           "fused": sa, "fused_launches_device_ms": summary(dev_ms, Q),
           "fused_host_ms_median": sa["median_ms"] - float(np.median(dev_ms)),
           "parent_route": sb, "parent_route_launch_rounds": STEPS + 2,
           "speedup_over_parent_route": sb["median_ms"] / sa["median_ms"],
           "max_abs_attr_difference_between_routes": worst,
           "max_abs_attr": float(np.abs(mine).max()),
           "gap": {"fused": gap_stats(ours["gap"]), "parent_route": gap_stats(theirs["gap"]), "by_rule": gaps},
           "findings": dict(s, relation_share={str(k): v for k, v in s["relation_share"].items()},
                            fidelity=fidelity),
           "config": {"device": torch.cuda.get_device_name(0),
                      "timed": "whole call incl. adjacency build, candidate lists and copy to numpy, device events"}}
    line = json.dumps(res)
    print(line, flush=True)
    out_path = out_path or os.path.join(ROOT, "profiles", "r18", "integrated_gradients.json")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    a = sys.argv[1:]
    main(int(a[0]) if a else 5, int(a[1]) if len(a) > 1 and a[1] != "all" else None, a[2] if len(a) > 2 else None)
