"""What held-out metrics cost inside fit() at the reference's size (fold 0: 845 nodes, D = 64, R = 4, HIP-graph
replay), per epoch, in three forms on one machine in one run:
  none    fit without validation;
  device  fit(validation_data=..., validation_freq=1): the second captured graph (forward + iddgcn_clf_metrics);
  host    a callback that runs predict, copies the probabilities back and calls classification_metrics each epoch.
Each figure is (t(warm + epochs) - t(warm)) / epochs of whole fit() calls, so graph capture and the first eager
epoch cancel; median of ``repeats``.  Also the general path of iddgcn_clf_metrics at n = 4e6 against torch.sort of
the same 64-bit keys.  Writes profiles/r14/validation.json.
usage: python tools/ab_validation.py [--epochs 200] [--warm 20] [--repeats 5] [--out profiles/r14/validation.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from iddgcn_amd import classification_metrics, get_adj_mats, get_IDDGCN_Model, ops  # noqa: E402
from iddgcn_amd.model import Callback  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ENT, N_REL = 845, 4


class HostRoute(Callback):
    def __init__(self, x_val, y_val):
        self.x_val, self.y_val, self.last = x_val, y_val, None

    def on_epoch_end(self, epoch, logs=None):
        self.last = classification_metrics(self.y_val, self.model.predict(self.x_val)[0])


def fit_seconds(d, x, x_val, y_val, form, epochs):
    model = get_IDDGCN_Model(N_ENT, N_REL, 64, 64, 7, None, 0, 0)
    model.neg_triples = d["X_train_neg"][None]
    kw = {}
    if form == "device":
        kw = dict(validation_data=(x_val, y_val))
    elif form == "host":
        kw = dict(callbacks=[HostRoute(x_val, y_val)])
    model.fit(x, None, epochs=2, verbose=0, **kw)          # library, allocator and adjacency cache warm
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    model.fit(x, None, epochs=epochs, verbose=0, **kw)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def general_path(n, repeats):
    rng = np.random.default_rng(0)
    dev = torch.device("cuda", 0)
    p = torch.as_tensor(rng.random(n).astype(np.float32), device=dev)
    y = torch.as_tensor((rng.random(n) < 0.5).astype(np.float32), device=dev)
    keys = (p.view(torch.int32).to(torch.int64) << 2) | y.to(torch.int64)
    counts = torch.empty((1, 9), dtype=torch.int64, device=dev)
    values = torch.empty((1, 8), dtype=torch.float64, device=dev)
    ws = ops.clf_metrics_workspace(n, 0, dev)

    def timed(fn):
        fn()
        out = []
        for _ in range(repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            out.append(a.elapsed_time(b))
        return statistics.median(out)

    return {"n": n, "clf_metrics_ms": timed(lambda: ops.clf_metrics(p, y, None, 0, 0.5, counts, values, ws)),
            "torch_sort_int64_ms": timed(lambda: torch.sort(keys))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=200)
    ap.add_argument("--warm", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--n-general", type=int, default=4 * 10 ** 6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14", "validation.json"))
    a = ap.parse_args()
    d = dict(np.load(os.path.join(ROOT, "tests", "golden", "fold0_data.npz")))
    X = d["X_train"][None]
    ids = np.arange(N_ENT)[None]
    x = [ids, X[:, :, 0], X[:, :, 1], X[:, :, 2], get_adj_mats(d["X_train"], N_ENT, N_REL)]
    Xt = np.concatenate([d["X_test"], d["neg_X_test"]])[None]
    x_val = [ids, Xt[:, :, 0], Xt[:, :, 1], Xt[:, :, 2],
             get_adj_mats(np.concatenate([d["X_train"], d["X_test"]]), N_ENT, N_REL)]
    y_val = np.r_[np.ones(len(d["X_test"])), np.zeros(len(d["neg_X_test"]))]
    res = {"epochs": a.epochs, "warm": a.warm, "repeats": a.repeats, "n_val": int(len(y_val)),
           "device": torch.cuda.get_device_name(0), "ms_per_epoch": {}}
    samples = {f: [] for f in ("none", "device", "host")}
    for _ in range(a.repeats):                              # round-robin: drift hits every form alike
        for form in samples:
            t_w = fit_seconds(d, x, x_val, y_val, form, a.warm)
            t_f = fit_seconds(d, x, x_val, y_val, form, a.warm + a.epochs)
            samples[form].append(1e3 * (t_f - t_w) / a.epochs)
    for form, s in samples.items():
        res["ms_per_epoch"][form] = {"median": statistics.median(s), "min": min(s), "max": max(s)}
    m = res["ms_per_epoch"]
    res["validation_cost_ms"] = {"device": m["device"]["median"] - m["none"]["median"],
                                 "host": m["host"]["median"] - m["none"]["median"]}
    res["general_path"] = general_path(a.n_general, a.repeats)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
