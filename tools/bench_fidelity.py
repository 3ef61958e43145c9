"""Deletion / insertion curves (explain.fidelity_curves): the fused kernel next to the per-variant route
(DeviceAdjacency.set_values + Engine.predict for every variant), in one process, alternating between the two, on fold 4
with the bundled weights, the reference's 288 test triples and explaiNE's bundled explanations (N = 845, R = 4,
D = 64, K = 10: 22 variants per triple).

Every timed region is a whole call (adjacency build, curve_steps, launches, copy to numpy) between two device events
and ends in a synchronise.  Per route: median and spread (min, max) over the rounds after one warm-up call of each.
The fused route's own split: device-event time around its launches alone against the whole call.  Acceptance: the
fused call's slowest round is faster than the per-variant route's fastest round (``accepted``).  The kernel's
registers and LDS come from the built library's code-object metadata (tools/kernel_regs.py); its occupancy follows
from them (one 256-thread workgroup per CU when the LDS block is above half of the CU's 160 KiB).

usage: python tools/bench_fidelity.py [rounds] [triples] [out.json]   -> one JSON line, also written to out.json
       (default profiles/r15/fidelity.json)
"""
import json
import os
import re
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from iddgcn_amd import explain as X  # noqa: E402
from iddgcn_amd import get_IDDGCN_Model  # noqa: E402
from tools import kernel_regs  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def summary(ms, Q):
    ms = np.asarray(ms)
    return {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max()),
            "median_us_per_triple": float(np.median(ms)) / Q * 1e3}


def kernel_resources():
    """{kernel: {vgpr, agpr, spills, scratch, lds_bytes, workgroups_per_cu}} of the curves kernels."""
    out = {}
    try:
        text = kernel_regs.notes(kernel_regs.LIB)
    except (OSError, FileNotFoundError) as e:          # no ROCm llvm tools beside the library
        return {"error": str(e)}
    for item in re.split(r"\n\s+- \.agpr_count", text):
        m = re.search(r"\.name:\s*(\S+)", item)
        if not m or m.group(1).endswith(".kd") or "curves_kernel" not in m.group(1):
            continue
        v = {k: int((re.search(re.escape(k) + r":\s*(\d+)", ".agpr_count" + item) or [None, "-1"])[1])
             for k in kernel_regs.KEYS}
        lds = v[".group_segment_fixed_size"]
        regs = v[".vgpr_count"]                        # the unified file: architectural VGPRs + AGPRs
        by_lds = (160 * 1024) // lds
        by_regs = 512 // max(regs, 1)                  # waves per SIMD; a 256-thread workgroup is one wave on each
        out[m.group(1)] = {"vgpr_total": regs, "agpr": v[".agpr_count"], "spills": v[".vgpr_spill_count"],
                           "scratch_bytes": v[".private_segment_fixed_size"], "lds_bytes": lds,
                           "workgroups_per_cu": min(by_lds, by_regs), "waves_per_simd": min(by_lds, by_regs)}
    return out


def main(rounds=5, n_triples=None, out_path=None):
    g = lambda n: dict(np.load(os.path.join(ROOT, "tests", "golden", n)))  # noqa: E731
    d, ex = g("fold4_data.npz"), g("explain_fold4.npz")
    test = ex["test_triples"].astype(np.int64)[:n_triples]
    preds = ex["explaine_preds"][:n_triples]
    adjacency = np.concatenate([d["X_train"].astype(np.int64), ex["test_triples"].astype(np.int64)])
    model = get_IDDGCN_Model(845, 4, 64, 64, 123, None, 0, 4)
    model.load_weights(os.path.join(ROOT, "tests", "golden", "weights_fold4.npz"))
    Q, K = len(test), preds.shape[1]
    stats = {}
    base = lambda: X.fidelity_curves(model, adjacency, test, preds, fused=False)  # noqa: E731
    new = lambda: X.fidelity_curves(model, adjacency, test, preds, fused=True, stats=stats)  # noqa: E731
    ref, ours = base(), new()                           # warm-up: device state, workspaces, allocator pools
    tb, tn, dev_ms = [], [], []
    for _ in range(rounds):                             # alternate the two routes
        tb.append(timed(base)[0])
        tn.append(timed(new)[0])
        a, b = stats["launch_events"]
        dev_ms.append(a.elapsed_time(b))
    b, n = summary(tb, Q), summary(tn, Q)
    s = X.fidelity_summary(ours)
    res = {"rounds": rounds, "Q": Q, "K": K, "variants_per_triple": 2 * (K + 1), "candidates": stats["candidates"],
           "per_variant": b, "fused": n, "speedup_median": b["median_ms"] / n["median_ms"],
           "fused_launches_device_ms": summary(dev_ms, Q),
           "fused_host_ms_median": n["median_ms"] - float(np.median(dev_ms)),
           "max_abs_difference": float(max(np.abs(ours[k] - ref[k]).max() for k in ("deletion", "insertion"))),
           "accepted": n["max_ms"] < b["min_ms"],
           "kernel": kernel_resources(),
           "explaine": dict(s["mean"], effective_share=s["effective_share"]),
           "config": {"device": torch.cuda.get_device_name(0),
                      "timed": "whole call incl. adjacency build, curve_steps and copy to numpy, device events"}}
    line = json.dumps(res)
    print(line, flush=True)
    out_path = out_path or os.path.join(ROOT, "profiles", "r15", "fidelity.json")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    a = sys.argv[1:]
    main(int(a[0]) if a else 5, int(a[1]) if len(a) > 1 and a[1] != "all" else None, a[2] if len(a) > 2 else None)
