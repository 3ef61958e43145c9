"""Explanation ground truth on the GPU (ground_truth.GroundTruthIndex), timed on two sets:

  bundled    the bundled tables: 1,754 response triples, 16,179 + 1,173 similarity rows, every row of dc a query
  synth200k  a seeded synthetic set: 2*10^5 response triples over 10^5 nodes (half mutations, half drugs), 2
             relations, similarity degree about 32 on each side (every node in 16 random rows of its table as the
             first end, so in about 16 more as the second), every row of dc a query: about 2*10^8 probes

Per set: the table build (two similarity-list CSRs + the dc table: radix sorts) and the query (COUNT, scan, FILL and
the one copy of total / error flag to the host), each a host clock around work that ends in a device synchronise,
median and (min, max) over the rounds after one warm-up; the probes (sum over the queries of |SM| + |SD| +
|SD| |SM|, computed on the host from the list lengths) per second of the query time; and the device result's
equality with the CPU restatement (tests/ref_ground_truth.py) where that is run: the bundled set, whose wall time is
printed for scale, and the first 64 queries of the synthetic set.

usage: python tools/bench_ground_truth.py [rounds]     -> text, one block per set
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from iddgcn_amd import ground_truth as G  # noqa: E402
from tests import ref_ground_truth as ref  # noqa: E402


def synthetic(nodes=100_000, responses=200_000, degree=32, relations=2, seed=0):
    rng = np.random.default_rng(seed)
    nm = nodes // 2

    def sim(lo, hi, rel):
        a = np.repeat(np.arange(lo, hi), degree // 2)
        b = lo + (a - lo) // 2000 * 2000 + rng.integers(0, 2000, len(a))       # a partner in the node's block of 2,000
        return np.stack([a, np.full(len(a), rel), b], 1).astype(np.int64)
    # the responses fill the first block of mutations x the first block of drugs at 2.5 % per relation, and a
    # node's similar nodes are in its block: that share of the probes hits
    dc = np.stack([rng.integers(0, 2000, responses), rng.integers(0, relations, responses),
                   nm + rng.integers(0, 2000, responses)], 1).astype(np.int64)
    return dc, sim(0, nm, 3), sim(nm, nodes, 2)


def probes(index, queries):
    mu_len = np.diff(index.mu[0].cpu().numpy().astype(np.int64))[queries[:, 0]]
    drug_len = np.diff(index.drug[0].cpu().numpy().astype(np.int64))[queries[:, 2]]
    return int((mu_len + drug_len + mu_len * drug_len).sum()), int(mu_len.max()), int(drug_len.max())


def timed(fn, rounds):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return out, np.median(ts), min(ts), max(ts)


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    dev = torch.device("cuda", 0)
    print(f"device: {torch.cuda.get_device_name(0)}; rounds: {rounds} after one warm-up; times in ms: median (min, max)")
    for name, (dc, mu, drug), n_check in (("bundled", ref.bundled(), None), ("synth200k", synthetic(), 64)):
        tables = [torch.as_tensor(x, device=dev) for x in (dc, mu, drug)]
        index, tb, tb0, tb1 = timed(lambda: G.GroundTruthIndex(*tables, device=dev), rounds)
        (ptr, tri), tq, tq0, tq1 = timed(lambda: index.query(), rounds)
        n, lm, ld = probes(index, dc)
        print(f"\n{name}: {len(dc)} response triples / queries, {len(mu)} + {len(drug)} similarity rows, "
              f"N = {index.N}, R = {index.R}")
        print(f"  probes {n} (longest lists {lm} / {ld}), ground-truth triples {int(ptr[-1])}, "
              f"longest {int((ptr[1:] - ptr[:-1]).max())}")
        print(f"  table build {tb * 1e3:9.3f} ({tb0 * 1e3:.3f}, {tb1 * 1e3:.3f})")
        print(f"  query       {tq * 1e3:9.3f} ({tq0 * 1e3:.3f}, {tq1 * 1e3:.3f})   {n / tq / 1e9:.3f} G probes/s")
        q = dc if n_check is None else dc[:n_check]
        t0 = time.perf_counter()
        rptr, rtri = ref.as_csr(ref.ground_truth(dc, mu, drug, q))
        t_cpu = time.perf_counter() - t0
        p, t = ptr.cpu().numpy(), tri.cpu().numpy()
        same = np.array_equal(p[:len(q) + 1], rptr) and np.array_equal(t[:rptr[-1]], rtri)
        print(f"  CPU restatement (dict lookups, one thread), {len(q)} queries: {t_cpu * 1e3:.1f} ms; "
              f"device result equal: {same}")
        if not same:
            sys.exit(1)


if __name__ == "__main__":
    main()
