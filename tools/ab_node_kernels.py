"""Kernel A/B of the node-level work of a config-3 step against a library built from another commit (the parent), on the
step's real buffers (the engine built as bench.py builds it, one training step first), the two libraries alternated
inside one process (`rounds` rounds; per library the first launch after the switch is reported apart from the `reps`
warm launches, each timed with HIP events):

  pair l    tail_seg_reduce + head_bwd_node (other library)  vs  tail_seg_reduce_head + head_dz (this one), layer l
            (l = 2: no dsum; l = 0: with dsum); dP, dsum, dWedge compared bitwise, dz by max|diff| / max|dz|
  tail l / head l   the two halves of the pair on their own
  head_dz   the other library's head_dz (8 lanes per node, serial segment walk) vs this one's R <= 2 form
  alpha, narrow, gather   the same call in both libraries; outputs compared bitwise

A piece is ahead when every warm launch of this library is below every warm launch of the other.  Then whole training
steps of this library with Engine.fuse_tail_head on and off, alternated.

usage: python tools/ab_node_kernels.py other/libiddgcn_hip.so [--config 3] [--reps 5] [--rounds 3]
"""
import argparse
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from bench import CONFIGS, reference_init  # noqa: E402
from iddgcn_amd import _lib as L  # noqa: E402
from iddgcn_amd import ops  # noqa: E402
from iddgcn_amd.engine import Engine, FlatParams, KerasAdam  # noqa: E402
from iddgcn_amd.graph import get_adj_mats  # noqa: E402
from iddgcn_amd.sampling import negative_samples  # noqa: E402
from iddgcn_amd.utils import synthetic_graph  # noqa: E402
from tools.bench_mem import load_lenient  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("other")
    ap.add_argument("--config", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    cfg = CONFIGS[a.config]
    N, R, D, M = cfg["N"], cfg["R"], cfg["D"], cfg["M"]
    dev = torch.device("cuda", 0)
    pos, neg0 = synthetic_graph(N, R, M, seed=0)
    neg = negative_samples(pos[::cfg["neg_every"]], N, 89, device=dev) if "neg_every" in cfg else neg0
    tri = np.concatenate([pos, neg])
    lab = np.concatenate([np.ones(len(pos), np.float32), np.zeros(len(neg), np.float32)])
    T = len(tri)
    eng = Engine(N, R, D, dev, gemm=cfg.get("gemm", "bf16x3"), features=cfg.get("features", "f32"))
    adj = get_adj_mats(pos, N, R, device=dev)
    ed = eng.edges(tri, lab)
    del pos, neg, tri, lab
    P, G = FlatParams(N, R, D, dev), FlatParams(N, R, D, dev)
    P.load(reference_init(np, N, R, D, 89))
    opt = KerasAdam(P)
    eng.train_step(P, G, opt, adj, ed, t_global=T)
    torch.cuda.synchronize()
    ws = eng.workspace(ed.T, True)
    this, other = L.lib(), load_lenient(a.other)
    print(f"config {a.config}: N {N} R {R} D {D} T {T}; other library {a.other} (ABI {other.iddgcn_abi_version()}), "
          f"this ABI {this.iddgcn_abi_version()}", flush=True)
    hd = ws.dOn_a
    e = lambda *s: torch.empty(*s, device=dev)          # noqa: E731
    dz_o, dz_n, S_t, W_t, We_t, dWa_t, dba_t = e(N, R), e(N, R), e(N, R), e(N, R), e(ed.T, R), e(D, R), e(R)

    def tail_plain(l):
        ops.tail_seg_reduce(ed.tptr, None, ws.Wedge[l], ws.xt[l], ws.P[l], ws.dP, ws.dWedge,
                            dsum=ws.dES if l == 0 else None)

    def head_plain(l):
        ops.head_bwd_node(hd, ws.P[l], ws.Ssm[l], ws.W[l], ws.dP, dz_o, hseg_ptr=ed.hptr, hperm=ed.hperm,
                          dWedge=ws.dWedge, dsum=ws.dES if l == 0 else None)

    def tail_head(l):
        ops.tail_seg_reduce_head(ed.tptr, ws.Wedge[l], ws.xt[l], ws.P[l], ws.dP, ws.dWedge, hd, ws.W[l], ws.dwh,
                                 dsum=ws.dES if l == 0 else None)

    def head_dz(l, out=None):
        ops.head_dz(ws.Ssm[l], ws.W[l], ed.hptr, ed.hperm, ws.dWedge, ws.dwh, dz_n if out is None else out)

    def both(f, g):
        return lambda: (f(), g())
    same = lambda: ops.alpha_fwd(ws.X[1], P["Wa3"], P["ba3"], S_t, W_t)     # noqa: E731
    narrow = lambda: ops.gemm_tn_narrow(ws.X[1], ws.dz, dWa_t, dba_t, ws.narrow_slab)   # noqa: E731
    gather = lambda: ops.gather_rows(ws.W[2], ed.h, We_t)                   # noqa: E731
    # name -> (call under the other library, call under this one, outputs to compare: (name, tensor fn, bitwise))
    pieces = {}
    for l in (2, 0):
        outs = [("dP", lambda: ws.dP, True), ("dWedge", lambda: ws.dWedge, True)]
        if l == 0:
            outs.append(("dsum", lambda: ws.dES, True))
        pieces[f"pair l={l}"] = (both(lambda l=l: tail_plain(l), lambda l=l: head_plain(l)),
                                 both(lambda l=l: tail_head(l), lambda l=l: head_dz(l)),
                                 outs + [("dz", None, False)])
        pieces[f"tail l={l}"] = (lambda l=l: tail_plain(l), lambda l=l: tail_head(l), [])
        pieces[f"head l={l}"] = (lambda l=l: head_plain(l), lambda l=l: head_dz(l), [])
    pieces["head_dz form"] = (lambda: head_dz(2, dz_o), lambda: head_dz(2), [("dz", None, False)])
    pieces["alpha"] = (same, same, [("S", lambda: S_t, True), ("W", lambda: W_t, True)])
    pieces["narrow"] = (narrow, narrow, [("dWa", lambda: dWa_t, True), ("dba", lambda: dba_t, True),
                                         ("slab", lambda: ws.narrow_slab, True)])
    pieces["gather w=2"] = (gather, gather, [("Wedge", lambda: We_t, True)])

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) * 1e3

    verdicts = {}
    for name, (f_other, f_this, outs) in pieces.items():
        warm = {"other": [], "this": []}
        kept = {}
        for rnd in range(a.rounds):
            for side, lib, fn in (("other", other, f_other), ("this", this, f_this)):
                L._lib = lib
                first = timed(fn)
                ts = [timed(fn) for _ in range(a.reps)]
                warm[side] += ts
                print(f"{name:14s} round {rnd} {side:5s} first {first:8.1f} us  warm " +
                      " ".join(f"{t:7.1f}" for t in ts), flush=True)
                if rnd == 0 and side == "other":    # (a pair starts from the tail kernel's fresh dP / dsum every launch)
                    for nm, get, _ in outs:
                        kept[nm] = (dz_o if get is None else get()).clone()
        L._lib = this
        for nm, get, bitwise in outs:
            got = dz_n if get is None else get()
            ref = kept[nm]
            if bitwise:
                print(f"{name:14s} {nm}: bitwise equal = {torch.equal(ref, got)}", flush=True)
            else:
                print(f"{name:14s} {nm}: max|diff| / max|ref| = "
                      f"{((ref.double() - got.double()).abs().max() / ref.double().abs().max()).item():.3e}", flush=True)
        kept.clear()
        ahead = max(warm["this"]) < min(warm["other"])
        verdicts[name] = (np.median(warm["other"]), np.median(warm["this"]), ahead)
        print(f"{name:14s} median other {verdicts[name][0]:8.1f} us, this {verdicts[name][1]:8.1f} us; every warm launch "
              f"of this library below every one of the other: {ahead}", flush=True)
    print("\npiece           other us   this us  ahead")
    for name, (o, t, ahead) in verdicts.items():
        print(f"{name:14s} {o:9.1f} {t:9.1f}  {ahead}")
    L._lib = this
    times = {True: [], False: []}
    for rnd in range(a.rounds):
        for val in (True, False):
            eng.fuse_tail_head = val
            eng.train_step(P, G, opt, adj, ed, t_global=T)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.reps):
                eng.train_step(P, G, opt, adj, ed, t_global=T)
            torch.cuda.synchronize()
            times[val].append((time.perf_counter() - t0) / a.reps * 1e3)
            print(f"round {rnd} step fuse_tail_head={val}: {times[val][-1]:.3f} ms/step", flush=True)
    for val in (True, False):
        print(f"fuse_tail_head={val}: median {np.median(times[val]):.3f} ms/step", flush=True)


if __name__ == "__main__":
    main()
