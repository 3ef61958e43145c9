"""Launch-trace A/B of Engine against another engine.py (the parent commit's): do the two issue the same launches?

One engine is built from each module, in one process, on the same parameters, gradients, optimizer state, adjacency,
scored edges and workspaces.  Every ``ops`` function the engine calls, the shard / comm objects' methods, the side
stream's fork and join and ``Engine._mark`` are wrapped: the wrapper records the call, then runs it.  A call is recorded
as the callee sees it (arguments bound to its signature, defaults filled in); a tensor as (buffer, shape, stride,
dtype), the buffer being its address where it lies in one of the shared buffers and, for a temporary, the rank of its
storage in order of first appearance; containers recursively, scalars as they are.  Each case runs other, this, other:
other against other shows the trace is deterministic, other against this must be equal element for element, and the
outputs (ws.p, ws.s, the gradient and parameter buffers, ranking and value_grads results) bitwise equal.  The first
differing call is printed.

The sharded cases use recording stand-ins with parallel.NodeShard's / RelationShard's / BucketedAllReduce's interface
(no process group) and are record-only: the launches are recorded, not run (their numbers would be meaningless).
``--record-only`` does that for every case; without a GPU it runs on CPU tensors (the side-stream cases left out).

usage: git show HEAD~1:iddgcn_amd/engine.py > /tmp/engine_parent.py
       python tools/engine_trace_ab.py --parent-engine /tmp/engine_parent.py [--record-only] [--case SUBSTRING]
"""
import argparse
import contextlib
import importlib.util
import inspect
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from iddgcn_amd import engine as this_engine  # noqa: E402
from iddgcn_amd import ops  # noqa: E402
from iddgcn_amd.graph import DeviceAdjacency, ScoredEdges, get_adj_mats  # noqa: E402
from iddgcn_amd.utils import synthetic_graph  # noqa: E402

OPS = ("spmm_csr sddmm_csr rowgemm rowgemm_batched gemm_tn sigma_tn gemm_tn_batched gemm_tn_narrow alpha_fwd combine "
       "distmult_bce distmult_bce_heads tail_seg_reduce tail_seg_reduce_head head_dz head_bwd_node head_wsum gather_rows "
       "reduce_slabs adam screen_chain rank_topk explain_seeds explain_row_grads").split()


class Recorder:
    def __init__(self, cuda):
        self.trace, self.execute, self.cuda = None, True, cuda
        self.shared = set()         # storage addresses of the buffers both engines share
        self.main = torch.cuda.current_stream().cuda_stream if cuda else None

    def share(self, *objs):
        """Note every tensor held by ``objs`` (attributes, one container level deep) as a shared buffer."""
        for o in objs:
            vals = list(vars(o).values()) if hasattr(o, "__dict__") else [o]
            for v in vals:
                for t in (v.values() if isinstance(v, dict) else v if isinstance(v, (list, tuple)) else [v]):
                    for u in (t if isinstance(t, (list, tuple)) else [t]):
                        if isinstance(u, torch.Tensor):
                            self.shared.add(u.untyped_storage().data_ptr())

    def desc(self, x):
        if isinstance(x, torch.Tensor):
            base = x.untyped_storage().data_ptr()
            if base in self.shared:
                buf = x.data_ptr()
            else:
                if base not in self.tmp:        # held until the trace ends, so that no later temporary takes its address
                    self.tmp[base] = len(self.tmp)
                    self.held.append(x)
                buf = ("tmp", self.tmp[base], x.data_ptr() - base)
            return (buf, tuple(x.shape), tuple(x.stride()), str(x.dtype))
        if isinstance(x, (list, tuple)):
            return tuple(self.desc(v) for v in x)
        if isinstance(x, dict):
            return tuple((k, self.desc(v)) for k, v in sorted(x.items()))
        if isinstance(x, (np.floating, np.integer)):
            return x.item()
        return x if isinstance(x, (int, float, str, bool, type(None))) else type(x).__name__

    def start(self):
        self.trace, self.tmp, self.held = [], {}, []

    def add(self, name, args):
        if self.trace is not None:
            side = self.cuda and torch.cuda.current_stream().cuda_stream != self.main
            self.trace.append((name, side, self.desc(args)))


def bound(sig, args, kw):
    b = sig.bind(*args, **kw)
    b.apply_defaults()
    return dict(b.arguments)


def wrap_ops(rec):
    """Replace the ``ops`` functions the engine calls (both engine modules import the one ``ops``)."""
    rg = inspect.signature(ops._rowgemm_args)
    for name in OPS:
        fn = getattr(ops, name)
        sig = rg if name == "rowgemm" else inspect.signature(fn)

        def wrapper(*args, _fn=fn, _sig=sig, _name=name, **kw):
            if _name == "rowgemm_batched":
                rec.add(_name, [bound(rg, c[:3], c[3]) for c in args[0]])
            else:
                rec.add(_name, bound(_sig, args, kw))
            if rec.execute:
                return _fn(*args, **kw)
        setattr(ops, name, wrapper)
    if rec.cuda:
        wait = torch.cuda.Stream.wait_stream

        def wait_stream(self, other):
            rec.add("wait_stream", [self.cuda_stream != rec.main, other.cuda_stream != rec.main])
            return wait(self, other)
        torch.cuda.Stream.wait_stream = wait_stream


def wrap_mark(rec, mod):
    mark = mod.Engine._mark

    @contextlib.contextmanager
    def _mark(self, name):
        rec.add("mark", ["enter", name])
        with mark(self, name):
            yield
        rec.add("mark", ["exit", name])
    mod.Engine._mark = _mark


class _Done:
    def wait(self):
        pass


class RowShard:
    """parallel.NodeShard's interface; the collectives record and return a completed handle."""

    def __init__(self, rec, cuts, rank, owner_e, device):
        self.rec, self.cuts, self.rank, self.world, self.owner_e = rec, list(cuts), rank, len(cuts) - 1, owner_e
        self.N, self.a, self.b = cuts[-1], cuts[rank], cuts[rank + 1]
        self._idx = torch.arange(self.a, self.b, dtype=torch.int32, device=device)
        self._ptr = torch.arange(0, self.b - self.a + 1, dtype=torch.int32, device=device)

    def owned_idx(self, device):
        return self._idx

    def owned_ptr(self, device):
        return self._ptr

    def all_gather(self, table, async_op=False):
        self.rec.add("row.all_gather", [table, async_op])
        return _Done()

    def reduce_scatter(self, table, async_op=False):
        self.rec.add("row.reduce_scatter", [table, async_op])
        return _Done()

    def broadcast_rows(self, table):
        self.rec.add("row.broadcast_rows", [table])
        return {k: _Done() for k in range(self.world)}

    def reduce_rows(self, table, k):
        self.rec.add("row.reduce_rows", [table, k])
        return _Done()


class RelShard:
    """parallel.RelationShard's interface (flat (relation, node) rows [a, b) of rank ``rank`` of ``world``)."""

    def __init__(self, rec, R, N, rank, world):
        self.rec, self.R, self.N = rec, R, N
        chunk = -(-R * N // world)
        self.a = min(R * N, rank * chunk)
        self.b = min(R * N, self.a + chunk)

    def pieces(self):
        out = [(r, max(self.a, r * self.N) - r * self.N, min(self.b, (r + 1) * self.N) - r * self.N)
               for r in range(self.R)]
        return [p for p in out if p[2] > p[1]]

    def all_gather(self, table):
        self.rec.add("rel.all_gather", [table])

    def reduce_scatter(self, table):
        self.rec.add("rel.reduce_scatter", [table])


class Comm:
    """parallel.BucketedAllReduce's interface: two row chunks, the buckets handed back in order."""

    def __init__(self, rec):
        self.rec, self.views = rec, []

    def row_chunks(self, n):
        return [(0, n // 2), (n // 2, n)]

    def ready(self, view):
        self.rec.add("comm.ready", [view])
        self.views.append(view)

    def finish_each(self, fn):
        views, self.views = self.views, []
        self.rec.add("comm.finish", [len(views)])
        for v in views:
            if fn is not None:
                fn(v)

    def finish(self):
        self.finish_each(None)


def load_engine(path):
    spec = importlib.util.spec_from_file_location("iddgcn_amd._engine_other", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def smoke_params(N, R, D, rng):
    p = {"E": rng.standard_normal((N, D)) / 8, "rel": rng.standard_normal((R, D))}
    for l in (1, 2, 3):
        p.update({f"K{l}": rng.standard_normal((R, D, D)) / D, f"S{l}": rng.standard_normal((D, D)) / 8,
                  f"Wa{l}": rng.standard_normal((D, R)) / 8, f"ba{l}": np.zeros(R)})
    return {k: v.astype(np.float32) for k, v in p.items()}


def first_difference(a, b):
    """(index, call of a, call of b) of the first call that differs ("(end)" past a trace's end), or None."""
    for i in range(max(len(a), len(b))):
        x, y = (a[i] if i < len(a) else "(end)"), (b[i] if i < len(b) else "(end)")
        if x != y:
            return i, x, y
    return None


def drop_marks(trace, names):
    return [c for c in trace if not (c[0] == "mark" and c[2][1] in names)]


class Case:
    """One engine shape and mode, with the steps to trace: (label, flags, fn(eng, c) -> {name: tensor})."""

    def __init__(self, rec, dev, name, N, R, D, steps, shard=None, execute=True, full_edges=False, **kw):
        self.rec, self.dev, self.name, self.steps, self.shard, self.kw = rec, dev, name, steps, shard, kw
        self.execute = execute and shard is None
        self.N, self.R, self.D = N, R, D
        pos, neg = synthetic_graph(N, R, 2000, seed=1)
        tri = np.concatenate([pos, neg])
        lab = np.concatenate([np.ones(len(pos), np.float32), np.zeros(len(neg), np.float32)])
        self.T = len(tri)
        rows = getattr(shard.get("row_shard"), "a", None) if shard else None
        if rows is not None and not full_edges:     # a node-partitioned rank's edges: those whose tail it owns
            sh = shard["row_shard"]
            keep = (tri[:, 2] >= sh.a) & (tri[:, 2] < sh.b)
            tri, lab = tri[keep], lab[keep]
        self.adj = DeviceAdjacency(get_adj_mats(pos, N, R), N, dev)
        self.ed = ScoredEdges(tri, lab, N, R, dev)
        self.queries = pos[:7]
        self.init = smoke_params(N, R, D, np.random.default_rng(5))
        self.P, self.G = this_engine.FlatParams(N, R, D, dev), this_engine.FlatParams(N, R, D, dev)
        self.opt = this_engine.KerasAdam(self.P)
        self.ws = {}

    def engine(self, mod):
        eng = mod.Engine(self.N, self.R, self.D, "cuda", **self.kw)
        eng.device = self.dev
        for k, v in (self.shard or {}).items():
            setattr(eng, k, v)
        return eng

    def run(self, eng, record=True):
        """Every step from the same initial state; returns (traces, outputs) per step."""
        out = []
        for label, flags, fn in self.steps:
            self.P.load(self.init)
            self.G.buf.zero_()
            self.opt.m.zero_()
            self.opt.v.zero_()
            self.opt.iterations = 0
            for k, v in flags.items():
                setattr(eng, k, v)
            eng._ws = self.ws
            self.rec.execute = self.execute
            if record:
                self.rec.start()
            res = fn(eng, self) or {}
            eng.finish_pending()
            trace, self.rec.trace = self.rec.trace, None
            self.ws.update(eng._ws)         # (Engine.workspace keeps one per mode: keep them all, so none is rebuilt)
            if self.rec.cuda:
                torch.cuda.synchronize()
            res.update(G=self.G.buf, P=self.P.buf)
            for (T, train), w in self.ws.items():
                res.update({f"p{T}{train}": w.p, f"s{T}{train}": w.s})
            out.append((trace, {k: v.clone() for k, v in res.items()} if self.execute else {}))
        return out


def s_train(eng, c):
    comm = Comm(c.rec) if c.shard else None
    for _ in range(2):
        eng.train_step(c.P, c.G, c.opt, c.adj, c.ed, t_global=c.T, comm=comm)


def s_predict(eng, c):
    p, s = eng.predict(c.P, c.adj, c.ed, logits=True)
    return {"pred_p": p, "pred_s": s}


def s_grads(eng, c):
    loss, p, s = eng.loss_and_grads(c.P, c.G, c.adj, c.ed, t_global=c.T, logits=True)
    return {"lg_p": p, "lg_s": s}


def s_rank(eng, c):
    out = {}
    for side in ("tail", "head"):
        r = eng.rank_candidates(c.P, c.adj, c.queries, side=side, k=5, max_edges=4 * c.N, fused=False)
        out.update({f"{side}_{k}": v for k, v in r.items()})
    return out


def s_value_grads(eng, c):
    dv, p = eng.value_grads(c.P, c.adj, c.ed, scale=0.5, grads=c.G)
    return {"vg_p": p, **{f"vg{i}": v for i, v in enumerate(dv)}}


def s_value_grads_batch(eng, c):
    return dict(eng.value_grads_batch(c.P, c.adj, c.queries, scale=0.5, max_entries=64))


def s_owner_off(eng, c):
    """A node-partitioned step whose dE rides in the all-reduce (e_owner off) and the bare forward / backward."""
    ws = eng.workspace(c.ed.T, True)
    eng.forward(c.P, c.adj, c.ed, ws, True)
    eng.backward(c.P, c.G, c.adj, c.ed, ws, Comm(c.rec), e_owner=False)
    eng.backward(c.P, c.G, c.adj, c.ed, ws, None, e_owner=False)


def cases(rec, dev):
    step3 = [("train_step", s_train), ("predict", s_predict), ("loss_and_grads", s_grads)]
    flagsets = [{}, {"fuse_tail_head": False}, {"fuse_sigma_tn": False}]
    if rec.cuda:
        flagsets += [dict(f, overlap=True) for f in flagsets]
    base = dict(fuse_tail_head=True, fuse_sigma_tn=True, overlap=False)
    allflags = [(f"{n} {f or ''}", dict(base, **f), fn) for f in flagsets for n, fn in step3]
    plain = [(n, base, fn) for n, fn in step3]
    rank = [("rank_candidates layered", base, s_rank)]
    shapes = [("N301 R2 D256 bf16x3", 301, 2, 256, allflags, dict(gemm="bf16x3")),
              ("N301 R2 D256 split", 301, 2, 256, plain, dict(gemm="split")),
              ("N301 R2 D256 exact", 301, 2, 256, plain, dict(gemm="exact")),
              ("N257 R3 D256 exact", 257, 3, 256, plain + rank, dict(gemm="exact")),
              ("N300 R8 D256 bf16 hilo", 300, 8, 256, plain, dict(gemm="bf16x3", features="bf16", edge_mfma="hilo")),
              ("N300 R8 D256 bf16 bf16", 300, 8, 256, plain, dict(gemm="bf16x3", features="bf16", edge_mfma="bf16")),
              ("N300 R4 D64 exact", 300, 4, 64, plain + rank + [("value_grads", base, s_value_grads),
                                                                ("value_grads_batch", base, s_value_grads_batch)],
               dict(gemm="exact"))]
    for name, N, R, D, steps, kw in shapes:
        yield Case(rec, dev, name, N, R, D, steps, **kw)
    sharded = [(n, f, fn) for n, f, fn in allflags if "overlap" not in n] + [("owner off", base, s_owner_off)]
    for name, N, R, D, _, kw in shapes:
        for cuts, rank_ in (([0, N // 3, 2 * N // 3, N], 1), ([0, N], 0), ([0, N // 2, N // 2, N], 1)):
            for owner_e in (True, False):
                for split in ((True, False) if owner_e else (False,)):
                    sh = RowShard(rec, cuts, rank_, owner_e, dev)
                    steps = [(n, dict(f, split_e_collectives=split), fn) for n, f, fn in sharded]
                    yield Case(rec, dev, f"{name} rows[{sh.a},{sh.b}) owner_e={owner_e} split={split}", N, R, D, steps,
                               shard={"row_shard": sh}, full_edges=sh.a == sh.b, **kw)
        for attr in ("node_shard", "spmm_shard"):
            yield Case(rec, dev, f"{name} {attr}", N, R, D, sharded[:-1],
                       shard={attr: RelShard(rec, R, N, 1, 3)}, **kw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-engine", required=True, help="the other engine.py (git show <rev>:iddgcn_amd/engine.py)")
    ap.add_argument("--record-only", action="store_true", help="record the launches, run none")
    ap.add_argument("--case", default="", help="only the cases whose name contains this")
    a = ap.parse_args()
    cuda = torch.cuda.is_available()
    if not cuda and not a.record_only:
        sys.exit("no GPU: use --record-only")
    dev = torch.device("cuda", 0) if cuda else torch.device("cpu")
    other = load_engine(a.parent_engine)
    rec = Recorder(cuda)
    wrap_ops(rec)
    wrap_mark(rec, other)
    wrap_mark(rec, this_engine)
    n_cases = n_calls = n_diff = n_nondet = 0
    for c in cases(rec, dev):
        if a.case not in c.name:
            continue
        c.execute = c.execute and not a.record_only
        eo, et = c.engine(other), c.engine(this_engine)
        c.run(eo, record=False)                     # every workspace and lazily made buffer exists from here on
        rec.shared = set()
        rec.share(c.P, c.G, c.opt, c.adj, c.ed, *c.ws.values(), *(c.shard or {}).values())
        runs = [c.run(e) for e in (eo, et, eo)]
        calls = bad = 0
        for (label, _, _), (t0, o0), (t1, o1), (t2, o2) in zip(c.steps, *runs):
            calls += len(t0)
            if t0 != t2:
                n_nondet += 1
                print(f"NOT DETERMINISTIC {c.name} / {label}: other vs other differ at {first_difference(t0, t2)}")
            t0m, t1m = (drop_marks(t, {"tail_fwd_gemm"}) for t in (t0, t1)) if "rank" in label else (t0, t1)
            d = first_difference(t0m, t1m)
            if d is not None:
                bad += 1
                print(f"DIFFERENT {c.name} / {label}: call {d[0]}\n  other: {d[1]}\n  this:  {d[2]}")
            for k in o0:
                for tag, o in (("this", o1), ("other again", o2)):
                    if not (o0[k].shape == o[k].shape and torch.equal(o0[k].view(torch.uint8).reshape(-1),
                                                                      o[k].view(torch.uint8).reshape(-1))):
                        bad += 1
                        print(f"OUTPUT DIFFERS {c.name} / {label}: {k} (other vs {tag})")
        n_cases, n_calls, n_diff = n_cases + 1, n_calls + calls, n_diff + bad
        print(f"case {c.name}: {len(c.steps)} steps, {calls} calls, {'run' if c.execute else 'record-only'}, "
              f"{bad} differences", flush=True)
    print(f"{n_cases} cases, {n_calls} calls, {n_nondet} non-deterministic traces, {n_diff} differences")
    sys.exit(1 if (n_diff or n_nondet) else 0)


if __name__ == "__main__":
    main()
