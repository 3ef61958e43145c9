"""Batched explaiNE on the GPU: the seeds kernel, the ragged SDDMM, the segment top-k, Engine.value_grads_batch and
explain.explaine_batched.

Bars (tests/test_gpu_explain.py's): a gradient may deviate from the float64 autograd reference by max(4 x the fp32
autograd's own deviation, 1e-5 of max|g|), per query; p by max(4 x the fp32 deviation, 1e-6).  Where two fp32 results
are compared with each other (the batched path against the per-triple Engine.value_grads) each is within that bar of
the reference, so they are within twice the bar of each other.  Batch independence and the selection are exact
(bitwise / identical indices)."""
import numpy as np
import pytest
import torch

from iddgcn_amd import _lib as L
from iddgcn_amd import explain as X
from iddgcn_amd import get_IDDGCN_Model, ops
from iddgcn_amd.engine import Engine, FlatParams
from iddgcn_amd.explain import explaine_batched, rank_sparse_gradient
from iddgcn_amd.graph import DeviceAdjacency, SparseAdj, get_adj_mats
from oracle import ref_explain
from oracle.ref_utils import get_adj_coo

pytestmark = pytest.mark.gpu
QS = (1, 2, 63, 64, 65, 200)          # the seeds kernel's query tile is 8: a power of two <= 64


def bits(t):
    return t.contiguous().view(torch.int32)


def make_params(N, R, D, rng, saturate=False):
    p = {"E": rng.standard_normal((N, D)) / 8}
    for l in (1, 2, 3):
        p.update({f"K{l}": rng.standard_normal((R, D, D)) / D, f"S{l}": rng.standard_normal((D, D)) / 8,
                  f"relw{l}": np.zeros(R), f"Wa{l}": rng.standard_normal((D, R)) / 8,
                  f"ba{l}": rng.standard_normal(R) / 8})
    p["rel"] = rng.standard_normal((R, D)) / np.sqrt(D / 64)
    if saturate:      # one-hot softmax rows, sigmoids driven to 0 / 1
        for l in (1, 2, 3):
            p[f"Wa{l}"] = p[f"Wa{l}"] * 60
            p[f"S{l}"] = p[f"S{l}"] * 6
            p[f"K{l}"] = p[f"K{l}"] * 12
    return {k: v.astype(np.float32) for k, v in p.items()}


def autograd_seeds(params, mats, q, dtype):
    """The reference formulation (ref_explain._layer's op order) with every query's own AE rows as leaves:
    (p (Q,), GH (Q, R, D), GT (Q, R, D)) = d p_q / d AE_r[h_q], d p_q / d AE_r[t_q] (separate leaves at h == t)."""
    P = {k: torch.tensor(np.asarray(v), dtype=dtype) for k, v in params.items()}
    E = P["E"]
    h, r, t = (torch.as_tensor(q[:, i]) for i in range(3))
    ae = torch.stack([torch.zeros_like(E).index_add(0, torch.as_tensor(m.rows), torch.as_tensor(
        np.asarray(m.values), dtype=dtype)[:, None] * E[torch.as_tensor(m.cols)]) for m in mats])
    aeh = ae[:, h].transpose(0, 1).clone().requires_grad_(True)
    aet = ae[:, t].transpose(0, 1).clone().requires_grad_(True)
    xh, xt = E[h], E[t]
    for l in (1, 2, 3):
        K, S = P[f"K{l}"], P[f"S{l}"]
        ho, to = xh @ S, xt @ S
        alpha = torch.softmax(xh @ P[f"Wa{l}"] + P[f"ba{l}"], dim=-1)
        for i in range(K.shape[0]):
            w = torch.sigmoid(alpha[:, i])[:, None]
            ho = ho + w * torch.einsum("qd,de->qe", aeh[:, i], K[i])
            to = to + w * torch.einsum("qd,de->qe", aet[:, i], K[i])
        xh, xt = torch.sigmoid(ho), torch.sigmoid(to)
    p = torch.sigmoid(torch.sum(xh * P["rel"][r] * xt, dim=-1))
    gh, gt = torch.autograd.grad(p.sum(), [aeh, aet])
    return p.detach().numpy().astype(np.float64), gh.numpy().astype(np.float64), gt.numpy().astype(np.float64)


def within_bar(ours, ref64, ref32, floor=1e-5, what=""):
    """|ours - ref64| <= max(4 |ref32 - ref64|, floor max|ref64|), maxima over one query's values; returns the
    (error, bar) pair for printing."""
    if not ours.size:
        return 0.0, 0.0
    err = np.abs(ours - ref64).max()
    bar = max(4 * np.abs(ref32 - ref64).max(), floor * np.abs(ref64).max())
    assert err <= bar, (what, err, bar)
    return err, bar


class Small:
    """N = 50: node 49 has no stored entry in any relation, relation-0 self loop at node 7."""

    def __init__(self, d, R, dev, saturate=False, seed=0):
        rng = np.random.default_rng(seed + 17 * d + R)
        N = self.N = 50
        self.d, self.R = d, R
        tri = np.stack([rng.integers(0, 49, 400), rng.integers(0, R, 400), rng.integers(0, 49, 400)], 1)
        tri = np.concatenate([tri, [[7, 0, 7]]])
        self.mats = get_adj_mats(tri, N, R)
        self.params = make_params(N, R, d, rng, saturate)
        q = np.stack([rng.integers(0, N, 200), rng.integers(0, R, 200), rng.integers(0, N, 200)], 1)
        q[1] = q[0]                                   # a repeated query
        q[2] = (7, 0, 7)                              # h == t
        q[3] = (49, R - 1, 3)                         # empty rows on the head side
        q[4] = (5, 0, 49)                             # .. on the tail side
        q[5] = (49, 0, 49)
        q[66] = (12, R - 1, 12)
        self.q = q
        self.eng = Engine(N, R, d, dev)
        self.P = FlatParams(N, R, d, dev)
        self.P.load(self.params)
        self.adj = DeviceAdjacency(self.mats, N, dev)
        self.dev = dev

    def tables(self):
        ws = self.eng.workspace(1, False)
        self.eng._node_tables(self.P, self.adj, ws)
        return ws

    def seeds(self, q, scale=1.0):
        ws = self.tables()
        i32 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32), device=self.dev)  # noqa: E731
        P = self.P
        return ops.explain_seeds(i32(q[:, 0]), i32(q[:, 1]), i32(q[:, 2]), ws.ES1, ws.P, ws.W, ws.Ssm, ws.X,
                                 (P["K1"], P["K2"], P["K3"]), P["S2"], P["S3"], P["Wa2"], P["Wa3"], P["rel"], scale)


# -- seeds -------------------------------------------------------------------------------------------
SEED_CASES = [(d, R, False) for d in (32, 64) for R in (1, 2, 4, 8)] + [(64, 4, True), (32, 2, True)]


@pytest.mark.parametrize("d,R,saturate", SEED_CASES)
def test_seeds_against_autograd_and_engine(d, R, saturate, cuda):
    """G and p of 200 queries against the float64 autograd of the AE rows (every query) and against the rows h, t of
    the dAE a single-triple Engine.value_grads leaves (the special queries and a few others); the batches Q < 200
    and a permuted batch give bitwise the same rows.  R = 1: the softmax has one entry, du = 0.
    Observed on an MI355X: the worst query's error is 0.03 to 0.26 of its bar over the ten cases."""
    c = Small(d, R, cuda, saturate)
    G, p = c.seeds(c.q)
    Gn, pn = G.cpu().numpy().astype(np.float64), p.cpu().numpy().astype(np.float64)
    p64, gh64, gt64 = autograd_seeds(c.params, c.mats, c.q, torch.float64)
    p32, gh32, gt32 = autograd_seeds(c.params, c.mats, c.q, torch.float32)
    worst = 0.0
    for j in range(len(c.q)):
        ref64, ref32 = np.stack([gh64[j], gt64[j]]), np.stack([gh32[j], gt32[j]])
        err, bar = within_bar(Gn[j], ref64, ref32, what=("G", j, c.q[j]))
        worst = max(worst, err / bar if bar else 0.0)
        assert abs(pn[j] - p64[j]) <= max(4 * abs(p32[j] - p64[j]), 1e-6), (j, pn[j], p64[j])
    print(f"seeds d={d} R={R} saturate={saturate}: worst error / bar {worst:.3f}")
    # the per-triple engine: rows h and t of its dAE (GH + GT on one row at h == t), its p
    for j in (0, 2, 3, 4, 5, 66, 100, 199):
        h, _, t = c.q[j]
        ed = c.eng.edges(c.q[j][None])
        _, pe = c.eng.value_grads(c.P, c.adj, ed)
        dAE = c.eng.workspace(ed.T, True).dAE.cpu().numpy().astype(np.float64)
        ours = np.stack([Gn[j, 0] + Gn[j, 1]] * 2) if h == t else Gn[j]
        ref64 = np.stack([gh64[j] + gt64[j]] * 2) if h == t else np.stack([gh64[j], gt64[j]])
        ref32 = np.stack([gh32[j] + gt32[j]] * 2) if h == t else np.stack([gh32[j], gt32[j]])
        eng_rows = np.stack([dAE[:, h], dAE[:, t]])
        _, bar = within_bar(eng_rows, ref64, ref32, what=("engine dAE", j))
        assert np.abs(ours - eng_rows).max() <= 2 * bar, (j, np.abs(ours - eng_rows).max(), bar)
        assert abs(pn[j] - float(pe[0])) <= 2 * max(4 * abs(p32[j] - p64[j]), 1e-6)
        other = np.ones(c.N, bool)
        other[[h, t]] = False
        assert not dAE[:, other].any()               # the row-locality identity on the per-triple path
    # batch independence
    for Q in QS[:-1]:
        Gq, pq = c.seeds(c.q[:Q])
        assert torch.equal(bits(Gq), bits(G[:Q])) and torch.equal(bits(pq), bits(p[:Q])), Q
    perm = np.random.default_rng(1).permutation(len(c.q))
    Gp, pp = c.seeds(c.q[perm])
    assert torch.equal(bits(Gp), bits(G[perm])) and torch.equal(bits(pp), bits(p[perm]))
    assert torch.equal(bits(G[0]), bits(G[1]))       # the repeated query
    if not saturate:                                 # the seed scale is linear (a power of two: exact)
        G3, p3 = c.seeds(c.q[:9], scale=0.25)
        assert torch.equal(bits(p3), bits(p[:9])) and torch.equal(bits(G3), bits(G[:9] * 0.25))


def test_ops_argument_checks(cuda):
    c = Small(64, 2, cuda)
    ws = c.tables()
    P = c.P
    i32 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32), device=cuda)  # noqa: E731
    h, r, t = (i32(c.q[:5, i]) for i in range(3))

    def seeds(**kw):
        a = dict(h=h, r=r, t=t, ES1=ws.ES1, P=ws.P, W=ws.W, Ssm=ws.Ssm, X=ws.X, K=(P["K1"], P["K2"], P["K3"]),
                 S2=P["S2"], S3=P["S3"], Wa2=P["Wa2"], Wa3=P["Wa3"], rel=P["rel"])
        a.update(kw)
        return ops.explain_seeds(**a)

    G, _ = seeds()
    for bad in (dict(h=h.long()), dict(ES1=ws.ES1.double()), dict(P=ws.P[:, :, :, ::2]), dict(W=ws.W.transpose(1, 2)),
                dict(X=ws.X[:2]), dict(K=(P["K1"], P["K2"])), dict(Wa2=None), dict(G=torch.empty(5, 2, 2, 32, device=cuda)),
                dict(S2=P["S2"][:32])):
        with pytest.raises(L.IddgcnError):
            seeds(**bad)
    qptr = torch.zeros(6, dtype=torch.int64, device=cuda)
    ent, gr = torch.full((4,), -7, dtype=torch.int32, device=cuda), torch.full((4,), -7.0, device=cuda)
    ops.explain_row_grads(h, t, c.adj.fwd_ptr, c.adj.fwd_col, G, P["E"], qptr, ent, gr)   # no room: nothing written
    assert (ent == -7).all() and (gr == -7).all()
    for bad in (dict(qptr=qptr.int()), dict(qptr=qptr[:5]), dict(ent=ent.long()), dict(gr=torch.empty(3, device=cuda)),
                dict(eoc=c.adj.fwd_src.int()), dict(G=G.double())):
        a = dict(qptr=qptr, ent=ent, gr=gr, eoc=None, G=G)
        a.update(bad)
        with pytest.raises(L.IddgcnError):
            ops.explain_row_grads(h, t, c.adj.fwd_ptr, c.adj.fwd_col, a["G"], P["E"], a["qptr"], a["ent"], a["gr"],
                                  a["eoc"])
    for k in (0, 65):
        with pytest.raises(L.IddgcnError):
            ops.explain_topk(qptr, ent, gr, k)
    with pytest.raises(L.IddgcnError):
        ops.explain_topk(qptr.int(), ent, gr, 3)
    with pytest.raises(L.IddgcnError):
        ops.explain_topk(qptr, ent, gr[:3], 3)
    te, tv, npos = ops.explain_topk(qptr, ent, gr, 3)                 # empty segments: all padding
    assert (te == -1).all() and torch.isinf(tv).all() and (tv < 0).all() and not npos.any()


# -- row gradients -------------------------------------------------------------------------------------
class Rows:
    """N = 320, R = 3: relation 2 is empty (the (0, 0) = 0 placeholder); relation-0 rows of degree 1, 63, 64, 65, 300
    at nodes 1..5, node 6 has no entry; E[10] = E[11] = E[12] (exact ties); the stored entries are shuffled (a
    non-identity entry order) and their values replaced."""

    def __init__(self, dev, d=64):
        rng = np.random.default_rng(3)
        N, R = self.N, self.R = 320, 3
        rows = []
        for node, deg in ((1, 1), (2, 63), (3, 64), (4, 65), (5, 300)):
            cols = np.sort(rng.choice(np.arange(7, N), deg, replace=False)) if deg < 300 else np.arange(10, 310)
            rows.append(np.stack([np.full(deg, node), np.zeros(deg, np.int64), cols], 1))
        rows.append(np.stack([np.full(6, 5), np.ones(6, np.int64), [10, 11, 12, 40, 41, 5]], 1))
        rows.append(np.array([[0, 0, 9], [0, 1, 5], [8, 1, 0]]))
        o = rng.integers(7, N, 600)
        rows.append(np.stack([o, rng.integers(0, 2, 600), rng.integers(0, N, 600)], 1))
        tri = np.concatenate(rows).astype(np.int64)
        mats = get_adj_mats(tri, N, R)
        assert mats[2].nnz == 1 and mats[2].values[0] == 0           # the placeholder
        self.mats = []
        for m in mats:
            o = rng.permutation(m.nnz)
            self.mats.append(SparseAdj(m.indices[o], m.values[o], N))
        self.params = make_params(N, R, d, rng)
        self.params["E"][11] = self.params["E"][12] = self.params["E"][10]
        self.values = [(0.25 + rng.random(m.nnz)).astype(np.float32) * m.values for m in self.mats]
        self.eng = Engine(N, R, d, dev)
        self.P = FlatParams(N, R, d, dev)
        self.P.load(self.params)
        self.adj = DeviceAdjacency(self.mats, N, dev)
        assert not torch.equal(self.adj.fwd_src, torch.arange(self.adj.total_nnz, device=dev))
        self.adj.set_values(torch.as_tensor(np.concatenate(self.values), device=dev))
        #                  deg 1     63         64         65        300 (+6)   h == t     empty row  placeholder rows
        self.q = np.array([(1, 0, 2), (2, 1, 3), (3, 0, 4), (4, 1, 5), (5, 0, 1), (5, 1, 5), (6, 0, 5), (0, 2, 3),
                           (4, 2, 0), (0, 0, 0), (6, 1, 6), (3, 0, 1)], np.int64)
        self.coo = [(np.stack([m.rows, m.cols], 1), m.values) for m in self.mats]


@pytest.fixture(scope="module")
def rows_case(cuda):
    c = Rows(cuda)
    c.out = c.eng.value_grads_batch(c.P, c.adj, c.q)
    c.per_triple = []
    for tr in c.q:
        dv, p = c.eng.value_grads(c.P, c.adj, c.eng.edges(tr[None]))
        c.per_triple.append((torch.cat(dv).cpu().numpy(), float(p[0])))
    return c


def test_row_grads_against_value_grads(rows_case):
    """Scattered into a dense zero vector, each query's candidates equal the per-triple Engine.value_grads; every
    entry outside the candidate list is exactly 0 there; candidate counts are deg(h) + deg(t) (one row at h == t)."""
    c = rows_case
    qp = c.out["qptr"].cpu().numpy()
    entry, grad, p = c.out["entry"].cpu().numpy(), c.out["grad"].cpu().numpy(), c.out["p"].cpu().numpy()
    total = c.adj.total_nnz
    rows_all = np.concatenate([m.rows for m in c.mats])
    assert qp[0] == 0 and qp[-1] == len(entry) == len(grad)
    for j, tr in enumerate(c.q):
        e, g = entry[qp[j]:qp[j + 1]], grad[qp[j]:qp[j + 1]]
        want = np.flatnonzero((rows_all == tr[0]) | (rows_all == tr[2]))
        assert len(np.unique(e)) == len(e) and np.array_equal(np.sort(e), want), (j, tr)
        dense = np.zeros(total, np.float32)
        dense[e] = g
        eng_dense, eng_p = c.per_triple[j]
        outside = np.ones(total, bool)
        outside[e] = False
        assert not eng_dense[outside].any(), (j, tr)
        p64, g64 = ref_explain.value_grads(c.params, tr, c.coo, values=c.values)
        p32, g32 = ref_explain.value_grads(c.params, tr, c.coo, values=c.values, dtype=torch.float32)
        ref64, ref32 = np.concatenate(g64), np.concatenate(g32).astype(np.float64)
        err, bar = within_bar(dense.astype(np.float64), ref64, ref32, what=("grad", j, tr))
        within_bar(eng_dense.astype(np.float64), ref64, ref32, what=("engine", j, tr))
        assert np.abs(dense - eng_dense).max() <= 2 * bar
        assert abs(p[j] - p64) <= max(4 * abs(p32 - p64), 1e-6)
        print(f"row grads {tuple(tr)}: {len(e)} candidates, error {err:.2e} (bar {bar:.2e})")
    deg = np.bincount(rows_all, minlength=c.N)
    assert np.array_equal(np.diff(qp), [deg[h] + (deg[t] if h != t else 0) for h, _, t in c.q])
    assert {1, 63, 64, 65, 306}.issubset({int(deg[n]) for n in range(1, 6)}) and deg[6] == 0


def test_row_grads_identity_entry_order_and_chunks(rows_case, cuda):
    """entry_of_csr = None writes the CSR position (fwd_pos maps entries onto it); max_entries splits the batch into
    chunks without changing a bit."""
    c = rows_case
    qp = c.out["qptr"]
    i32 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32), device=cuda)  # noqa: E731
    h, r, t = (i32(c.q[:, i]) for i in range(3))
    ws = c.eng.workspace(1, False)
    c.eng._node_tables(c.P, c.adj, ws)
    P = c.P
    G, _ = ops.explain_seeds(h, r, t, ws.ES1, ws.P, ws.W, ws.Ssm, ws.X, (P["K1"], P["K2"], P["K3"]), P["S2"], P["S3"],
                             P["Wa2"], P["Wa3"], P["rel"])
    ent, gr = torch.empty_like(c.out["entry"]), torch.empty_like(c.out["grad"])
    ops.explain_row_grads(h, t, c.adj.fwd_ptr, c.adj.fwd_col, G, P["E"], qp, ent, gr)
    assert torch.equal(c.adj.fwd_src[ent.long()].int(), c.out["entry"])
    assert torch.equal(bits(gr), bits(c.out["grad"]))
    for max_entries in (1, 200, 500):
        o = c.eng.value_grads_batch(c.P, c.adj, c.q, max_entries=max_entries)
        for k in ("p", "grad"):
            assert torch.equal(bits(o[k]), bits(c.out[k])), (max_entries, k)
        assert torch.equal(o["entry"], c.out["entry"]) and torch.equal(o["qptr"], qp)
    half = c.eng.value_grads_batch(c.P, c.adj, c.q, scale=0.5)
    assert torch.equal(bits(half["grad"]), bits(c.out["grad"] * 0.5))


# -- top-k ---------------------------------------------------------------------------------------------
def stable_topk(entry, val, k):
    """numpy's stable descending order over the segment in ascending entry order."""
    o = np.argsort(entry, kind="stable")
    e, v = entry[o], val[o]
    top = np.argsort(-v, kind="stable")[:k]
    ids = np.full(k, -1, np.int32)
    vals = np.full(k, -np.inf, np.float32)
    ids[:len(top)], vals[:len(top)] = e[top], v[top]
    return ids, vals


@pytest.mark.parametrize("k", [1, 10, 64])
def test_topk_against_stable_argsort(k, cuda):
    """Segments shorter than k (padding), one longer than a sorting pass (960) and one of several passes; many exact
    ties, +-0.0, all-negative and all-zero segments; n_pos."""
    rng = np.random.default_rng(k)
    lens = [0, 1, 5, 63, 64, 65, 100, 960, 961, 2500, 7, 30]
    segs = []
    for i, n in enumerate(lens):
        v = np.round(rng.standard_normal(n), 1).astype(np.float32)
        v[rng.random(n) < 0.15] = 0.0
        v[rng.random(n) < 0.15] = -0.0
        if i == 10:
            v = -np.abs(v) - 1
        if i == 11:
            v = np.where(rng.random(n) < 0.5, 0.0, -0.0).astype(np.float32)
        segs.append((rng.permutation(5000)[:n].astype(np.int32), v))
    qptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    entry, val = np.concatenate([s[0] for s in segs]), np.concatenate([s[1] for s in segs])
    te, tv, npos = ops.explain_topk(torch.as_tensor(qptr, device=cuda), torch.as_tensor(entry, device=cuda),
                                    torch.as_tensor(val, device=cuda), k)
    te, tv, npos = te.cpu().numpy(), tv.cpu().numpy(), npos.cpu().numpy()
    for i, (e, v) in enumerate(segs):
        ids, vals = stable_topk(e, v, k)
        assert np.array_equal(te[i], ids), (i, te[i], ids)
        assert np.array_equal(tv[i].view(np.uint32), vals.view(np.uint32)), (i, tv[i], vals)   # the sign of 0 too
        assert npos[i] == int((v > 0).sum())


def test_topk_ties_from_identical_rows(rows_case):
    """E[10] = E[11] = E[12]: node 5's entries at those columns tie exactly and are ordered by entry id; the
    selection over value_grads_batch's segments equals the stable argsort, and where n_pos >= k the host merge."""
    c = rows_case
    qp = c.out["qptr"].cpu().numpy()
    entry, grad = c.out["entry"].cpu().numpy(), c.out["grad"].cpu().numpy()
    j = 4                                              # (5, 0, 1)
    e, g = entry[qp[j]:qp[j + 1]], grad[qp[j]:qp[j + 1]]
    cols_all = np.concatenate([m.cols for m in c.mats])
    rows_all = np.concatenate([m.rows for m in c.mats])
    rel_all = np.repeat(np.arange(c.R), c.adj.nnz)
    for n in (0, 1):
        tied = g[(rows_all[e] == 5) & (rel_all[e] == n) & np.isin(cols_all[e], (10, 11, 12))]
        assert len(tied) == 3 and tied[0] == tied[1] == tied[2]
    for k in (10, 64):
        te, tv, npos = (x.cpu().numpy() for x in ops.explain_topk(c.out["qptr"], c.out["entry"], c.out["grad"], k))
        for i in range(len(c.q)):
            ei, gi = entry[qp[i]:qp[i + 1]], grad[qp[i]:qp[i + 1]]
            ids, vals = stable_topk(ei, gi, k)
            assert np.array_equal(te[i], ids) and np.array_equal(tv[i].view(np.uint32), vals.view(np.uint32)), (k, i)
            assert npos[i] == int((gi > 0).sum())
            if npos[i] >= k:
                mi, ms = rank_sparse_gradient(ei, gi, c.adj.total_nnz, k)
                assert np.array_equal(mi, te[i]) and np.array_equal(ms, tv[i])


# -- batch independence --------------------------------------------------------------------------------
def test_batch_independence(cuda):
    """A query's p, candidates, gradients and top-k are bitwise the same alone, inside a batch of 200 and after
    permuting the batch (G: test_seeds_against_autograd_and_engine)."""
    c = Small(64, 4, cuda)

    def run(q):
        o = c.eng.value_grads_batch(c.P, c.adj, q)
        te, tv, npos = ops.explain_topk(o["qptr"], o["entry"], o["grad"], 10)
        qp = o["qptr"].cpu().numpy()
        return [(bits(o["p"][j:j + 1]).item(), o["entry"][qp[j]:qp[j + 1]].cpu().numpy().tobytes(),
                 o["grad"][qp[j]:qp[j + 1]].cpu().numpy().tobytes(), te[j].cpu().numpy().tobytes(),
                 tv[j].cpu().numpy().tobytes(), int(npos[j])) for j in range(len(q))]

    whole = run(c.q)
    for j in (0, 2, 5, 66, 199):
        assert run(c.q[j:j + 1])[0] == whole[j], j
    perm = np.random.default_rng(2).permutation(len(c.q))
    shuffled = run(c.q[perm])
    assert all(shuffled[i] == whole[perm[i]] for i in range(len(perm)))
    assert whole[0] == whole[1]


# -- end to end: fold 4, bundled weights ---------------------------------------------------------------
N_ENT, N_REL = 845, 4


def _check_topk(our_p, our_s, ref_p, ref_s, tol):
    """tests/test_gpu_explain.py's rule: scores within tol, triples identical where the reference scores are
    separated by more than tol."""
    np.testing.assert_allclose(np.sort(our_s)[::-1], np.sort(ref_s)[::-1], rtol=0, atol=tol)
    sep = np.ones(len(ref_s), bool)
    gaps = np.abs(np.diff(ref_s)) > tol
    sep[:-1] &= gaps
    sep[1:] &= gaps
    assert np.array_equal(our_p[sep], ref_p[sep])


@pytest.fixture(scope="module")
def fold4(golden, cuda):
    d, ex, w = golden("fold4_data.npz"), golden("explain_fold4.npz"), golden("weights_fold4.npz")
    model = get_IDDGCN_Model(N_ENT, N_REL, 64, 64, 123, None, 0, 4)
    model.load_weights("tests/golden/weights_fold4.npz")
    adjacency = np.concatenate([d["X_train"].astype(np.int64), ex["test_triples"]])
    test = ex["test_triples"]
    coo = get_adj_coo(adjacency, N_ENT, N_REL)
    oracle = {10: [], 64: []}
    for tr in test[:6]:                               # ref_explain.explaine's loop, the gradients shared by both k
        g = ref_explain.value_grads(w, tr, coo)[1]
        for k in oracle:
            oracle[k].append(ref_explain.get_pred(coo, g, k))
    eager_p, eager_s = X.explaine(model, adjacency, test[:12], top_k=64, graph=False)
    return model, adjacency, test, oracle, eager_p, eager_s


@pytest.mark.parametrize("k", [10, 64])
def test_explaine_batched_end_to_end(k, fold4):
    """explaine_batched on the first 12 test triples against explaine(graph=False) (the stable order's first k of its
    top 64) and, for the first 6, against the float64 oracle.  At k = 64 some triples have fewer than 64 positive
    candidates: the zero class fills the rest, exactly the oracle's triples in its order."""
    model, adjacency, test, oracle, eager_p, eager_s = fold4
    ours_p, ours_s = explaine_batched(model, adjacency, test[:12], top_k=k)
    assert ours_p.shape == (12, k, 3) and ours_s.shape == (12, k)
    assert ours_p.dtype == np.int64 and ours_s.dtype == np.float32
    filled = 0
    for j in range(12):
        ref_p, ref_s = eager_p[j, :k], eager_s[j, :k]
        _check_topk(ours_p[j], ours_s[j], ref_p, ref_s, 2e-4 * np.abs(ref_s).max())
        zero = ref_s == 0
        assert np.array_equal(ours_p[j][zero], ref_p[zero]) and not ours_s[j][zero].any()
    for j in range(6):
        ref_p, ref_s = oracle[k][j]
        _check_topk(ours_p[j], ours_s[j], ref_p, ref_s, 2e-4 * np.abs(ref_s).max())
        zero = ref_s == 0
        filled += int(zero.sum())
        assert np.array_equal(ours_p[j][zero], ref_p[zero]) and not ours_s[j][zero].any()
    if k == 64:
        assert filled > 0                             # real data reaches the zero fill


def test_explaine_batched_small_nnz_and_empty(cuda):
    """top_k beyond the stored entries (k = total nnz: zeros, then the negatives) against explaine(graph=False); no
    triples."""
    N, R = 12, 2
    rng = np.random.default_rng(4)
    tri = np.stack([rng.integers(0, N, 14), rng.integers(0, R, 14), rng.integers(0, N, 14)], 1)
    model = get_IDDGCN_Model(N, R, 32, 32, 123, None, 0, 0)
    q = tri[:5]
    for top_k in (5, 100):
        a_p, a_s = explaine_batched(model, tri, q, top_k=top_k)
        b_p, b_s = X.explaine(model, tri, q, top_k=top_k, graph=False)
        assert a_p.shape == b_p.shape and a_s.shape == b_s.shape
        for j in range(len(q)):
            _check_topk(a_p[j], a_s[j], b_p[j], b_s[j], 2e-4 * np.abs(b_s[j]).max())
    e_p, e_s = explaine_batched(model, tri, np.zeros((0, 3), np.int64), top_k=5)
    assert e_p.shape == (0, 5, 3) and e_s.shape == (0, 5)


def test_outside_the_envelope_raises(cuda):
    rng = np.random.default_rng(0)
    N, R = 40, 2
    tri = np.stack([rng.integers(0, N, 100), rng.integers(0, R, 100), rng.integers(0, N, 100)], 1)
    mats = get_adj_mats(tri, N, R)
    for kw in (dict(dim=256), dict(dim=256, gemm="split", features="bf16"), dict(dim=128)):
        D = kw.pop("dim")
        eng = Engine(N, R, D, cuda, **kw)
        P = FlatParams(N, R, D, cuda)
        with pytest.raises(L.IddgcnError, match="explaine"):
            eng.value_grads_batch(P, eng.adjacency(mats), tri[:3])
    for attr in ("node_shard", "spmm_shard", "row_shard"):
        eng = Engine(N, R, 64, cuda)
        P = FlatParams(N, R, 64, cuda)
        setattr(eng, attr, object())
        with pytest.raises(L.IddgcnError):
            eng.value_grads_batch(P, eng.adjacency(mats), tri[:3])
    eng = Engine(N, R, 64, cuda)
    P = FlatParams(N, R, 64, cuda)
    adj = eng.adjacency(mats)
    for bad in ([[N, 0, 1]], [[0, R, 1]], [[0, 0, -1]], [[0, 0]]):
        with pytest.raises(L.IddgcnError):
            eng.value_grads_batch(P, adj, np.array(bad))
    model = get_IDDGCN_Model(N, R, 256, 256, 123, None, 0, 0)
    with pytest.raises(L.IddgcnError, match="explaine"):
        explaine_batched(model, tri, tri[:2])
