"""Explainers on the MI355X path: the reference's three link-prediction
explainers, driven by the same HIP engine as training.

* explaiNE (explanation/explaiNE.py): for each test triple, the gradient of the predicted
  probability w.r.t. every adjacency VALUE (``tape.gradient(pred, adj_mat.values)``,
  explaiNE.py:85-94), ranked, top-k (``get_pred``, explaiNE.py:12-32).
* GNNExplainer (explanation/GnnExplainer.py) and the IDDGCN explainer
  (explanation/IDDGCN_explain.py): per test triple, the computation graph (edges touching the
  head or the tail, GnnExplainer.py:13-24) is masked as ``adj * sigmoid(mask)``; the masks are
  trained for a few epochs with Keras Adam on ``-before_pred * log(pred + 1e-5)`` (plus, for the
  IDDGCN explainer, a relation-ratio structure loss, IDDGCN_explain.py:30-41), then the masked
  values above a threshold are ranked.

All three need one primitive on the hot path: the gradient of the prediction w.r.t. the adjacency
values.  ``Engine.value_grads`` gets it from one forward + backward with the prediction seed and
one SDDMM (``iddgcn_sddmm_csr_f32``); masked values go to the device CSR with
``DeviceAdjacency.set_values`` (no rebuild).  Reference semantics kept on purpose:
* the Adam optimizer of the mask explainers is created ONCE and shared by all test triples (its
  iterations and moment slots carry over; the masks are reset to ``init_value`` after each triple,
  GnnExplainer.py:72-73), and it is the dense-variable form (ApplyAdam) over the full (N, N) mask
  of every relation;
* ranking is stable descending (Python ``sorted(..., reverse=True)`` in get_pred).
TF's seeded ``tf.random.normal`` mask init cannot be replayed without TF: pass ``init_value`` to
use a specific one (default: numpy N(0,1) with the given seed).

``mask_explainer_batched`` (``gnn_explainer_batched`` / ``iddgcn_explainer_batched``) runs the same mask training from
each triple's candidate entries alone, every epoch of a triple in one workgroup, with the shared Adam kept as sparse
per-entry state (see the section below).

``fidelity_curves`` scores any of their outputs against the model itself: the deletion and insertion curves of each
triple's explanation, every variant of a triple in one fused kernel (``fidelity_summary``, ``random_explanations``).

``counterfactual_batched`` optimises what those curves measure: a greedy search for the few edges whose removal flips
a prediction, every decision on the device; ``occlusion_batched`` ranks edges by their exact leave-one-out effect.

``integrated_gradients_batched`` gives signed per-edge attributions that add up to the prediction's change against the
graph without those edges, every quadrature node of a triple in one fused kernel (``integrated_gradients_summary``).
"""
import contextlib
import time

import numpy as np
import torch

from . import ops
from ._lib import PATH_MAX_STEPS, TOPK_MAX, IddgcnError
from .engine import layer_tuples
from .graph import DeviceAdjacency, _as_triples, get_adj_mats


# -- host helpers (pure numpy) ---------------------------------------------------------------
def get_neighbors(data, node_idx):
    """GnnExplainer.py:13-17: triples with head == node, then triples with tail == node."""
    data = _as_triples(data)
    return np.concatenate([data[data[:, 0] == node_idx], data[data[:, 2] == node_idx]], 0)


def get_computation_graph(head, rel, tail, data):
    """GnnExplainer.py:19-24 / IDDGCN_explain.py:21-27 (duplicates kept; get_adj_mats dedups)."""
    return np.concatenate([get_neighbors(data, head), get_neighbors(data, tail)], 0)


def get_pred(adj_mats, value_grads, top_k):
    """explaiNE.get_pred (explaiNE.py:12-32) on per-relation value gradients (numpy arrays).

    Scores are visited relation by relation in entry order and ranked by a stable descending sort;
    returns ([top_k, 3] triples (head, rel, tail), [top_k] scores)."""
    rels = np.concatenate([np.full(len(g), r, np.int64) for r, g in enumerate(value_grads)])
    idx = np.concatenate([np.arange(len(g), dtype=np.int64) for g in value_grads])
    score = np.concatenate([np.asarray(g, np.float32) for g in value_grads])
    order = np.argsort(-score, kind="stable")[:top_k]
    triples = np.array([[adj_mats[rels[k]].indices[idx[k], 1], rels[k], adj_mats[rels[k]].indices[idx[k], 2]]
                        for k in order], dtype=np.int64).reshape(-1, 3)
    return triples, score[order]


def _model_state(model):
    eng = model._device_state()
    return eng, model._params


# -- explaiNE -------------------------------------------------------------------------------
def explaine(model, adjacency_data, test_triples, top_k=10, graph=True):
    """explaiNE.py __main__ loop (lines 57-101) for one fold: ADJACENCY_DATA = train ∪ test, one
    prediction-gradient per test triple.  Returns (preds [n, top_k, 3], scores [n, top_k]).

    graph=True (default): the per-triple work — the single-edge layout, forward + backward with the
    prediction seed, SDDMM, and the stable descending ranking (torch.sort on the device) — is
    captured once in a HIP graph and replayed per triple with no host round trip; graph=False runs
    the same launches eagerly and ranks on the host (get_pred)."""
    eng, params = _model_state(model)
    N, R = model.num_entities, model.num_relations
    adj_mats = get_adj_mats(adjacency_data, N, R)
    dadj = DeviceAdjacency(adj_mats, N, eng.device)
    triples = _as_triples(test_triples)
    if not graph:
        preds, scores = [], []
        for tr in triples:
            dv, _ = eng.value_grads(params, dadj, eng.edges(tr[None]))
            p, s = get_pred(adj_mats, [g.cpu().numpy() for g in dv], top_k)
            preds.append(p)
            scores.append(s)
        return np.stack(preds), np.stack(scores)
    return _ExplaineGraph(eng, params, dadj, top_k).run(triples)


def rank_sparse_gradient(entry, grad, total_nnz, top_k):
    """get_pred's ranking of a full (total_nnz,) gradient vector that is zero outside its candidate list, without
    building it (pure numpy).  ``entry`` (distinct ids in [0, total_nnz)) and ``grad`` are one query's candidates;
    every other entry has gradient 0.  The stable descending order of the full vector is: the positive candidates
    (descending, ties by ascending id), then the zero class — every non-candidate entry and every candidate that is
    exactly 0 — by ascending id, then the negative candidates.  Returns (ids [k], scores [k] float32),
    k = min(top_k, total_nnz); work O(len(entry) + k), not O(total_nnz)."""
    entry = np.asarray(entry, np.int64)
    grad = np.asarray(grad, np.float32)
    if entry.ndim != 1 or entry.shape != grad.shape:
        raise ValueError(f"entry and grad must be 1-d and of one length, got {entry.shape} and {grad.shape}")
    k = min(int(top_k), int(total_nnz))
    by_id = np.argsort(entry, kind="stable")
    entry, grad = entry[by_id], grad[by_id]
    pos, neg = grad > 0, grad < 0
    pe, pg = entry[pos], grad[pos]
    o = np.argsort(-pg, kind="stable")[:k]                       # ids ascend already: ties keep ascending id
    ids, sc = [pe[o]], [pg[o]]
    need = k - len(o)
    if need > 0:
        # the first `need` ids of the zero class lie in [0, need + #non-zero candidates)
        nonzero = entry[pos | neg]
        zid = np.setdiff1d(np.arange(min(int(total_nnz), need + len(nonzero)), dtype=np.int64), nonzero,
                           assume_unique=True)[:need]
        zs = np.zeros(len(zid), np.float32)
        zc = ~(pos | neg)                                         # zero-valued candidates keep their stored sign
        if len(zid) and zc.any():
            ze, zg = entry[zc], grad[zc]
            at = np.minimum(np.searchsorted(zid, ze), len(zid) - 1)
            hit = zid[at] == ze
            zs[at[hit]] = zg[hit]
        ids.append(zid)
        sc.append(zs)
        need -= len(zid)
    if need > 0:
        ne, ng = entry[neg], grad[neg]
        o = np.argsort(-ng, kind="stable")[:need]
        ids.append(ne[o])
        sc.append(ng[o])
    return np.concatenate(ids), np.concatenate(sc).astype(np.float32)


def explaine_batched(model, adjacency_data, test_triples, top_k=10, stats=None):
    """explaine for all test triples in a fixed number of launches (Engine.value_grads_batch + ops.explain_topk):
    the same return contract, (preds [n, k, 3], scores [n, k]) with k = min(top_k, total nnz), and the ranking of the
    FULL gradient vector as get_pred gives it.  The gradient of a triple's prediction is zero outside the adjacency
    rows of its head and tail, so only those candidates are computed; a triple with at least k positive candidates
    is ranked by the kernel, the others (and every triple when k > 64) are completed on the host from their
    candidate list (rank_sparse_gradient).  fp32 features with D in {32, 64}: IddgcnError otherwise (use explaine).
    ``stats``: an optional dict that receives ``host_completed`` (triples finished on the host) and
    ``host_complete_s`` (the seconds that took), for tools/bench_explain_batched.py."""
    eng, params = _model_state(model)
    N, R = model.num_entities, model.num_relations
    adj_mats = get_adj_mats(adjacency_data, N, R)
    dadj = DeviceAdjacency(adj_mats, N, eng.device)
    triples = _as_triples(test_triples)
    n, total = len(triples), dadj.total_nnz
    k = min(int(top_k), total)
    out = eng.value_grads_batch(params, dadj, triples)
    row, col, rel, _ = _entry_table(dadj, real=False)
    trip_all = np.stack([row, rel, col], 1).astype(np.int64)
    ids = np.zeros((n, k), np.int64)
    scores = np.zeros((n, k), np.float32)
    if n == 0 or k == 0:
        return trip_all[ids], scores
    kk = min(k, TOPK_MAX)
    with eng._mark("xb_topk"):
        te, tv, npos = ops.explain_topk(out["qptr"], out["entry"], out["grad"], kk)
    npos = npos.cpu().numpy()
    done = (npos >= k) if kk == k else np.zeros(n, bool)
    ids[done], scores[done] = te.cpu().numpy()[done], tv.cpu().numpy()[done]
    t0 = time.perf_counter()
    if not done.all():
        qp, entry, grad = out["qptr"].cpu().numpy(), out["entry"].cpu().numpy(), out["grad"].cpu().numpy()
        for j in np.flatnonzero(~done):
            ids[j], scores[j] = rank_sparse_gradient(entry[qp[j]:qp[j + 1]], grad[qp[j]:qp[j + 1]], total, k)
    if stats is not None:
        stats.update(host_completed=int((~done).sum()), host_complete_s=time.perf_counter() - t0)
    return trip_all[ids], scores


class _SingleEdge:
    """A one-triple ScoredEdges whose device arrays are rewritten in place from a device (3,) int64
    triple (so a captured graph can be replayed for any triple)."""

    def __init__(self, eng, triple_buf):
        self.T, self.y = 1, None
        dev = eng.device
        self._tr = triple_buf
        self._ar = torch.arange(eng.N + 1, device=dev)
        self.h = torch.zeros(1, dtype=torch.int32, device=dev)
        self.r = torch.zeros(1, dtype=torch.int32, device=dev)
        self.t = torch.zeros(1, dtype=torch.int32, device=dev)
        self.tptr = torch.zeros(eng.N + 1, dtype=torch.int32, device=dev)
        self.hptr = torch.zeros(eng.N + 1, dtype=torch.int32, device=dev)
        self.hperm = torch.zeros(1, dtype=torch.int32, device=dev)
        self.inv = torch.zeros(1, dtype=torch.int64, device=dev)

    def refresh(self):
        """Device-side layout of the single edge (ScoredEdges semantics, graph-capturable)."""
        self.h.copy_(self._tr[0:1])
        self.r.copy_(self._tr[1:2])
        self.t.copy_(self._tr[2:3])
        self.tptr.copy_(self._ar > self._tr[2])      # segment of tail t is [tptr[t], tptr[t+1]) = [0, 1)
        self.hptr.copy_(self._ar > self._tr[0])

    def unsort(self, x):
        return x


class _ExplaineGraph:
    def __init__(self, eng, params, dadj, top_k):
        dev = eng.device
        self.k = min(top_k, dadj.total_nnz)
        self.tr = torch.zeros(3, dtype=torch.int64, device=dev)
        self.ed = _SingleEdge(eng, self.tr)
        row, col, rel, _ = _entry_table(dadj, real=False)
        self.trip_all = torch.as_tensor(np.stack([row, rel, col], 1), device=dev)
        self.eng, self.params, self.dadj = eng, params, dadj

        def body():
            self.ed.refresh()
            dv, _ = eng.value_grads(params, dadj, self.ed)
            s = torch.cat(dv)
            val, idx = torch.sort(s, descending=True, stable=True)   # == sorted(..., reverse=True)
            self.out_s = val[:self.k]
            self.out_t = self.trip_all[idx[:self.k]]

        self.tr.copy_(torch.zeros(3, dtype=torch.int64))
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):                 # warm-up: workspaces, allocator pools
            body()
        torch.cuda.current_stream(dev).wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            body()

    def run(self, triples):
        n = len(triples)
        dev = self.eng.device
        tr_all = torch.as_tensor(np.asarray(triples, np.int64), device=dev)
        out_t = torch.empty(n, self.k, 3, dtype=torch.int64, device=dev)
        out_s = torch.empty(n, self.k, dtype=torch.float32, device=dev)
        for j in range(n):                            # launches only, no host synchronisation
            self.tr.copy_(tr_all[j])
            self.graph.replay()
            out_t[j].copy_(self.out_t)
            out_s[j].copy_(self.out_s)
        return out_t.cpu().numpy(), out_s.cpu().numpy()


# -- mask explainers -------------------------------------------------------------------------
class MaskAdam:
    """Keras 2.7 Adam on dense mask variables (TF ApplyAdam form, the iddgcn_adam_f32 kernel),
    moments and iteration count persisting across calls like the reference's shared optimizer."""

    def __init__(self, shape, device, learning_rate=1e-3, beta_1=0.9, beta_2=0.999, epsilon=1e-7):
        self.lr, self.b1, self.b2, self.eps = learning_rate, beta_1, beta_2, epsilon
        self.m = torch.zeros(shape, dtype=torch.float32, device=device)
        self.v = torch.zeros(shape, dtype=torch.float32, device=device)
        self.iterations = 0

    def apply(self, var, grad):
        self.iterations += 1
        f = np.float32
        t = f(self.iterations)
        alpha = f(self.lr) * np.sqrt(f(1) - f(self.b2) ** t) / (f(1) - f(self.b1) ** t)
        ops.adam(var, self.m, self.v, grad, alpha, self.b1, self.b2, self.eps, 0)


def structure_loss_grad(values, rel_of_entry, num_relations, target_ratios):
    """IDDGCN_explain.structure_loss (lines 30-41) and its gradient w.r.t. each masked value:
    ratios_r = sum(values of r) / sum(values); loss = mean((target - ratios)^2)."""
    counts = torch.zeros(num_relations, dtype=values.dtype, device=values.device).index_add_(0, rel_of_entry, values)
    total = counts.sum()
    ratios = counts / total
    target = torch.as_tensor(np.asarray(target_ratios), dtype=values.dtype, device=values.device)
    loss = ((target - ratios) ** 2).mean()
    dl_dratio = 2.0 * (ratios - target) / num_relations
    dl_dcount = (dl_dratio - (dl_dratio * ratios).sum()) / total        # d ratio_j / d count_r = (δ_jr - ratio_j)/C
    return loss, dl_dcount[rel_of_entry]


def _select(dadj, mvals, threshold, top_k):
    """Masked values above the threshold, relation by relation (skipping a relation whose kept
    (row, col) indices sum to 0, GnnExplainer.py:56-66), ranked descending, top_k."""
    mv = mvals.detach().cpu().numpy()
    trip, sc = [], []
    for r in range(dadj.num_relations):
        a, b = dadj.rel_offsets[r], dadj.rel_offsets[r + 1]
        keep = mv[a:b] > threshold
        rows, cols = dadj.rows[r][keep], dadj.cols[r][keep]
        if rows.sum() + cols.sum() == 0:
            continue
        trip.append(np.stack([rows, np.full(rows.shape, r, np.int64), cols], 1))
        sc.append(mv[a:b][keep])
    if not trip:
        return np.zeros((0, 3), np.int64), np.zeros((0,), np.float32)
    trip, sc = np.concatenate(trip), np.concatenate(sc)
    order = np.argsort(-sc, kind="stable")[:top_k]
    return trip[order], sc[order]


def mask_explainer(model, adjacency_data, test_triples, *, num_epochs=5, learning_rate=1e-3, threshold=0.2,
                   init_value=None, seed=123, target_ratios=None, top_k=10, optimizer=None, return_masks=False):
    """GNNExplainer.replica_step (GnnExplainer.py:26-74) and, with ``target_ratios``, the IDDGCN
    explainer's wgnnexplainer_step (IDDGCN_explain.py:43-118: loss = (pred_loss + struct_loss)/2).

    Returns (list of [k, 3] triples (head, rel, tail), list of [k] masked scores[, final masked
    values per triple]).  ``optimizer``: a MaskAdam to continue from (one is created otherwise)."""
    eng, params = _model_state(model)
    N, R = model.num_entities, model.num_relations
    dev = eng.device
    if init_value is None:
        init_value = np.random.default_rng(seed).standard_normal((N, N)).astype(np.float32)
    init = torch.as_tensor(np.asarray(init_value, np.float32).reshape(N, N), device=dev)
    masks = init.expand(R, N, N).contiguous()
    opt = optimizer or MaskAdam((R, N, N), dev, learning_rate)
    preds, scores, finals = [], [], []
    for tr in _as_triples(test_triples):
        comp = get_computation_graph(int(tr[0]), int(tr[1]), int(tr[2]), adjacency_data)
        adj_mats = get_adj_mats(comp, N, R)
        dadj = DeviceAdjacency(adj_mats, N, dev)
        rel_of = torch.as_tensor(np.repeat(np.arange(R), dadj.nnz), device=dev)
        flat = torch.as_tensor(np.concatenate([r * N * N + dadj.rows[r] * N + dadj.cols[r] for r in range(R)]),
                               device=dev)
        base = dadj.base_values
        ed = eng.edges(tr[None])
        dadj.set_values(base)
        before = eng.predict(params, dadj, ed)                        # unmasked prediction, constant
        for _ in range(num_epochs):
            sig = torch.sigmoid(masks.view(-1)[flat])
            mvals = base * sig
            dadj.set_values(mvals)
            dv, p = eng.value_grads(params, dadj, ed)                  # d pred / d masked values
            g = torch.cat(dv) * (-before / (p + 1e-5))                  # d(-before log(pred+1e-5))
            if target_ratios is not None:
                _, gs = structure_loss_grad(mvals, rel_of, R, target_ratios)
                g = (g + gs) * 0.5
            grad = torch.zeros(R * N * N, dtype=torch.float32, device=dev)
            grad[flat] = g * base * sig * (1.0 - sig)
            opt.apply(masks.view(-1), grad)
        mvals = base * torch.sigmoid(masks.view(-1)[flat])
        t_, s_ = _select(dadj, mvals, threshold, top_k)
        preds.append(t_)
        scores.append(s_)
        if return_masks:
            finals.append(mvals.cpu().numpy())
        masks.copy_(init.expand(R, N, N))                              # mask.assign(init_value)
    return (preds, scores, finals) if return_masks else (preds, scores)


def gnn_explainer(model, adjacency_data, test_triples, num_epochs=5, learning_rate=1e-3, threshold=0.2, **kw):
    """GnnExplainer.py defaults: 5 epochs, lr 1e-3, threshold 0.2, no structure loss."""
    return mask_explainer(model, adjacency_data, test_triples, num_epochs=num_epochs, learning_rate=learning_rate,
                          threshold=threshold, **kw)


def iddgcn_explainer(model, adjacency_data, test_triples, num_epochs=10, learning_rate=1e-3, threshold=0.15,
                     target_ratios=(0.4, 0.4, 0.1, 0.1), **kw):
    """IDDGCN_explain.py defaults: 10 epochs, lr 1e-3, threshold 0.15, ratios [.4, .4, .1, .1]."""
    if len(target_ratios) != model.num_relations:
        raise IddgcnError("target_ratios needs one entry per relation")
    return mask_explainer(model, adjacency_data, test_triples, num_epochs=num_epochs, learning_rate=learning_rate,
                          threshold=threshold, target_ratios=target_ratios, **kw)


# -- batched mask explainers ---------------------------------------------------------------------
# The computation graph of (h, r, t) is every stored entry whose row or column is h or t: its rows h and t are the
# full graph's rows h and t, and the prediction reads A_r only through AE_r[h] and AE_r[t].  So one epoch of mask
# training needs the triple's candidate entries, their E rows and a few dozen D x D mat-vecs: every epoch of a triple
# runs in one workgroup (ops.mask_explain).  The reference's one shared Adam is kept exactly with sparse state: m, v
# and a "steps applied" count per stored entry of the FULL graph, the moments decayed lazily over the steps an entry
# sat out (the dense optimizer decays them with zero gradients; what it does to masks outside the current
# computation graph is never read, the masks being reset after every triple).  Triples that share an entry run in
# input order, in successive launches (mask_schedule).
ROLE_HEAD, ROLE_TAIL = 1, 2      # candidate role bits: the entry's row is h / is t (0: only its column is h or t)


def _entry_table(dadj, real=True):
    """(row, col, rel, real) of every stored entry of ``dadj`` in entry order (host); real = not the (0,0) = 0
    placeholder of an empty relation (one copy of the values from the device; None with ``real=False``)."""
    row, col = np.concatenate(dadj.rows), np.concatenate(dadj.cols)
    rel = np.repeat(np.arange(dadj.num_relations, dtype=np.int64), dadj.nnz)
    return row, col, rel, (dadj.base_values.cpu().numpy() != 0) if real else None


@contextlib.contextmanager
def _launch_events(stats):
    """Brackets a launch sequence with a pair of recorded device events, left in ``stats["launch_events"]`` (nothing
    when ``stats`` is None)."""
    if stats is None:
        yield
        return
    ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    ev[0].record()
    yield
    ev[1].record()
    stats.update(launch_events=ev)


def _checked_triples(test_triples, R):
    """(n, 3) int64 triples whose relations lie in [0, R)."""
    triples = _as_triples(test_triples)
    if len(triples) and (triples[:, 1].min() < 0 or triples[:, 1].max() >= R):
        raise IddgcnError("triple relation index out of range [0, num_relations)")
    return triples


def _fused_or_layered(model, adjacency_data, test_triples, fused, message):
    """How an explainer with a fused per-query route and a layered one opens: (eng, params, checked triples, the
    resolved ``fused`` — IddgcnError ``message`` when the kernels are demanded outside their envelope —, the device
    adjacency of ``adjacency_data``)."""
    N, R = model.num_entities, model.num_relations
    triples = _checked_triples(test_triples, R)                    # refused before any device work
    eng, params = _model_state(model)
    fused = eng.resolve_fused(fused, eng.per_query_ok(), message)
    return eng, params, triples, fused, DeviceAdjacency(get_adj_mats(adjacency_data, N, R), N, eng.device)


def _note_route(stats, fused, cand, **more):
    """The ``stats`` every such explainer leaves: the route taken and the candidate count."""
    if stats is not None:
        stats.update(fused=bool(fused), candidates=int(len(cand["entry"])), **more)


class _EditedAdjacency:
    """The layered routes' scaffolding: ``base``, the stored values in fp32, of which every variant is an edited clone
    handed to ``dadj.set_values``; ``entry``, the candidates' entry ids on the device; ``edges(q)``, triple q as the
    ScoredEdges Engine.predict / value_grads take; and the stored values back in ``dadj`` on the way out."""

    def __init__(self, eng, dadj, triples, cand):
        self.eng, self.dadj, self.triples = eng, dadj, triples
        self.base = dadj.base_values.to(torch.float32)
        self.entry = torch.as_tensor(cand["entry"].astype(np.int64), device=eng.device)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.dadj.set_values(self.base)

    def edges(self, q):
        return self.eng.edges(self.triples[q][None])


def mask_candidates(dadj, triples):
    """The computation graphs of Q triples as candidate lists over the full adjacency ``dadj`` (a DeviceAdjacency of
    get_adj_mats(adjacency_data), host entry order: relation-major, row-major sorted).  A triple's candidates are the
    distinct stored entries with row in {h, t} or column in {h, t}, in ascending entry id — restricted to the triple
    that is get_adj_mats(get_computation_graph(..))'s order within every relation; the (0,0) = 0 placeholders are no
    candidates (their value and gradient are exactly 0).  Returns (qptr int64 [Q + 1], entry int32, rel int32, col
    int32, role int32): role has ROLE_HEAD set when the entry's row is h (it feeds AE[h]) and ROLE_TAIL when it is t."""
    tr = _as_triples(triples)
    N = dadj.num_entities
    if tr.size and (tr[:, [0, 2]].min() < 0 or tr[:, [0, 2]].max() >= N):
        raise IddgcnError("triple entity index out of range [0, num_entities)")
    row, col, rel, real = _entry_table(dadj)
    ids = np.flatnonzero(real)
    by_row = ids[np.argsort(row[ids], kind="stable")]
    rptr = np.searchsorted(row[by_row], np.arange(N + 1))
    by_col = ids[np.argsort(col[ids], kind="stable")]
    cptr = np.searchsorted(col[by_col], np.arange(N + 1))
    segs, roles = [], []
    for h, _, t in tr:
        nodes = (h,) if h == t else (h, t)
        e = np.unique(np.concatenate([by_row[rptr[n]:rptr[n + 1]] for n in nodes] +
                                     [by_col[cptr[n]:cptr[n + 1]] for n in nodes]))
        segs.append(e)
        roles.append((row[e] == h) * ROLE_HEAD | (row[e] == t) * ROLE_TAIL)
    qptr = np.concatenate([[0], np.cumsum([len(e) for e in segs])]).astype(np.int64)
    entry = np.concatenate(segs).astype(np.int64) if segs else np.zeros(0, np.int64)
    role = np.concatenate(roles) if roles else np.zeros(0, np.int64)
    i32 = np.int32
    return qptr, entry.astype(i32), rel[entry].astype(i32), col[entry].astype(i32), role.astype(i32)


def mask_schedule(qptr, entry, total_nnz, schedule="levels"):
    """The launch level (1-based) of every triple.  The shared optimizer state makes triples whose computation graphs
    share an entry run in input order: greedily, a triple's level is 1 + the highest level of any earlier triple that
    touched one of its entries (1 when there is none).  ``schedule="sequential"``: one triple per level."""
    Q = len(qptr) - 1
    if schedule == "sequential":
        return np.arange(1, Q + 1, dtype=np.int64)
    if schedule != "levels":
        raise ValueError(f"schedule must be 'levels' or 'sequential', got {schedule!r}")
    last = np.zeros(int(total_nnz), np.int64)
    levels = np.zeros(Q, np.int64)
    for q in range(Q):
        e = entry[qptr[q]:qptr[q + 1]]
        levels[q] = 1 + (last[e].max() if len(e) else 0)
        last[e] = levels[q]
    return levels


def mask_adam_alphas(learning_rate, beta_1, beta_2, first, count):
    """MaskAdam.apply's fp32 step size of iterations first .. first + count - 1."""
    f = np.float32
    t = np.arange(first, first + count).astype(f)
    return (f(learning_rate) * np.sqrt(f(1) - f(beta_2) ** t) / (f(1) - f(beta_1) ** t)).astype(f)


def select_candidates(entry, rel, values, row, col, num_relations, threshold, top_k):
    """_select on one triple's candidate list (host): values > threshold, relation by relation (a relation whose kept
    (row, col) indices sum to 0 — nothing kept, or only (0, 0) — is skipped), stable descending, top_k.
    ``row`` / ``col``: the full adjacency's entry table.  Returns ([k, 3] int64 triples, [k] float32 scores)."""
    values = np.asarray(values, np.float32)
    keep = values > threshold
    for r in range(num_relations):
        sel = keep & (rel == r)
        if sel.any() and row[entry[sel]].sum() + col[entry[sel]].sum() == 0:
            keep = keep & ~sel
    e, sc = entry[keep].astype(np.int64), values[keep]
    order = np.argsort(-sc, kind="stable")[:top_k]
    e = e[order]
    return np.stack([row[e], rel[keep][order].astype(np.int64), col[e]], 1).reshape(-1, 3), sc[order]


def masks_layout(rel, values, num_relations):
    """One triple's final masked values in mask_explainer's return_masks layout: per relation in computation-graph
    entry order, a single 0.0 (the placeholder) for a relation that is empty in the computation graph."""
    values = np.asarray(values, np.float32)
    return np.concatenate([values[rel == r] if (rel == r).any() else np.zeros(1, np.float32)
                           for r in range(num_relations)])


def mask_explainer_batched(model, adjacency_data, test_triples, *, num_epochs=5, learning_rate=1e-3, threshold=0.2,
                           init_value=None, seed=123, target_ratios=None, top_k=10, optimizer=None,
                           return_masks=False, schedule="levels", stats=None):
    """mask_explainer with every epoch of a triple in one workgroup and one launch per schedule level
    (ops.mask_explain): the same return contract and the same shared-optimizer semantics.  A ``MaskAdam`` passed in
    seeds the per-entry state from its dense m / v and offsets the step count by its ``iterations``; on return it holds
    what the per-triple path would have left, so the two paths continue each other.  fp32 features, D in {32, 64},
    1 <= R <= 8, unsharded engine: IddgcnError otherwise (use the per-triple mask_explainer).  With ``target_ratios``
    a triple with no candidate makes the reference divide 0 by 0: IddgcnError up front; without, it returns empty
    lists.  ``stats``: an optional dict that receives ``levels``, ``candidates`` and ``launch_events`` (a pair of
    recorded device events around the launches), for tools/bench_explain_masks.py."""
    eng, params = _model_state(model)
    N, R = model.num_entities, model.num_relations
    dev = eng.device
    eng.require_per_query("mask_explainer_batched takes D in {32, 64}, fp32 features, 1 <= R <= 8 and an unsharded "
                          "engine: use the per-triple mask_explainer for this model")
    if target_ratios is not None and len(target_ratios) != R:
        raise IddgcnError("target_ratios needs one entry per relation")
    triples = _checked_triples(test_triples, R)
    Q = len(triples)
    if init_value is None:
        init_value = np.random.default_rng(seed).standard_normal((N, N)).astype(np.float32)
    init = np.asarray(init_value, np.float32).reshape(N, N)
    dadj = DeviceAdjacency(get_adj_mats(adjacency_data, N, R), N, dev)
    total = dadj.total_nnz
    qptr, entry, crel, ccol, crole = mask_candidates(dadj, triples)
    if target_ratios is not None and Q and (np.diff(qptr) == 0).any():
        bad = triples[np.flatnonzero(np.diff(qptr) == 0)[0]]
        raise IddgcnError(f"triple {tuple(int(x) for x in bad)} has no entry in its computation graph: the "
                          "relation-ratio loss divides 0 by 0 there")
    levels = mask_schedule(qptr, entry, total, schedule)
    n_levels = int(levels.max()) if Q else 0
    order = np.argsort(levels, kind="stable")
    level_ptr = np.concatenate([[0], np.cumsum(np.bincount(levels, minlength=n_levels + 1)[1:])])
    row, col, rel_all, _ = _entry_table(dadj, real=False)
    g = eng.to_device
    if optimizer is None:
        lr, b1, b2, eps, it0 = learning_rate, 0.9, 0.999, 1e-7, 0
        m = torch.zeros(total, dtype=torch.float32, device=dev)
        v = torch.zeros(total, dtype=torch.float32, device=dev)
    else:
        lr, b1, b2, eps, it0 = optimizer.lr, optimizer.b1, optimizer.b2, optimizer.eps, optimizer.iterations
        if tuple(optimizer.m.shape) != (R, N, N):
            raise IddgcnError(f"optimizer state must be {(R, N, N)}, got {tuple(optimizer.m.shape)}")
        flat = g(rel_all * N * N + row * N + col, np.int64)
        m, v = optimizer.m.view(-1)[flat].contiguous(), optimizer.v.view(-1)[flat].contiguous()
    steps = torch.zeros(total, dtype=torch.int32, device=dev)
    n_steps = Q * num_epochs
    alpha = g(mask_adam_alphas(lr, b1, b2, it0 + 1, n_steps), np.float32)
    out = torch.empty(len(entry), dtype=torch.float32, device=dev)
    d_qptr, d_entry = g(qptr, np.int64), g(entry)
    if Q:
        eng.finish_pending()
        with _launch_events(stats), eng._mark("mask_explain"):
            ops.mask_explain(params["E"], *layer_tuples(params), params["rel"], g(triples[:, 0]), g(triples[:, 1]),
                             g(triples[:, 2]), d_qptr, d_entry, g(crel), g(ccol), g(crole),
                             g(init[row, col], np.float32), m, v, steps, alpha, out, g(order), level_ptr, num_epochs,
                             0, b1, b2, eps, None if target_ratios is None else g(target_ratios, np.float32))
    if stats is not None:
        stats.update(levels=n_levels, candidates=int(len(entry)))
    if optimizer is not None:
        # what the dense optimizer holds after n_steps more steps: every moment decayed, the touched entries'
        # (decayed from their last step to the end) scattered back
        f32 = lambda x: torch.tensor(float(np.float32(x)), dtype=torch.float32, device=dev)  # noqa: E731
        gap = (n_steps - steps).to(torch.float32)
        optimizer.m.mul_(float(np.float32(b1)) ** n_steps)
        optimizer.v.mul_(float(np.float32(b2)) ** n_steps)
        optimizer.m.view(-1)[flat] = m * torch.pow(f32(b1), gap)
        optimizer.v.view(-1)[flat] = v * torch.pow(f32(b2), gap)
        optimizer.iterations = it0 + n_steps

    preds, scores, finals = [], [], []
    k = int(top_k)
    entry64 = entry.astype(np.int64)
    if Q and len(entry) and 1 <= k <= TOPK_MAX:
        # the selection on the device: drop what the threshold or the (0,0)-only rule rejects, then the segment top-k
        q_of = np.repeat(np.arange(Q), np.diff(qptr))
        seg = g(q_of * R + crel, np.int64)
        kept = out > threshold
        n_kept = torch.bincount(seg[kept], minlength=Q * R)
        is00 = g((row[entry64] == 0) & (col[entry64] == 0), np.bool_)
        score = torch.where(kept & ~(is00 & (n_kept[seg] == 1)), out, torch.full_like(out, -np.inf))
        te, tv, _ = ops.explain_topk(d_qptr, d_entry, score, k)
        te, tv = te.cpu().numpy().astype(np.int64), tv.cpu().numpy()
        for q in range(Q):
            ok = tv[q] > -np.inf
            e = te[q][ok]
            preds.append(np.stack([row[e], rel_all[e], col[e]], 1).reshape(-1, 3))
            scores.append(tv[q][ok])
        vals = out.cpu().numpy() if return_masks else None
    else:
        vals = out.cpu().numpy()
        for q in range(Q):
            a, b = qptr[q], qptr[q + 1]
            p_, s_ = select_candidates(entry64[a:b], crel[a:b], vals[a:b], row, col, R, threshold, max(k, 0))
            preds.append(p_)
            scores.append(s_)
    if return_masks:
        finals = [masks_layout(crel[qptr[q]:qptr[q + 1]], vals[qptr[q]:qptr[q + 1]], R) for q in range(Q)]
    return (preds, scores, finals) if return_masks else (preds, scores)


def gnn_explainer_batched(model, adjacency_data, test_triples, num_epochs=5, learning_rate=1e-3, threshold=0.2, **kw):
    """gnn_explainer's defaults on the batched path."""
    return mask_explainer_batched(model, adjacency_data, test_triples, num_epochs=num_epochs,
                                  learning_rate=learning_rate, threshold=threshold, **kw)


def iddgcn_explainer_batched(model, adjacency_data, test_triples, num_epochs=10, learning_rate=1e-3, threshold=0.15,
                             target_ratios=(0.4, 0.4, 0.1, 0.1), **kw):
    """iddgcn_explainer's defaults on the batched path."""
    if len(target_ratios) != model.num_relations:
        raise IddgcnError("target_ratios needs one entry per relation")
    return mask_explainer_batched(model, adjacency_data, test_triples, num_epochs=num_epochs,
                                  learning_rate=learning_rate, threshold=threshold, target_ratios=target_ratios, **kw)


# -- fidelity: deletion and insertion curves -------------------------------------------------------
# Do the edges an explanation names drive the prediction?  deletion[q, j]: the probability of triple q with the first
# j explanation edges removed from the adjacency; insertion[q, j]: with ONLY those edges left in rows h and t.  A
# variant edits rows h and t alone, and the prediction reads A_r only through AE_r[h] and AE_r[t], so all 2 (K + 1)
# variants of a triple are pairs of edited rows pushed through the three layers (Engine.edit_curves, one workgroup per
# tile of variants); no ground-truth file is involved.
def _padded_explanations(preds, n):
    """(n, K, 3) int64 with -1 rows past a short list's end, from an (n, K, 3) array or a list of (k_i, 3) arrays."""
    if isinstance(preds, np.ndarray) and preds.ndim == 3:
        out = preds.astype(np.int64)
    else:
        lists = [np.asarray(p, np.int64).reshape(-1, 3) for p in preds]
        out = np.full((len(lists), max((len(p) for p in lists), default=1), 3), -1, np.int64)
        for j, p in enumerate(lists):
            out[j, :len(p)] = p
    if out.shape[0] != n or out.shape[2] != 3:
        raise IddgcnError(f"preds must hold one (k, 3) explanation per triple ({n}), got {out.shape}")
    if not 1 <= out.shape[1] <= TOPK_MAX:
        raise IddgcnError(f"explanations must have between 1 and {TOPK_MAX} edges, got {out.shape[1]}")
    return out


def _row_candidates(dadj, triples):
    """mask_candidates restricted to role != 0 (the entry's row is h or t) and each candidate's stored value, as the
    candidate table's common part — ``qptr`` (n + 1,) int64; ``entry``, ``rel``, ``col``, ``role`` int32; ``val`` fp32 —
    and the query of every candidate (int64)."""
    qptr, entry, crel, ccol, crole = mask_candidates(dadj, triples)
    keep = crole != 0
    q_of = np.repeat(np.arange(len(qptr) - 1), np.diff(qptr))[keep]
    qptr = np.concatenate([[0], np.cumsum(np.bincount(q_of, minlength=len(qptr) - 1))]).astype(np.int64)
    entry = entry[keep]
    val = dadj.base_values.cpu().numpy().astype(np.float32)[entry]
    i32 = lambda a: a.astype(np.int32, copy=False)  # noqa: E731
    return dict(qptr=qptr, entry=i32(entry), rel=i32(crel[keep]), col=i32(ccol[keep]), role=i32(crole[keep]),
                val=val), q_of


def curve_steps(dadj, triples, preds, undirected=False):
    """The candidates of each triple's deletion / insertion curves and the step at which each one flips (host).

    A triple's candidates are the stored, non-placeholder entries of ``dadj`` whose row is h or t (mask_candidates
    with role != 0, same order).  Explanation edge j = (i, rel, c) names the stored entry (row i, col c) of ``rel``;
    the candidate it names gets ``step`` j unless an earlier edge named it.  An edge that names no candidate of its
    triple (not stored, only its column is h or t, a duplicate, padding) is inert.  ``undirected``: edge j also flips
    the entry (c, rel, i) when that is a candidate.  Returns a dict of host arrays: ``qptr`` (n + 1,) int64; per
    candidate ``entry``, ``rel``, ``col``, ``role``, ``step`` (int32; -1: never flips) and ``val`` (fp32);
    ``effective`` (n, K) bool: edge j flipped at least one candidate; ``K``."""
    tr = _as_triples(triples)
    n, N, total = len(tr), dadj.num_entities, dadj.total_nnz
    ex = _padded_explanations(preds, n)
    K = ex.shape[1]
    cand, q_of = _row_candidates(dadj, tr)
    entry = cand["entry"]
    # stored (rel, row, col) -> entry id, through one sorted 64-bit key
    row, col, rel, real = _entry_table(dadj)
    ids = np.flatnonzero(real)
    key = (rel[ids] * N + row[ids]) * N + col[ids]
    order = np.argsort(key, kind="stable")
    key, ids = key[order], ids[order]
    # (triple, entry id) -> candidate index: the candidate lists ascend by (triple, entry)
    ckey = q_of.astype(np.int64) * total + entry
    step = np.full(len(entry), K, np.int64)
    e_i, e_r, e_c = ex[:, :, 0], ex[:, :, 1], ex[:, :, 2]
    ok = (e_i >= 0) & (e_i < N) & (e_c >= 0) & (e_c < N) & (e_r >= 0) & (e_r < dadj.num_relations)
    qq, jj = np.nonzero(ok)
    for a, b in ((e_i, e_c), (e_c, e_i)) if undirected else ((e_i, e_c),):
        want = (e_r[qq, jj] * N + a[qq, jj]) * N + b[qq, jj]
        at = np.minimum(np.searchsorted(key, want), max(len(key) - 1, 0))
        stored = key[at] == want if len(key) else np.zeros(len(want), bool)
        wantc = qq[stored] * total + ids[at[stored]]
        atc = np.minimum(np.searchsorted(ckey, wantc), max(len(ckey) - 1, 0))
        hit = ckey[atc] == wantc if len(ckey) else np.zeros(len(wantc), bool)
        np.minimum.at(step, atc[hit], jj[stored][hit])
    step[step == K] = -1
    effective = np.zeros((n, K), bool)
    effective[q_of[step >= 0], step[step >= 0]] = True
    return dict(cand, step=step.astype(np.int32), effective=effective, K=K)


def _curves_layered(eng, params, dadj, triples, cand, K):
    """One set_values + Engine.predict per variant (any width and mode): the route a user had before the fused kernel,
    its cross-check and its timing baseline."""
    dev = eng.device
    n = len(triples)
    out = torch.empty(2, n, K + 1, dtype=torch.float32, device=dev)
    qp = cand["qptr"]
    step = torch.as_tensor(cand["step"].astype(np.int64), device=dev)
    val = torch.as_tensor(cand["val"], device=dev)
    with _EditedAdjacency(eng, dadj, triples, cand) as adj:
        for q in range(n):
            ed = adj.edges(q)
            e, st, v = (x[qp[q]:qp[q + 1]] for x in (adj.entry, step, val))
            zero = torch.zeros_like(v)
            for j in range(K + 1):
                flipped = (st >= 0) & (st < j)
                for which, keep in ((0, ~flipped), (1, flipped)):
                    vals = adj.base.clone()
                    vals[e] = torch.where(keep, v, zero)
                    dadj.set_values(vals)
                    out[which, q, j] = eng.predict(params, dadj, ed)[0]
    return out[0], out[1]


def fidelity_curves(model, adjacency_data, test_triples, preds, *, undirected=False, fused=None, stats=None):
    """Deletion and insertion curves of one ranked explanation per test triple.

    ``preds``: an (n, K, 3) array or a list of (k_i, 3) arrays of (head, rel, tail) edges, best first, as the
    explainers return them (K = the longest list, 1 <= K <= 64; a short list is padded with inert steps).
    deletion[q, j] is the model's probability for triple q with the candidates named by its first j edges set to 0,
    insertion[q, j] the probability with only those kept and every other stored entry of rows h and t set to 0
    (curve_steps has the exact rules); deletion[:, 0] is the unedited prediction.

    ``fused``: None picks the fused kernel (Engine.edit_curves) for fp32 features, D in {32, 64}, R <= 8 and an
    unsharded engine; False runs one set_values + predict per variant on the layered kernels (any width); True
    demands the kernel (IddgcnError outside its envelope).  ``stats``: an optional dict that receives ``fused``,
    ``candidates`` and, on the fused route, ``launch_events`` (a pair of recorded device events around the launches).
    Returns a dict of numpy arrays: ``p`` (n,), ``deletion`` (n, K + 1), ``insertion`` (n, K + 1), ``effective``
    (n, K) bool."""
    eng, params, triples, fused, dadj = _fused_or_layered(
        model, adjacency_data, test_triples, fused,
        "fidelity_curves: the fused kernel takes D in {32, 64}, fp32 features, 1 <= R <= 8 and an unsharded engine: "
        "use fused=False for this model")
    cand = curve_steps(dadj, triples, preds, undirected)
    K = cand["K"]
    if fused:
        with _launch_events(stats):
            dele, ins = eng.edit_curves(params, dadj, triples, cand, K)
    else:
        dele, ins = _curves_layered(eng, params, dadj, triples, cand, K)
    _note_route(stats, fused, cand)
    dele, ins = dele.cpu().numpy(), ins.cpu().numpy()
    return dict(p=dele[:, 0].copy(), deletion=dele, insertion=ins, effective=cand["effective"])


def fidelity_summary(curves):
    """Per-triple and mean fidelity of fidelity_curves' result (host).  fidelity_plus = p - deletion[:, K]: the drop
    when the whole explanation is deleted (larger: the edges matter); fidelity_minus = p - insertion[:, K]: what is
    lost when only the explanation is kept (smaller: the edges suffice); deletion_auc / insertion_auc: the trapezoid
    area under each curve over j / K; effective_share: the share of explanation edges that flipped a candidate.
    Returns a dict: the four per-triple (n,) float64 arrays, ``effective_share`` and ``mean`` (a dict of their
    means)."""
    p = np.asarray(curves["p"], np.float64)
    dele, ins = np.asarray(curves["deletion"], np.float64), np.asarray(curves["insertion"], np.float64)
    K = dele.shape[1] - 1
    if K < 1 or ins.shape != dele.shape or p.shape != dele.shape[:1]:
        raise ValueError(f"curves must hold p (n,) and deletion / insertion (n, K + 1), got {p.shape}, {dele.shape}, "
                         f"{ins.shape}")
    auc = lambda y: (y[:, :-1] + y[:, 1:]).sum(1) / (2.0 * K)  # noqa: E731
    eff = np.asarray(curves["effective"], bool)
    out = dict(fidelity_plus=p - dele[:, K], fidelity_minus=p - ins[:, K], deletion_auc=auc(dele),
               insertion_auc=auc(ins), effective_share=float(eff.mean()) if eff.size else 0.0)
    out["mean"] = {k: float(v.mean()) if len(v) else 0.0 for k, v in out.items() if isinstance(v, np.ndarray)}
    return out


def random_explanations(dadj, triples, k, seed=0):
    """The baseline beside every fidelity number: per triple, k stored entries drawn without replacement from its
    candidate rows (the entries whose row is h or t), uniformly, as (head, rel, tail) edges.  Returns a list of
    (min(k, candidates), 3) int64 arrays; seeded (numpy default_rng)."""
    tr = _as_triples(triples)
    k = int(k)
    if k < 1:
        raise ValueError(f"k must be positive, got {k}")
    cand, q_of = _row_candidates(dadj, tr)
    qptr, entry = cand["qptr"], cand["entry"]
    row = _entry_table(dadj, real=False)[0]
    draw = np.random.default_rng(seed).random(len(entry))
    order = np.lexsort((draw, q_of))                                # a random order inside every triple's segment
    edges = np.stack([row[entry], cand["rel"].astype(np.int64), cand["col"].astype(np.int64)], 1)[order]
    return [edges[qptr[q]:min(qptr[q] + k, qptr[q + 1])] for q in range(len(tr))]


# -- counterfactual edge sets and occlusion scores ---------------------------------------------------
# Which few edges, if they were not in the graph, would change this call?  The deterministic answer to the question
# the deletion curve measures: remove the most damaging candidate, re-evaluate, repeat until the prediction crosses
# the threshold (include/iddgcn_explain.h has the exact rules).  Step 0's table is the exact leave-one-out change of
# the probability for every edge the prediction can see (occlusion_batched).  Every p(F) is the deletion forward of
# fidelity_curves, bit for bit, so a returned edge list's deletion curve IS the search's path.
def counterfactual_candidates(dadj, triples, undirected=False, exclude_target=False, relations=None):
    """curve_steps' candidates of each triple with the search's two per-candidate rules (host).

    ``partner``: with ``undirected``, candidate (i, rel, c) and candidate (c, rel, i) of the same triple are removed
    together — the segment-relative index of the other one, -1 when there is none (always when i == c); both are
    candidates only when i and c both lie in {h, t}.  ``eligible``: False for the entries (h, r, t) / (t, r, h) with
    ``exclude_target`` and for every relation outside ``relations`` (None: all) — such a candidate stays in the graph
    and is never evaluated.  Returns a dict of host arrays: ``qptr`` (n + 1,) int64; per candidate ``entry``, ``rel``,
    ``col``, ``role``, ``row``, ``partner`` (int32), ``val`` (fp32) and ``eligible`` (bool)."""
    tr = _as_triples(triples)
    n, N, R = len(tr), dadj.num_entities, dadj.num_relations
    cand, q_of = _row_candidates(dadj, tr)
    qptr, crel, ccol = cand["qptr"], cand["rel"], cand["col"]
    crow = _entry_table(dadj, real=False)[0][cand["entry"]]
    C = len(crow)
    within = np.arange(C) - qptr[:-1][q_of]
    partner = np.full(C, -1, np.int64)
    if undirected and C:
        # (triple, rel, row, col) -> candidate: the lists ascend by (triple, entry id) = (triple, rel, row, col)
        key = ((q_of * R + crel) * N + crow) * N + ccol
        want = ((q_of * R + crel) * N + ccol) * N + crow
        at = np.minimum(np.searchsorted(key, want), C - 1)
        hit = (key[at] == want) & (at != np.arange(C))
        partner[hit] = within[at[hit]]
    eligible = np.ones(C, bool)
    if exclude_target and C:
        h, r, t = (tr[q_of, c] for c in range(3))
        eligible &= ~((crel == r) & (((crow == h) & (ccol == t)) | ((crow == t) & (ccol == h))))
    if relations is not None:
        rels = np.asarray(list(relations), np.int64).reshape(-1)
        if len(rels) and (rels.min() < 0 or rels.max() >= R):
            raise IddgcnError("relations: index out of range [0, num_relations)")
        eligible &= np.isin(crel, rels)
    return dict(cand, row=crow.astype(np.int32), partner=partner.astype(np.int32), eligible=eligible)


def _lowering(p0, toward, threshold):
    """The search's direction per triple from the unedited fp32 probabilities: True lowers p, False raises it."""
    if toward not in ops.CF_MODES:
        raise IddgcnError(f"toward must be 'flip', 'lower' or 'raise', got {toward!r}")
    p0 = np.asarray(p0, np.float32)
    if toward == "flip":
        return p0 > np.float32(threshold)
    return np.full(p0.shape, toward == "lower")


def _counterfactual_layered(eng, params, dadj, triples, cand, K, toward, threshold):
    """The search with one set_values + Engine.predict per evaluated variant and the kernels' rules on the host (any
    width and mode): the fused route's cross-check and its timing baseline.  Host arrays, counterfactual_search's
    keys."""
    n, qp, thr = len(triples), cand["qptr"], np.float32(threshold)
    C = len(cand["entry"])
    out = dict(path=np.zeros((n, K + 1), np.float32), chosen=np.full((n, K), -1, np.int32),
               n_steps=np.zeros(n, np.int32), flipped=np.zeros(n, np.int32), cstep=np.full(C, -1, np.int32),
               loo=np.full(C, np.nan, np.float32))
    with _EditedAdjacency(eng, dadj, triples, cand) as adj:
        for q in range(n):
            ed = adj.edges(q)
            a, b = int(qp[q]), int(qp[q + 1])
            e, part, elig = adj.entry[a:b], cand["partner"][a:b], cand["eligible"][a:b]
            gone = np.zeros(b - a, bool)

            def p_without(extra):
                drop = gone.copy()
                drop[list(extra)] = True
                vals = adj.base.clone()
                vals[e[torch.as_tensor(np.flatnonzero(drop), device=eng.device)]] = 0
                dadj.set_values(vals)
                return np.float32(eng.predict(params, dadj, ed)[0].item())

            p = p_without(())
            out["path"][q] = p
            lower = bool(_lowering(p, toward, threshold))
            crossed = lambda v: (not v > thr) if lower else bool(v > thr)  # noqa: E731
            with_partner = lambda j: [j] + ([part[j]] if part[j] >= 0 else [])  # noqa: E731
            live = np.flatnonzero(elig)
            pj = np.array([p_without(with_partner(j)) for j in live], np.float32)
            out["loo"][a + live] = pj
            for i in range(K):
                if crossed(p) or not len(live):
                    break
                if i > 0:
                    pj = np.array([p_without(with_partner(j)) for j in live], np.float32)
                best = int(np.lexsort((live, pj if lower else -pj))[0])
                j, p = int(live[best]), pj[best]
                gone[with_partner(j)] = True
                out["cstep"][a + np.flatnonzero(gone & (out["cstep"][a:b] < 0))] = i
                out["chosen"][q, i], out["path"][q, i + 1:], out["n_steps"][q] = j, p, i + 1
                live = np.flatnonzero(elig & ~gone)
            out["flipped"][q] = crossed(p)
    return out


def _counterfactual_run(model, adjacency_data, test_triples, K, toward, threshold, undirected, exclude_target,
                        relations, fused, stats):
    """The shared body of counterfactual_batched and occlusion_batched: (triples, dadj, cand, result, fused, eng)."""
    if not 0 <= K <= TOPK_MAX:
        raise IddgcnError(f"the search takes between 0 and {TOPK_MAX} steps, got {K}")
    _lowering(0.0, toward, threshold)
    eng, params, triples, fused, dadj = _fused_or_layered(
        model, adjacency_data, test_triples, fused,
        "counterfactual search: the fused kernels take D in {32, 64}, fp32 features, 1 <= R <= 8 and an unsharded "
        "engine: use fused=False for this model")
    cand = counterfactual_candidates(dadj, triples, undirected, exclude_target, relations)
    if fused:
        with _launch_events(stats):
            res = eng.counterfactual_search(params, dadj, triples, cand, K, toward, threshold)
    else:
        res = _counterfactual_layered(eng, params, dadj, triples, cand, K, toward, threshold)
    _note_route(stats, fused, cand)
    return triples, dadj, cand, res, fused, eng


def _candidate_edges(cand):
    return np.stack([cand["row"], cand["rel"], cand["col"]], 1).astype(np.int64)


def counterfactual_batched(model, adjacency_data, test_triples, max_edges=10, *, toward="flip", threshold=0.5,
                           undirected=False, exclude_target=False, relations=None, fused=None,
                           return_occlusion=False, stats=None):
    """Per test triple, a small set of stored edges whose removal moves the prediction across ``threshold``, found by
    greedy deletion: at every step each remaining eligible candidate (counterfactual_candidates) is removed in turn on
    top of those already gone, and the one that leaves the smallest probability (largest when raising; equal values:
    the lowest entry id) goes — even when nothing improves.  The search stops when the prediction has crossed the
    threshold (a triple already on the target side takes no step), after ``max_edges`` steps (0 .. 64) or when no
    eligible candidate is left.  No random numbers; every probability is fidelity_curves' deletion forward bit for bit.

    ``toward``: "flip" lowers p where p > threshold and raises it elsewhere; "lower" / "raise" fix the direction.
    ``undirected``: an edge between h and t goes together with its stored reverse, as one step.  ``exclude_target``:
    never remove (h, r, t) / (t, r, h) themselves; ``relations``: only remove edges of these relations.  ``fused``:
    None takes the kernels (Engine.counterfactual_search) for fp32 features, D in {32, 64}, R <= 8 and an unsharded
    engine; False runs one set_values + predict per evaluated variant (any width); True demands the kernels.
    ``stats``: an optional dict that receives ``fused``, ``candidates`` and, fused, ``launch_events``.

    Returns a dict: ``p`` (n,) the unedited predictions; ``direction`` (n,) +1 where the search lowers p, -1 where it
    raises it; ``edges``: a list of (n_edges[q], 3) int64 (head, rel, tail) arrays in removal order, ready for
    fidelity_curves (same ``undirected``) and evaluate_explanations; ``path`` (n, max_edges + 1): the probability after
    0, 1, .. removals, repeating its last value past the end — the deletion curve of ``edges``; ``chosen``
    (n, max_edges) the candidate index of each step, -1 padded; ``n_edges`` (n,); ``flipped`` (n,) bool; with
    ``return_occlusion``, ``occlusion``: a list of (candidates, 3) edge arrays and a list of the probabilities with
    each one removed alone (NaN: not eligible), per triple."""
    K = int(max_edges)
    triples, dadj, cand, res, fused, eng = _counterfactual_run(model, adjacency_data, test_triples, K, toward,
                                                               threshold, undirected, exclude_target, relations,
                                                               fused, stats)
    res = {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in res.items()}
    qp, edges_of = cand["qptr"], _candidate_edges(cand)
    n_steps = res["n_steps"].astype(np.int64)
    out = dict(p=res["path"][:, 0].copy(),
               direction=np.where(_lowering(res["path"][:, 0], toward, threshold), 1, -1).astype(np.int64),
               edges=[edges_of[qp[q] + res["chosen"][q, :n_steps[q]].astype(np.int64)] for q in range(len(triples))],
               path=res["path"], chosen=res["chosen"], n_edges=n_steps, flipped=res["flipped"].astype(bool))
    if return_occlusion:
        out["occlusion"] = ([edges_of[qp[q]:qp[q + 1]] for q in range(len(triples))],
                            [res["loo"][qp[q]:qp[q + 1]] for q in range(len(triples))])
    return out


def occlusion_batched(model, adjacency_data, test_triples, top_k=10, *, toward="flip", threshold=0.5,
                      undirected=False, exclude_target=False, relations=None, fused=None, stats=None):
    """Occlusion scores as an explainer: per test triple the ``top_k`` (1 .. 64) eligible candidates whose removal
    alone moves the prediction most in the search's direction.  The score of candidate j is p - p(without j) when
    lowering and its negative when raising — exact, one edited forward per candidate; descending, ties by ascending
    entry id (ops.explain_topk on the fused route).  The selection keywords are counterfactual_batched's.  Returns the
    explainers' (list of (k_q, 3) int64 (head, rel, tail) arrays, list of (k_q,) fp32 scores), k_q = min(top_k,
    eligible candidates)."""
    k = int(top_k)
    if not 1 <= k <= TOPK_MAX:
        raise IddgcnError(f"top_k must be in [1, {TOPK_MAX}], got {top_k}")
    triples, dadj, cand, res, fused, eng = _counterfactual_run(model, adjacency_data, test_triples, 0, toward,
                                                               threshold, undirected, exclude_target, relations,
                                                               fused, stats)
    n = len(triples)
    q_of = np.repeat(np.arange(n), np.diff(cand["qptr"]))
    p0 = res["path"][:, 0]
    if fused:                                                      # the scores stay on the device
        dev = eng.device
        sign = torch.as_tensor(np.where(_lowering(p0.cpu().numpy(), toward, threshold), 1.0, -1.0).astype(np.float32),
                               device=dev)
        qd = torch.as_tensor(q_of, device=dev)
        score = torch.where(torch.as_tensor(cand["eligible"], device=dev), sign[qd] * (p0[qd] - res["loo"]),
                            torch.full_like(res["loo"], -np.inf))
    else:
        sign = np.where(_lowering(p0, toward, threshold), 1.0, -1.0).astype(np.float32)
        score = np.where(cand["eligible"], sign[q_of] * (p0[q_of] - res["loo"]), -np.inf).astype(np.float32)
    return _rank_candidates(eng, dadj, cand, n, score, k, mark="occlusion_topk")


def counterfactual_summary(result):
    """What a batch of searches found (host), from counterfactual_batched's dict: ``flip_rate``; ``mean_size`` and
    ``median_size`` of the sets that flipped their prediction (0.0 when none did); ``mean_shift`` = the mean
    |p - path[:, -1]|; ``relation_share``: the share of the removed edges per relation ({} when nothing was removed);
    ``n``."""
    p = np.asarray(result["p"], np.float64)
    path = np.asarray(result["path"], np.float64)
    flipped = np.asarray(result["flipped"], bool)
    size = np.asarray(result["n_edges"], np.int64)
    if path.ndim != 2 or not (len(p) == len(path) == len(flipped) == len(size) == len(result["edges"])):
        raise ValueError("result must be counterfactual_batched's dict")
    sets = size[flipped]
    rels = np.concatenate([np.asarray(e, np.int64).reshape(-1, 3)[:, 1] for e in result["edges"]] +
                          [np.zeros(0, np.int64)])
    ids, counts = np.unique(rels, return_counts=True)
    return dict(n=len(p), flip_rate=float(flipped.mean()) if len(p) else 0.0,
                mean_size=float(sets.mean()) if len(sets) else 0.0,
                median_size=float(np.median(sets)) if len(sets) else 0.0,
                mean_shift=float(np.abs(p - path[:, -1]).mean()) if len(p) else 0.0,
                relation_share={int(r): float(c) / len(rels) for r, c in zip(ids, counts)})


# -- integrated gradients: additive edge attributions ------------------------------------------------
# How much of this prediction does each edge carry?  Signed scores that add up to p(graph) - p(baseline), the baseline
# being the graph without the triple's eligible candidates: attr_j = val_j * integral over alpha in [0, 1] of
# d p / d a_j along a_j = alpha val_j (include/iddgcn_explain.h has the exact rules).  Deterministic; the completeness
# gap sum_j attr_j - (p - p_baseline) is returned with every call and measures the quadrature's error.  The bundled
# weights saturate, so p(alpha) is close to a step: the default rule is Gauss-Legendre, which needs far fewer nodes
# than the textbook midpoint sum there (DESIGN.md has the table).
def quadrature_rule(steps, quadrature="gauss"):
    """The nodes and weights (float64, (steps,) each) of a rule on [0, 1]: "gauss" (Gauss-Legendre, exact for
    polynomials of degree 2 steps - 1) or "midpoint".  The weights sum to 1, the nodes lie inside (0, 1)."""
    m = int(steps)
    if not 1 <= m <= PATH_MAX_STEPS:
        raise IddgcnError(f"steps must be in [1, {PATH_MAX_STEPS}], got {steps}")
    if quadrature == "gauss":
        x, w = np.polynomial.legendre.leggauss(m)
        return 0.5 * (x + 1.0), 0.5 * w
    if quadrature == "midpoint":
        return (np.arange(m) + 0.5) / m, np.full(m, 1.0 / m)
    raise IddgcnError(f"quadrature must be 'gauss' or 'midpoint', got {quadrature!r}")


def _candidate_subset(cand, idx):
    """The candidate dict of the queries ``idx`` (in that order) and the places of its candidates in the full arrays."""
    qp = np.asarray(cand["qptr"], np.int64)
    idx = np.asarray(idx, np.int64)
    lens = qp[idx + 1] - qp[idx]
    sub_qp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    pos = np.repeat(qp[idx] - sub_qp[:-1], lens) + np.arange(sub_qp[-1])
    sub = {k: (np.asarray(v)[pos] if k != "qptr" else sub_qp) for k, v in cand.items()}
    return sub, pos


def _refine_by_gap(run, cand, n, steps, quadrature, tol, max_steps):
    """The ``tol`` schedule: every triple with the m-node rule, then the triples whose |gap| > tol again with twice
    the nodes, until they pass or the next rule would exceed ``max_steps``; one host read of gap per round.
    ``run(idx, sub_cand, alpha, omega)`` returns the tensors attr / total / p_full / p_base / gap of the queries
    ``idx``.  Returns (dict of tensors over all queries, steps_used (n,) int64, rounds)."""
    m = int(steps)
    idx = np.arange(n)
    out, used, rounds = None, np.full(n, m, np.int64), 0
    while True:
        sub, pos = (cand, None) if out is None else _candidate_subset(cand, idx)
        res = run(idx, sub, *quadrature_rule(m, quadrature))
        rounds += 1
        if out is None:
            out = res
        else:
            at = torch.as_tensor(idx, device=res["gap"].device)
            out["attr"][torch.as_tensor(pos, device=res["attr"].device)] = res["attr"]
            for nm in ("total", "p_full", "p_base", "gap"):
                out[nm][at] = res[nm]
        used[idx] = m
        if tol is None or 2 * m > int(max_steps) or not len(idx):
            break
        bad = np.abs(res["gap"].cpu().numpy().astype(np.float64)) > float(tol)
        idx, m = idx[bad], 2 * m
        if not len(idx):
            break
    return out, used, rounds


def _path_layered(eng, params, dadj, triples, cand, alpha, omega):
    """The path one node at a time on the layered kernels (any width and mode): per (triple, node) one set_values and
    Engine.value_grads, Engine.predict for the two end points.  The fused route's cross-check; device tensors."""
    dev = eng.device
    n, qp = len(triples), cand["qptr"]
    val = torch.as_tensor(cand["val"], device=dev)
    elig = torch.as_tensor(np.asarray(cand["eligible"], bool), device=dev)
    attr = torch.zeros(len(cand["entry"]), dtype=torch.float64, device=dev)
    ends = torch.empty(2, n, dtype=torch.float32, device=dev)
    with _EditedAdjacency(eng, dadj, triples, cand) as adj:
        for q in range(n):
            ed = adj.edges(q)
            sl = slice(int(qp[q]), int(qp[q + 1]))
            e, v, el = adj.entry[sl], val[sl], elig[sl]
            for i, a in enumerate((0.0, 1.0)):
                vals = adj.base.clone()
                vals[e] = torch.where(el, v * a, v)
                dadj.set_values(vals)
                ends[i, q] = eng.predict(params, dadj, ed)[0]
            for a, w in zip(alpha, omega):
                vals = adj.base.clone()
                vals[e] = torch.where(el, v * float(np.float32(a)), v)
                dadj.set_values(vals)
                dv, _ = eng.value_grads(params, dadj, ed)
                attr[sl] += float(np.float32(w)) * torch.cat(dv)[e].double()
    attr = torch.where(elig, attr * val.double(), torch.zeros_like(attr))
    q_of = torch.as_tensor(np.repeat(np.arange(n), np.diff(qp)), device=dev)
    total = torch.zeros(n, dtype=torch.float64, device=dev).index_add_(0, q_of, attr)
    gap = total - (ends[1].double() - ends[0].double())
    return dict(attr=attr.float(), total=total.float(), p_full=ends[1], p_base=ends[0], gap=gap.float())


def _rank_candidates(eng, dadj, cand, n, score, k, mark="attribution_topk"):
    """occlusion_batched's ranking of per-candidate scores (-inf: not ranked): descending, ties by ascending entry id,
    k_q = min(k, finite scores).  A device tensor is ranked by ops.explain_topk (a launch marked ``mark``), a host
    array on the host.  Returns (list of (k_q, 3) int64 edge arrays, list of (k_q,) fp32 scores)."""
    qp, edges_of = cand["qptr"], _candidate_edges(cand)
    q_of = np.repeat(np.arange(n), np.diff(qp))
    preds, scores = [], []
    if isinstance(score, torch.Tensor):
        with eng._mark(mark):
            te, tv, _ = ops.explain_topk(eng.to_device(qp, np.int64), eng.to_device(cand["entry"]), score, k)
        te, tv = te.cpu().numpy().astype(np.int64), tv.cpu().numpy()
        # entry id -> candidate: the segments ascend by entry id
        total = dadj.total_nnz
        ckey = q_of.astype(np.int64) * total + cand["entry"]
        for q in range(n):
            ok = np.isfinite(tv[q]) & (te[q] >= 0)
            preds.append(edges_of[np.searchsorted(ckey, q * total + te[q][ok])])
            scores.append(tv[q][ok])
        return preds, scores
    for q in range(n):
        a, b = qp[q], qp[q + 1]
        o = np.lexsort((cand["entry"][a:b], -score[a:b]))
        o = o[np.isfinite(score[a:b][o])][:k]
        preds.append(edges_of[a:b][o])
        scores.append(score[a:b][o])
    return preds, scores


def integrated_gradients_batched(model, adjacency_data, test_triples, top_k=10, *, steps=256, quadrature="gauss",
                                 nodes=None, tol=None, max_steps=1024, toward="flip", threshold=0.5,
                                 exclude_target=False, relations=None, fused=None, return_attributions=False,
                                 stats=None):
    """Integrated-gradients edge attributions: per test triple, how much of the prediction each stored edge of rows h
    and t carries.  The path scales the values of the triple's eligible candidates (counterfactual_candidates; the
    others stay in the graph and get no attribution) from 0 to their stored values; attr_j = val_j * the integral of
    d p / d a_j along it, by the rule ``quadrature`` ("gauss": Gauss-Legendre on [0, 1]; "midpoint": the textbook sum)
    with ``steps`` nodes, or by ``nodes`` = (alpha, omega), which overrides both.  No random numbers.  Completeness:
    the attributions of a triple add up to p - p_baseline up to ``gap``, the rule's error; with ``tol`` the triples
    whose |gap| > tol are run again with twice the nodes until they pass or the next rule would exceed ``max_steps``
    (one host read of gap per round).

    The ranking is occlusion_batched's: the score is attr_j where the prediction is to be lowered (``toward``,
    ``threshold``: as there, from the unedited prediction) and -attr_j where it is to be raised, eligible candidates
    only, descending, ties by ascending entry id, ``top_k`` in 1 .. 64.  ``fused``: None takes the kernels
    (Engine.integrated_gradients) for fp32 features, D in {32, 64}, R <= 8 and an unsharded engine; False runs one
    set_values + Engine.value_grads per (triple, node) on the layered kernels (any width); True demands the kernels.
    ``stats``: an optional dict that receives ``fused``, ``candidates``, ``rounds`` and, fused, ``launch_events``.

    Returns a dict: ``p`` and ``p_baseline`` (n,); ``direction`` (n,) +1 where the ranking lowers p, -1 where it
    raises it; ``edges``: a list of (k_q, 3) int64 (head, rel, tail) arrays, ready for fidelity_curves and
    evaluate_explanations; ``scores``: a list of (k_q,) fp32; ``total`` and ``gap`` (n,); ``steps_used`` (n,);
    ``relation_attribution`` (n, R): the attributions summed per relation (its rows sum to ``total``); with
    ``return_attributions``, ``attributions``: a list of (candidates, 3) edge arrays and a list of their attributions
    (NaN: not eligible), per triple."""
    k = int(top_k)
    if not 1 <= k <= TOPK_MAX:
        raise IddgcnError(f"top_k must be in [1, {TOPK_MAX}], got {top_k}")
    _lowering(0.0, toward, threshold)
    if nodes is not None:
        if tol is not None:
            raise IddgcnError("tol doubles the rule's nodes: it cannot be combined with explicit nodes")
        al, om = (np.asarray(x, np.float64).reshape(-1) for x in nodes)
        if al.shape != om.shape or not 1 <= len(al) <= PATH_MAX_STEPS:
            raise IddgcnError(f"nodes must be (alpha, omega) of one length in [1, {PATH_MAX_STEPS}]")
    else:
        quadrature_rule(steps, quadrature)                         # refuses a bad rule before any device work
        if tol is not None and not int(steps) <= int(max_steps) <= PATH_MAX_STEPS:
            raise IddgcnError(f"max_steps must lie in [steps, {PATH_MAX_STEPS}], got {max_steps}")
    eng, params, triples, fused, dadj = _fused_or_layered(
        model, adjacency_data, test_triples, fused,
        "integrated gradients: the fused kernels take D in {32, 64}, fp32 features, 1 <= R <= 8 and an unsharded "
        "engine: use fused=False for this model")
    cand = counterfactual_candidates(dadj, triples, False, exclude_target, relations)
    n, R = len(triples), model.num_relations

    def run(idx, sub, alpha, omega):
        if fused:
            return eng.integrated_gradients(params, dadj, triples[idx], sub, alpha, omega)
        return _path_layered(eng, params, dadj, triples[idx], sub, alpha, omega)

    with _launch_events(stats) if fused else contextlib.nullcontext():
        if nodes is not None:
            res, used, rounds = run(np.arange(n), cand, al, om), np.full(n, len(al), np.int64), 1
        else:
            res, used, rounds = _refine_by_gap(run, cand, n, steps, quadrature, tol, max_steps)
    _note_route(stats, fused, cand, rounds=rounds)
    host = {nm: v.cpu().numpy() for nm, v in res.items()}
    # the fused route ranks on the device (ops.explain_topk), the per-node route on the host
    rank = lambda s: _rank_candidates(eng, dadj, cand, n, torch.as_tensor(s, device=eng.device) if fused else s, k)  # noqa: E731
    return _attribution_result(cand, n, R, host, used, toward, threshold, rank, return_attributions)


def _attribution_result(cand, n, R, host, used, toward, threshold, rank, return_attributions=False):
    """integrated_gradients_batched's dict from the host copies of the kernel's outputs; ``rank(score)`` ranks the
    per-candidate fp32 scores (-inf: not eligible)."""
    qp = cand["qptr"]
    q_of = np.repeat(np.arange(n), np.diff(qp))
    lower = _lowering(host["p_full"], toward, threshold)
    sign = np.where(lower, 1.0, -1.0).astype(np.float32)
    score = np.where(cand["eligible"], sign[q_of] * host["attr"], -np.inf).astype(np.float32)
    edges, scores = rank(score)
    rel_attr = np.zeros((n, R), np.float64)
    np.add.at(rel_attr, (q_of, cand["rel"].astype(np.int64)), host["attr"].astype(np.float64))
    out = dict(p=host["p_full"], p_baseline=host["p_base"], direction=np.where(lower, 1, -1).astype(np.int64),
               edges=edges, scores=scores, total=host["total"], gap=host["gap"], steps_used=used,
               relation_attribution=rel_attr)
    if return_attributions:
        edges_of = _candidate_edges(cand)
        table = np.where(cand["eligible"], host["attr"], np.nan).astype(np.float32)
        out["attributions"] = ([edges_of[qp[q]:qp[q + 1]] for q in range(n)],
                               [table[qp[q]:qp[q + 1]] for q in range(n)])
    return out


def integrated_gradients_summary(result, tol=1e-3):
    """How complete a batch of attributions is (host), from integrated_gradients_batched's dict: ``mean_abs_gap`` and
    ``max_abs_gap``; ``within_tol``: the share of triples with |gap| <= ``tol``; ``mean_shift`` = the mean
    |p - p_baseline|; ``relation_share``: per relation, its share of sum |relation_attribution| ({} when that is 0);
    ``mean_steps``; ``n``."""
    gap = np.abs(np.asarray(result["gap"], np.float64))
    p, pb = np.asarray(result["p"], np.float64), np.asarray(result["p_baseline"], np.float64)
    ra = np.abs(np.asarray(result["relation_attribution"], np.float64))
    if ra.ndim != 2 or not (len(gap) == len(p) == len(pb) == len(ra)):
        raise ValueError("result must be integrated_gradients_batched's dict")
    n, mass = len(gap), float(ra.sum())
    return dict(n=n, mean_abs_gap=float(gap.mean()) if n else 0.0, max_abs_gap=float(gap.max()) if n else 0.0,
                within_tol=float((gap <= tol).mean()) if n else 0.0,
                mean_shift=float(np.abs(p - pb).mean()) if n else 0.0,
                relation_share={int(r): float(ra[:, r].sum() / mass) for r in range(ra.shape[1])} if mass else {},
                mean_steps=float(np.mean(result["steps_used"])) if n else 0.0)


def explanation_metrics(preds, gt, top=5, exp_num=10):
    """eval_test.py:15-39: Precision@top / Recall@top / F1@top of one explanation against its
    ground-truth triples (both orientations of each predicted triple count)."""
    preds_set = set(map(tuple, np.asarray(preds)))
    flip = np.flip(np.asarray(preds), axis=1)
    flip_set = set(map(tuple, flip))
    gt_set = set(map(tuple, np.asarray(gt)))
    pl, fl = list(preds_set), list(flip_set)
    tp = len(set(pl[:top]) & gt_set) + len(set(fl[:top]) & gt_set)
    fp = top - tp
    fn = exp_num - (len(preds_set & gt_set) + len(flip_set & gt_set))
    precision = tp / (tp + fp) if tp + fp > 0 else 0
    recall = tp / (tp + fn) if tp + fn > 0 else 0
    f1 = 2 * precision * recall / (precision + recall) if precision + recall > 0 else 0
    return precision, recall, f1
