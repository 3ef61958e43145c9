"""Integrated gradients over the adjacency values restated in torch on the CPU, vectorised over queries in
tests/ref_fidelity.curves' style — a test helper.

Per node alpha the candidates' path values a_j (val_j alpha when eligible, val_j otherwise) are a leaf tensor; the AE
rows are built from them, pushed through oracle.ref_explain._layer's op order, and g_j = d p_q / d a_j comes from
autograd (a candidate belongs to one query, so one backward of sum_q p_q gives every query's gradients).
tests/test_integrated_gradients_host.py holds g to oracle.ref_explain.value_grads on the edited full COO (1e-12)."""
import numpy as np
import torch


def _tensors(params, triples, cand, dtype):
    P = {k: torch.tensor(np.asarray(v), dtype=dtype) for k, v in params.items()}
    tr = np.asarray(triples, np.int64)
    qptr = np.asarray(cand["qptr"], np.int64)
    q_of = np.repeat(np.arange(len(tr)), np.diff(qptr))
    rel, col, role = (np.asarray(cand[k], np.int64) for k in ("rel", "col", "role"))
    R = P["rel"].shape[0]
    rows = [torch.as_tensor((q_of * 2 + side) * R + rel) for side in (0, 1)]
    feeds = [torch.as_tensor((role >> side) & 1).to(dtype) for side in (0, 1)]
    return P, tr, rows, feeds, P["E"][torch.as_tensor(col)]


def forward(P, tr, rows, feeds, ecol, a, detach_weights=False):
    """p (Q,) for the candidates' values ``a`` (C,).  ``detach_weights``: the dynamic weights are treated as constants
    by autograd (a WRONG gradient on purpose: the host test shows that the GPU bars catch it)."""
    E = P["E"]
    Q = len(tr)
    R, D = P["rel"].shape
    h, r, t = (torch.as_tensor(tr[:, i]) for i in range(3))
    ae = torch.zeros(Q * 2 * R, D, dtype=E.dtype)
    for side in (0, 1):
        ae = ae.index_add(0, rows[side], (a * feeds[side])[:, None] * ecol)
    ae = ae.view(Q, 2, R, D)
    xh, xt = E[h], E[t]
    for l in (1, 2, 3):
        Kl, S, Wa, ba = P[f"K{l}"], P[f"S{l}"], P[f"Wa{l}"], P[f"ba{l}"]
        ho, to = xh @ S, xt @ S
        alpha = torch.softmax(xh @ Wa + ba, dim=-1)
        if detach_weights:
            alpha = alpha.detach()
        for i in range(R):
            w = torch.sigmoid(alpha[:, i])[:, None]
            ho = ho + w * (ae[:, 0, i] @ Kl[i])
            to = to + w * (ae[:, 1, i] @ Kl[i])
        xh, xt = torch.sigmoid(ho), torch.sigmoid(to)
    return torch.sigmoid(torch.sum(xh * P["rel"][r] * xt, dim=-1))


def path_values(cand, alpha, dtype):
    val = torch.tensor(np.asarray(cand["val"]), dtype=dtype)
    elig = torch.as_tensor(np.asarray(cand["eligible"], bool))
    return torch.where(elig, val * alpha, val)


def gradients(params, triples, cand, alpha, dtype=torch.float64, detach_weights=False):
    """(p (Q,), g (C,)): f_q(alpha) and g_j(alpha) = d f_q / d a_j for every candidate, float64 numpy, computed in
    ``dtype``."""
    P, tr, rows, feeds, ecol = _tensors(params, triples, cand, dtype)
    a = path_values(cand, torch.tensor(float(alpha), dtype=dtype), dtype).requires_grad_(True)
    p = forward(P, tr, rows, feeds, ecol, a, detach_weights)
    g = torch.autograd.grad(p.sum(), a)[0] if len(a) else torch.zeros(0, dtype=dtype)
    return p.detach().numpy().astype(np.float64), g.numpy().astype(np.float64)


def integrate(params, triples, cand, alpha, omega, dtype=torch.float64, detach_weights=False, times_val=True):
    """The definition of include/iddgcn_explain.h for the rule (alpha, omega): a dict of float64 numpy arrays ``attr``
    (C,; exactly 0 where not eligible), ``total``, ``p_full``, ``p_base``, ``gap`` (Q,), computed in ``dtype`` (nodes
    and weights rounded to it first).  ``times_val`` False leaves val_j out of attr_j (a WRONG answer on purpose)."""
    P, tr, rows, feeds, ecol = _tensors(params, triples, cand, dtype)
    al = torch.tensor(np.asarray(alpha, np.float64), dtype=dtype)
    om = torch.tensor(np.asarray(omega, np.float64), dtype=dtype)
    C, Q = len(cand["rel"]), len(tr)
    acc = torch.zeros(C, dtype=dtype)
    for i in range(len(al)):
        a = path_values(cand, al[i], dtype).requires_grad_(True)
        if C:
            acc = acc + om[i] * torch.autograd.grad(forward(P, tr, rows, feeds, ecol, a, detach_weights).sum(), a)[0]
    val = torch.tensor(np.asarray(cand["val"]), dtype=dtype)
    elig = torch.as_tensor(np.asarray(cand["eligible"], bool))
    attr = torch.where(elig, (val if times_val else torch.ones_like(val)) * acc, torch.zeros_like(acc))
    with torch.no_grad():
        ends = [forward(P, tr, rows, feeds, ecol, path_values(cand, torch.tensor(x, dtype=dtype), dtype))
                for x in (0.0, 1.0)]
    qptr = np.asarray(cand["qptr"], np.int64)
    q_of = torch.as_tensor(np.repeat(np.arange(Q), np.diff(qptr)))
    total = torch.zeros(Q, dtype=dtype).index_add(0, q_of, attr)
    gap = total - (ends[1] - ends[0])
    f64 = lambda x: x.numpy().astype(np.float64)  # noqa: E731
    return dict(attr=f64(attr), total=f64(total), p_full=f64(ends[1]), p_base=f64(ends[0]), gap=f64(gap))


def attr_bar(ref64, ref32, qptr):
    """The GPU bar for attr, per query: max(4 max_j |attr32_j - attr64_j|, 2^-20 max_j |attr64_j|) (0 for an empty
    query); and the bars for p_full / p_base: max(4 |p32 - p64|, 1e-6).  Returns (bar_attr (Q,), bar_full, bar_base)."""
    qptr = np.asarray(qptr, np.int64)
    Q = len(qptr) - 1
    dev = np.abs(ref32["attr"] - ref64["attr"])
    mag = np.abs(ref64["attr"])
    bar = np.zeros(Q)
    for q in range(Q):
        if qptr[q + 1] > qptr[q]:
            sl = slice(qptr[q], qptr[q + 1])
            bar[q] = max(4 * dev[sl].max(), 2.0 ** -20 * mag[sl].max())
    pb = lambda k: np.maximum(4 * np.abs(ref32[k] - ref64[k]), 1e-6)  # noqa: E731
    return bar, pb("p_full"), pb("p_base")


def edited_values(dadj, cand, q, alpha):
    """The full adjacency's value lists (one float64 array per relation, entry order) with query ``q``'s eligible
    candidates scaled by ``alpha``: what oracle.ref_explain.value_grads takes."""
    vals = dadj.base_values.cpu().numpy().astype(np.float64)
    a, b = cand["qptr"][q], cand["qptr"][q + 1]
    e = np.asarray(cand["entry"][a:b], np.int64)
    v = cand["val"][a:b].astype(np.float64)
    vals[e] = np.where(cand["eligible"][a:b], v * alpha, v)
    off = dadj.rel_offsets
    return [vals[off[r]:off[r + 1]] for r in range(dadj.num_relations)]
